"""The model of mi_zset_recode with the entropy stage (MI_ZPACK_ENTROPY), over zrecode_cases.py -- which stays as
it is -- and zentropy_cases.py.  THE RULE is zrecode_cases.recode_form's with two things widened: a stored form may be form H
(it is decoded through the unwrap), and with the flag the candidate is the level's form WITH THE STAGE OVER IT
(zentropy_cases.compress_chunk_h).  A stored form is replaced if and only if the candidate is strictly smaller; a form that does
not decode, or whose pad is not zero, stays.  No engine code is involved."""
import numpy as np

import zentropy_cases as ze
import zpack_cases as zc
import zrecode_cases as zr


def plain_of(stored_bytes, length):
    """what a stored form of any of the four kinds decodes to; None for one that breaks a rule"""
    rule, plain = ze.chunk_rule(stored_bytes, length)
    return plain if rule == 0 else None


def candidate(plain, level, entropy):
    return ze.compress_chunk_h(plain, level) if entropy else zr.coded(plain, level)


def recode_form(stored_bytes, length, level, entropy):
    stored_bytes = bytes(stored_bytes)
    plain = plain_of(stored_bytes, length)
    if plain is None:
        return stored_bytes
    cand = candidate(plain, level, entropy)
    return cand if len(cand) < len(stored_bytes) else stored_bytes


def forms_of(zentries, zblob):
    """a zpack -> its stored forms, entry by entry"""
    return [bytes(zblob[int(e["offset"]):int(e["offset"]) + int(e["stored"])]) for e in zentries]


def recode_forms(forms, lengths, level, entropy, pads_ok=None):
    """the forms held after one call -> (forms, how many were replaced, how many do not decode)"""
    out, replaced, undecodable = [], 0, 0
    for i, (f, n) in enumerate(zip(forms, lengths)):
        if plain_of(f, n) is None or (pads_ok is not None and not pads_ok[i]):
            undecodable += 1
            out.append(f)
            continue
        now = recode_form(f, n, level, entropy)
        replaced += len(now) < len(f)
        out.append(now)
    return out, replaced, undecodable


def cut_of(digests, lengths, forms):
    """the zpack mi_zset_zpack cuts for these digests in this order, holding these forms -> (entries, blob)"""
    entries = np.zeros(len(forms), dtype=zc.ZENTRY_DTYPE)
    parts, at = [], 0
    for i, f in enumerate(forms):
        entries["digest"][i] = digests[i]
        entries["offset"][i], entries["chunk_index"][i], entries["length"][i], entries["stored"][i] = at, i, lengths[i], len(f)
        parts.append(f + bytes(zc.round16(len(f)) - len(f)))
        at += zc.round16(len(f))
    return entries, b"".join(parts)


def census(forms, lengths):
    out = [[0, 0] for _ in range(4)]
    for f, n in zip(forms, lengths):
        k = ze.form_of(f, n)
        out[k][0] += 1
        out[k][1] += len(f)
    return out
