"""Models of the two cuts that serve a compressed set to a plainer reader, in Python, from the existing models
alone: nothing here restates a format.

  the unwrapped cut (mi_zset_zpack_unwrapped)   per entry zentropy_cases.huff_decode's inner bytes for a form H span, the span
                                                itself otherwise, laid out by round16 in order of first occurrence;
  the plain cut (mi_zset_pack)                  fetch_cases.model_subpack over zentropy_cases.expand_chunk.

A STORE here is what a compressed set holds: {digest: (stored form, length, the pad bytes behind it)}, the first form of a digest
winning as in the set."""
import numpy as np

import fetch_cases as fc
import zentropy_cases as ze
import zpack_cases as zc

PLAN_TILE = 2048                                                   # csrc/mi_plan.h: rows per block of the sizing and entries passes
WAVE_GRID = 65536                                                  # csrc/mi_zserve.hip: both one-wave-a-row kernels launch min(n, 65536) workgroups


def store_add(store, zentries, zblob):
    """the entries of one zpack into a store; a digest met again keeps its first form"""
    for k in range(len(zentries)):
        off, n, stored = int(zentries["offset"][k]), int(zentries["length"][k]), int(zentries["stored"][k])
        store.setdefault(zentries["digest"][k].tobytes(), (bytes(zblob[off:off + stored]), n, bytes(zblob[off + stored:off + zc.round16(stored)])))
    return store


def unwrapped_form(stored, length):
    """what the unwrapped cut carries for one stored form: the inner form of a form H span, else the span"""
    return ze.huff_decode(stored, length)[1] if ze.is_form_h(stored, length) else bytes(stored)


def unwrap_rule(stored, length, pad=b""):
    """the rule the unwrapped cut refuses one held form with, 0 for none: a form H row that does not unwrap (8..11) or whose pad
    is not zero (7); a row that is moved verbatim is not looked at"""
    if not ze.is_form_h(stored, length):
        return 0
    try:
        ze.huff_decode(stored, length)
    except ze.Refused as e:
        return e.rule
    return ze.RULE_PAD if any(pad) else 0


def decode_rule(stored, length, pad=b""):
    """the rule the plain cut refuses one held form with, 0 for none: zentropy_cases.first_refused's, for one entry"""
    rule, _ = ze.chunk_rule(stored, length)
    return rule or (ze.RULE_PAD if any(pad) else 0)


def _firsts(digests):
    seen, rows = set(), []
    for r, k in enumerate(fc._rows(digests)):
        if k not in seen:
            seen.add(k)
            rows.append((r, k))
    return rows


def first_refused(store, digests, rule_of):
    """(request row, rule) of the smallest requested row rule_of (unwrap_rule / decode_rule) refuses; None if none"""
    for r, k in _firsts(digests):
        rule = rule_of(*store[k])
        if rule:
            return r, rule
    return None


def model_zpack_unwrapped(store, digests):
    """-> (ZENTRY_DTYPE entries, blob): every distinct requested digest once, in order of first occurrence, chunk_index = the
    request row of that occurrence, form H replaced by its inner form, pads zero.  KeyError for a digest the store lacks"""
    rows = _firsts(digests)
    out = np.zeros(len(rows), dtype=zc.ZENTRY_DTYPE)
    parts, at = [], 0
    for i, (r, k) in enumerate(rows):
        stored, n, _ = store[k]
        form = unwrapped_form(stored, n)
        out["digest"][i] = np.frombuffer(k, dtype=np.uint8)
        out["offset"][i], out["chunk_index"][i], out["length"][i], out["stored"][i] = at, r, n, len(form)
        parts.append(form + bytes(zc.round16(len(form)) - len(form)))
        at += zc.round16(len(form))
    return out, b"".join(parts)


def model_pack(store, digests, alg=None):
    """-> (pack_cases.ENTRY_DTYPE entries, blob): fetch_cases.model_subpack over the expanded chunks of the requested digests"""
    plain = {}
    for _, k in _firsts(digests):
        stored, n, _ = store[k]
        plain[k] = ze.expand_chunk(stored, n)
    return fc.model_subpack(plain, digests, alg)


def forms_in(store, digests):
    """the request's distinct digests by form (zentropy_cases.form_of's numbers) -> [count] * 4"""
    out = [0, 0, 0, 0]
    for _, k in _firsts(digests):
        out[ze.form_of(store[k][0], store[k][1])] += 1
    return out


def many_rows_conditions(is_h, n_rows):
    """for a request of every row once, in row order: the requested rows that are form H, the tile boundaries of the sizing pass
    with a form H row on EACH side, and the form H rows a workgroup of the wave kernels meets on its second trip"""
    n_h = int(np.count_nonzero(is_h))
    both = sum(1 for t in range(PLAN_TILE, n_rows, PLAN_TILE) if is_h[t - 1] and is_h[t])
    second = int(np.count_nonzero(is_h[WAVE_GRID:]))
    return n_h, both, second
