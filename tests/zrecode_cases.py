"""The model of recoding a compressed pack set in place (mi_zset_recode, include/makisu_mi.h "recoding a compressed set in place",
DESIGN.md 4.15), in pure Python over zpack_cases.py, zpack2_cases.py and zprune_cases.py: recode_form is THE RULE for one entry;
Store (zprune_cases.Store with a recode) predicts the held forms, mi_zset_info, mi_zset_usage, which blobs are rewritten and
every counter of mi_recode_info -- peak_extra_bytes from the sizes of what a call of ONE round allocates.  No engine code is
involved."""
import functools

import numpy as np

import zpack_cases as zc
import zpack2_cases as z2
import zprune_cases as pr

TILE = pr.TILE
DEFAULT_SCRATCH = 256 << 20
alloc = pr.alloc


@functools.lru_cache(maxsize=None)
def coded(plain, level):
    """what the coder of `level` stores for a chunk"""
    return zc.compress_chunk(plain) if level == 1 else z2.compress_chunk2(plain)


def plain_of(stored_bytes, length):
    """what a stored form decodes to; None for one that breaks a decoding rule"""
    stored_bytes = bytes(stored_bytes)
    if len(stored_bytes) == length:
        return stored_bytes
    try:
        return zc.lz4_block_decode(stored_bytes, length)
    except ValueError:
        return None


def recode_form(stored_bytes, length, level):
    """THE RULE: the form held afterwards -- the candidate (what the coder of the level stores for the decoded bytes) if and
    only if it is strictly smaller than the stored form, else the stored form verbatim; a form that does not decode stays"""
    stored_bytes = bytes(stored_bytes)
    plain = plain_of(stored_bytes, length)
    if plain is None:
        return stored_bytes
    cand = coded(plain, level)
    return cand if len(cand) < len(stored_bytes) else stored_bytes


def worst_span(n):
    return zc.round16(n + n // 255 + 16)


def need(length, stored):
    """what an entry takes of a round's scratch: the plain bytes of a coded entry, and the worst-case coded span"""
    return (zc.round16(length) if stored < length else 0) + worst_span(length)


class Store(pr.Store):
    """zprune_cases.Store with mi_zset_recode"""

    def total_need(self):
        return sum(need(v[0], v[2]) for v in self.held.values())

    def min_rounds(self, scratch_bytes):
        """a lower bound of n_rounds: no round takes more than the bound, unless it is one entry alone"""
        bound = max(scratch_bytes or DEFAULT_SCRATCH, max(need(v[0], v[2]) for v in self.held.values()))
        return -(-self.total_need() // bound)

    def recode(self, level, verify=False, scratch_bytes=0):
        """-> every field of mi_recode_info but the times (n_rounds and peak_extra_bytes: of a call whose entries fit ONE round);
        the store afterwards is what the set must be"""
        n, cap, n_blobs = len(self.held), self.slots, len(self.blobs)
        info = dict.fromkeys(["n_digests", "n_recoded", "n_raw_recoded", "n_undecodable", "stored_before", "stored_after", "live_before",
                              "live_after", "n_blobs_rewritten", "n_blobs_freed", "freed_bytes", "new_blob_bytes", "n_rounds",
                              "peak_extra_bytes"], 0)
        info["n_digests"] = n
        info["stored_before"] = info["stored_after"] = sum(v[2] for v in self.held.values())
        if n == 0:
            return info
        info["live_before"] = info["live_after"] = sum(len(v[1]) for v in self.held.values())
        assert self.total_need() <= (scratch_bytes or DEFAULT_SCRATCH), "the model's sizes are those of one round"
        info["n_rounds"] = 1
        new = {}
        for k, (length, span, stored, bid) in self.held.items():
            form = span[:stored]
            if plain_of(form, length) is None or any(span[stored:]):
                info["n_undecodable"] += 1
                continue
            now = recode_form(form, length, level)
            if len(now) < stored:
                new[k] = now
        nb = (cap + TILE - 1) // TILE
        # bases, marks, totals, the scan; the rows (five words), rules, candidates, new sizes, blobs (a word each), the list of
        # replaced rows; VERIFY: the hashing pass's strings and digests; the scratch
        extra = alloc(n_blobs * 8) + alloc(n_blobs) + alloc(128) + alloc(2 * nb * 8) + alloc(5 * n * 8) + 4 * alloc(n * 4) + alloc(n * 8)
        if verify:
            extra += alloc(2 * n * 8) + alloc(n * 32)
        extra += alloc(self.total_need())
        info["peak_extra_bytes"] = extra
        if not new:
            return info
        staged = sum(zc.round16(len(f)) for f in new.values())
        rewritten = sorted({self.held[k][3] for k in new})
        moved = [k for k, v in self.held.items() if v[3] in rewritten]
        for k, f in new.items():
            length, _, stored, bid = self.held[k]
            info["n_raw_recoded"] += 1 if stored == length else 0
            self.held[k] = (length, f + bytes(zc.round16(len(f)) - len(f)), len(f), bid)
        blob_bytes = sum(len(self.held[k][1]) for k in moved)
        new_cap = 1024
        while new_cap < 2 * n:
            new_cap *= 2
        table = alloc(new_cap * 8) + alloc(new_cap * 48)
        nb2 = (n + TILE - 1) // TILE
        # the staging piece, the move's scan, THE NEW BLOB, the move list, the per-row addresses, the new table, the records, the
        # insert's scratch; VERIFY: the recheck's strings and digests
        extra += alloc(staged) + alloc(2 * nb2 * 8) + alloc(blob_bytes) + alloc(4 * len(moved) * 8) + alloc(n * 8)
        extra += table + alloc(n * 48) + alloc(n + 16) + alloc(n * 8 + 16) + alloc(64)
        if verify:
            extra += alloc(2 * len(new) * 8) + alloc(len(new) * 32)
        info["peak_extra_bytes"] = extra
        info["n_recoded"] = len(new)
        info["stored_after"] = sum(v[2] for v in self.held.values())
        info["live_after"] = sum(len(v[1]) for v in self.held.values())
        info["n_blobs_rewritten"] = info["n_blobs_freed"] = len(rewritten)
        info["freed_bytes"] = sum(alloc(self.blobs[b]) for b in rewritten)
        info["new_blob_bytes"] = blob_bytes
        for b in rewritten:
            del self.blobs[b]
        bid = self.next_blob
        self.next_blob += 1
        self.blobs[bid] = blob_bytes
        for k in moved:
            v = self.held[k]
            self.held[k] = (v[0], v[1], v[2], bid)
        self.slots, self.table_bytes = new_cap, table
        return info

    def cut(self, digests):
        """the zpack mi_zset_zpack cuts for distinct digests -> (entries, blob): the held forms on the 16-byte grid, ZERO pads"""
        keys = pr._keys(digests)
        entries = np.zeros(len(keys), dtype=zc.ZENTRY_DTYPE)
        parts, at = [], 0
        for i, k in enumerate(keys):
            length, span, stored, _ = self.held[k]
            entries["digest"][i] = np.frombuffer(k, dtype=np.uint8)
            entries["offset"][i], entries["chunk_index"][i], entries["length"][i], entries["stored"][i] = at, i, length, stored
            parts.append(span[:stored] + bytes(len(span) - stored))
            at += len(span)
        return entries, b"".join(parts)


# ---- the inputs: the planted chunks of both levels' tests, once each ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted():
    """-> (names, chunks): zpack_cases.planted_chunks() and zpack2_cases.planted_chunks2(), deduplicated by their bytes"""
    names, chunks, seen = [], [], set()
    for name, chunk, _ in list(zc.planted_chunks()) + list(z2.planted_chunks2()):
        if chunk in seen:
            continue
        seen.add(chunk)
        names.append(name)
        chunks.append(bytes(chunk))
    return names, chunks


@functools.lru_cache(maxsize=None)
def classes():
    """the planted chunks by what level 2 does to level 1's form -> (smaller, same, larger): lists of chunk numbers; of
    `smaller`, raw_at_1: those level 1 keeps raw"""
    _, chunks = planted()
    smaller, same, larger, raw_at_1 = [], [], [], []
    for i, c in enumerate(chunks):
        a, b = len(coded(c, 1)), len(coded(c, 2))
        (smaller if b < a else same if b == a else larger).append(i)
        if b < a and a == len(c):
            raw_at_1.append(i)
    return smaller, same, larger, raw_at_1


def zpack_at(chunks, level, alg=None, digests=None):
    """distinct chunks -> (zentries, zblob) as the model of `level` codes them, in this order"""
    import pack_cases as pc
    entries, blob = zc.pack_of(chunks, pc.SHA256 if alg is None else alg)
    if digests is not None:
        entries = entries.copy()
        entries["digest"] = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    return zc.model_compress(entries, blob) if level == 1 else z2.model_compress2(entries, blob)


def raw_zpack(chunks, alg=None):
    """distinct chunks -> a zpack with every entry raw (stored == length)"""
    import pack_cases as pc
    return zc.build_zpack([zc._entry(c, len(c), c) for c in chunks], pc.SHA256 if alg is None else alg)
