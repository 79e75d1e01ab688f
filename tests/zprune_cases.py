"""The model of pruning a compressed pack set in place (mi_zset_prune, include/makisu_mi.h "pruning a compressed set in place",
DESIGN.md 4.12), in pure Python over zpack_cases.py: a dict digest -> (length, the stored form's bytes INCLUDING THE PAD AS ADDED,
stored, blob id) and the blobs' sizes.  It predicts the held set, mi_zset_info, mi_zset_usage, per-blob live bytes, which blobs
a prune frees or compacts for a given permille, and every field of mi_prune_info except the times -- peak_extra_bytes from the
sizes of what the call allocates.  No engine code is involved."""
import functools

import numpy as np

import zpack_cases as zc

TILE = 2048                                            # slots a block of the plan's scan covers


def alloc(n):
    """what an allocation of n bytes takes from the device: n rounded up to 256, plus 256 bytes of slack"""
    return (n + 255) // 256 * 256 + 256


def grown(n):
    """what a buffer that may grow takes (a table made by create or by an add): one eighth on top, plus 256"""
    return n + n // 8 + 256


def _keys(digests):
    d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    return [bytes(x) for x in d]


class Store:
    """a compressed pack set as the calls see it"""

    def __init__(self, hint=0):
        self.held = {}                                 # digest -> (length, span bytes with the pad, stored, blob id)
        self.blobs = {}                                # blob id -> bytes as added (a compaction blob: the moved bytes); insertion order
        self.next_blob = 0
        self.n_packs = self.n_entries = self.blob_bytes = 0
        self.slots = 1024
        while self.slots < 2 * hint:
            self.slots *= 2
        self.table_bytes = grown(self.slots * 8) + grown(self.slots * 48)

    # ---- adds ---------------------------------------------------------------------------------------------------------------
    def add(self, zentries, zblob):
        n = len(zentries)
        self.n_packs += 1
        if n == 0:
            return
        need = (len(self.held) + n) * 2
        if need > self.slots:
            while self.slots < need:
                self.slots *= 2
            self.table_bytes = grown(self.slots * 8) + grown(self.slots * 48)
        bid = self.next_blob
        self.next_blob += 1
        self.blobs[bid] = len(zblob)
        for en in zentries:
            at, stored = int(en["offset"]), int(en["stored"])
            self.held.setdefault(bytes(en["digest"]), (int(en["length"]), bytes(zblob[at:at + zc.round16(stored)]), stored, bid))
        self.n_entries += n
        self.blob_bytes += sum(zc.round16(int(s)) for s in zentries["stored"])

    # ---- what the getters answer ------------------------------------------------------------------------------------------------
    def info(self):
        return {"n_packs": self.n_packs, "n_entries": self.n_entries, "n_digests": len(self.held), "blob_bytes": self.blob_bytes,
                "stored_bytes": sum(v[2] for v in self.held.values()), "chunk_bytes": sum(v[0] for v in self.held.values())}

    def live(self):
        """blob id -> the sum of round16(stored) over the held digests that lie in it"""
        out = {b: 0 for b in self.blobs}
        for _, span, _, bid in self.held.values():
            out[bid] += len(span)
        return out

    def usage(self):
        return {"n_blobs": len(self.blobs), "resident_bytes": sum(alloc(b) for b in self.blobs.values()),
                "live_bytes": sum(self.live().values()), "table_slots": self.slots, "table_bytes": self.table_bytes}

    def missing(self, digests):
        """-> held flags per row"""
        return [1 if k in self.held else 0 for k in _keys(digests)]

    # ---- the prune --------------------------------------------------------------------------------------------------------------
    def prune(self, digests, keep=True, permille=0):
        """-> every field of mi_prune_info but the times; the store afterwards is what the set must be"""
        keys = _keys(digests)
        named = set(keys)
        n, cap, n_blobs = len(keys), self.slots, len(self.blobs)
        info = dict.fromkeys(["n_rows", "n_unknown", "n_dropped", "dropped_stored_bytes", "dropped_chunk_bytes", "n_blobs_freed", "freed_bytes",
                              "n_blobs_compacted", "moved_bytes", "n_blobs_sparse_kept", "peak_extra_bytes"], 0)
        info["n_rows"] = n
        info["n_unknown"] = sum(1 for k in keys if k not in self.held)
        victims = [k for k in self.held if (k in named) != keep]
        info["n_dropped"] = len(victims)
        info["dropped_stored_bytes"] = sum(self.held[k][2] for k in victims)
        info["dropped_chunk_bytes"] = sum(self.held[k][0] for k in victims)
        extra = alloc(n * 32) + alloc(cap) + alloc(cap * 4) + 2 * alloc(n_blobs * 8) + alloc(64)        # request, marks, per-slot blob, bases, sums, totals
        if not victims:
            info["peak_extra_bytes"] = extra
            return info
        for k in victims:
            del self.held[k]
        live = self.live()
        dead = [b for b in self.blobs if live[b] == 0]
        sparse = [b for b in self.blobs if 0 < live[b] * 1000 < permille * self.blobs[b]]
        moved = sum(live[b] for b in sparse)
        n_move = sum(1 for v in self.held.values() if v[3] in sparse)
        if sparse:
            nb = (cap + TILE - 1) // TILE
            extra += alloc(n_blobs) + alloc((2 * nb + 8) * 8) + alloc(moved)                              # fates, the scan, THE NEW BLOB
            extra += alloc(4 * n_move * 8) + alloc(cap * 8)                                              # the move list, the per-slot addresses
        survive = len(self.held)
        new_cap = 1024
        while new_cap < 2 * survive:
            new_cap *= 2
        table = alloc(new_cap * 8) + alloc(new_cap * 48)
        extra += table + alloc(survive * 48) + alloc(survive + 16) + alloc(survive * 8 + 16) + alloc(64)  # records, the insert's scratch
        info["peak_extra_bytes"] = extra
        info["n_blobs_freed"] = len(dead) + len(sparse)
        info["freed_bytes"] = sum(alloc(self.blobs[b]) for b in dead + sparse)
        info["n_blobs_compacted"] = len(sparse)
        info["moved_bytes"] = moved
        for b in dead + sparse:
            del self.blobs[b]
        if sparse:
            bid = self.next_blob
            self.next_blob += 1
            self.blobs[bid] = moved
            for k, v in self.held.items():
                if v[3] in sparse:
                    self.held[k] = (v[0], v[1], v[2], bid)
        self.slots, self.table_bytes = new_cap, table
        return info


def crafted_digests(n, rng, first=1):
    """n opaque digests (for unverified sets) whose first eight bytes are first, first + 1, ... (little endian): in a table of more
    than first + n slots entry k is AT HOME in slot first + k and nothing collides, so the slot order -- the order of a prune's move
    list, and so of its new blob -- is the entries' order"""
    dig = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for k in range(n):
        dig[k, :8] = np.frombuffer(int(first + k).to_bytes(8, "little"), dtype=np.uint8)
    return dig


EDGE_SEED = 3


@functools.lru_cache(maxsize=None)
def edge_store(seed=EDGE_SEED):
    """test 4's zpack: 2 649 chunks of 13 to 40 bytes, most of them raw, every 50th coded (13 to 40 bytes of one value), under
    crafted digests.  Every 4th entry up to 2 400 is a victim for good; of the rest, survivors(n) takes the LAST entry -- whose
    span ends on the source blob's last unit and, having the largest tag, on the new blob's -- and the first n - 1 others.
    -> (chunks, digests, zentries, zblob, candidates)"""
    import zset_cases as qc
    rng = np.random.default_rng(seed)
    n_all = 2649
    chunks = []
    for i in range(n_all):
        n = 13 + int(rng.integers(0, 28))
        chunks.append(bytes([i // 50 + 1]) * n if i % 50 == 0 else rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    assert len(set(chunks)) == n_all
    dig = crafted_digests(n_all, rng)
    _, _, ze, zb = qc.zpack_of(chunks, digests=dig)
    victims = set(range(0, 2400, 4))
    cand = [n_all - 1] + [i for i in range(n_all - 1) if i not in victims]
    return chunks, dig, ze, zb, cand


def edge_layout(ze, survivors):
    """the new blob a prune that compacts edge_store's blob must make: the survivors' spans in slot order = entry order
    -> [(entry, offset, bytes)], total"""
    out, at = [], 0
    for i in sorted(survivors):
        span = zc.round16(int(ze["stored"][i]))
        out.append((i, at, span))
        at += span
    return out, at


def three_fates(seed=201):
    """test 1's store: three zpacks -- A dies wholly, B keeps half, C keeps all -- with raw and coded entries and stored sizes
    = 0, 1 and 15 (mod 16) among the survivors of B.  C is large, so that the memory claim has something to be below.
    -> (chunk lists a, b, c; the numbers of b's chunks that stay)"""
    rng = np.random.default_rng(seed)
    a = [zc.text_like(700, 1), rng.integers(0, 256, 90, dtype=np.uint8).tobytes(), zc.text_like(3000, 2)]
    b = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),         # raw, stored = 0 (mod 16)
         zc.text_like(900, 3),
         rng.integers(0, 256, 33, dtype=np.uint8).tobytes(),         # raw, 1
         zc.text_like(1200, 4),
         zc.tail_chunk(rng, 7, 15),                                  # coded, 15
         zc.text_like(2500, 5),
         zc.tail_chunk(rng, 3, 1),                                   # coded, 1
         rng.integers(0, 256, 500, dtype=np.uint8).tobytes()]
    c = [rng.integers(0, 256, 30000 + 16 * i, dtype=np.uint8).tobytes() for i in range(5)] + [zc.text_like(4096, 6)]
    return a, b, c, [0, 2, 4, 6]
