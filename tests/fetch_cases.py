"""The chunk fetch's model, in pure Python, over pack_cases.py and restore_cases.py: what mi_packset_missing must answer and the
pack mi_packset_pack must cut (include/makisu_mi.h "fetch only what is missing"), from a store {digest: chunk bytes}
(restore_cases.chunk_store) and a request of digests.  No engine code is involved.  Also the planted inputs the GPU tests
rest on (tests/test_gpu_chunk_fetch.py), so that tests/test_host_chunk_fetch.py can state their properties without a GPU."""
import numpy as np

import pack_cases as pc

TILE = 16384              # bytes of a sub-pack's blob one workgroup of the gather writes
TILE_ENTRIES = 1024       # ... and the most entries that reach into it (an entry takes a 16-byte unit at least)
PLAN_BLOCK = 2048         # request rows per block of the plan's scan; 256 blocks go through the second level at a time


def _rows(digests):
    d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    raw = d.tobytes()
    return [raw[32 * i:32 * i + 32] for i in range(len(d))]


def model_missing(store, digests, lengths=None):
    """-> (held: uint8[n], want_rows: uint64[n_want], info: dict of mi_want_info's six counters).  A stated length of 0 or
    one that differs from a HELD chunk's raises ValueError naming the smallest such row."""
    keys = _rows(digests)
    n = len(keys)
    lens = None if lengths is None else [int(x) for x in np.asarray(lengths).reshape(-1)]
    assert lens is None or len(lens) == n
    held = np.zeros(n, dtype=np.uint8)
    seen, want = set(), []
    info = dict(n_rows=n, n_distinct=0, n_held=0, n_want=0, held_bytes=0, want_bytes=0)
    for r, k in enumerate(keys):
        has = store.get(k)
        held[r] = has is not None
        if lens is not None and (lens[r] == 0 or (has is not None and len(has) != lens[r])):
            raise ValueError("row %d" % r)
        if k in seen:
            continue
        seen.add(k)
        info["n_distinct"] += 1
        if has is not None:
            info["n_held"] += 1
            info["held_bytes"] += len(has)
        else:
            info["n_want"] += 1
            info["want_bytes"] += lens[r] if lens is not None else 0
            want.append(r)
    return held, np.array(want, dtype=np.uint64), info


def model_subpack(store, digests, alg=None):
    """-> (entries in pack_cases.ENTRY_DTYPE, blob): every distinct requested digest once, in order of first occurrence,
    chunk_index = the request row of that occurrence, the layout of pack_cases.model_pack.  A digest the store lacks raises
    KeyError.  alg (pack_cases.SHA256 / BLAKE2S): also hold every chunk against its digest; None: the digests are opaque."""
    keys = _rows(digests)
    seen, rows, parts, offs = set(), [], [], []
    at = 0
    for r, k in enumerate(keys):
        if k in seen:
            continue
        seen.add(k)
        piece = store[k]
        assert len(piece) > 0
        if alg is not None:
            assert pc.HASHES[alg](piece).digest() == k, r
        rows.append(r)
        offs.append(at)
        parts.append(piece + b"\0" * (pc.round16(len(piece)) - len(piece)))
        at += pc.round16(len(piece))
    entries = np.zeros(len(rows), dtype=pc.ENTRY_DTYPE)
    if rows:
        entries["digest"] = np.frombuffer(b"".join(keys[r] for r in rows), dtype=np.uint8).reshape(-1, 32)
        entries["offset"] = offs
        entries["chunk_index"] = rows
        entries["length"] = [len(store[keys[r]]) for r in rows]
    return entries, b"".join(parts)


def raw_pack(digests, chunks, pad=0):
    """a pack of the given chunks under the given (possibly fake) digests, in the given order, the pad bytes `pad`: what an
    unverified source may look like.  -> (entries, blob)"""
    entries = np.zeros(len(chunks), dtype=pc.ENTRY_DTYPE)
    parts, at = [], 0
    for k, piece in enumerate(chunks):
        entries["offset"][k], entries["chunk_index"][k], entries["length"][k] = at, k, len(piece)
        parts.append(piece + bytes([pad]) * (pc.round16(len(piece)) - len(piece)))
        at += pc.round16(len(piece))
    if len(chunks):
        entries["digest"] = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    return entries, b"".join(parts)


def fake_digests(rng, n):
    """n distinct opaque digests (a set added without verification takes any 32 bytes)"""
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d[:, 8:16] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)        # distinct whatever the rest is
    return d


# ---- the planted tile-edge request -----------------------------------------------------------------------------------------
# In SUB-PACK order (= request order, every digest once).  Offsets follow from the lengths, each rounded up to 16:
#   [0, 1 008)          sixteen entries of 48 + r bytes, r = 0..15: every length residue mod 16
#   [1 008, 1 088)      1, 15, 16, 17 bytes
#   [1 088, 16 384)     one entry of 15 296 bytes: it ENDS on tile 0's last byte
#   [16 384, 32 768)    1 024 entries of 16 bytes: the first BEGINS on tile 1's first byte, the tile holds 1 024 entries
#   [32 768, 98 304)    one entry of 65 536 bytes: tiles 2..5, none of which holds another entry
#   [98 304, 98 352)    33 bytes: the blob's size is not a multiple of the tile
EDGE_LENGTHS = [48 + r for r in range(16)] + [1, 15, 16, 17] + [15296] + [16] * 1024 + [65536] + [33]


def edge_case(seed=61, pad=0xA5):
    """-> (request digests, chunks, source packs): the planted lengths under fake digests; the SOURCE is two packs that hold
    the chunks in another order (reversed, odd and even positions apart) with NON-ZERO pad bytes"""
    rng = np.random.default_rng(seed)
    n = len(EDGE_LENGTHS)
    dig = fake_digests(rng, n)
    chunks = [rng.integers(1, 256, k, dtype=np.uint8).tobytes() for k in EDGE_LENGTHS]      # no zero byte: a pad cannot pass for data
    order = list(range(n))[::-1]
    packs = [raw_pack(dig[sel], [chunks[i] for i in sel], pad) for sel in (order[0::2], order[1::2])]
    return dig, chunks, packs


def tripled_request(rng, digests):
    """every digest three times, interleaved: three shuffles of the rows merged at random -> (request, the rows' sources)"""
    n = len(digests)
    src = np.concatenate([rng.permutation(n) for _ in range(3)])
    src = src[rng.permutation(3 * n)]
    return np.ascontiguousarray(digests[src]), src
