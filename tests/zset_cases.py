"""The compressed pack set's model, in pure Python, over zpack_cases.py, fetch_cases.py and restore_cases.py: the zpack
mi_zset_zpack must cut (include/makisu_mi.h "compressed pack sets") from zpacks and a request of digests -- the
stored forms moved as they are -- and the planted inputs of tests/test_gpu_chunk_zset.py, so that
tests/test_host_chunk_zset.py can state their properties without a GPU.  No engine code is involved."""
import numpy as np

import fetch_cases as fc
import pack_cases as pc
import zpack_cases as zc


def stored_store(zpacks):
    """zpacks: (entries, blob) pairs -> digest bytes -> (length, the stored form's bytes); a digest met again is kept once
    (the first form wins)"""
    store = {}
    for entries, blob in zpacks:
        for en in entries:
            at, stored = int(en["offset"]), int(en["stored"])
            store.setdefault(bytes(en["digest"]), (int(en["length"]), bytes(blob[at:at + stored])))
    return store


def model_cut(zpacks, digests):
    """-> (entries in zc.ZENTRY_DTYPE, blob): model_subpack composed with the stored forms -- every distinct requested digest
    once, in order of first occurrence, chunk_index = the request row of that occurrence, entry k at the sum of round16(stored)
    before it, the pads ZERO whatever the sources held.  A digest no zpack holds raises KeyError."""
    store = stored_store(zpacks)
    keys = fc._rows(digests)
    seen, rows, parts = set(), [], []
    for r, k in enumerate(keys):
        if k in seen:
            continue
        seen.add(k)
        rows.append((r, k, store[k]))
    entries = np.zeros(len(rows), dtype=zc.ZENTRY_DTYPE)
    at = 0
    for i, (r, k, (length, piece)) in enumerate(rows):
        entries["digest"][i] = np.frombuffer(k, dtype=np.uint8)
        entries["offset"][i], entries["chunk_index"][i], entries["length"][i], entries["stored"][i] = at, r, length, len(piece)
        parts.append(piece + b"\0" * (zc.round16(len(piece)) - len(piece)))
        at += zc.round16(len(piece))
    return entries, b"".join(parts)


def zpack_of(chunks, alg=pc.SHA256, digests=None):
    """distinct chunks -> the zpack the model makes of the plain pack that holds them in this order (digests: opaque ones
    instead of the chunks' own) -> (plain entries, plain blob, zentries, zblob)"""
    entries, blob = zc.pack_of(chunks, alg)
    if digests is not None:
        entries = entries.copy()
        entries["digest"] = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    zentries, zblob = zc.model_compress(entries, blob)
    return entries, blob, zentries, zblob


def with_pads(zentries, zblob, pad):
    """the same zpack with every pad byte `pad`: what an unverified source may look like"""
    out = bytearray(zblob)
    for en in zentries:
        end = int(en["offset"]) + int(en["stored"])
        for i in range(end, int(en["offset"]) + zc.round16(int(en["stored"]))):
            out[i] = pad
    return bytes(out)


def digests_of(chunks, alg=pc.SHA256):
    return np.frombuffer(b"".join(pc.HASHES[alg](c).digest() for c in chunks), dtype=np.uint8).reshape(-1, 32)


def recipe(chunks, order, alg=pc.SHA256, dig=None):
    """the recipe that lists chunks[k] for k in order -> (digests (n, 32) uint8, lengths uint32)"""
    dig = digests_of(chunks, alg) if dig is None else dig
    return np.ascontiguousarray(dig[list(order)]), np.array([len(chunks[k]) for k in order], dtype=np.uint32)


# ---- the planted rows of the fused restore: every length once raw and once coded -------------------------------------------
ROW_LENGTHS = [1, 12, 13, 15, 16, 17, 31, 32, 33, 64 * 16 + 5, 65536]
LONG_MATCH = 19 + 255 * 64                 # a match length whose extension bytes take more than one round of 64


def restore_rows(seed=71):
    """-> [(name, chunk, coded?)]: ROW_LENGTHS raw (a filler: nothing to find in it; under 13 bytes always raw) and coded (13
    bytes and more: a period of 1 or 2 for the short ones, planted copies for 64 * 16 + 5, a period of 3 over 65 536), then
    the planted chunks of zpack_cases that carry the offsets, literal runs and match lengths the decoder has edges at"""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(ROW_LENGTHS):
        out.append(("raw %d" % n, bytes(zc.filler(rng, n)), False))
        if n < zc.MIN_CHUNK:
            continue
        if n <= 33:
            unit = bytes([0x61 + i, 0x30 + i]) if n in (15, 17, 32) else bytes([0x41 + i])    # offsets 2 and 1 (13 bytes: only 1 fits)
            chunk = (unit * n)[:n]
        elif n < 65536:
            chunk, _ = zc.planted(rng, n, [(0, 300, 273), (100, 700, 274)])
        else:
            chunk = (b"xyz" * n)[:n]
        out.append(("coded %d" % n, chunk, True))
    planted = {name: chunk for name, chunk, _ in zc.planted_chunks()}
    for name in ["offset 1", "offset 2", "offset 63", "offset 64", "offset 65", "literal run 269", "literal run 270", "literal run 271",
                 "match length 273", "match length 274"]:
        out.append((name, planted[name], True))
    assert len({c for _, c, _ in out}) == len(out)
    return out


def residue_files(rows):
    """sixteen files over the rows' chunks: file r begins with a row of r bytes (r > 0), so every row that follows begins at
    every destination residue mod 16 once over the files (a file begins on a 256-byte boundary); raw and coded rows alternate
    so that each kind follows the other, and every file ends with two digests it has held before.
    -> (chunks, per file the list of chunk numbers)"""
    chunks = [c for _, c, _ in rows]
    rng = np.random.default_rng(72)
    shifts = [bytes(zc.filler(rng, r)) if r >= 8 else bytes(rng.integers(1, 256, r, dtype=np.uint8)) for r in range(1, 16)]
    base = len(chunks)
    chunks = chunks + shifts
    assert len(set(chunks)) == len(chunks)
    raw = [k for k, (_, _, coded) in enumerate(rows) if not coded]
    cod = [k for k, (_, _, coded) in enumerate(rows) if coded]
    order = []
    for i in range(max(len(raw), len(cod))):                       # raw, coded, coded, raw, raw, coded, ...: both orders
        pair = [raw[i % len(raw)], cod[i % len(cod)]]
        order += pair if i % 2 == 0 else pair[::-1]
    files = []
    for r in range(16):
        files.append(([base + r - 1] if r else []) + order + [order[1], order[0]])
    return chunks, files
