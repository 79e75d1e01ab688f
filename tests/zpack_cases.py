"""The compressed pack's model, in Python: from a plain pack (entries, blob) it produces the entries and the blob
mi_pack_compress must produce, byte for byte (include/makisu_mi.h "compressed packs"), and it expands a
compressed pack again with a decoder written from the LZ4 block format alone.  No engine code is involved.

The parse, as the kernel is specified: one chunk at a time, a table of 4 096 positions (zeros), the hash of the 4 bytes at pos
(u32 * 2654435761) >> 20.  The chunk is walked in STEPS of 64 consecutive positions [p, p + 64) capped at n - 12; every position
of a step looks at the table AS IT WAS BEFORE THE STEP; a candidate c counts if c < pos, pos - c <= 65535 and the 4 bytes are
equal.  No candidate: all positions go in, p += 64.  Else the LOWEST position with a candidate wins, the match is extended up
to n - 5, the sequence is emitted, p = the match's end, and the step's positions below the new p go in.  Two positions of a step
in one slot: the greater wins.  The block is kept if it is smaller than n - (n >> 4); chunks under 13 bytes are raw."""
import hashlib

import numpy as np

import pack_cases as pc

ZENTRY_DTYPE = np.dtype({"names": ["digest", "offset", "chunk_index", "length", "stored"],
                         "formats": [("u1", 32), "<u8", "<u8", "<u4", "<u4"], "offsets": [0, 32, 40, 48, 52], "itemsize": 56})
TABLE = 4096
STEP = 64
MAX_OFFSET = 65535
MIN_CHUNK = 13


def round16(n):
    return (n + 15) // 16 * 16


def _lengths(n):
    """the extension bytes behind a nibble of 15 for the value n >= 15"""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def sequence(literals, offset=None, match_len=None):
    """one LZ4 sequence; offset None: the last one, literals only"""
    lit, ml = len(literals), 0 if offset is None else match_len - 4
    out = bytes([(min(lit, 15) << 4) | min(ml, 15)])
    if lit >= 15:
        out += _lengths(lit)
    out += bytes(literals)
    if offset is not None:
        out += bytes([offset & 255, offset >> 8])
        if ml >= 15:
            out += _lengths(ml)
    return out


def parse(data, table=None):
    """-> the sequences of one chunk as (literal run, offset, match length) triples; the last is (run, None, None).  table: None
    for the kernel's own, 4 096 zeros for every chunk; an int64 array of TABLE positions is used IN PLACE instead -- the caller
    sees what the parse left in it, and may begin another chunk's parse on it (what a coder that does not clear its table would
    do: tests/store_rows_cases.py's wrong model)"""
    n = len(data)
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    assert n >= MIN_CHUNK
    quad = (a[:-3].astype(np.uint32) | a[1:-2].astype(np.uint32) << 8 | a[2:-1].astype(np.uint32) << 16 | a[3:].astype(np.uint32) << 24)
    hashes = ((quad.astype(np.uint64) * 2654435761 & 0xFFFFFFFF) >> 20).astype(np.int64)
    if table is None:
        table = np.zeros(TABLE, dtype=np.int64)
    assert table.shape == (TABLE,) and table.dtype == np.int64
    last, limit = n - 12, n - 5
    p = anchor = 0
    out = []
    while p <= last:
        pos = np.arange(p, min(p + STEP, last + 1))
        h = hashes[pos]
        c = table[h]                                               # the table as it was before the step
        ok = (c < pos) & (pos - c <= MAX_OFFSET) & (quad[np.minimum(c, pos)] == quad[pos])
        hit = np.flatnonzero(ok)
        if len(hit) == 0:
            np.maximum.at(table, h, pos)
            p = int(pos[-1]) + 1
            continue
        m, mc = int(pos[hit[0]]), int(c[hit[0]])                   # the lowest position with a candidate
        mlen = 4
        theirs, mine = a[mc + 4:mc + 4 + (limit - m - 4)], a[m + 4:limit]
        differ = np.flatnonzero(theirs != mine)
        mlen += int(differ[0]) if len(differ) else len(mine)
        out.append((m - anchor, m - mc, mlen))
        p = anchor = m + mlen
        keep = pos < p
        np.maximum.at(table, h[keep], pos[keep])
    out.append((n - anchor, None, None))
    return out


def encode(data, sequences):
    at, out = 0, []
    for lit, off, mlen in sequences:
        out.append(sequence(data[at:at + lit], off, mlen))
        at += lit + (mlen or 0)
    assert at == len(data)
    return b"".join(out)


def compress_chunk(data):
    """-> the stored form: the LZ4 block if it is smaller than n - (n >> 4), else the bytes as they are"""
    data = bytes(data)
    n = len(data)
    if n < MIN_CHUNK:
        return data
    block = encode(data, parse(data))
    assert len(block) <= n + n // 255 + 16
    return block if len(block) < n - (n >> 4) else data


def model_compress(entries, blob):
    """a plain pack -> (entries as a ZENTRY_DTYPE array, the compressed blob as bytes)"""
    out = np.zeros(len(entries), dtype=ZENTRY_DTYPE)
    parts, at = [], 0
    for k in range(len(entries)):
        off, n = int(entries["offset"][k]), int(entries["length"][k])
        assert n > 0
        stored = compress_chunk(blob[off:off + n])
        out["digest"][k], out["chunk_index"][k] = entries["digest"][k], entries["chunk_index"][k]
        out["offset"][k], out["length"][k], out["stored"][k] = at, n, len(stored)
        parts.append(stored + b"\0" * (round16(len(stored)) - len(stored)))
        at += round16(len(stored))
    return out, b"".join(parts)


def lz4_block_decode(src, n):
    """one LZ4 block -> n bytes, written from the block format (lz4_Block_format.md), not from the kernel; ValueError for
    anything a block may not hold"""
    src, out, i = bytes(src), bytearray(), 0
    while True:
        if i >= len(src):
            raise ValueError("no token")
        token = src[i]
        i += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if i >= len(src):
                    raise ValueError("literal length cut")
                lit += src[i]
                i += 1
                if src[i - 1] != 255:
                    break
        if i + lit > len(src) or len(out) + lit > n:
            raise ValueError("literals")
        out += src[i:i + lit]
        i += lit
        if i == len(src):
            break
        if i + 2 > len(src):
            raise ValueError("offset cut")
        off = src[i] | src[i + 1] << 8
        i += 2
        if off == 0 or off > len(out):
            raise ValueError("offset")
        ml = token & 15
        if ml == 15:
            while True:
                if i >= len(src):
                    raise ValueError("match length cut")
                ml += src[i]
                i += 1
                if src[i - 1] != 255:
                    break
        ml += 4
        if len(out) + ml > n:
            raise ValueError("match")
        for _ in range(ml):
            out.append(out[-off])
    if len(out) != n:
        raise ValueError("short")
    return bytes(out)


def model_expand(zentries, zblob):
    """a compressed pack -> the plain pack (pc.ENTRY_DTYPE entries, blob), laid out as mi_batch_pack_chunks lays one out"""
    out = np.zeros(len(zentries), dtype=pc.ENTRY_DTYPE)
    parts, at = [], 0
    for k in range(len(zentries)):
        off, n, stored = int(zentries["offset"][k]), int(zentries["length"][k]), int(zentries["stored"][k])
        piece = zblob[off:off + stored]
        plain = bytes(piece) if stored == n else lz4_block_decode(piece, n)
        assert len(plain) == n
        out["digest"][k], out["chunk_index"][k], out["offset"][k], out["length"][k] = zentries["digest"][k], zentries["chunk_index"][k], at, n
        parts.append(plain + b"\0" * (round16(n) - n))
        at += round16(n)
    return out, b"".join(parts)


def pack_of(chunks, alg=pc.SHA256):
    """chunks as one plain pack: one file per chunk"""
    return pc.model_pack([(i, 0, len(c)) for i, c in enumerate(chunks)], chunks, None, alg)


# ---- planting: a filler without a 4-byte repeat, copies laid in by hand ---------------------------------------------------------
def filler(rng, n):
    """n random bytes in which no 4 bytes occur twice, so the parse finds nothing in them: checked, not hoped for (a position
    whose 4 bytes occur earlier is drawn again until none is left)"""
    a = rng.integers(0, 256, n, dtype=np.uint8)
    while n >= 8:
        quad = a[:-3].astype(np.uint32) | a[1:-2].astype(np.uint32) << 8 | a[2:-1].astype(np.uint32) << 16 | a[3:].astype(np.uint32) << 24
        order = np.argsort(quad, kind="stable")
        again = order[1:][quad[order][1:] == quad[order][:-1]]
        if len(again) == 0:
            break
        a[again] = rng.integers(0, 256, len(again), dtype=np.uint8)
    return bytearray(a.tobytes())


def plant(buf, src, dst, length):
    """bytes [src, src + length) of buf copied to [dst, ...), byte by byte (an overlapping copy repeats itself); the byte behind
    the copy is made to DIFFER from the byte the source goes on with, so the match is exactly `length` long"""
    for i in range(length):
        buf[dst + i] = buf[src + i]
    if dst + length < len(buf) and buf[dst + length] == buf[src + length]:
        buf[dst + length] ^= 0x55
    return buf


def planted(rng, n, copies):
    """a filler of n bytes with the copies (src, dst, length) laid in, in ascending dst order and not touching each other;
    -> (chunk, the sequence list these copies ARE: every copy one match, everything else literals).  The model's parse is held
    against that list (a table slot taken over by a later position would hide a source): fillers are drawn until it agrees."""
    want, anchor = [], 0
    for src, dst, length in copies:
        want.append((dst - anchor, dst - src, length))
        anchor = dst + length
    want.append((n - anchor, None, None))
    for _ in range(200):
        buf = filler(rng, n)
        for src, dst, length in copies:
            plant(buf, src, dst, length)
        if parse(buf) == want:
            return bytes(buf), want
    raise AssertionError("no filler gives %r" % (copies,))


def tail_chunk(rng, length_mod, stored_mod):
    """a chunk that is stored as an LZ4 block with length = length_mod and stored = stored_mod (mod 16): k literals, a match
    of m, a few literals -- the block is k + tail + 6 bytes for n = k + m + tail"""
    for m in range(40, 56):
        for k in range(120, 136):
            n = k + m + 8
            if n % 16 != length_mod or (k + 8 + 6) % 16 != stored_mod:
                continue
            data, _ = planted(rng, n, [(0, k, m)])
            stored = compress_chunk(data)
            assert len(stored) == k + 14 < n - (n >> 4)
            return data
    raise AssertionError((length_mod, stored_mod))


def hash_of(data, pos):
    v = int.from_bytes(bytes(data[pos:pos + 4]), "little")
    return (v * 2654435761 & 0xFFFFFFFF) >> 20


# ---- the malformed table, each stream built by hand ------------------------------------------------------------------------------
_A = bytes(range(100, 120))                                        # 20 literals
_B = bytes(range(200, 206))                                        # the last 6
GOOD_PLAIN = _A + _A[:8] + _B                                      # 34 bytes
GOOD_STREAM = sequence(_A, 20, 8) + sequence(_B)                   # 31 bytes


def _entry(stream, length, plain=None, stored=None, pad=0, offset=None):
    return {"stream": bytes(stream), "length": length, "plain": plain, "stored": len(stream) if stored is None else stored, "pad": pad,
            "offset": offset}


def malformed_table():
    """-> [(name, [entry specs], index of the entry that must be named)]"""
    good = _entry(GOOD_STREAM, 34, GOOD_PLAIN)
    t = [
        ("offset 0", [_entry(sequence(_A, 0, 8) + sequence(_B), 34)], 0),
        ("offset one beyond the bytes produced", [_entry(sequence(_A, 21, 8) + sequence(_B), 34)], 0),
        ("literal run one byte past the stored span", [_entry(sequence(_A, 20, 8) + bytes([7 << 4]) + _B, 35)], 0),
        ("length extension cut off by the span's end", [_entry(sequence(_A, 20, 8) + bytes([15 << 4, 255]), 400)], 0),
        ("match one byte past length", [_entry(sequence(_A, 20, 8), 27)], 0),
        ("output one byte short", [_entry(GOOD_STREAM, 35)], 0),
        ("one stored byte left over", [_entry(GOOD_STREAM + b"\0", 34, GOOD_PLAIN)], 0),
        ("non-zero pad", [_entry(GOOD_STREAM, 34, GOOD_PLAIN, pad=0xA5)], 0),
        ("stored > length", [_entry(b"0123456789abcdef0", 16, b"0123456789abcdef")], 0),
        ("stored == 0", [_entry(b"", 5, b"01234")], 0),
        ("overlap", [dict(good), dict(good, offset=16)], 1),
        ("off-grid offset", [dict(good, offset=8)], 0),
    ]
    return t


def build_zpack(specs, alg=pc.SHA256):
    """entry specs -> (ZENTRY_DTYPE entries, blob): laid out on the grid unless a spec says where it lies"""
    entries = np.zeros(len(specs), dtype=ZENTRY_DTYPE)
    blob, at = bytearray(), 0
    for k, s in enumerate(specs):
        off = at if s["offset"] is None else s["offset"]
        span = round16(len(s["stream"]))
        if len(blob) < off + span:
            blob += bytes(off + span - len(blob))
        blob[off:off + len(s["stream"])] = s["stream"]
        for i in range(off + len(s["stream"]), off + span):
            blob[i] = s["pad"]
        plain = s["plain"] if s["plain"] is not None else bytes(s["length"])
        entries["digest"][k] = np.frombuffer(pc.HASHES[alg](plain).digest(), dtype=np.uint8)
        entries["offset"][k], entries["chunk_index"][k], entries["length"][k], entries["stored"][k] = off, k, s["length"], s["stored"]
        at = max(at, off + span)
    return entries, bytes(blob)


def malformed_zpacks(alg=pc.SHA256):
    """every row of the table alone and with a good entry in front -> [(name, entries, blob, bad index)]"""
    out = []
    good = _entry(GOOD_STREAM, 34, GOOD_PLAIN)
    for name, specs, bad in malformed_table():
        out.append((name, *build_zpack(specs, alg), bad))
        shifted = [dict(s, offset=None if s["offset"] is None else s["offset"] + 32) for s in specs]
        out.append((name + ", behind a good entry", *build_zpack([dict(good)] + shifted, alg), bad + 1))
    return out


def sha(data):
    return hashlib.sha256(bytes(data)).digest()


# ---- the planted chunks of tests/test_gpu_chunk_zpack.py: (name, chunk, the sequence list it was planted to have, or None) ------
LENGTHS = [1, 12, 13, 16, 17, 63, 64, 65, 76, 4095, 65536]
LITERAL_RUNS = [14, 15, 16, 269, 270, 271]
MATCH_LENGTHS = [4, 18, 19, 20, 273, 274]
OFFSETS = [1, 2, 3, 15, 16, 17, 63, 64, 65]


def text_like(n, salt):
    """n bytes that compress: a phrase with a counter"""
    out = bytearray()
    i = 0
    while len(out) < n:
        out += b"%d: the layer's chunk %d of %d, salt %d; " % (i, i * 7, n, salt)
        i += 1
    return bytes(out[:n])


def planted_chunks(seed=91):
    rng = np.random.default_rng(seed)
    out = []
    for n in LENGTHS:                                              # every length, once random and once with repeats in it
        out.append(("random %d" % n, bytes(rng.integers(0, 256, n, dtype=np.uint8).tobytes()), None))
        out.append(("text %d" % n, text_like(n, n), None))
    # a literal run of exactly L in front of a match: a first match (source in step 0, found in step 1) ends at 108, so the
    # next step begins OFF the 64-grid; the second match lies L bytes behind it
    for run in LITERAL_RUNS:
        at = 108 + run + 8 + 6                                     # (a copy of 60 bytes behind it: the saving that keeps the block)
        out.append(("literal run %d" % run, *planted(rng, at + 60 + 20, [(0, 100, 8), (20, 108 + run, 8), (30, at, 60)])))
    for m in MATCH_LENGTHS:
        more = [(30, 300 + m + 6, 60)] if m < 100 else []
        out.append(("match length %d" % m, *planted(rng, 300 + m + 6 + 60 + 20, [(0, 300, m)] + more)))
    n = 400                                                        # a match that runs to exactly n - 5: the source goes on, the limit ends it
    for _ in range(200):
        buf = filler(rng, n)
        plant(buf, 10, 300, 100)
        want = [(300, 290, 95), (5, None, None)]
        if parse(buf) == want:
            out.append(("match to n - 5", bytes(buf), want))
            break
    out.append(("match at n - 12", *planted(rng, 300, [(30, 150, 60), (7, 288, 7)])))
    for _ in range(200):                                           # ... and at n - 11: not taken, the bytes stay literals
        buf = filler(rng, 300)
        plant(buf, 30, 150, 60)
        plant(buf, 7, 289, 6)
        want = [(150, 120, 60), (90, None, None)]
        if parse(buf) == want:
            out.append(("match at n - 11", bytes(buf), want))
            break
    # offsets: steps 0 and 1 find nothing and go into the table whole; the copy begins at 128, lane 0 of the third step (an
    # offset below the length repeats itself: a period)
    for off in OFFSETS:
        out.append(("offset %d" % off, *planted(rng, 128 + 40 + 20, [(128 - off, 128, 40)])))
    out.append(("zeros", bytes(65536), [(1, 1, 65530), (5, None, None)]))
    out.append(("period 3", b"abc" * 1000, [(3, 3, 2992), (5, None, None)]))
    out.append(("candidate in lane 63", *planted(rng, 205 + 60 + 20, [(10, 128 + 63, 8), (30, 205, 60)])))
    # two positions of one step with the same 4 bytes (5 and 40: the repeat at 40 has its source in the same step and is not
    # found); a later step that looks for them finds the GREATER one -- 4 bytes long, where the lesser would have given 8
    for _ in range(200):
        buf = filler(rng, 300)
        buf[40:44] = buf[5:9]
        buf[150:158] = buf[5:13]
        plant(buf, 60, 200, 60)
        want = [(150, 110, 4), (0, 145, 4), (42, 140, 60), (40, None, None)]
        if parse(buf) == want:
            out.append(("two positions in one slot", bytes(buf), want))
            break
    # the raw rule: 128 literals, a match, 8 literals -- the block is 141 bytes.  n = 150: exactly n - (n >> 4), stored raw;
    # n = 151 (a match one byte longer): one byte below, stored as LZ4
    for n, m in ((150, 14), (151, 15)):
        out.append(("block of 141 for %d" % n, *planted(rng, n, [(5, 128, m)])))
    names = [x[0] for x in out]
    assert len(set(names)) == len(names) == 2 * len(LENGTHS) + len(LITERAL_RUNS) + len(MATCH_LENGTHS) + len(OFFSETS) + 9, names
    return out
