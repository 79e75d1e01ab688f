"""Zpack level 2's model, in Python: the denser parse mi_pack_compress(MI_ZPACK_LEVEL2) must reproduce byte for byte (DESIGN.md
4.14, csrc/mi_lz4_wave_enc2.h).  The stored form is the same standard LZ4 block as level 1's (zpack_cases.py, which this file
leaves as it is and borrows the block writer, the decoder, the filler and the planting from); only the parse differs.

Level 1's outer rules stay: one chunk at a time, STEPS of 64 consecutive positions [p, p + 64) capped at n - 12, every position
of a step looks at the tables AS THEY WERE BEFORE THE STEP, the greater position wins a slot, a match starts at or before n - 12
and ends at or before n - 5, offsets 1..65535, the block is kept if it is smaller than n - (n >> 4), chunks under 13 bytes are raw.

  (a) two tables of 4 096 positions (zeros): T4 keyed by (u32 at pos * 2654435761) >> 20, T8 by (u64 at pos * 0x9E3779B185EBCA87
      mod 2^64) >> 52.  A candidate c of either table counts if c < pos, pos - c <= 65535 and the 4 bytes at c and pos are equal;
  (b) every position with a candidate measures each candidate's match length, capped at CAP = 4 + 64 and at n - 5 - pos, keeps
      the longer, and on a tie the greater source position;
  (c) f = the lowest position of the step with a candidate, L_f its length.  Among the positions i in [f, f + L_f) with a
      candidate the one with the greatest L_i - (i - f) wins -- a later match must be longer by more than the literals it
      leaves in front of it -- and ties go to the lower position.  A winner at CAP is extended up
      to n - 5; then it is extended BACKWARDS while the byte before the match equals the byte before the source, the match start
      is above `anchor` and the source position above 0;
  (d) every position from p to the match's end (capped at n - 12) goes into both tables, the positions inside the match included.
No candidate in a step: its positions go into both tables, p += 64.

parse2's keyword arguments switch the elements off one by one for tools/zpack_model_ratio.py; with all four off it IS
zpack_cases.parse.  The kernel implements the defaults (all on)."""
import numpy as np

import zpack_cases as zc

TABLE = 4096
STEP = 64
CAP = 4 + 64
MAX_OFFSET = zc.MAX_OFFSET
MIN_CHUNK = zc.MIN_CHUNK
K4 = 2654435761
K8 = 0x9E3779B185EBCA87
_IDX = np.arange(CAP, dtype=np.int64)
_LANES = np.arange(STEP, dtype=np.int64)


def hashes_of(data):
    """-> (a, quad, h4, h8): the bytes, the u32 at every position up to n - 4, T4's key there, T8's key up to n - 8"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    quad = (a[:-3].astype(np.uint32) | a[1:-2].astype(np.uint32) << 8 | a[2:-1].astype(np.uint32) << 16 | a[3:].astype(np.uint32) << 24)
    h4 = ((quad.astype(np.uint64) * np.uint64(K4) & np.uint64(0xFFFFFFFF)) >> np.uint64(20)).astype(np.int64)
    octo = quad[:-4].astype(np.uint64) | quad[4:].astype(np.uint64) << np.uint64(32)
    with np.errstate(over="ignore"):
        h8 = ((octo * np.uint64(K8)) >> np.uint64(52)).astype(np.int64)
    return a, quad, h4, h8


def hash4_of(data, pos):
    return zc.hash_of(data, pos)


def hash8_of(data, pos):
    v = int.from_bytes(bytes(data[pos:pos + 8]), "little")
    return (v * K8 & 0xFFFFFFFFFFFFFFFF) >> 52


def _lengths(a, pos, c, ok, limit):
    """the capped match length of every position's candidate (0 where there is none)"""
    out = np.zeros(len(pos), dtype=np.int64)
    rows = np.flatnonzero(ok)
    if len(rows) == 0:
        return out
    P = pos[rows, None] + _IDX
    C = c[rows, None] + _IDX
    top = len(a) - 1
    eq = (a[np.minimum(P, top)] == a[np.minimum(C, top)]) & (P < limit)
    first = np.argmin(eq, axis=1)
    out[rows] = np.where(eq.all(axis=1), CAP, first)
    return out


def parse2(data, two_tables=True, choose=True, backward=True, dense=True):
    """-> the sequences of one chunk as (literal run, offset, match length) triples; the last is (run, None, None)"""
    n = len(data)
    assert n >= MIN_CHUNK
    a, quad, h4, h8 = hashes_of(data)
    t4, t8 = np.zeros(TABLE, dtype=np.int64), np.zeros(TABLE, dtype=np.int64)
    last, limit = n - 12, n - 5
    p = anchor = 0
    out = []
    while p <= last:
        pos = np.arange(p, min(p + STEP, last + 1))
        k4 = h4[pos]
        c4 = t4[k4]                                               # the tables as they were before the step
        ok4 = (c4 < pos) & (pos - c4 <= MAX_OFFSET) & (quad[np.minimum(c4, pos)] == quad[pos])
        if two_tables:
            k8 = h8[pos]
            c8 = t8[k8]
            ok8 = (c8 < pos) & (pos - c8 <= MAX_OFFSET) & (quad[np.minimum(c8, pos)] == quad[pos])
        else:
            c8, ok8 = c4, np.zeros(len(pos), dtype=bool)
        has = ok4 | ok8
        if not has.any():
            np.maximum.at(t4, k4, pos)
            if two_tables:
                np.maximum.at(t8, k8, pos)
            p = int(pos[-1]) + 1
            continue
        l4, l8 = _lengths(a, pos, c4, ok4, limit), _lengths(a, pos, c8, ok8, limit)
        use8 = ok8 & ((l8 > l4) | ((l8 == l4) & (c8 > c4)))
        c, length = np.where(use8, c8, c4), np.where(use8, l8, l4)
        f = int(np.flatnonzero(has)[0])                           # the lowest position with a candidate
        w = f
        if choose:
            lanes = _LANES[:len(pos)]
            score = np.where(has & (lanes >= f) & (lanes < f + length[f]), length - (lanes - f), -STEP)
            w = int(np.argmax(score))                             # the first of the best scores: ties go to the lower position
        m, mc, mlen = int(pos[w]), int(c[w]), int(length[w])
        if mlen == CAP:                                           # the cap ended it: on, up to n - 5
            theirs, mine = a[mc + mlen:mc + (limit - m)], a[m + mlen:limit]
            differ = np.flatnonzero(theirs != mine)
            mlen += int(differ[0]) if len(differ) else len(mine)
        if backward:
            while m > anchor and mc > 0 and a[m - 1] == a[mc - 1]:
                m, mc, mlen = m - 1, mc - 1, mlen + 1
        out.append((m - anchor, m - mc, mlen))
        nxt = m + mlen
        ins = np.arange(p, min(nxt, last + 1)) if dense else pos[pos < nxt]
        np.maximum.at(t4, h4[ins], ins)
        if two_tables:
            np.maximum.at(t8, h8[ins], ins)
        p = anchor = nxt
    out.append((n - anchor, None, None))
    return out


def compress_chunk2(data, **elements):
    """-> the stored form at level 2: the LZ4 block if it is smaller than n - (n >> 4), else the bytes as they are"""
    data = bytes(data)
    n = len(data)
    if n < MIN_CHUNK:
        return data
    block = zc.encode(data, parse2(data, **elements))
    assert len(block) <= n + n // 255 + 16
    return block if len(block) < n - (n >> 4) else data


def model_compress2(entries, blob):
    """a plain pack -> (entries as a ZENTRY_DTYPE array, the compressed blob as bytes) at level 2: zpack_cases.model_compress
    with the other parse"""
    out = np.zeros(len(entries), dtype=zc.ZENTRY_DTYPE)
    parts, at = [], 0
    for k in range(len(entries)):
        off, n = int(entries["offset"][k]), int(entries["length"][k])
        assert n > 0
        stored = compress_chunk2(blob[off:off + n])
        out["digest"][k], out["chunk_index"][k] = entries["digest"][k], entries["chunk_index"][k]
        out["offset"][k], out["length"][k], out["stored"][k] = at, n, len(stored)
        parts.append(stored + b"\0" * (zc.round16(len(stored)) - len(stored)))
        at += zc.round16(len(stored))
    return out, b"".join(parts)


# ---- planting: zpack_cases' filler and plant, held against THIS parse -------------------------------------------------------------
def planted2(rng, n, copies):
    """zpack_cases.planted for level 2: a filler of n bytes with the copies (src, dst, length) laid in; -> (chunk, the sequence
    list these copies ARE).  Fillers are drawn until parse2 agrees (a slot of either table taken over by a later position, or a
    byte in front of a copy that happens to equal the byte in front of its source, would change the list)"""
    want, anchor = [], 0
    for src, dst, length in copies:
        want.append((dst - anchor, dst - src, length))
        anchor = dst + length
    want.append((n - anchor, None, None))
    return built2(rng, n, lambda buf: [zc.plant(buf, *c) for c in copies], want)


def built2(rng, n, lay, want, also=None):
    """a filler of n bytes that `lay` writes into, drawn until parse2 gives `want` (and `also`, if given, holds)"""
    for _ in range(400):
        buf = zc.filler(rng, n)
        lay(buf)
        if parse2(buf) == want and (also is None or also(bytes(buf))):
            return bytes(buf), want
    raise AssertionError("no filler gives %r" % (want,))


def _differ(buf, at, other):
    """the byte at `at` made to differ from the byte at `other`"""
    if buf[at] == buf[other]:
        buf[at] ^= 0x55


def colliding_tail(head, target):
    """4 bytes w with hash8(head + w) == target (head: 4 bytes), by counting: one in 4 096 fits"""
    base = int.from_bytes(head, "little")
    for w in range(1, 1 << 24):
        if ((base | w << 32) * K8 & 0xFFFFFFFFFFFFFFFF) >> 52 == target:
            return w.to_bytes(4, "little")
    raise AssertionError("no tail")


CAP_LENGTHS = [CAP - 1, CAP, CAP + 63, CAP + 64, CAP + 65]
PERIODS = [1, 2, 3]


def planted_chunks2(seed=191):
    """(name, chunk, the sequence list it was planted to have under parse2, or None) -- every chunk at most 64 KiB"""
    rng = np.random.default_rng(seed)
    out = []
    for n in zc.LENGTHS:                                           # every length, once random and once with repeats in it
        out.append(("random %d" % n, bytes(rng.integers(0, 256, n, dtype=np.uint8).tobytes()), None))
        out.append(("text %d" % n, zc.text_like(n, n + 1), None))
    # level 1's edges, in level 1's layouts: a literal run of exactly L in front of a match, match lengths and offsets at the
    # extension bytes' edges
    for run in zc.LITERAL_RUNS:
        at = 108 + run + 8 + 6
        out.append(("literal run %d" % run, *planted2(rng, at + 60 + 20, [(0, 100, 8), (20, 108 + run, 8), (30, at, 60)])))
    for m in zc.MATCH_LENGTHS:
        more = [(30, 300 + m + 6, 60)] if m < 100 else []
        out.append(("match length %d" % m, *planted2(rng, 300 + m + 6 + 60 + 20, [(0, 300, m)] + more)))
    for off in zc.OFFSETS:
        out.append(("offset %d" % off, *planted2(rng, 128 + 40 + 20, [(128 - off, 128, 40)])))
    out.append(("candidate in lane 63", *planted2(rng, 205 + 60 + 20, [(10, 128 + 63, 8), (30, 205, 60)])))
    # (a) the two tables.  Q = the 4 bytes at 10 occur again at 40 (the same step: no match there), so T4's slot holds 40,
    # whose match is 4 long; T8's slot of the 8 bytes at 10 still holds 10: at 150 the 8-byte table's candidate wins
    def lay(buf):
        buf[40:44] = buf[10:14]
        _differ(buf, 44, 14)
        zc.plant(buf, 10, 150, 20)
    out.append(("the 8-byte table's candidate is longer", *built2(rng, 200, lay, [(150, 140, 20), (30, None, None)],
                lambda c: hash4_of(c, 40) == hash4_of(c, 150) and hash8_of(c, 40) != hash8_of(c, 150))))
    # ... and the reverse.  Both tables hold a position with the 4 bytes of 150: T4 the greater one (30: 7 bytes long), T8 an
    # older one (8) whose 8 bytes are OTHER bytes with the same hash (4 long).  With `tie`, 30's match is 4 long as well: equal
    # lengths, the greater source wins.  (A tail whose first byte happens to agree with 154 is drawn again.)
    for name, keep in (("the 4-byte table's candidate is longer", 7), ("equal lengths: the greater source", 4)):
        def lay(buf, keep=keep):
            buf[150:150 + keep] = buf[30:30 + keep]
            _differ(buf, 150 + keep, 30 + keep)
            buf[8:12] = buf[150:154]
            buf[12:16] = colliding_tail(bytes(buf[8:12]), hash8_of(buf, 150))
            zc.plant(buf, 70, 200, 60)                             # (the saving that keeps the block)
        out.append((name, *built2(rng, 280, lay, [(150, 120, keep), (50 - keep, 130, 60), (20, None, None)],
                    lambda c: hash8_of(c, 8) == hash8_of(c, 150) and c[8:12] == c[150:154] and c[12] != c[154] and c[8:16] != c[150:158])))
    # (c) the choice.  150 has a match of 6 with 10; 152, inside it, one of `second` with 30 (the 4 bytes at 12 are those at 30):
    # 30 - 2 > 6, the later lane wins; 8 - 2 = 6, a tie: the lower lane keeps it, and 156 finds the rest
    for name, second, want in (("a later lane inside the first's match wins", 30, [(152, 122, 30), (18, 130, 60), (20, None, None)]),
                               ("a score tie goes to the lower lane", 8, [(150, 140, 6), (0, 122, 4), (40, 130, 60), (20, None, None)])):
        def lay(buf, second=second):
            buf[12:16] = buf[30:34]
            _differ(buf, 16, 34)
            buf[150:152] = buf[10:12]
            zc.plant(buf, 30, 152, second)
            zc.plant(buf, 70, 200, 60)                             # (the saving that keeps the block)
        out.append((name, *built2(rng, 280, lay, want)))
    # ... and a lane BEYOND the first's match (156 = 150 + 6) does not compete, however long its match: two sequences
    out.append(("a later lane beyond the first's match does not win", *planted2(rng, 220, [(10, 150, 6), (30, 156, 30)])))
    # (b) the cap: a lane's own length one byte under it and at it, and the wave's extension 63, 64 and 65 bytes beyond it
    for m in CAP_LENGTHS:
        out.append(("match length %d, the cap is %d" % (m, CAP), *planted2(rng, 300 + m + 20, [(10, 300, m)])))
    # backward extension.  Source [70, 100) and its copy [110, 140) begin in ONE step, which does not see its own positions; the
    # next step's lane 0 (128) finds 88 and goes back to 110, where the bytes in front differ
    out.append(("backwards to a differing byte", *built2(rng, 180, lambda buf: zc.plant(buf, 70, 110, 30), [(110, 40, 30), (40, None, None)],
                lambda c: c[109] != c[69])))
    # ... to `anchor`, taking every pending literal.  [140, 148) copies 4, [148, 178) copies [20, 50).  The 8 bytes at 20 occur
    # again at 54, so 148 finds 54 (8 long) in both tables; 149's 8 bytes are only at 21: lane 1 wins with 29, goes back one byte
    # and stops at the anchor although the bytes in front (147 and 19) agree: literal run 0
    def lay(buf):
        buf[54:62] = buf[20:28]
        _differ(buf, 62, 28)
        buf[19] = buf[11]
        zc.plant(buf, 4, 140, 8)
        zc.plant(buf, 20, 148, 30)
    out.append(("backwards to the anchor: literal run 0", *built2(rng, 200, lay, [(140, 136, 8), (0, 128, 30), (22, None, None)],
                lambda c: c[147] == c[19] and c[148:156] == c[54:62])))
    # ... and at source position 0: the copy of [0, 30) is found where it begins; the byte in front of it is the chunk's LAST
    # byte, which an index of -1 would read in Python
    def lay(buf):
        zc.plant(buf, 0, 100, 30)
        buf[99] = buf[len(buf) - 1]
    out.append(("backwards stops at source position 0", *built2(rng, 160, lay, [(100, 100, 30), (30, None, None)], lambda c: c[99] == c[-1])))
    # (d) a source INSIDE an earlier match.  [128, 228) copies [10, 110): level 1 remembers the positions of that step only (up to
    # 191).  [300, 320) copies [225, 245): three bytes of the match's tail and the literals behind it -- bytes that occur nowhere
    # else.  Level 2 finds 225; level 1 finds nothing before 303 <-> 228
    def lay(buf):
        zc.plant(buf, 10, 128, 100)
        zc.plant(buf, 225, 300, 20)
    out.append(("a source inside an earlier match", *built2(rng, 340, lay, [(128, 118, 100), (72, 75, 20), (20, None, None)],
                lambda c: zc.parse(c) == [(128, 118, 100), (75, 75, 17), (20, None, None)])))
    # ... and [300, 316) copies [215, 231): 13 bytes of the match's tail, which [97, 110) holds too, and 3 literals.  Without the
    # positions inside the match the older source is found, 13 long; backward extension cannot make up for it
    def lay(buf):
        zc.plant(buf, 10, 128, 100)
        zc.plant(buf, 215, 300, 16)
    out.append(("a longer source inside an earlier match", *built2(rng, 340, lay, [(128, 118, 100), (72, 85, 16), (24, None, None)],
                lambda c: parse2(c, dense=False)[1] == (72, 203, 13) and zc.parse(c)[1] == (72, 203, 13))))
    # the ends: a match that runs to exactly n - 5, one that starts at n - 12, one at n - 11 that is not taken
    out.append(("match to n - 5", *built2(rng, 400, lambda buf: zc.plant(buf, 10, 300, 100), [(300, 290, 95), (5, None, None)],
                lambda c: c[-5:] == c[105:110])))
    out.append(("match at n - 12", *planted2(rng, 300, [(30, 150, 60), (7, 288, 7)])))
    out.append(("match at n - 11", *built2(rng, 300, lambda buf: [zc.plant(buf, 30, 150, 60), zc.plant(buf, 7, 289, 6)],
                                           [(150, 120, 60), (90, None, None)])))
    # periods: [120 - k, 168) has period k and begins in the step before the one that finds it (lane 0, 128): backwards to 120
    for k in PERIODS:
        out.append(("period %d, backwards" % k, *built2(rng, 188, lambda buf, k=k: zc.plant(buf, 120 - k, 120, 48), [(120, k, 48), (20, None, None)])))
    out.append(("zeros", bytes(65536), [(1, 1, 65530), (5, None, None)]))
    out.append(("period 3", b"abc" * 1000, [(3, 3, 2992), (5, None, None)]))
    # the raw rule: 128 literals, a match, 8 literals -- the block is 141 bytes.  n = 150: exactly n - (n >> 4), stored raw;
    # n = 151 (a match one byte longer): one byte below, stored as LZ4
    for n, m in ((150, 14), (151, 15)):
        out.append(("block of 141 for %d" % n, *planted2(rng, n, [(5, 128, m)])))
    names = [x[0] for x in out]
    assert len(set(names)) == len(names), names
    assert all(len(c) <= 65536 for _, c, _ in out)
    for name, chunk, want in out:                                  # a planted parse shows in the stored form: none of them is raw
        assert want is None or name == "block of 141 for 150" or len(compress_chunk2(chunk)) < len(chunk), name
    return out
