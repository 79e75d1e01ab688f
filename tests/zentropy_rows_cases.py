"""Inputs for the entropy stage's tests at sizes and edges zentropy_cases.py does not reach, and their model -- which IS
zentropy_cases.py's, called row by row: nothing here restates the format.

MANY ROWS (many_rows).  One pack of N_ROWS = 65 536 + 4 096 + 5 distinct chunks.  The two constants, from the code:
  UNWRAP_GRID  csrc/mi_zentropy.hip, ZhUnwrap::run: zh_unwrap_kernel is launched with min(n, 65536) workgroups of one wave, and
               the kernel's loop `for (k = blockIdx.x; k < n; k += gridDim.x)` sends workgroup j on to row j + 65 536;
  PLAN_TILE    csrc/mi_plan.h: kPlanTile = kPlanBlock * kPlanPer = 256 * 8 rows per block of zh_classify_kernel and zh_place_kernel.
Rows [0, 4 096) and [65 536, N_ROWS) -- the rows of the unwrap's first workgroups on BOTH their trips -- are mostly form H, over
raw (16 symbols at random, 520..775 bytes) and over LZ4 (letters with one planted copy, 700..1 499 bytes), with short LZ4 and raw
rows between them; the rows between the two zones are raw (24..64 random bytes) and LZ4 (64 bytes of a short period) except at
k % 2 048 in {0, 1, 2 047}, where a form H row stands on each side of every tile boundary.  Inner lengths differ from row to
row, so the places zh_place_kernel gives are no multiples of anything.

EDGE FORMS (edge_forms): forms H no coder of this project produces and the format allows, built by zentropy_cases.huff_form.
THE KEEP RULE (edge_chunks_h): chunks whose form H is exactly on, and one byte under, the bound h < under - (under >> 4)."""
import functools

import numpy as np

import pack_cases as pc
import zentropy_cases as ze
import zpack_cases as zc

UNWRAP_GRID = 65536
PLAN_TILE = 2048
ZONE = 2 * PLAN_TILE                                               # the form H zone at the front, and again behind UNWRAP_GRID
N_ROWS = UNWRAP_GRID + ZONE + 5
LEVEL2_ROWS = 300                                                  # rows [0, 300) once more at level 2, a pack of their own
LETTERS = b"etaoin shrdlu"


# ---- many rows --------------------------------------------------------------------------------------------------------------------------
def _tag(k):
    return int(k).to_bytes(3, "little")                            # every generated chunk holds its row's number: no two are equal


def _h_over_raw(rng, k):
    n = 520 + (k * 61) % 256
    return _tag(k) + (rng.integers(0, 16, n - 3, dtype=np.uint8) + 0x40).tobytes()


def _h_over_lz4(rng, k):
    n = 700 + (k * 37) % 800                                        # (under some 630 bytes these letters do not pay for the header)
    buf = bytearray(_tag(k)) + bytearray(LETTERS[int(v)] for v in rng.integers(0, 13, n - 3))
    return bytes(zc.plant(buf, 10, n // 2, n // 4))


def _short_raw(rng, k):
    return _tag(k) + rng.integers(0, 256, 21 + (k * 7) % 41, dtype=np.uint8).tobytes()      # 24..64 bytes


def _short_lz4(rng, k):
    # 64 bytes, a period of 1..7 from position 0 (a chunk this short is one step of the parse, which finds position 0 alone);
    # the row's number at the end, among the last literals
    return bytes((k + j % (1 + k % 7)) & 255 for j in range(61)) + _tag(k)


def row_chunk(rng, k):
    """row k's chunk: the kind is a function of k alone, the bytes come from the one generator in row order"""
    if k % PLAN_TILE in (0, 1, PLAN_TILE - 1):
        return _h_over_lz4(rng, k) if (k // PLAN_TILE) % 2 else _h_over_raw(rng, k)
    if k < ZONE or k >= UNWRAP_GRID:
        return (_h_over_raw, _h_over_raw, _h_over_lz4, _h_over_raw, _h_over_lz4, _h_over_raw, _short_lz4, _short_raw)[k % 8](rng, k)
    return _short_raw(rng, k) if k % 3 else _short_lz4(rng, k)


class Rows:
    """chunks, the plain pack (entries, blob), the model's level-1 zpack with the stage (zentries, zblob), every row's form
    (zentropy_cases.form_of) and stored form, the census, and the level-1 zpack WITHOUT the stage (ze1, zb1)"""


@functools.lru_cache(maxsize=None)
def many_rows(seed=977):
    """computed once per process: both test modules share it"""
    rng = np.random.default_rng(seed)
    r = Rows()
    r.chunks = [row_chunk(rng, k) for k in range(N_ROWS)]
    r.entries, r.blob = zc.pack_of(r.chunks)
    r.lengths = [len(c) for c in r.chunks]
    r.stored = [ze.compress_chunk_h(c, 1) for c in r.chunks]        # THE MODEL, every row
    r.forms = np.array([ze.form_of(s, n) for s, n in zip(r.stored, r.lengths)])
    r.zentries, r.zblob = _layout(r.entries, r.stored)
    r.census = ze.count_forms(r.zentries, r.zblob)
    r.is_h = r.forms >= 2
    # the form under every form H: what a level-1 coder WITHOUT the stage stores (form H wraps exactly that; the decoder that
    # takes it out again is the model's, written from the format)
    r.under = [ze.huff_decode(s, n)[1] if h else s for s, n, h in zip(r.stored, r.lengths, r.is_h)]
    r.ze1, r.zb1 = _layout(r.entries, r.under)
    r.digests = np.ascontiguousarray(r.entries["digest"])
    r.lens32 = r.entries["length"].astype(np.uint32)
    return r


def _layout(entries, stored):
    """stored forms in entry order -> (ZENTRY_DTYPE entries, blob), as zentropy_cases.model_compress_h lays them out"""
    out = np.zeros(len(entries), dtype=zc.ZENTRY_DTYPE)
    out["digest"], out["chunk_index"], out["length"] = entries["digest"], entries["chunk_index"], entries["length"]
    sizes = np.array([len(s) for s in stored], dtype=np.uint64)
    spans = (sizes + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    out["stored"] = sizes
    out["offset"] = np.cumsum(spans) - spans
    return out, b"".join(s + bytes(-len(s) % 16) for s in stored)


@functools.lru_cache(maxsize=None)
def level2_rows():
    """rows [0, LEVEL2_ROWS) as a pack of their own and the model's level-2 zpack with the stage"""
    chunks = many_rows().chunks[:LEVEL2_ROWS]
    entries, blob = zc.pack_of(chunks)
    want_e, want_b = ze.model_compress_h(entries, blob, 2)
    return chunks, entries, blob, want_e, want_b


DAMAGE = {"reserved byte": ze.RULE_HEADER, "pad bit": ze.RULE_BITS, "unassigned code": ze.RULE_BITS}


def damaged(rows, how):
    """the model's zpack with two form H rows broken -> (zentries, zblob, a, b, the rule a breaks): row a >= UNWRAP_GRID + 100
    has its reserved byte set (rule 8), a pad bit of its stream 0 set (rule 11) or is replaced by unassigned_behind() (rule 11,
    the entries behind it laid out anew); a later row b has a code length of 12 (rule 9).  Both rows are met on the unwrap's
    second trip; a is the smaller, so a is the row every reader must name"""
    stored = list(rows.stored)
    h_rows = [k for k in range(UNWRAP_GRID + 100, N_ROWS) if rows.is_h[k]]
    if how == "reserved byte":
        a = h_rows[0]
        stored[a] = ze._with(stored[a], 3, b"\1")
    elif how == "pad bit":
        a = next(k for k in h_rows if ze._pad_bits(stored[k]) > 0)
        stored[a] = ze._hurt_stream(stored[a], "pad")
    else:
        a = next(k for k in h_rows if rows.forms[k - UNWRAP_GRID] == 3)
        stored[a] = unassigned_behind(rows.stored[a - UNWRAP_GRID], rows.lengths[a])
    b = next(k for k in h_rows if k > a + 40)
    stored[b] = ze._with(stored[b], 8, bytes([stored[b][8] | 0x0C]))
    return _layout(rows.entries, stored) + (a, b, DAMAGE[how])


def form_lens(form):
    lens = []
    for v in form[8:ze.HEAD]:
        lens += [v & 15, v >> 4]
    return lens


def decode_table(lens, before=None):
    """the 2 048-entry table zh_unwrap_row (csrc/mi_huff_wave.h) builds: entry i is (symbol, length) of the code the low bits
    of i begin with, (0, 0) where they begin with nobody's.  `before`: what the entries held before the fill -- None for zeros,
    as the kernel clears them for every row"""
    table = [(0, 0)] * (1 << ze.MAX_BITS) if before is None else list(before)
    codes = ze.canonical_codes(lens)
    for s in range(256):
        if lens[s]:
            for i in range(codes[s], 1 << ze.MAX_BITS, 1 << lens[s]):
                table[i] = (s, lens[s])
    return table


def table_decode(form, table):
    """a form H whose header, code and stream sizes are sound, decoded by table lookups as the device decodes it -> the inner
    bytes, or None where a stream meets an entry of length 0, runs out of bits or ends with a byte or a set bit left over"""
    streams, n = form[2] + 1, int.from_bytes(form[4:8], "little")
    out, at = bytearray(n), ze.HEAD + 2 * streams
    for s in range(streams):
        size = int.from_bytes(form[ze.HEAD + 2 * s:ze.HEAD + 2 * s + 2], "little")
        acc, have = int.from_bytes(form[at:at + size], "little"), 8 * size
        at += size
        for i in range(s, n, streams):
            sym, l = table[acc & ((1 << ze.MAX_BITS) - 1)]
            if l == 0 or l > have:
                return None
            out[i], acc, have = sym, acc >> l, have - l
        if have >= 8 or acc:
            return None
    return bytes(out)


def unassigned_behind(prev_form, length):
    """a form H (kind 2, one stream) of `length` bytes that breaks rule 11 ONLY through an entry of the table that is nobody's:
    the code is one symbol of one bit (the code '1' is unassigned), the stream is zero bits but for a 1 where the sixth symbol is
    due.  It is sized for a decoder that has NOT cleared its table behind prev_form -- a complete code, so every entry is
    somebody's: there the 1 bit finds prev_form's entry 1, a code of l bits, and the stream holds exactly the
    (length - 1) + l bits that such a decoder consumes, so that it would ACCEPT the form (table_decode says so in the host
    test).  A decoder that clears its table refuses the sixth symbol, whatever the stream's size"""
    _, l = decode_table(form_lens(prev_form))[1]
    assert l > 0
    bits = length - 1 + l
    stream = (1 << 5).to_bytes((bits + 7) // 8, "little")
    table = bytearray(128)
    table[3] = 0x10                                                # symbol 7: one bit
    return bytes([0, 2, 0, 0]) + length.to_bytes(4, "little") + bytes(table) + len(stream).to_bytes(2, "little") + stream


# ---- a good form H under the wrong digest ------------------------------------------------------------------------------------------------
def good_specs():
    """the four entries of zentropy_cases.good_zpack: LZ4, H over LZ4, raw, H over raw"""
    raw = bytes(range(40))
    return [zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN), zc._entry(ze.GOOD_H, len(ze.GOOD_PLAIN), ze.GOOD_PLAIN), zc._entry(raw, 40, raw),
            zc._entry(ze.GOOD_H2, len(ze.GOOD_PLAIN2), ze.GOOD_PLAIN2)]


def wrong_digest_zpacks(alg=pc.SHA256):
    """a sound form H -- over LZ4 (GOOD_H) and over raw (GOOD_H2) -- under the digest of OTHER bytes of the same length (the chunk
    with one bit of its first byte turned), alone and behind good entries of all four forms -> [(name, entries, blob, bad index)]"""
    out = []
    for kind, form, plain in (("over lz4", ze.GOOD_H, ze.GOOD_PLAIN), ("over raw", ze.GOOD_H2, ze.GOOD_PLAIN2)):
        other = bytes([plain[0] ^ 1]) + plain[1:]
        bad = zc._entry(form, len(plain), plain=other)
        out.append(("form H %s, alone" % kind, *zc.build_zpack([bad], alg), 0))
        out.append(("form H %s, behind good entries" % kind, *zc.build_zpack(good_specs() + [bad], alg), 4))
    return out


# ---- edge forms for the decoder ---------------------------------------------------------------------------------------------------------
def fibonacci_chunk(terms=22):
    """zentropy_cases.fibonacci_inner with 22 terms: 46 367 bytes, short enough to be a chunk"""
    fib = [1, 1]
    while len(fib) < terms:
        fib.append(fib[-1] + fib[-2])
    a = np.repeat(np.arange(terms, dtype=np.uint8) * 7 + 3, fib)
    return a[np.random.default_rng(5).permutation(len(a))].tobytes()


FLAT_SEED = 1


def flat_chunk():
    """65 536 bytes in which all 256 values occur and whose form H (kind 2) is smaller than the chunk.  Uniformly random bytes
    cannot give that: their counts are so even that the code is 8 bits for (nearly) every symbol and the form is the chunk plus
    its 200 bytes of header -- flat_uniform_size() says by how much -- and stored < length is structural.  So: 256 values with
    unequal counts, 64 of them 512 times, 64 of them 256 times and 128 of them 128 times, shuffled: a code of 7, 8 and 9 bits
    that is COMPLETE (64 / 128 + 64 / 256 + 128 / 512 = 1; checked in the host test), so every one of the table's 2 048
    entries is some symbol's, and a form of 63 700 bytes"""
    a = np.repeat(np.arange(256, dtype=np.uint8), [(512, 256, 128, 128)[s % 4] for s in range(256)])
    assert len(a) == 65536
    return a[np.random.default_rng(FLAT_SEED).permutation(len(a))].tobytes()


def flat_uniform_size(seed=FLAT_SEED):
    c = np.random.default_rng(seed).integers(0, 256, 65536, dtype=np.uint8).tobytes()
    return ze.huff_size(c)


def block_of_length(want):
    """a chunk whose level-1 LZ4 block is exactly `want` bytes and is kept: a run of zeros (position 1 finds position 0 through
    the empty table's zeros, as in bytes(1000)) and distinct bytes behind it, found by a short search over the run's length and
    the tail's, in the model"""
    for tail in range(5, want):
        for run in (1000, 1300, 2000, 300, 700):
            c = bytes(run) + bytes(range(33, 33 + tail))
            if len(zc.compress_chunk(c)) == want < len(c):
                return c
    raise AssertionError("no chunk with a block of %d bytes" % want)


@functools.lru_cache(maxsize=None)
def edge_forms():
    """-> [(name, the form H, the chunk it must restore)]; every form is smaller than its chunk (the structural check asks that)"""
    out = []
    zeros = bytes(1000)
    for s in (64, 33, 32):                                         # a block of 14 bytes: streams 14.. hold no symbol
        out.append(("zeros over %d streams" % s, ze.huff_form(zc.compress_chunk(zeros), 1, s), zeros))
    for s in (32, 64):
        for inner in (s - 1, s, s + 1):
            c = block_of_length(inner)
            out.append(("a block of %d bytes over %d streams" % (inner, s), ze.huff_form(zc.compress_chunk(c), 1, s), c))
    fib = fibonacci_chunk()
    out.append(("a code clamped from 21 bits", ze.huff_form(fib, 2), fib))
    flat = flat_chunk()
    out.append(("a flat code of 256 symbols", ze.huff_form(flat, 2), flat))
    one = b"\x07" * 2000
    for s in (32, 1):
        out.append(("one symbol over %d streams" % s, ze.huff_form(one, 2, s), one))
    for name, form, chunk in out:
        assert 0 < len(form) < len(chunk), name
    return out


def edge_zpacks(alg=pc.SHA256):
    """every edge form alone, and all DISTINCT chunks' forms in one zpack -> [(name, entries, blob, [chunks])]"""
    forms = edge_forms()
    out = [(name, *zc.build_zpack([zc._entry(f, len(c), c)], alg), [c]) for name, f, c in forms]
    seen, specs, chunks = set(), [], []
    for name, f, c in forms:                                       # (zeros and the one-symbol chunk come at several stream counts)
        if c not in seen:
            seen.add(c)
            specs.append(zc._entry(f, len(c), c))
            chunks.append(c)
    out.append(("all of them", *zc.build_zpack(specs, alg), chunks))
    return out


# ---- the keep rule on its line -----------------------------------------------------------------------------------------------------------
EDGE_RAW_SEED, EDGE_RAW_ON, EDGE_RAW_UNDER = 1000, 3331, 3332
EDGE_LZ4_SEEDS = tuple(range(1, 9))                                # the search: these seeds, these lengths, at most 640 candidates
EDGE_LZ4_LENGTHS = range(600, 680)                                 # (13 letters, a quarter copied: h meets the bound near 630 bytes)
EDGE_LZ4_MAX = 640


def keep_margin(chunk, level):
    """h - bound for the level's form of this chunk: form H is kept if and only if this is < 0"""
    under = ze.under_form(chunk, level)
    return ze.huff_size(under) - (len(under) - (len(under) >> 4))


def letters_chunk(n, seed):
    rng = np.random.default_rng(seed)
    buf = bytearray(LETTERS[int(v)] for v in rng.integers(0, 13, n))
    return bytes(zc.plant(buf, 10, n // 2, n // 4))


@functools.lru_cache(maxsize=None)
def edge_lz4_pair():
    """-> ((chunk, margin), (chunk, margin), candidates tried): over the planted letters, the first chunk with h - bound == 0 and
    the first with -1 at level 1, each with an LZ4 block under it; if the search ends without one, the nearest on that side"""
    on = under = None
    best_on, best_under = None, None
    tried = 0
    for seed in EDGE_LZ4_SEEDS:
        for n in EDGE_LZ4_LENGTHS:
            if tried == EDGE_LZ4_MAX or (on and under):
                break
            tried += 1
            c = letters_chunk(n, seed)
            if len(zc.compress_chunk(c)) == n:
                continue
            m = keep_margin(c, 1)
            if m >= 0 and (best_on is None or m < best_on[1]):
                best_on = (c, m)
            if m < 0 and (best_under is None or m > best_under[1]):
                best_under = (c, m)
            on = on or ((c, m) if m == 0 else None)
            under = under or ((c, m) if m == -1 else None)
    return on or best_on, under or best_under, tried


def edge_chunks_h():
    """(name, chunk, h - bound at level 1)"""
    a = np.random.default_rng(EDGE_RAW_SEED).integers(0, 128, 6000, dtype=np.uint8)
    out = [("raw, on the bound", a[:EDGE_RAW_ON].tobytes()), ("raw, one under the bound", a[:EDGE_RAW_UNDER].tobytes())]
    on, under, _ = edge_lz4_pair()
    out += [("lz4, on the bound", on[0]), ("lz4, under the bound", under[0])]
    return [(name, c, keep_margin(c, 1)) for name, c in out]


def model_forms(chunks, level, alg=pc.SHA256):
    entries, blob = zc.pack_of(chunks, alg)
    return (entries, blob) + tuple(ze.model_compress_h(entries, blob, level))
