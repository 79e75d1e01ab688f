"""The zpack entropy stage's model, in Python: the form mi_pack_compress(MI_ZPACK_ENTROPY) must reproduce byte for byte, and a
decoder of it written from the format alone (include/makisu_mi.h "compressed packs", FORMAT).  zpack_cases.py and
zpack2_cases.py stay as they are: this file borrows their parses, their block decoder and their planting.

Form H wraps the form under it -- the chunk's LZ4 block (kind 1) or, where none was kept, its plain bytes (kind 2) -- in a
byte-wise Huffman code, symbol i of the inner bytes in stream i mod S:

    byte 0      0x00 (no LZ4 block begins with it: a match at output position 0 has no source)
    byte 1      kind, 1 or 2            byte 2   S - 1 (0..63)          byte 3   0
    bytes 4..7  the inner length, u32 little-endian (kind 1: 0 < inner < length; kind 2: inner == length)
    128 bytes   256 code lengths of 4 bits, symbol 2k in the low nibble of byte k; 0 = absent, 1..11
    2 S bytes   every stream's size in bytes, u16 little-endian
    streams     canonical codes by (length, symbol) ascending, packed as deflate packs them: LSB first, codes bit-reversed, the
                last byte of a stream padded with zero bits

THE CODE LENGTHS, a pure function of the 256 counts (code_lengths):
  1. the symbols that occur, sorted by (count, symbol) ascending, are the leaves.  One leaf: its length is 1;
  2. Huffman by the two-queue merge: the leaves in that order in one queue, the merged nodes in the order they were made in the
     other; each step takes the lighter front twice, the LEAF on a tie, and appends the sum.  A leaf's length is its depth;
  3. lengths above 11 become 11;
  4. while the Kraft sum (2^(11 - length) over the leaves) is above 2^11: of the leaves shorter than 11 bits the LONGEST -- on a
     tie the first in the order of 1. -- grows by one bit.  (The sum may end below 2^11: an incomplete code is legal.)

The coder always uses S = 32, makes form H only for chunks of at most 65 536 bytes and keeps it only if it is smaller than the
form under it by more than a sixteenth of that form, h < under - (under >> 4): the rule that decides raw against LZ4.

The decoder's refusals continue host_lz4.h's numbering and are checked in this order: 8 header, 9 code, 10 stream sizes, 11 bits,
then 1..6 for the inner block of kind 1 (huff_decode, expand_chunk)."""
import numpy as np

import pack_cases as pc
import zpack_cases as zc
import zpack2_cases as z2

MAX_BITS = 11
STREAMS = 32
MAX_STREAMS = 64
MAX_CHUNK = 65536
HEAD = 8 + 128                                                     # the fixed part in front of the stream sizes
RULE_HEADER, RULE_CODE, RULE_SIZES, RULE_BITS = 8, 9, 10, 11
RULE_PAD = 7


class Refused(ValueError):
    def __init__(self, rule, why):
        ValueError.__init__(self, "rule %d: %s" % (rule, why))
        self.rule = rule


# ---- the code ----------------------------------------------------------------------------------------------------------------------
def code_lengths(counts, limit=MAX_BITS):
    """256 counts -> 256 code lengths (0: the symbol does not occur), by the rule in this file's head"""
    leaves = sorted((int(c), s) for s, c in enumerate(counts) if c)
    n = len(leaves)
    lens = [0] * 256
    if n == 0:
        return lens
    if n == 1:
        lens[leaves[0][1]] = 1
        return lens
    weight = [c for c, _ in leaves] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    i, j = 0, n                                                    # the two queues' fronts: leaves, merged nodes
    for k in range(n, 2 * n - 1):
        for _ in range(2):
            if i < n and (j >= k or weight[i] <= weight[j]):       # the leaf on a tie
                take, i = i, i + 1
            else:
                take, j = j, j + 1
            weight[k] += weight[take]
            parent[take] = k
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    ln = [min(d, limit) for d in depth[:n]]
    kraft = sum(1 << (limit - l) for l in ln)
    while kraft > 1 << limit:
        best = -1
        for k in range(n):
            if ln[k] < limit and (best < 0 or ln[k] > ln[best]):
                best = k
        ln[best] += 1
        kraft -= 1 << (limit - ln[best])
    for k in range(n):
        lens[leaves[k][1]] = ln[k]
    return lens


def _reverse(v, bits):
    out = 0
    for _ in range(bits):
        out, v = out << 1 | (v & 1), v >> 1
    return out


def canonical_codes(lens):
    """-> 256 codes as they go into the stream (bit-reversed: the first bit of the code is bit 0), by (length, symbol)"""
    codes, nxt = [0] * 256, 0
    for l in range(1, max(lens) + 1):
        for s in range(256):
            if lens[s] == l:
                codes[s] = _reverse(nxt, l)
                nxt += 1
        nxt <<= 1
    return codes


def pack_stream(symbols, lens, codes):
    acc = nbits = 0
    for s in symbols:
        acc |= codes[s] << nbits
        nbits += lens[s]
    return acc.to_bytes((nbits + 7) // 8, "little")


def huff_form(inner, kind, streams=STREAMS, limit=MAX_BITS):
    """the inner bytes -> form H, whatever its size"""
    inner = bytes(inner)
    assert inner and kind in (1, 2) and 1 <= streams <= MAX_STREAMS and limit <= 15
    lens = code_lengths(np.bincount(np.frombuffer(inner, dtype=np.uint8), minlength=256), limit)
    codes = canonical_codes(lens)
    parts = [pack_stream(inner[s::streams], lens, codes) for s in range(streams)]
    table = bytes(lens[2 * k] | lens[2 * k + 1] << 4 for k in range(128))
    sizes = b"".join(len(p).to_bytes(2, "little") for p in parts)
    return bytes([0, kind, streams - 1, 0]) + len(inner).to_bytes(4, "little") + table + sizes + b"".join(parts)


def huff_size(inner, streams=STREAMS, limit=MAX_BITS):
    """len(huff_form(...)) without building it (limit None: the unlimited Huffman code, for tools/zentropy_model_ratio.py)"""
    a = np.frombuffer(bytes(inner), dtype=np.uint8)
    lens = np.array(code_lengths(np.bincount(a, minlength=256), 64 if limit is None else limit), dtype=np.int64)
    bits = lens[a]
    return HEAD + 2 * streams + sum((int(bits[s::streams].sum()) + 7) // 8 for s in range(streams))


def under_form(data, level):
    return zc.compress_chunk(data) if level == 1 else z2.compress_chunk2(data)


def compress_chunk_h(data, level, streams=STREAMS):
    """-> the stored form with the entropy stage on: form H over the level's form where that is smaller by more than a sixteenth"""
    data = bytes(data)
    under = under_form(data, level)
    if len(data) > MAX_CHUNK:
        return under
    if huff_size(under, streams) >= len(under) - (len(under) >> 4):
        return under
    return huff_form(under, 1 if len(under) < len(data) else 2, streams)


def model_compress_h(entries, blob, level):
    """a plain pack -> (entries as a ZENTRY_DTYPE array, the compressed blob as bytes) with the stage on"""
    out = np.zeros(len(entries), dtype=zc.ZENTRY_DTYPE)
    parts, at = [], 0
    for k in range(len(entries)):
        off, n = int(entries["offset"][k]), int(entries["length"][k])
        stored = compress_chunk_h(blob[off:off + n], level)
        out["digest"][k], out["chunk_index"][k] = entries["digest"][k], entries["chunk_index"][k]
        out["offset"][k], out["length"][k], out["stored"][k] = at, n, len(stored)
        parts.append(stored + b"\0" * (zc.round16(len(stored)) - len(stored)))
        at += zc.round16(len(stored))
    return out, b"".join(parts)


# ---- the decoder, from the format ---------------------------------------------------------------------------------------------------
def huff_decode(span, length):
    """one form H of a chunk of `length` bytes -> (kind, the inner bytes); Refused(rule) otherwise"""
    span = bytes(span)
    if len(span) < 8 or span[0] != 0 or span[1] not in (1, 2) or span[2] >= MAX_STREAMS or span[3] != 0 or length > MAX_CHUNK:
        raise Refused(RULE_HEADER, "header")
    kind, streams, inner = span[1], span[2] + 1, int.from_bytes(span[4:8], "little")
    if (kind == 1 and not 0 < inner < length) or (kind == 2 and inner != length) or len(span) < HEAD + 2 * streams:
        raise Refused(RULE_HEADER, "inner length or span")
    lens = []
    for b in span[8:HEAD]:
        lens += [b & 15, b >> 4]
    if max(lens) > MAX_BITS or max(lens) == 0 or sum(1 << (MAX_BITS - l) for l in lens if l) > 1 << MAX_BITS:
        raise Refused(RULE_CODE, "code lengths")
    sizes = [int.from_bytes(span[HEAD + 2 * s:HEAD + 2 * s + 2], "little") for s in range(streams)]
    if sum(sizes) != len(span) - HEAD - 2 * streams:
        raise Refused(RULE_SIZES, "stream sizes")
    table = {}
    codes = canonical_codes(lens)
    for s in range(256):
        if lens[s]:
            table[(lens[s], codes[s])] = s
    out = bytearray(inner)
    at = HEAD + 2 * streams
    for s in range(streams):
        acc, have, pos = int.from_bytes(span[at:at + sizes[s]], "little"), 8 * sizes[s], 0
        at += sizes[s]
        for i in range(s, inner, streams):
            for l in range(1, MAX_BITS + 1):
                if pos + l <= have and (l, acc >> pos & ((1 << l) - 1)) in table:
                    out[i] = table[(l, acc >> pos & ((1 << l) - 1))]
                    pos += l
                    break
            else:
                raise Refused(RULE_BITS, "stream %d ends or meets an unassigned code" % s)
        if (pos + 7) // 8 != sizes[s] or acc >> pos:
            raise Refused(RULE_BITS, "stream %d has a byte left over or a pad bit set" % s)
    return kind, bytes(out)


def is_form_h(stored, length):
    return len(stored) < length and stored[0] == 0


def chunk_rule(stored, length):
    """the rule that refuses one stored form (pads apart), 0 for none, and what it decodes to"""
    stored = bytes(stored)
    if len(stored) == length:
        return 0, stored
    inner, kind = stored, 1
    if stored[0] == 0:
        try:
            kind, inner = huff_decode(stored, length)
        except Refused as e:
            return e.rule, None
    if kind == 2:
        return 0, inner
    rule, plain = lz4_rule(inner, length)
    return rule, plain


def lz4_rule(src, n):
    """host_lz4.h's rule for one block, restated: (rule, the plain bytes or None)"""
    src, out, ip = bytes(src), bytearray(), 0
    stored = len(src)

    def extension(v):
        nonlocal ip
        while True:
            if ip >= stored:
                return None
            b = src[ip]
            ip += 1
            v += b
            if b != 255:
                return v

    while True:
        if ip >= stored:
            return 6, None
        token = src[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            lit = extension(lit)
            if lit is None:
                return 4, None
        if lit > stored - ip:
            return 3, None
        if lit > n - len(out):
            return 5, None
        out += src[ip:ip + lit]
        ip += lit
        if ip == stored:
            return (0, bytes(out)) if len(out) == n else (6, None)
        if stored - ip < 2:
            return 4, None
        off = src[ip] | src[ip + 1] << 8
        ip += 2
        if off == 0:
            return 1, None
        if off > len(out):
            return 2, None
        ml = token & 15
        if ml == 15:
            ml = extension(ml)
            if ml is None:
                return 4, None
        ml += 4
        if ml > n - len(out):
            return 5, None
        for _ in range(ml):
            out.append(out[-off])


def expand_chunk(stored, length):
    rule, plain = chunk_rule(stored, length)
    if rule:
        raise Refused(rule, "does not decode")
    return plain


def form_of(stored, length):
    """0 raw, 1 LZ4, 2 H over LZ4, 3 H over raw: the order of mi_zforms' fields"""
    if len(stored) == length:
        return 0
    if stored[0] != 0:
        return 1
    return 2 if stored[1] == 1 else 3


def count_forms(zentries, zblob):
    """-> [[n, stored bytes]] * 4 in form_of's order"""
    out = [[0, 0] for _ in range(4)]
    for k in range(len(zentries)):
        off, n, stored = int(zentries["offset"][k]), int(zentries["length"][k]), int(zentries["stored"][k])
        f = form_of(zblob[off:off + stored], n)
        out[f][0] += 1
        out[f][1] += stored
    return out


def model_expand_h(zentries, zblob):
    """zpack_cases.model_expand for packs that may hold form H"""
    out = np.zeros(len(zentries), dtype=pc.ENTRY_DTYPE)
    parts, at = [], 0
    for k in range(len(zentries)):
        off, n, stored = int(zentries["offset"][k]), int(zentries["length"][k]), int(zentries["stored"][k])
        plain = expand_chunk(zblob[off:off + stored], n)
        out["digest"][k], out["chunk_index"][k], out["offset"][k], out["length"][k] = zentries["digest"][k], zentries["chunk_index"][k], at, n
        parts.append(plain + b"\0" * (zc.round16(n) - n))
        at += zc.round16(n)
    return out, b"".join(parts)


def first_refused(zentries, zblob):
    """(entry, rule) of the smallest entry that does not decode or whose pad is not zero, as mi_zpack_check and the device
    find it; None if every entry decodes (structure and digests are not this function's)"""
    for k in range(len(zentries)):
        off, n, stored = int(zentries["offset"][k]), int(zentries["length"][k]), int(zentries["stored"][k])
        rule, _ = chunk_rule(zblob[off:off + stored], n)
        if rule == 0 and any(zblob[off + stored:off + zc.round16(stored)]):
            rule = RULE_PAD
        if rule:
            return k, rule
    return None


# ---- hand-built inputs ----------------------------------------------------------------------------------------------------------------
def de_bruijn(k, n):
    """the lexicographically least de Bruijn sequence B(k, n) as a list of k ** n symbols: every n-gram once (cyclically)"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def fibonacci_inner():
    """24 symbols with counts 1, 1, 2, 3, 5, ...: the unlimited Huffman code is 23 bits deep; 121 392 bytes, shuffled by a fixed
    rule.  Only ever an INNER form (huff_form is called on it directly): no chunk is that long"""
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    a = np.repeat(np.arange(24, dtype=np.uint8) * 7 + 3, fib)
    return a[np.random.default_rng(5).permutation(len(a))].tobytes()


def four_symbols(n=320):
    """n bytes over 4 symbols, as poor in repeats as 4 symbols allow, that BOTH parses leave raw and the stage takes: kind 2.
    Only 256 four-grams exist, so a chunk long enough to pay for form H's 200 bytes of header repeats some; a repeat of 4 bytes
    costs a parse 3 bytes for 4, and the block is kept only a sixteenth under the chunk: at 320 bytes the few repeats do not
    get it there, and 200 + 32 streams of 3 bytes do.  Searched, not hoped for: symbol orders and rotations of B(4, 4) in a row
    until the models agree"""
    base = de_bruijn(4, 4)
    rng = np.random.default_rng(44)
    for _ in range(400):
        out = []
        while len(out) < n:
            perm, rot = rng.permutation(4), int(rng.integers(0, 256))
            out += [b"ACGT"[perm[v]] for v in base[rot:] + base[:rot]]
        c = bytes(out[:n])
        if all(len(under_form(c, lv)) == n and is_form_h(compress_chunk_h(c, lv), n) for lv in (1, 2)):
            return c
    raise AssertionError("no chunk of 4 symbols stays raw under both parses")


def sixteen_symbols(n=4096):
    """a prefix of B(16, 4): no 4 bytes occur twice, so no parse finds anything, and 4 bits a symbol: kind 2"""
    return bytes(0x40 + v for v in de_bruijn(16, 4)[:n])


H_LENGTHS = [13, 64, 255, 256, 257, 4095, 8192, 65535, 65536, 65537]


def planted_chunks_h(seed=291):
    """(name, chunk) -- what tests/test_gpu_chunk_zentropy.py codes; the four forms all occur at both levels"""
    rng = np.random.default_rng(seed)
    out = []
    for n in H_LENGTHS:
        out.append(("random %d" % n, rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
        out.append(("text %d" % n, zc.text_like(n, n + 2)))
    out.append(("zeros", bytes(65536)))
    out.append(("four symbols", four_symbols()))
    out.append(("sixteen symbols", sixteen_symbols()))
    out.append(("two symbols", bytes(rng.integers(0, 2, 3000, dtype=np.uint8) * 0x41 + 0x20)))
    # planted matches in a filler of letters: the LZ4 block is kept, and its literals are text the stage codes
    for n, copies in ((3000, [(10, 1500, 700)]), (5000, [(0, 2048, 300), (100, 3000, 900)])):
        buf = bytearray(b"etaoin shrdlu"[int(v)] for v in rng.integers(0, 13, n))
        for c in copies:
            zc.plant(buf, *c)
        out.append(("planted matches %d" % n, bytes(buf)))
    skew = rng.choice(np.arange(256, dtype=np.uint8), 8192, p=np.arange(256, 0, -1) ** 4.0 / (np.arange(256, 0, -1) ** 4.0).sum())
    out.append(("skewed bytes", skew.astype(np.uint8).tobytes()))
    return out


# ---- the malformed table: form H built by hand, one row per rule and branch ------------------------------------------------------------
GOOD_PLAIN = zc.text_like(2000, 17)
GOOD_INNER = zc.compress_chunk(GOOD_PLAIN)
GOOD_H = huff_form(GOOD_INNER, 1)
GOOD_PLAIN2 = sixteen_symbols(1024)
GOOD_H2 = huff_form(GOOD_PLAIN2, 2)


def _with(form, at, value):
    out = bytearray(form)
    out[at:at + len(value)] = value
    return bytes(out)


def _sizes_at(form):
    return HEAD, form[2] + 1


def _hurt_stream(form, which):
    """the good form with its stream 0 rebuilt: `which` says how"""
    streams = form[2] + 1
    at = HEAD + 2 * streams
    size0 = int.from_bytes(form[HEAD:HEAD + 2], "little")
    s0, rest = form[at:at + size0], form[at + size0:]
    if which == "cut":                                             # one byte less, the sizes agree: the symbols run out of bits
        s0 = s0[:-1]
    elif which == "left over":                                     # one zero byte more, the sizes agree
        s0 = s0 + b"\0"
    elif which == "pad":                                           # the top bit of the last byte set (the pad, if there is one)
        s0 = s0[:-1] + bytes([s0[-1] | 0x80])
    return form[:HEAD] + len(s0).to_bytes(2, "little") + form[HEAD + 2:at] + s0 + rest


def _pad_bits(form):
    """how many pad bits stream 0 of a good form ends with"""
    lens = []
    for b in form[8:HEAD]:
        lens += [b & 15, b >> 4]
    _, inner = huff_decode(form, 1 << 16)
    return -sum(lens[s] for s in inner[0::form[2] + 1]) % 8


def _unassigned_form():
    """an incomplete code (one symbol, length 1: the code '1' is nobody's) and a stream that holds a 1 bit where a symbol is due"""
    inner = b"\x07" * 2000
    form = bytearray(huff_form(inner, 2, 1))
    assert len(form) == HEAD + 2 + 250
    form[HEAD + 2] = 0x10                                          # the fifth symbol's bit
    return bytes(form), len(inner)


def malformed_table():
    """-> [(name, [entry specs as zpack_cases.build_zpack takes them], index of the entry that must be named, the rule)]"""
    e = zc._entry
    L, L2 = len(GOOD_PLAIN), len(GOOD_PLAIN2)
    good_table = GOOD_H[8:HEAD]
    over = bytes([0x11]) * 2 + bytes(126)                          # four symbols of length 1: Kraft 2 * 2^11
    assert _pad_bits(GOOD_H) > 0, "stream 0 of the good form must end inside a byte for the pad row"
    unassigned, un_len = _unassigned_form()
    wrong_inner = huff_form(zc.sequence(GOOD_PLAIN[:100], 101, 900) + zc.sequence(GOOD_PLAIN[:6]), 1)      # offset beyond: rule 2
    short_inner = huff_form(GOOD_INNER, 1)                          # decodes to 2 000 bytes where 2 001 are stated: rule 6
    t = [
        ("kind 0", [e(_with(GOOD_H, 1, b"\0"), L)], 0, 8),
        ("kind 3", [e(_with(GOOD_H, 1, b"\3"), L)], 0, 8),
        ("reserved byte set", [e(_with(GOOD_H, 3, b"\1"), L)], 0, 8),
        ("65 streams", [e(_with(GOOD_H, 2, b"\x40"), L)], 0, 8),
        ("kind 1, inner length 0", [e(_with(GOOD_H, 4, bytes(4)), L)], 0, 8),
        ("kind 1, inner length == length", [e(_with(GOOD_H, 4, L.to_bytes(4, "little")), L)], 0, 8),
        ("kind 2, inner length one short", [e(_with(GOOD_H2, 4, (L2 - 1).to_bytes(4, "little")), L2)], 0, 8),
        ("span ends inside the header", [e(GOOD_H[:6], L)], 0, 8),
        ("span ends inside the table", [e(GOOD_H[:100], L)], 0, 8),
        ("span ends inside the stream sizes", [e(GOOD_H[:HEAD + 63], L)], 0, 8),
        ("form H on a chunk of 65 537", [e(GOOD_H, 65537)], 0, 8),
        ("a code length of 12", [e(_with(GOOD_H, 8, bytes([good_table[0] | 0x0C])), L)], 0, 9),
        ("no symbol at all", [e(_with(GOOD_H, 8, bytes(128)), L)], 0, 9),
        ("an over-subscribed code", [e(_with(GOOD_H, 8, over), L)], 0, 9),
        ("stream sizes one above the span", [e(_with(GOOD_H, HEAD, (int.from_bytes(GOOD_H[HEAD:HEAD + 2], "little") + 1).to_bytes(2, "little")), L)], 0, 10),
        ("stream sizes one below the span", [e(GOOD_H + b"\0", L)], 0, 10),
        ("a stream ends before its symbols", [e(_hurt_stream(GOOD_H, "cut"), L)], 0, 11),
        ("a stream has a whole byte left over", [e(_hurt_stream(GOOD_H, "left over"), L)], 0, 11),
        ("a pad bit is set", [e(_hurt_stream(GOOD_H, "pad"), L)], 0, 11),
        ("an unassigned code", [e(unassigned, un_len)], 0, 11),
        ("the inner block's offset is beyond", [e(wrong_inner, 1006)], 0, 2),
        ("the inner block's output is short", [e(short_inner, L + 1)], 0, 6),
        ("non-zero pad behind form H", [e(GOOD_H, L, GOOD_PLAIN, pad=0xA5)], 0, 7),
    ]
    for name, specs, _, _ in t:                                    # (stored > length would be the structural check's, not a decoder's)
        assert all(0 < len(s["stream"]) < s["length"] for s in specs), name
    return t


def malformed_zpacks(alg=pc.SHA256):
    """every row alone and behind two good entries (one LZ4, one H) -> [(name, entries, blob, bad index, rule)]"""
    out = []
    front = [zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN), zc._entry(GOOD_H2, len(GOOD_PLAIN2), GOOD_PLAIN2)]
    for name, specs, bad, rule in malformed_table():
        out.append((name, *zc.build_zpack(specs, alg), bad, rule))
        out.append((name + ", behind good entries", *zc.build_zpack([dict(s) for s in front] + specs, alg), bad + 2, rule))
    return out


def good_zpack(alg=pc.SHA256):
    """a hand-built zpack of all four forms that every reader must accept"""
    raw = bytes(range(40))
    specs = [zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN), zc._entry(GOOD_H, len(GOOD_PLAIN), GOOD_PLAIN), zc._entry(raw, 40, raw),
             zc._entry(GOOD_H2, len(GOOD_PLAIN2), GOOD_PLAIN2)]
    return zc.build_zpack(specs, alg)
