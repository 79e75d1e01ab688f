"""The device deflate coder's model, in Python (include/makisu_mi.h FORMAT, "the device deflate leg"): the blob
mi_deflate_buffer must reproduce byte for byte.  Everything here is a pure function of the input bytes.

PIECES.  The input is cut into pieces of 65 536 bytes (the last one shorter).  A piece knows nothing of its neighbours.  Its
stored form is (D), one dynamic-Huffman block (BFINAL 0, BTYPE 2) followed by an empty stored block (three zero bits, zero
bits to the byte boundary, 00 00 FF FF), or (S), stored blocks of at most 65 535 bytes (a full piece: 65 535 + 1).  (D) is kept
only where it is SMALLER than (S); its size is computed from the counts and the code lengths alone (piece_plan).

THE PARSE (parse): level 1's step rule.  A table of 4 096 positions, all zero at the piece's start.  The wave advances in steps
of 64 consecutive positions [p, p + 64), capped at n - 4 (the last position with four bytes): position pos reads its four bytes
v and the slot (v * 2654435761 mod 2^32) >> 20 as the table was BEFORE the step.  A candidate c counts if c < pos,
pos - c <= 32 768 and the four bytes are equal.  No candidate: all positions of the step go into the table (the greater
position wins a slot).  Otherwise the LOWEST position with a candidate wins, its match is extended to the piece's end (LZ4's
n - 12 and n - 5 restrictions are gone: deflate has none), the pending literals and the match are emitted, p becomes the
match's end and the step's positions BELOW the new p go into the table.  A piece under 4 bytes is literals.

THE SPLIT (split_length): a match of L >= 4 bytes becomes (L - 3) // 258 matches of 258 bytes and a rest r = L - 258 * that
(3 <= r <= 260); r <= 258 is one match, r = 259 or 260 is r - 3 and 3.  All at the match's distance.

THE CODE LENGTHS (code_lengths), a pure function of the counts and the limit (15, 15, 7):
  1. the symbols that occur, sorted by (count, symbol) ascending, are the leaves.  None: no lengths.  One leaf: length 1 (only
     the distance code can have one leaf: literal/length has the end-of-block symbol and a second one, the code-length code has
     a length and a zero or a second length);
  2. Huffman by the two-queue merge, the lighter front twice, the LEAF on a tie; a leaf's length is its depth;
  3. lengths above the limit become the limit;
  4. while the Kraft sum is above 2^limit: of the leaves shorter than the limit the LONGEST -- on a tie the first in the order
     of 1. -- grows by one bit;
  5. while the Kraft sum is below 2^limit by d: of the leaves whose own term 2^(limit - length) is at most d the SHORTEST -- on a
     tie the LAST in the order of 1. -- shrinks by one bit.  (A leaf of the greatest length always qualifies: every term, and so
     d, is a multiple of its term.)  The code is COMPLETE when this ends.

THE HEADER (header_symbols): HLIT and HDIST cut the trailing zero lengths (at least 257 and 1); the two length lists are one
sequence.  At position i with value v and r equal values from i on:  v == 0, r >= 11: symbol 18 for min(r, 138);  v == 0,
r >= 3: symbol 17 for r;  v != 0, the value before i is v too and r >= 3: symbol 16 for min(r, 6);  else v itself.
HCLEN cuts the trailing zeros of the code-length code's lengths in RFC 1951's order (at least 4)."""
import zlib

PIECE = 65536
HASH_BITS = 12
MIN_MATCH = 4
MAX_DIST = 32768
MAX_LEN = 258
N_LITLEN, N_DIST, N_CL = 286, 30, 19
EOB = 256
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

# RFC 1951 3.2.5
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def length_symbol(length):
    """-> (symbol, extra bits, extra value) of a match length 3..258"""
    assert 3 <= length <= MAX_LEN
    k = max(i for i in range(29) if LEN_BASE[i] <= length)
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def dist_symbol(dist):
    assert 1 <= dist <= MAX_DIST
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, DIST_EXTRA[k], dist - DIST_BASE[k]


_LEN_SYM = [None] * 3 + [length_symbol(l) for l in range(3, MAX_LEN + 1)]
_DIST_SYM = {}


def _dist_symbol(dist):
    r = _DIST_SYM.get(dist)
    if r is None:
        r = _DIST_SYM[dist] = dist_symbol(dist)
    return r


def split_length(length):
    """a match of `length` >= 3 bytes -> deflate match lengths, each 3..258"""
    assert length >= 3
    full = (length - 3) // MAX_LEN
    rest = length - MAX_LEN * full
    return [MAX_LEN] * full + ([rest - 3, 3] if rest > MAX_LEN else [rest])


# ---- the parse -----------------------------------------------------------------------------------------------------------------------
def parse(piece, max_dist=MAX_DIST, split=split_length):
    """one piece -> its items in order: an int 0..255 for a literal, (length, distance) for a match"""
    b = bytes(piece)
    n = len(b)
    assert 0 < n <= PIECE
    items = []
    table = [0] * (1 << HASH_BITS)
    p = anchor = 0
    last = n - MIN_MATCH
    while p <= last:
        cnt = min(64, last + 1 - p)
        hs, win = [], None
        for lane in range(cnt):
            pos = p + lane
            v = b[pos:pos + 4]
            h = ((int.from_bytes(v, "little") * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)
            hs.append(h)
            c = table[h]
            if win is None and c < pos and pos - c <= max_dist and b[c:c + 4] == v:
                win = (pos, c)
        if win is None:
            for lane in range(cnt):
                if table[hs[lane]] < p + lane:
                    table[hs[lane]] = p + lane
            p += cnt
            continue
        mpos, mc = win
        mlen = MIN_MATCH
        while mpos + mlen < n and b[mpos + mlen] == b[mc + mlen]:
            mlen += 1
        items.extend(b[anchor:mpos])
        items.extend((l, mpos - mc) for l in split(mlen))
        nxt = mpos + mlen
        for lane in range(cnt):
            if p + lane < nxt and table[hs[lane]] < p + lane:
                table[hs[lane]] = p + lane
        p = anchor = nxt
    items.extend(b[anchor:])
    return items


def expand(items):
    """what a decoder makes of the items"""
    out = bytearray()
    for it in items:
        if isinstance(it, tuple):
            l, d = it
            assert 3 <= l <= MAX_LEN and 1 <= d <= MAX_DIST and d <= len(out)
            for _ in range(l):
                out.append(out[-d])
        else:
            out.append(it)
    return bytes(out)


def count_symbols(items):
    ll, dd = [0] * N_LITLEN, [0] * N_DIST
    for it in items:
        if isinstance(it, tuple):
            ll[_LEN_SYM[it[0]][0]] += 1
            dd[_dist_symbol(it[1])[0]] += 1
        else:
            ll[it] += 1
    ll[EOB] = 1
    return ll, dd


# ---- the codes -----------------------------------------------------------------------------------------------------------------------
def code_lengths(counts, limit, report=None, complete=True):
    """counts -> code lengths (0: the symbol does not occur), by the rule in this file's head.  report (a dict) takes
    "free_depth", the greatest depth before the limit was applied.  complete=False leaves step 5 out (a wrong model)"""
    leaves = sorted((int(c), s) for s, c in enumerate(counts) if c)
    n = len(leaves)
    lens = [0] * len(counts)
    if report is not None:
        report["free_depth"] = 0 if n == 0 else 1
    if n == 0:
        return lens
    if n == 1:
        lens[leaves[0][1]] = 1
        return lens
    weight = [c for c, _ in leaves] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    i, j = 0, n
    for k in range(n, 2 * n - 1):
        for _ in range(2):
            if i < n and (j >= k or weight[i] <= weight[j]):
                take, i = i, i + 1
            else:
                take, j = j, j + 1
            weight[k] += weight[take]
            parent[take] = k
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    if report is not None:
        report["free_depth"] = max(depth[:n])
    ln = [min(d, limit) for d in depth[:n]]
    full = 1 << limit
    kraft = sum(1 << (limit - l) for l in ln)
    while kraft > full:
        best = -1
        for k in range(n):
            if ln[k] < limit and (best < 0 or ln[k] > ln[best]):
                best = k
        ln[best] += 1
        kraft -= 1 << (limit - ln[best])
    while complete and kraft < full:
        d = full - kraft
        best = -1
        for k in range(n):
            if (1 << (limit - ln[k])) <= d and (best < 0 or ln[k] <= ln[best]):
                best = k
        kraft += 1 << (limit - ln[best])
        ln[best] -= 1
    for k in range(n):
        lens[leaves[k][1]] = ln[k]
    return lens


def kraft_sum(lens, limit):
    return sum(1 << (limit - l) for l in lens if l)


def _reverse(v, bits):
    out = 0
    for _ in range(bits):
        out, v = out << 1 | (v & 1), v >> 1
    return out


def canonical_codes(lens):
    """-> the codes as they go into the stream (bit-reversed), by (length, symbol)"""
    codes, nxt = [0] * len(lens), 0
    for l in range(1, max(lens) + 1 if lens else 1):
        for s in range(len(lens)):
            if lens[s] == l:
                codes[s] = _reverse(nxt, l)
                nxt += 1
        nxt <<= 1
    return codes


def header_symbols(ll_lens, d_lens):
    """-> (HLIT, HDIST, [(symbol, extra bits, extra value)]) by the greedy rule in this file's head"""
    hlit = max(257, max(s for s in range(N_LITLEN) if ll_lens[s]) + 1)
    hdist = max([1] + [s + 1 for s in range(N_DIST) if d_lens[s]])
    seq = list(ll_lens[:hlit]) + list(d_lens[:hdist])
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            t = min(r, 138)
            out.append((18, 7, t - 11))
        elif v == 0 and r >= 3:
            t = r
            out.append((17, 3, t - 3))
        elif v != 0 and i > 0 and seq[i - 1] == v and r >= 3:
            t = min(r, 6)
            out.append((16, 2, t - 3))
        else:
            t = 1
            out.append((v, 0, 0))
        i += t
    return hlit, hdist, out


class Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0
        self.acc |= value << self.n
        self.n += bits
        self.total += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def stored_form(piece):
    out = bytearray()
    for at in range(0, len(piece), 65535):
        part = piece[at:at + 65535]
        out += bytes((0, len(part) & 255, len(part) >> 8, ~len(part) & 255, (~len(part) >> 8) & 255)) + part
    return bytes(out)


def stored_size(n):
    return n + 5 * ((n + 65534) // 65535)


def piece_plan(piece, report=None, **wrong):
    """-> dict: items, the three codes' lengths, the header's symbols, the sizes of (D) and (S) in bytes, the form kept.
    report: takes "ll_free_depth", "d_free_depth", "cl_free_depth".  **wrong: max_dist, split, complete (wrong models)"""
    complete = wrong.pop("complete", True)
    items = parse(piece, **wrong)
    ll_cnt, d_cnt = count_symbols(items)
    rep = {}
    ll_lens = code_lengths(ll_cnt, 15, rep, complete)
    ll_free = rep["free_depth"]
    d_lens = code_lengths(d_cnt, 15, rep, complete)
    d_free = rep["free_depth"]
    hlit, hdist, hsyms = header_symbols(ll_lens, d_lens)
    cl_cnt = [0] * N_CL
    for s, _, _ in hsyms:
        cl_cnt[s] += 1
    cl_lens = code_lengths(cl_cnt, 7, rep, complete)
    if report is not None:
        report.update(ll_free_depth=ll_free, d_free_depth=d_free, cl_free_depth=rep["free_depth"])
    hclen = max(4, max(k + 1 for k in range(N_CL) if cl_lens[CL_ORDER[k]]))
    header_bits = 3 + 5 + 5 + 4 + 3 * hclen + sum(cl_lens[s] + eb for s, eb, _ in hsyms)
    body_bits = sum(c * l for c, l in zip(ll_cnt, ll_lens)) + sum(c * l for c, l in zip(d_cnt, d_lens))
    body_bits += sum(c * LEN_EXTRA[s - 257] for s, c in enumerate(ll_cnt) if s > 256) + sum(c * DIST_EXTRA[s] for s, c in enumerate(d_cnt))
    d_size = (header_bits + body_bits + 3 + 7) // 8 + 4               # (the end-of-block code is in body_bits: its count is 1)
    s_size = stored_size(len(piece))
    return dict(items=items, ll_lens=ll_lens, d_lens=d_lens, cl_lens=cl_lens, hlit=hlit, hdist=hdist, hclen=hclen, hsyms=hsyms,
                header_bits=header_bits, d_size=d_size, s_size=s_size, dynamic=d_size < s_size, n_dist_symbols=sum(1 for c in d_cnt if c))


def dynamic_form(plan):
    """the (D) form of a planned piece, whatever its size"""
    w = Bits()
    w.put(0, 1)
    w.put(2, 2)
    w.put(plan["hlit"] - 257, 5)
    w.put(plan["hdist"] - 1, 5)
    w.put(plan["hclen"] - 4, 4)
    cl_lens = plan["cl_lens"]
    for k in range(plan["hclen"]):
        w.put(cl_lens[CL_ORDER[k]], 3)
    cl_codes = canonical_codes(cl_lens)
    for s, eb, ev in plan["hsyms"]:
        w.put(cl_codes[s], cl_lens[s])
        w.put(ev, eb)
    assert w.total == plan["header_bits"]
    ll_lens, d_lens = plan["ll_lens"], plan["d_lens"]
    ll_codes, d_codes = canonical_codes(ll_lens), canonical_codes(d_lens)
    for it in plan["items"]:
        if isinstance(it, tuple):
            s, eb, ev = _LEN_SYM[it[0]]
            w.put(ll_codes[s], ll_lens[s])
            w.put(ev, eb)
            s, eb, ev = _dist_symbol(it[1])
            w.put(d_codes[s], d_lens[s])
            w.put(ev, eb)
        else:
            w.put(ll_codes[it], ll_lens[it])
    w.put(ll_codes[EOB], ll_lens[EOB])
    w.put(0, 3)
    w.align()
    out = bytes(w.out) + b"\x00\x00\xff\xff"
    assert len(out) == plan["d_size"], (len(out), plan["d_size"])
    return out


def piece_form(piece, **wrong):
    plan = piece_plan(piece, **wrong)
    return dynamic_form(plan) if plan["dynamic"] else stored_form(bytes(piece))


def deflate_blob(data, info=None, **wrong):
    """the whole input -> the pieces' stored forms end to end (no gzip header, no final block).  info (a dict): the counts
    mi_deflate_info reports"""
    data = bytes(data)
    out = bytearray()
    n_dyn = n_pieces = 0
    for at in range(0, len(data), PIECE):
        piece = data[at:at + PIECE]
        plan = piece_plan(piece, **wrong)
        n_pieces += 1
        n_dyn += plan["dynamic"]
        out += dynamic_form(plan) if plan["dynamic"] else stored_form(piece)
    if info is not None:
        info.update(n_pieces=n_pieces, n_dynamic=n_dyn, n_stored=n_pieces - n_dyn, in_bytes=len(data), out_bytes=len(out))
    return bytes(out)


def deflate_bound(n):
    """what mi_deflate_bound returns: every piece stored"""
    return n + 10 * ((n + PIECE - 1) // PIECE)


def inflate(blob):
    d = zlib.decompressobj(-15)
    out = d.decompress(bytes(blob) + b"\x03\x00")
    assert d.eof and not d.unused_data
    return out


def gzip_member(tar):
    """what the layer writer's device leg writes for the tar stream"""
    return (bytes((0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 255)) + deflate_blob(tar) + b"\x03\x00" +
            (zlib.crc32(tar) & 0xFFFFFFFF).to_bytes(4, "little") + (len(tar) & 0xFFFFFFFF).to_bytes(4, "little"))


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    import numpy as np
    return np.random.default_rng(seed)


def text(n, seed=1):
    words = [b"layer", b"commit", b"digest", b"tar", b"gzip", b"chunk", b"the", b"of", b"and", b"makisu", b"wave", b"piece", b"\n", b"0123456789"]
    r = _rng(seed)
    out = bytearray()
    while len(out) < n:
        out += words[int(r.integers(len(words)))] + b" "
    return bytes(out[:n])


def random_bytes(n, seed=2):
    return _rng(seed).integers(0, 256, n, dtype="uint8").tobytes()


def symbols(n, k, seed=3):
    return (_rng(seed).integers(0, k, n, dtype="uint8") + 65).astype("uint8").tobytes()


def planted(distance, seed=4):
    """16 random bytes A, zeros, A again `distance` bytes after its first occurrence, 8 more random bytes.  The zeros are one
    match of distance 1, so A's positions are still in the table when the parse reaches the repeat: it is taken at 32 768
    (the slot of A's first four bytes holds position 0, as an empty one does) and refused at 32 769"""
    r = random_bytes(24 + distance - MAX_DIST, seed)
    at = distance - MAX_DIST
    a = bytes(x | 1 for x in r[at:at + 16])                         # (no zero byte: the run of zeros ends where A begins)
    return r[:at] + a + bytes(distance - 16) + a + r[at + 16:]


def no_match():
    """a piece without one match that is still kept as (D): the de Bruijn sequence B(4, 4) and its first three symbols again,
    259 bytes over four symbols in which no four bytes recur"""
    k, n = 4, 4
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
    return bytes(65 + x for x in seq + seq[:3])


def one_distance(n=700):
    """a compressible piece whose matches all have one distance symbol: a period of 1"""
    return b"\x07" * n


LENGTHS = (0, 1, 12, 13, 63, 64, 65, 65535, 65536, 65537, 3 * 65536 + 5)


def skewed_literals(seed, n_sym=40):
    """a piece whose literal counts grow like Fibonacci numbers: the free Huffman depth passes 15"""
    r = _rng(seed)
    counts, a, b = [], 1, 1
    while len(counts) < n_sym and sum(counts) + a <= 60000:
        counts.append(a)
        a, b = b, a + b
    syms = r.permutation(256)[:len(counts)]
    out = []
    for s, c in zip(syms, counts):
        out += [int(s)] * c
    out = bytearray(out)
    # shuffled: runs would become matches and the literal counts would not be these
    idx = r.permutation(len(out))
    return bytes(bytearray(out[i] for i in idx))


# ---- pieces found by seeded searches over the model ------------------------------------------------------------------------------------
def copies_piece(seed, n_fib=18, a_len=4096, a_syms=16):
    """4 096 random bytes over 16 symbols, then 6 764 copies out of them, each followed by the byte 0xEE: the copies' lengths
    take 18 length symbols with Fibonacci counts (2 584 of 4 bytes ... 1 of 51), so that the literal/length code wants to be
    deep.  What the parse makes of it is the model's business: the search below asks it"""
    r = _rng(seed)
    import numpy as np
    fib = [1, 1]
    while len(fib) < n_fib:
        fib.append(fib[-1] + fib[-2])
    lens = [4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67][:n_fib]
    ops = np.concatenate([np.full(c, l) for l, c in zip(lens, fib[::-1])])
    ops = ops[r.permutation(len(ops))]
    a = r.integers(0, a_syms, a_len, dtype=np.uint8).tobytes()
    out = bytearray(a)
    for l in ops:
        s = int(r.integers(0, a_len - int(l)))
        out += a[s:s + int(l)] + b"\xee"
    return bytes(out)


LL_CLAMP_SEED = 6          # find_ll_clamped() from 0 ends here
CL_CLAMP_SEED = 447        # find_cl_clamped() from 0 ends here


def find_ll_clamped(first=0, limit=200):
    """-> (seed, piece): the first copies_piece kept as (D) whose literal/length code is deeper than 15 bits before the limit"""
    for seed in range(first, limit):
        piece, rep = copies_piece(seed), {}
        if piece_plan(piece, rep)["dynamic"] and rep["ll_free_depth"] > 15:
            return seed, piece
    raise AssertionError("no seed below %d" % limit)


_NS, _NC = 100, 78


def records_piece(seed):
    """records (c1, c2, s): c1, c2 the two base-78 digits of the record's number (bytes 100..177 and 178..255: no four bytes
    recur, the piece has NO match), s out of 100 symbols whose counts come in nine groups of 34, 21, 13, 8, 5, 3, 2, 1, 1 symbols
    with one power-of-two frequency a group: the literal code's lengths then come in nine values with Fibonacci counts, which the
    code-length code wants to code deeper than 7 bits.  -> the piece, or None where the counts do not fit 78 * 78 records"""
    import numpy as np
    r = _rng(seed)
    groups = [34, 21, 13, 8, 5, 3, 2, 1, 1]
    lens = r.permutation(np.arange(5, 15))[:9]
    tot = int(r.integers(6000, 20000))
    sc = []
    for g, l in zip(groups, lens):
        sc += [max(1, int(round(tot * 2.0 ** -int(l) * r.uniform(0.8, 1.2))))] * g
    sc = [int(x) for x in r.permutation(sc)]
    n_rec = sum(sc)
    if n_rec > _NC * _NC:
        return None
    s = np.concatenate([np.full(c, k, dtype=np.uint8) for k, c in enumerate(sc) if c])
    s = s[r.permutation(n_rec)]
    i = np.arange(n_rec)
    return np.stack([_NS + i // _NC, _NS + _NC + i % _NC, s], axis=1).astype(np.uint8).tobytes()


def find_cl_clamped(first=0, limit=5000):
    """-> (seed, piece): the first records_piece kept as (D) whose code-length code is deeper than 7 bits before the limit.  A
    piece without a match needs no parse to be judged: its counts are its bytes' (the plan of the piece found is asserted)"""
    import numpy as np
    for seed in range(first, limit):
        piece = records_piece(seed)
        if piece is None:
            continue
        ll = [int(c) for c in np.bincount(np.frombuffer(piece, dtype=np.uint8), minlength=N_LITLEN)]
        ll[EOB] = 1
        _, _, hsyms = header_symbols(code_lengths(ll, 15), [0] * N_DIST)
        cl = [0] * N_CL
        for sym, _, _ in hsyms:
            cl[sym] += 1
        rep = {}
        code_lengths(cl, 7, rep)
        if rep["free_depth"] > 7:
            rep = {}
            plan = piece_plan(piece, rep)
            assert plan["n_dist_symbols"] == 0 and rep["cl_free_depth"] > 7
            if plan["dynamic"]:
                return seed, piece
    raise AssertionError("no seed below %d" % limit)


NEAR_SEEDS = {-1: 13, 0: 51, 1: 184}      # find_near_stored(delta) from 0 ends here


def near_piece(seed):
    r = _rng(1000 + seed)
    return symbols(int(r.integers(24, 200)), int(r.integers(2, 40)), 2000 + seed)


def find_near_stored(delta, first=0, limit=20000):
    """-> (seed, piece): the first near_piece whose (D) form is `delta` bytes larger than its (S) form (-1: kept by one byte;
    +1: not kept by one byte)"""
    for seed in range(first, limit):
        piece = near_piece(seed)
        plan = piece_plan(piece)
        if plan["d_size"] - plan["s_size"] == delta:
            return seed, piece
    raise AssertionError("no seed below %d" % limit)
