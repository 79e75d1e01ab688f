"""The device inflate's model (csrc/mi_inflate_wave.h, csrc/host_inflate.h), written from RFC 1951 and RFC 1952: the gzip
header, the candidates, a bit-exact decoder of one segment with the numbered rules, the rows, the live chain, the verdicts and the
rounds for a window -- what mi_inflate_buffer must reproduce -- and the builders of the tests' inputs.  Pure functions of the bytes.

THE FORMAT RULE.  A candidate is a byte offset p with gz[p - 4:p] == 00 00 FF FF and p <= n - 8; the first byte behind the gzip header
is one too.  The segment from a candidate c is decoded from bit 8 c until (a) an EMPTY stored block with BFINAL 0 has been read (the
segment ends at the byte behind it), (b) a block with BFINAL 1 has been read (END, at the next byte boundary) or (c) a rule is
broken.  The live chain starts at the header's end and follows the ends to END, which must lie at n - 8; other candidates are dead.

WRITING.  Deflate lays a member block by block from tokens -- stored with chosen pad bits, fixed, dynamic with GIVEN code lengths, a
given run of code-length symbols and a given HCLEN --, and planted_streams() holds the members made with it: every branch of the
decoder that no compressor's output takes.  trace() is the decode with a collector: which of those branches a segment reached.
"""
import zlib

import deflate_cases as dc

MARKER = b"\x00\x00\xff\xff"
WINDOW = 64 << 20

# the rules, numbered as csrc/host_inflate.h numbers them
(OK, BLOCK_TYPE, STORED_LEN, TOO_MANY_CODES, LENGTH_CODE, REPEAT, NO_END_OF_BLOCK, CODE, SYMBOL, INPUT_ENDS, DISTANCE, BEYOND_WINDOW) = range(12)
# how the decode from a candidate ended
SEG_ENDS, SEG_FINAL, SEG_BROKEN, SEG_TOO_LONG = range(4)
DONE, NOT_PARALLEL, INVALID = "done", "not_parallel", "invalid"


# ---- the gzip header (RFC 1952) ------------------------------------------------------------------------------------------------------
def gzip_header(gz):
    """the header's length, or None: wrong magic, a method other than 8, a reserved flag bit, a wrong FHCRC, or no end"""
    n = len(gz)
    if n < 10 or gz[0] != 0x1f or gz[1] != 0x8b or gz[2] != 8 or gz[3] & 0xE0:
        return None
    flg, at = gz[3], 10
    if flg & 4:
        if n - at < 2:
            return None
        at += 2 + (gz[at] | gz[at + 1] << 8)
        if at > n:
            return None
    for bit in (8, 16):
        if flg & bit:
            end = gz.find(b"\x00", at)
            if end < 0:
                return None
            at = end + 1
    if flg & 2:
        if n - at < 2 or (zlib.crc32(gz[:at]) & 0xFFFF) != (gz[at] | gz[at + 1] << 8):
            return None
        at += 2
    return at


def candidates(gz, header):
    n, out, at = len(gz), set(), 0
    if header <= n - 8:
        out.add(header)
    while True:
        at = gz.find(MARKER, at)
        if at < 0 or at + 4 > n - 8:
            break
        out.add(at + 4)
        at += 1
    return sorted(out)


# ---- one segment (RFC 1951) ----------------------------------------------------------------------------------------------------------
def _build(lens):
    """the canonical code of the lengths -> (over-subscribed, code space left, symbols coded, longest length, table): the table is
    indexed by the next `longest` bits of the stream and holds (symbol, length) or None (no symbol has this pattern)"""
    cnt = [0] * 16
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    left, longest = 1, 0
    for l in range(1, 16):
        left = (left << 1) - cnt[l]
        if left < 0:
            return True, 0, 0, 0, None
        if cnt[l]:
            longest = l
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    table = [None] * (1 << longest)
    for sym, l in enumerate(lens):
        if l:
            c, r = nxt[l], 0
            nxt[l] += 1
            for _ in range(l):
                r, c = r << 1 | (c & 1), c >> 1
            for j in range(r, 1 << longest, 1 << l):
                table[j] = (sym, l)
    return False, left, sum(cnt), longest, table


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _build([5] * 32))
    return _FIXED


class _Broken(Exception):
    def __init__(self, rule, bit=None):
        self.rule, self.bit = rule, bit


RING, ROOM = 512, 258                                    # kInfRing, and the room a token is placed with


def _decode(gz, start, limit, stop_at_empty, labels, wrong):
    """decode_segment's and trace's one body -> (row, bytes).  labels: None, or the set that takes what the decode reached; wrong: the
    names of the subtly wrong decoders that are switched on (WRONGS)"""
    n, nbits = len(gz), 8 * len(gz)
    out = bytearray()
    pos = 8 * start
    note = labels.add if labels is not None else (lambda label: None)
    fill = seen = 0                                      # the write pass's staging ring, replayed: its fill, its fill at the last barrier
    prev = "header"                                      # what stands in front of the next token: a block's header, a literal, a match

    def take(k):
        nonlocal pos
        v = (int.from_bytes(gz[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << k) - 1)
        pos += k
        return v

    def symbol(built, which=None):
        nonlocal pos
        longest, table = built[3], built[4]
        e = table[(int.from_bytes(gz[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << longest) - 1)] if longest else None
        if e is None or (e[1] == 15 and "walk14" in wrong):
            raise _Broken(SYMBOL)
        pos += e[1]
        if which:
            note((which, e[1]))
        return e[0]

    def ends():
        if pos > nbits:
            raise _Broken(INPUT_ENDS)

    def incomplete(b):                                   # allowed only as a single code of length 1
        return b[1] > 0 and not (b[3] == 1 and b[2] == 1)

    try:
        while True:
            offset = pos & 7
            bfinal, btype = take(1), take(2)
            ends()
            if btype == 3:
                raise _Broken(BLOCK_TYPE)
            if btype == 0:
                pad = take(-pos & 7)
                ln, nln = take(16), take(16)
                ends()
                if ln ^ 0xFFFF != nln:
                    raise _Broken(STORED_LEN)
                byte = pos >> 3
                if ln == 0 and not bfinal and stop_at_empty:
                    return dict(status=SEG_ENDS, end=byte, out_bytes=len(out), rule=0, bit=pos), bytes(out)
                if byte + ln > n:
                    raise _Broken(INPUT_ENDS, nbits)
                if len(out) + ln > limit:
                    raise _Broken(BEYOND_WINDOW)
                note(("stored", offset, pad != 0, fill > 0))
                fill = seen = 0                          # (the flush in front of the stored copy)
                out += gz[byte:byte + ln]
                pos = 8 * (byte + ln)
            else:
                if btype == 1:
                    lit, dist = _fixed()
                else:
                    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
                    ends()
                    if hlit > 286 or hdist > 30:
                        raise _Broken(TOO_MANY_CODES)
                    note(("hclen", hclen))
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[dc.CL_ORDER[i]] = take(3)
                    ends()
                    clb = _build(cl)
                    if clb[0] or clb[1] != 0:
                        raise _Broken(LENGTH_CODE)
                    lens, prev_len = [], 0
                    while len(lens) < hlit + hdist:
                        s = symbol(clb)
                        if s < 16:
                            lens.append(s)
                            prev_len = s
                        else:
                            if s == 16:
                                if not lens:
                                    raise _Broken(REPEAT)
                                val, rep = prev_len, 3 + take(2)
                            elif s == 17:
                                val, rep = 0, 3 + take(3)
                            else:
                                val, rep = 0, 11 + take(7)
                            have = len(lens)
                            if have + rep > hlit + hdist:
                                raise _Broken(REPEAT)
                            across = have < hlit < have + rep
                            note(("repeat", s, across, have + rep == hlit + hdist))
                            if across:
                                note(("across_in_trip", (hlit - have) // 64))    # the trip of the lane loop (64 lengths a trip) the boundary falls in
                                if "clip_repeat" in wrong:
                                    rep = hlit - have
                            lens += [val] * rep
                            prev_len = val
                        ends()
                    if lens[256] == 0:
                        raise _Broken(NO_END_OF_BLOCK)
                    lit, dist = _build(lens[:hlit]), _build(lens[hlit:])
                    if lit[0] or incomplete(lit):
                        raise _Broken(CODE)
                    if dist[0] or (dist[2] != 0 and incomplete(dist)):
                        raise _Broken(CODE)
                    if lit[1] > 0:
                        note(("lit_incomplete",))
                    note(("dist_codes", dist[2]))
                    if (hlit, hdist) == (286, 30):
                        note(("widest",))
                prev = "header"
                while True:
                    if fill > RING - ROOM:               # (the flush in front of a token)
                        note(("flush", fill))
                        fill = seen = 0
                    s = symbol(lit, "lit_bits")
                    if s < 256:
                        ends()
                        if len(out) + 1 > limit:
                            raise _Broken(BEYOND_WINDOW)
                        out.append(s)
                        fill += 1
                        prev = "literal"
                        continue
                    if s == 256:
                        ends()
                        break
                    if s > 285:
                        raise _Broken(SYMBOL)
                    xbits = dc.LEN_EXTRA[s - 257]
                    if s == 285 and "sym285" in wrong:
                        xbits, x = 5, take(5)
                        length = 227 + x
                    else:
                        x = take(xbits)
                        length = dc.LEN_BASE[s - 257] + x
                    d = symbol(dist, "dist_bits")
                    if d > 29:
                        raise _Broken(SYMBOL)
                    dx = take(dc.DIST_EXTRA[d])
                    distance = dc.DIST_BASE[d] + dx + (1 if d == 29 and "last_dist_base" in wrong else 0)
                    ends()
                    if distance > len(out):
                        raise _Broken(DISTANCE)
                    if len(out) + length > limit:
                        raise _Broken(BEYOND_WINDOW)
                    if x == 0:
                        note(("len", s, "zero"))
                    if x == (1 << xbits) - 1:
                        note(("len", s, "max"))
                    if dx == 0:
                        note(("dist", d, "zero"))
                    if dx == (1 << dc.DIST_EXTRA[d]) - 1:
                        note(("dist", d, "max"))
                    src = len(out) - distance
                    if distance == 32768 and src <= 1:
                        note(("far", src))
                    flushed, fresh = len(out) - fill, min(length, distance)
                    note(("match", "flushed" if src + fresh <= flushed else "ring" if src >= flushed else "across", distance < length))
                    if src + fresh > flushed + seen:     # (the barrier in front of a source the lanes have not all seen)
                        note(("barrier", prev))
                        seen = fill
                    fill += length
                    note(("fill", fill))
                    prev = "match"
                    if distance >= length:
                        out += out[src:src + length]
                    elif "no_mod" in wrong:              # bytes that are not there yet read as zero
                        out += bytes(out[src:]) + bytes(length - distance)
                    else:
                        for _ in range(length):
                            out.append(out[-distance])
            if bfinal:
                return dict(status=SEG_FINAL, end=(pos + 7) >> 3, out_bytes=len(out), rule=0, bit=pos), bytes(out)
    except _Broken as e:
        status = SEG_TOO_LONG if e.rule == BEYOND_WINDOW else SEG_BROKEN
        return dict(status=status, end=0, out_bytes=len(out), rule=e.rule, bit=pos if e.bit is None else e.bit), bytes(out)


def decode_segment(gz, start, limit=WINDOW, stop_at_empty=True):
    """the segment from byte `start` -> (row, its bytes).  row: dict(status, end, out_bytes, rule, bit).  Bits behind the member's last
    byte read as zero and break INPUT_ENDS at the next check, as the kernel's reader does.  stop_at_empty=False is the WRONG decoder
    that reads on behind an empty stored block"""
    return _decode(gz, start, limit, stop_at_empty, None, ())


WRONGS = ("sym285", "last_dist_base", "no_mod", "clip_repeat", "walk14")


def trace(gz, start, limit=WINDOW, wrong=()):
    """the same decode as decode_segment (one body) -> (row, its bytes, the set of labels it reached).

    THE LABELS.  ("lit_bits", l) / ("dist_bits", l): a literal/length or distance code of l bits was read in a block;
    ("len", symbol, "zero" / "max") and ("dist", symbol, "zero" / "max"): a match was placed whose length or distance symbol had none or
    all of its extra bits set (a symbol without extra bits gives both);  ("far", k): a match of distance 32 768 whose source is the
    segment's byte k, k = 0 or 1;  ("hclen", h);  ("repeat", 16 / 17 / 18, the run crosses the HLIT | HDIST boundary, it ends exactly on
    HLIT + HDIST) and, where it crosses, ("across_in_trip", t): the boundary falls in trip t of a loop that fills 64 lengths a trip;
    ("lit_incomplete",): the literal/length code is the one code of length 1;  ("dist_codes", how many distance symbols are coded);
    ("widest",): HLIT 286 with HDIST 30;  ("stored", the bit offset of the block's first bit in its byte, the pad bits are not all zero,
    the ring holds bytes): a stored block other than the empty one that ends the segment;  ("match", where its source lies -- "flushed",
    "ring" or "across" the line between them --, it overlaps itself: distance < length);  ("barrier", "literal" / "match" / "header"): the
    source reaches into what the wave put into the ring since its last barrier, and what stood in front of the match;  ("fill", f): the
    ring's fill behind a match;  ("flush", f): the flush in front of a token, taken at fill f.

    THE RING is the write pass's staging (csrc/mi_inflate_wave.h), replayed by the three rules stated there: it is flushed in front of
    a token once fill > kInfRing - 258 = 254, in front of a stored block's copy, and at the segment's end; `ring_seen` is the fill at
    the last barrier, and a match whose source min(length, distance) bytes end above flushed + ring_seen takes a barrier first.

    wrong: names out of WRONGS -- "sym285": symbol 285 read as 227 + five extra bits;  "last_dist_base": distance symbol 29's base one
    too far;  "no_mod": an overlapping match copied as a plain one (bytes not yet there read as zero);  "clip_repeat": a repeat that
    crosses the HLIT | HDIST boundary ends at HLIT;  "walk14": no code of 15 bits is found"""
    assert set(wrong) <= set(WRONGS), wrong
    labels = set()
    row, out = _decode(gz, start, limit, True, labels, wrong)
    return row, out, labels


def rows(gz, window=WINDOW):
    """every candidate's row: [(candidate, row)], ascending -- what inflate_size_kernel leaves"""
    header = gzip_header(gz)
    return [(c, decode_segment(gz, c, window)[0]) for c in candidates(gz, header)]


def rounds(sizes, window=WINDOW):
    """the live segments' output sizes -> the number of rounds whose output fits the window"""
    n, fill = 0, 0
    for k, b in enumerate(sizes):
        if k == 0 or fill + b > window:
            n, fill = n + 1, 0
        fill += b
    return n


def plan(gz, window=WINDOW, stop_at_empty=True, wrong=()):
    """what mi_inflate_buffer says of the member: dict(result = DONE / NOT_PARALLEL / INVALID, out, rule, at_in, at_out, n_candidates,
    n_segments, n_rounds, sizes).  Only the live chain's candidates are decoded.  wrong: trace()'s wrong decoders"""
    gz = bytes(gz)
    n = len(gz)
    res = dict(result=INVALID, out=b"", rule=0, at_in=0, at_out=0, n_candidates=0, n_segments=0, n_rounds=0, sizes=[])
    header = gzip_header(gz)
    if header is None or n < header + 9:
        return res
    cand = candidates(gz, header)
    res["n_candidates"] = len(cand)
    at, out = header, bytearray()
    while True:
        assert at in cand, (at, "a segment's end is a candidate by construction")
        row, data = _decode(gz, at, window, stop_at_empty, None, wrong)
        res.update(at_in=at, at_out=len(out), rule=row["rule"], n_segments=res["n_segments"] + 1)
        if row["status"] == SEG_BROKEN:
            res["result"] = NOT_PARALLEL if row["rule"] == DISTANCE else INVALID
            return res
        if row["status"] == SEG_TOO_LONG:
            res["result"] = NOT_PARALLEL
            return res
        out += data
        res["sizes"].append(len(data))
        if row["status"] == SEG_FINAL:
            if row["end"] < n - 8:
                res["result"] = NOT_PARALLEL                 # more members, or bytes behind the trailer
            elif row["end"] > n - 8:
                res.update(result=INVALID, rule=INPUT_ENDS)  # no room for the trailer
            elif zlib.crc32(out) != int.from_bytes(gz[-8:-4], "little") or len(out) & 0xFFFFFFFF != int.from_bytes(gz[-4:], "little"):
                res.update(result=INVALID, rule=0)
            else:
                res.update(result=DONE, out=bytes(out), n_rounds=rounds(res["sizes"], window))
            return res
        if row["end"] > n - 8:                               # the segment ends where only the trailer may lie
            res.update(result=INVALID, rule=INPUT_ENDS)
            return res
        at = row["end"]


def zlib_inflates(gz):
    """zlib's word on the member: its bytes, or None where it refuses (an error, an unfinished stream, bytes left over)"""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(bytes(gz))
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data else None


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
HEADER = bytes((0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255))


def member(stream, data, header=HEADER):
    """a gzip member around a complete deflate stream of `data`"""
    return header + stream + (zlib.crc32(data) & 0xFFFFFFFF).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little")


def host_leg(data, level=6, block=1 << 20, strategy=zlib.Z_DEFAULT_STRATEGY):
    """the layer writer's host leg: deflateReset + deflate(Z_SYNC_FLUSH) on every block, then the final empty block 03 00"""
    stream = b""
    for at in range(0, len(data), block):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        stream += c.compress(data[at:at + block]) + c.flush(zlib.Z_SYNC_FLUSH)
    return member(stream + b"\x03\x00", data)


def no_reset(data, block=1 << 16, level=6):
    """ONE zlib stream with Z_SYNC_FLUSH every `block` bytes: the markers are there, the matches reach across them"""
    c, stream = zlib.compressobj(level, zlib.DEFLATED, -15), b""
    for at in range(0, len(data), block):
        stream += c.compress(data[at:at + block]) + c.flush(zlib.Z_SYNC_FLUSH)
    return member(stream + c.flush(zlib.Z_FINISH), data)


def one_stream(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return member(c.compress(data) + c.flush(zlib.Z_FINISH), data)


def stored_leg(data, header=HEADER):
    """the device leg's form of incompressible pieces, without the coder: every 65 536-byte piece as stored blocks (65 535 and 1)"""
    stream = b"".join(dc.stored_form(data[at:at + dc.PIECE]) for at in range(0, len(data), dc.PIECE))
    return member(stream + b"\x03\x00", data, header)


def plant(data, at):
    return data[:at] + MARKER + data[at + 4:]


def planted_cases():
    """random bytes, pieces stored, with 00 00 FF FF where a search finds it and the chain does not: name -> (member, data)"""
    base = dc.random_bytes(2 * dc.PIECE + 300, 71).replace(b"\x00\x00", b"\x01\x01")
    cases = {}
    d = plant(base, 1000)                                    # in the middle of a stored block
    cases["middle"] = (stored_leg(d), d)
    d = plant(base, 65535 - 4)                               # the last four data bytes of a stored block: a true block boundary
    cases["block_end"] = (stored_leg(d), d)
    d = plant(base, 65534)                                   # across the 65 535 | 1 split and into the next piece
    cases["straddle"] = (stored_leg(d), d)
    fname = bytes((0x1f, 0x8b, 8, 8, 0, 0, 0, 0, 0, 0)) + b"\xff\xffname\x00"   # XFL 0, OS 0, then FNAME: the marker ends inside it
    cases["fname"] = (stored_leg(base, fname), base)
    return cases


def repeat_at(distance, seed=72):
    """16 bytes, random bytes that never repeat them, the 16 bytes again `distance` behind their first occurrence"""
    a = bytes(range(200, 216))
    r = bytes(x % 199 for x in dc.random_bytes(distance - 16, seed))
    return a + r + a + b"tail"


def two_piece():
    """a two-piece blob of the device leg's form, about 2 KB: the base of the corruption cases (the pieces are cut by hand: a piece of
    the leg's is 65 536 bytes, the format does not care)"""
    a, b = dc.text(3000, 73), dc.text(2500, 74) + dc.random_bytes(40, 75)
    return member(dc.piece_form(a) + dc.piece_form(b) + b"\x03\x00", a + b), a + b


def source_at_start():
    """two blocks of the host leg's form, each a run of bytes and the same run again: the first match of either segment has its
    source at the segment's first byte (distance == the bytes produced so far)"""
    a, b = bytes(x % 251 for x in dc.random_bytes(300, 76)), bytes(x % 241 for x in dc.random_bytes(258, 77))
    data = a + a + b + b
    return host_leg(data, 9, 600), data


def with_fname(gz, k):
    """the member with k more header bytes: an FNAME of k - 1 letters (the member had none)"""
    assert k >= 1 and not gz[3] & 8
    return gz[:3] + bytes((gz[3] | 8,)) + gz[4:10] + b"n" * (k - 1) + b"\x00" + gz[10:]


def ends_on_last_bit():
    """a member WITHOUT its trailer whose final block's end-of-block code ends on the last bit of the last byte, a multiple of 256
    bytes long (under the guard allocator its last byte is then the allocation's last)"""
    for k in range(200):
        data = dc.text(900 + k, 78)
        gz = one_stream(data)
        if decode_segment(gz, 10)[0]["bit"] % 8 == 0:
            cut = gz[:-8]
            return with_fname(cut, 256 - len(cut) % 256)
    raise AssertionError("no such stream among 200")


def cut_in_last_segment():
    """a three-piece member cut inside its last segment, a multiple of 256 bytes long"""
    gz, _ = two_piece()
    cut = gz[:len(gz) - 100]
    return with_fname(cut, 256 - len(cut) % 256)


def code_bits(lens, symbols):
    """the symbols under the canonical code of `lens`, as the stream holds them: (bytes, bit count)"""
    table = _build(lens)[4]
    acc = n = 0
    for s in symbols:
        l = lens[s]
        j = next(j for j in range(1 << l) if table[j] == (s, l))     # the code, its first bit lowest
        acc |= j << n
        n += l
    return acc.to_bytes((n + 7) // 8 + 4, "little"), n


class _Bits:
    """a deflate stream written by hand: values with their first bit lowest, Huffman codes with their first bit highest"""
    def __init__(self):
        self.acc = self.n = 0

    def put(self, v, k):
        self.acc |= v << self.n
        self.n += k
        return self

    def code(self, c, k):
        for i in range(k - 1, -1, -1):
            self.put(c >> i & 1, 1)
        return self

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _dynamic(hlit, hdist, cl, bfinal=1, hclen=None, w=None):
    """BFINAL, BTYPE 2 and the header up to the code-length code's lengths (cl: symbol -> length; hclen: as many of CL_ORDER as needed, or
    the number given), behind what w holds"""
    need = max([4] + [dc.CL_ORDER.index(s) + 1 for s in cl if cl[s]])
    hclen = need if hclen is None else hclen
    assert need <= hclen <= 19
    w = (_Bits() if w is None else w).put(bfinal, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
    for s in dc.CL_ORDER[:hclen]:
        w.put(cl.get(s, 0), 3)
    return w


def rule_streams():
    """every rule pinned by a stream of a few bytes: rule -> the member around it (no stream gets as far as its trailer).  BEYOND_WINDOW is not here: it needs no special stream, only a window"""
    out = {}
    out[BLOCK_TYPE] = _Bits().put(1, 1).put(3, 2)
    out[STORED_LEN] = _Bits().put(1, 1).put(0, 2).put(0, 5).put(1, 16).put(0, 16)
    out[TOO_MANY_CODES] = _Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4)
    out[LENGTH_CODE] = _dynamic(257, 1, {})                                          # no code-length code at all: incomplete
    out[REPEAT] = _dynamic(257, 1, {16: 1, 17: 1}).code(0, 1).put(0, 2)              # "repeat the previous length" comes first
    # 18 twice: 138 + 120 zeros are all 258 lengths, so there is no end-of-block code
    out[NO_END_OF_BLOCK] = _dynamic(257, 1, {0: 1, 18: 1}).code(1, 1).put(127, 7).code(1, 1).put(109, 7)
    # four literal/length codes of length 1 (0, 1, 2 and 256): over-subscribed
    out[CODE] = (_dynamic(257, 1, {1: 1, 18: 1}).code(0, 1).code(0, 1).code(0, 1).code(1, 1).put(127, 7).code(1, 1).put(104, 7).code(0, 1).code(0, 1))
    out[SYMBOL] = _Bits().put(1, 1).put(1, 2).code(0xC6, 8)                          # the fixed code's 286
    out[INPUT_ENDS] = _Bits().put(0, 1).put(1, 2).code(0x30 + 97, 8).put(31, 5)                # a literal, and the block never ends
    # a literal, then length 3 at distance 2: one byte before the segment's first
    out[DISTANCE] = _Bits().put(1, 1).put(1, 2).code(0x30 + 97, 8).code(1, 7).code(1, 5).code(0, 7)
    res = {}
    for rule, w in out.items():
        stream = w.bytes()
        res[rule] = HEADER + stream + (bytes(8) if rule != INPUT_ENDS else b"\xff" * 8)     # (ones: literals up to the last bit)
    return res


# ---- streams from tokens: what no compressor writes ------------------------------------------------------------------------------------
EOB = 256
EMPTY = b"\x00" + MARKER                                 # the empty stored block with BFINAL 0, from a byte boundary


class _Stream(_Bits):
    """_Bits that spills its whole bytes, so that a member of tens of KB is written in linear time"""
    def __init__(self):
        self.done, self.acc, self.k = bytearray(), 0, 0

    @property
    def n(self):
        return 8 * len(self.done) + self.k

    def put(self, v, k):
        assert 0 <= v < 1 << k or k == 0
        self.acc |= v << self.k
        self.k += k
        while self.k >= 8:
            self.done.append(self.acc & 255)
            self.acc >>= 8
            self.k -= 8
        return self

    def bytes(self):
        return bytes(self.done) + (bytes((self.acc,)) if self.k else b"")


def length_run(seq):
    """code lengths (both lists, one sequence) -> a valid run of code-length symbols [(symbol, extra value)], greedily: 18 for 11 to 138
    zeros, 17 for 3 to 10, 16 for 3 to 6 copies of the length in front.  A test that wants a repeat at a given place writes that
    symbol itself between the runs of the parts around it (a run of a part never begins with 16)"""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            t = min(r, 138)
            out.append((18, t - 11))
        elif v == 0 and r >= 3:
            t = r
            out.append((17, t - 3))
        elif v != 0 and i > 0 and seq[i - 1] == v and r >= 3:
            t = min(r, 6)
            out.append((16, t - 3))
        else:
            t = 1
            out.append((v, 0))
        i += t
    return out


def run_lengths(run):
    """what a decoder makes of a run of code-length symbols"""
    out = []
    for s, x in run:
        out += [s] if s < 16 else [out[-1]] * (3 + x) if s == 16 else [0] * (3 + x) if s == 17 else [0] * (11 + x)
    return out


_RUN_EXTRA = {16: 2, 17: 3, 18: 7}


class Deflate:
    """a gzip member written block by block from tokens.  A token is a literal 0..255, EOB, or a match (length symbol, its extra bits'
    value, distance symbol, its extra bits' value).  `data` is what the tokens mean, worked out here; a match never reaches before its
    segment's first byte"""
    def __init__(self):
        self.w, self.data, self.seg = _Stream(), bytearray(), 0

    def _tokens(self, tokens, lit_lens, dist_lens):
        lit, dist = dc.canonical_codes(lit_lens), dc.canonical_codes(dist_lens)
        for t in tokens:
            if isinstance(t, tuple):
                ls, lx, ds, dx = t
                assert lit_lens[ls] and dist_lens[ds], t
                self.w.put(lit[ls], lit_lens[ls]).put(lx, dc.LEN_EXTRA[ls - 257]).put(dist[ds], dist_lens[ds]).put(dx, dc.DIST_EXTRA[ds])
                length, distance = dc.LEN_BASE[ls - 257] + lx, dc.DIST_BASE[ds] + dx
                assert length <= 258 and distance <= len(self.data) - self.seg, t
                for _ in range(length):
                    self.data.append(self.data[-distance])
            else:
                assert lit_lens[t], t
                self.w.put(lit[t], lit_lens[t])
                if t != EOB:
                    self.data.append(t)
        assert tokens[-1] == EOB and EOB not in tokens[:-1]
        return self

    def stored(self, payload, bfinal=0, pad=0):
        """pad: the bits between the header and LEN, the first one lowest (as many of them as there are)"""
        self.w.put(bfinal, 1).put(0, 2)
        k = -self.w.n & 7
        self.w.put(pad & ((1 << k) - 1), k).put(len(payload), 16).put(len(payload) ^ 0xFFFF, 16)
        self.w.done += payload
        self.data += payload
        if not payload and not bfinal:
            self.seg = len(self.data)                    # the segment ends here
        return self

    def fixed(self, tokens, bfinal=0):
        self.w.put(bfinal, 1).put(1, 2)
        return self._tokens(tokens, [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32)

    def dynamic(self, tokens, lit_lens, dist_lens, bfinal=0, run=None, hclen=None, cl_lens=None):
        """the code lengths as GIVEN (HLIT and HDIST are the lists' lengths: trailing zeros are written), the run of code-length symbols
        as given (or length_run's), the code-length code as given (or a complete one over the run's symbols)"""
        seq = list(lit_lens) + list(dist_lens)
        run = length_run(seq) if run is None else run
        assert run_lengths(run) == seq, "the run does not spell the lengths"
        if cl_lens is None:
            cnt = [0] * 19
            for s, _ in run:
                cnt[s] += 1
            if sum(1 for c in cnt if c) < 2:             # one code of length 1 would be incomplete: a second symbol takes the other half
                cnt[0 if not cnt[0] else 18] += 1
            cl_lens = dc.code_lengths(cnt, 7)
        _dynamic(len(lit_lens), len(dist_lens), dict(enumerate(cl_lens)), bfinal, hclen, self.w)
        cl = dc.canonical_codes(cl_lens)
        for s, x in run:
            assert cl_lens[s], s
            self.w.put(cl[s], cl_lens[s]).put(x, _RUN_EXTRA.get(s, 0))
        return self._tokens(tokens, list(lit_lens), list(dist_lens))

    def member(self):
        data = bytes(self.data)
        return member(self.w.bytes(), data), data


def noise(n, seed):
    """n bytes 1..250: no zero, no 0xFF -- no marker by accident"""
    return bytes(1 + x % 250 for x in dc.random_bytes(n, seed))


def _lens(n, **given):
    """n code lengths, zero but for the ones given as s<symbol>=length"""
    out = [0] * n
    for k, v in given.items():
        out[int(k[1:])] = v
    return out


def _both(bits):
    return sorted({0, (1 << bits) - 1})


LIVE_TILE_ENDS = [2048 * k + k - 5 for k in range(1, 10)]           # p mod 2048 = 2044 .. 2047, 0 .. 4; p mod 8 = every value
DEAD_TILE_ENDS = [2048 * k + r for k, rs in ((10, (-4, 0, 4)), (11, (-3, 1)), (12, (-2, 2)), (13, (-1, 3))) for r in rs]
N_EMPTY = 3000
_PLANTED = None


def required_labels():
    """what the planted members must reach between them: every label the members written by zlib and by this library's deflate leg
    never reach, and the neighbours that make each list whole"""
    req = {("lit_bits", l) for l in range(11, 16)} | {("dist_bits", l) for l in range(9, 16)}
    req |= {("len", s, e) for s in range(257, 286) for e in ("zero", "max")} | {("dist", s, e) for s in range(30) for e in ("zero", "max")}
    req |= {("far", 0), ("far", 1), ("hclen", 4), ("hclen", 19), ("lit_incomplete",), ("widest",)}
    req |= {("repeat", s, True, False) for s in (16, 17, 18)} | {("repeat", 17, False, True), ("repeat", 18, False, True)}
    req |= {("across_in_trip", t) for t in (0, 1, 2)} | {("dist_codes", k) for k in (0, 1, 30)}
    req |= {("stored", 0, True, False)} | ring_labels()
    req |= {("match", w, o) for w in ("flushed", "ring", "across") for o in (False, True)}
    req |= {("barrier", "literal"), ("barrier", "match"), ("flush", 255)}
    return req


def ring_labels():
    """the staging ring's: an overlapping match whose source lies across the flushed line, a ring filled to 511 and to 512, a stored
    block that arrives while the ring holds bytes (at every bit offset; at offset 5 there are no pad bits)"""
    return {("match", "across", True), ("fill", 511), ("fill", 512)} | {("stored", o, o != 5, True) for o in range(8)}


def planted_streams():
    """name -> (member, data, the labels it must reach: the union of trace() over its candidates, dead ones included).  Written by hand,
    block by block: every branch of the decoder that no compressor's output takes.  History comes from a stored block in front"""
    global _PLANTED
    if _PLANTED is not None:
        return _PLANTED
    P = {}

    def add(name, d, labels):
        gz, data = d.member() if isinstance(d, Deflate) else d
        P[name] = (gz, data, set(labels))

    # every length symbol, none and all of its extra bits set; 284 + 31 is the other way to write 258
    toks = [(s, x, (s * 7 + x) % 14, 0) for s in range(257, 286) for x in _both(dc.LEN_EXTRA[s - 257])]
    add("lengths", Deflate().stored(noise(300, 81)).fixed(toks + [EOB], 1), {("len", s, e) for s in range(257, 286) for e in ("zero", "max")})

    # distance 32 768 from the segment's first byte (written as 284 + 31), then every distance symbol; the stored block's pad bits are 10101
    toks = [(284, 31, 29, 8191)] + [(257, 0, s, x) for s in range(30) for x in _both(dc.DIST_EXTRA[s])]
    add("far_first", Deflate().stored(noise(32768, 82), pad=0b10101).fixed(toks + [EOB], 1),
        {("dist", s, e) for s in range(30) for e in ("zero", "max")} | {("far", 0), ("stored", 0, True, False), ("match", "flushed", False)})
    # ... and from its second byte: one literal more in front
    add("far_second", Deflate().stored(noise(32768, 83)).fixed([7, (258, 0, 29, 8191), (285, 0, 29, 8191), EOB], 1), {("far", 1)})

    # a literal/length code of 1, 2, ..., 15, 15 bits, every one read; no distance code; the code-length code needs all of CL_ORDER
    lit = _lens(257, **{"s%d" % (65 + k): k + 1 for k in range(15)}, s256=15)
    add("long_literals", Deflate().dynamic(list(range(65, 80)) * 3 + [EOB], lit, [0], 1),
        {("lit_bits", l) for l in range(11, 16)} | {("hclen", 19), ("dist_codes", 0)})
    # the same lengths as a distance code
    lit = _lens(258, s65=2, s66=2, s256=2, s257=2)
    toks = [65] + [(257, 0, s, x) for s in range(16) for x in _both(dc.DIST_EXTRA[s])] + [66, EOB]
    add("long_distances", Deflate().stored(noise(300, 84)).dynamic(toks, lit, list(range(1, 16)) + [15], 1), {("dist_bits", l) for l in range(9, 16)})
    # HLIT 286 with HDIST 30
    toks = list(range(100, 140)) + [(285, 0, 3, 0), (264, 0, 5, 1), (284, 30, 9, 7), 255, 0, (285, 0, 29, 0), EOB]
    add("widest", Deflate().stored(noise(24577, 85)).dynamic(toks, [8] * 226 + [9] * 60, [4] * 2 + [5] * 28, 1), {("widest",), ("dist_codes", 30)})

    # dead candidates in a stored block: HCLEN 4 (only 16, 17, 18 and 0 have a length: there is no end-of-block code), and an 18 that runs
    # across HLIT with 119 and with 132 lengths in front of it, 64 lengths a trip of the lane loop (no VALID block has more than 29 zeros
    # between its end-of-block code and HLIT).  Each ends as NO_END_OF_BLOCK, at a bit that tells where the run went
    def no_code(hlit, hdist, reps):
        w = _dynamic(hlit, hdist, {0: 1, 18: 1}, 0)
        for r in reps:                                   # (the code-length code: 0 is the bit 0, 18 the bit 1)
            w.code(1, 1).put(r - 11, 7) if r else w.code(0, 1)
        return MARKER + w.bytes()
    payload = noise(40, 86) + no_code(257, 1, (138, 120)) + noise(9, 87) + no_code(257, 30, (138, 138, 11)) + noise(9, 88) + no_code(270, 7, (138, 138, 0))
    add("dead_headers", Deflate().stored(payload + noise(30, 89), 1),
        {("hclen", 4), ("across_in_trip", 1), ("across_in_trip", 2), ("repeat", 18, False, True)})

    # 16, 17 and 18 across the HLIT | HDIST boundary in blocks that are valid and use both codes
    d = Deflate().stored(noise(2100, 90))
    lit, dist = _lens(258, s65=2, s66=2, s256=2, s257=2), [2, 2, 2, 2, 0]
    d.dynamic([65, 66, 65, (257, 0, 0, 0), (257, 0, 3, 0), EOB], lit, dist, run=length_run(lit[:257]) + [(16, 2), (0, 0)])
    lit, dist = _lens(261, s65=2, s66=2, s256=2, s257=2), [0, 0, 2, 2, 2, 2]
    d.dynamic([66, 65, (257, 0, 2, 0), (257, 0, 5, 1), EOB], lit, dist, run=length_run(lit[:258]) + [(17, 2)] + [(2, 0)] * 4)
    lit, dist = _lens(286, s65=2, s66=2, s256=2, s257=2), [0] * 20 + [3] * 6 + [4] * 4
    d.dynamic([65, (257, 0, 20, 0), (257, 0, 21, 77), (257, 0, 22, 0), 66, EOB], lit, dist, 1, run=length_run(lit[:258]) + [(18, 48 - 11)] + length_run(dist[20:]))
    add("repeats_across", d, {("repeat", s, True, False) for s in (16, 17, 18)} | {("across_in_trip", 0)})

    # a 17 and an 18 that end exactly on HLIT + HDIST
    lit = _lens(258, s65=2, s66=2, s256=2, s257=2)
    d = Deflate().dynamic([65, 66, (257, 0, 1, 0), EOB], lit, [1, 1] + [0] * 5).dynamic([66, 65, 65, (257, 0, 0, 0), EOB], lit, [1, 1] + [0] * 20, 1)
    add("ends_on_total", d, {("repeat", 17, False, True), ("repeat", 18, False, True)})

    # the block whose only code is end-of-block, alone and in front of a block with output; one distance code of length 1
    only = _lens(257, s256=1)
    add("eob_only", Deflate().dynamic([EOB], only, [0], 1), {("lit_incomplete",)})
    add("eob_only_first", Deflate().dynamic([EOB], only, [0]).fixed([104, 105, (257, 0, 1, 0), EOB], 1), {("lit_incomplete",)})
    lit = _lens(286, s65=2, s66=2, s256=2, s285=2)
    add("one_distance_code", Deflate().dynamic([65, 66, (285, 0, 0, 0), 65, EOB], lit, [1], 1), {("dist_codes", 1)})

    # literals to fill 253, 254 and 255, then a match of 258: the ring filled to 511 and to 512, and the flush taken at its lowest fill
    d = Deflate()
    for k, fill in enumerate((253, 254, 255)):
        d.fixed(list(noise(fill, 91 + k)) + [(285, 0, (0, 2, 5)[k], 0), 33, EOB]).stored(noise(7, 94 + k))
    add("ring_filled", d.stored(b"", 1), {("fill", 511), ("fill", 512), ("flush", 255)})

    # a match whose source lies across the flushed line: `lits` literals behind a flush, then distance > lits; most overlap themselves
    d = Deflate()
    for k, (dist, lits, ls, lx) in enumerate(((2, 1, 264, 0), (3, 1, 285, 0), (63, 31, 285, 0), (64, 32, 277, 9), (65, 32, 284, 30), (257, 128, 285, 0),
                                              (1, 0, 285, 0), (100, 50, 276, 1))):
        ds, _, dx = dc.dist_symbol(dist)
        d.stored(noise(300, 100 + k), pad=0xFF).fixed(list(noise(lits, 110 + k)) + [(ls, lx, ds, dx), 35, EOB])
    add("source_across", d.stored(noise(5, 120), 1), {("match", "across", True), ("match", "across", False), ("match", "flushed", True)})

    # the source wholly in the ring and not yet seen by every lane: a match straight behind literals, and one straight behind that match
    d = Deflate()
    for k, dist in enumerate((1, 2, 3, 63, 64, 65)):
        ds, _, dx = dc.dist_symbol(dist)
        first, second = dc.length_symbol(dist + 3), dc.length_symbol(max(3, dist + 1))
        d.fixed(list(noise(dist + 2, 130 + k)) + [(first[0], first[2], ds, dx), (second[0], second[2], ds, dx), (257, 0, 2, 0), 36, EOB]).stored(noise(3, 140 + k))
    add("source_in_ring", d.stored(b"", 1), {("match", "ring", True), ("match", "ring", False), ("barrier", "literal"), ("barrier", "match")})

    # a stored block behind Huffman output at every bit offset, its pad bits ones: a fixed block from a byte boundary with b literals of
    # nine bits ends at bit 3 + 8 a + 9 b + 7
    d = Deflate().stored(noise(20, 150))
    for offset in range(8):
        d.fixed([200] * ((offset - 2) % 8) + [72, 73, 74, EOB]).stored(noise(11 + offset, 151 + offset), pad=0xFF)
    add("stored_offsets", d.stored(b"", 1), ring_labels() - {("match", "across", True), ("fill", 511), ("fill", 512)})

    # candidates at the marking tiles' edges (2 048 positions a tile, 8 a thread): live empty stored blocks that end at LIVE_TILE_ENDS,
    # dead markers at DEAD_TILE_ENDS -- three and two in a row: 00 00 FF FF 00 00 FF FF -- and 00 00 00 FF FF in the middle of a tile
    d = Deflate()
    for p in LIVE_TILE_ENDS:
        d.stored(noise(p - 20 - len(d.w.done), 160 + p % 50)).stored(b"")
        assert 10 + len(d.w.done) == p
    tail = bytearray(noise(2048 * 14 - 20 - len(d.w.done), 170))
    at = 10 + len(d.w.done) + 5                           # the member's offset of the payload's first byte
    for p in DEAD_TILE_ENDS + [2048 * 13 + 1000]:
        tail[p - 4 - at:p - at] = MARKER
    tail[2048 * 13 + 1000 - 5 - at] = 0
    add("tile_edges", d.stored(bytes(tail), 1), ())

    # a marker whose candidate is n - 8 (it counts), and one whose candidate would be n - 7: 00 00 FF, then a CRC-32 that begins with FF
    add("marker_at_n_minus_8", Deflate().stored(noise(50, 171) + MARKER, 1), ())
    k = next(k for k in range(1 << 16) if zlib.crc32(noise(50, 172) + k.to_bytes(2, "little") + b"\x00\x00\xff") & 255 == 255)
    add("marker_at_n_minus_7", Deflate().stored(noise(50, 172) + k.to_bytes(2, "little") + b"\x00\x00\xff", 1), ())

    # 3 000 empty stored blocks in a row: 3 000 live segments without output, alone ...
    add("empty_segments", (member(EMPTY * N_EMPTY + b"\x03\x00", b""), b""), ())
    # ... and between a segment of exactly 1 MiB (a window of MI_INFLATE_WINDOW_MB=1: the empty ones sit at the round's end) and one more
    d = Deflate().fixed([0] + [(285, 0, 0, 0)] * 4064 + [(276, 4, 0, 0), EOB])
    assert len(d.data) == 1 << 20
    for _ in range(N_EMPTY):
        d.stored(b"")
    add("empty_segments_between", d.stored(noise(100, 173), 1), ())

    # 77 KB out of 400 bytes: from some starts the output passes a window of 64 KiB
    add("long_run", Deflate().fixed([1, 2, 3] + [(285, 0, 2, 0)] * 300 + [EOB], 1), {("match", "flushed", True)})
    _PLANTED = P
    return P


def far_layer():
    """a layer whose tar is one file, written so that the first match has distance 32 768 and its source at the segment's first byte
    (the tar header's): -> (blob, tar, the file's bytes)"""
    import layer_blob_cases as lc
    toks = [(284, 31, 29, 8191), 70, (257, 0, 29, 8191), (285, 0, 29, 0), EOB]
    size = 32768 - 512 + 258 + 1 + 3 + 258
    d = Deflate().stored(lc.raw_header("far", size) + noise(32768 - 512, 174), pad=0b01010).fixed(toks)
    content = bytes(d.data[512:])
    assert len(content) == size
    return d.stored(bytes(-size % 512) + lc.END, 1).member() + (content,)


def member_labels(gz, window=WINDOW):
    """the union of trace() over the member's candidates, and every candidate's row"""
    labels, out = set(), []
    for c in candidates(gz, gzip_header(gz)):
        row, _, got = trace(gz, c, window)
        labels |= got
        out.append((c, row))
    return labels, out
