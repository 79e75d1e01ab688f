"""The device inflate's model (csrc/mi_inflate_wave.h, csrc/host_inflate.h), written from RFC 1951 and RFC 1952: the gzip
header, the candidates, a bit-exact decoder of one segment with the numbered rules, the rows, the live chain, the verdicts and the
rounds for a window -- what mi_inflate_buffer must reproduce -- and the builders of the tests' inputs.  Pure functions of the bytes.

THE FORMAT RULE.  A candidate is a byte offset p with gz[p - 4:p] == 00 00 FF FF and p <= n - 8; the first byte behind the gzip header
is one too.  The segment from a candidate c is decoded from bit 8 c until (a) an EMPTY stored block with BFINAL 0 has been read (the
segment ends at the byte behind it), (b) a block with BFINAL 1 has been read (END, at the next byte boundary) or (c) a rule is
broken.  The live chain starts at the header's end and follows the ends to END, which must lie at n - 8; other candidates are dead.
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


def decode_segment(gz, start, limit=WINDOW, stop_at_empty=True):
    """the segment from byte `start` -> (row, its bytes).  row: dict(status, end, out_bytes, rule, bit).  Bits behind the member's last
    byte read as zero and break INPUT_ENDS at the next check, as the kernel's reader does.  stop_at_empty=False is the WRONG decoder
    that reads on behind an empty stored block"""
    n, nbits = len(gz), 8 * len(gz)
    out = bytearray()
    pos = 8 * start

    def take(k):
        nonlocal pos
        v = (int.from_bytes(gz[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << k) - 1)
        pos += k
        return v

    def symbol(built):
        nonlocal pos
        longest, table = built[3], built[4]
        e = table[(int.from_bytes(gz[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << longest) - 1)] if longest else None
        if e is None:
            raise _Broken(SYMBOL)
        pos += e[1]
        return e[0]

    def ends():
        if pos > nbits:
            raise _Broken(INPUT_ENDS)

    def incomplete(b):                                   # allowed only as a single code of length 1
        return b[1] > 0 and not (b[3] == 1 and b[2] == 1)

    try:
        while True:
            bfinal, btype = take(1), take(2)
            ends()
            if btype == 3:
                raise _Broken(BLOCK_TYPE)
            if btype == 0:
                pos += -pos & 7
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
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[dc.CL_ORDER[i]] = take(3)
                    ends()
                    clb = _build(cl)
                    if clb[0] or clb[1] != 0:
                        raise _Broken(LENGTH_CODE)
                    lens, prev = [], 0
                    while len(lens) < hlit + hdist:
                        s = symbol(clb)
                        if s < 16:
                            lens.append(s)
                            prev = s
                        else:
                            if s == 16:
                                if not lens:
                                    raise _Broken(REPEAT)
                                val, rep = prev, 3 + take(2)
                            elif s == 17:
                                val, rep = 0, 3 + take(3)
                            else:
                                val, rep = 0, 11 + take(7)
                            if len(lens) + rep > hlit + hdist:
                                raise _Broken(REPEAT)
                            lens += [val] * rep
                            prev = val
                        ends()
                    if lens[256] == 0:
                        raise _Broken(NO_END_OF_BLOCK)
                    lit, dist = _build(lens[:hlit]), _build(lens[hlit:])
                    if lit[0] or incomplete(lit):
                        raise _Broken(CODE)
                    if dist[0] or (dist[2] != 0 and incomplete(dist)):
                        raise _Broken(CODE)
                while True:
                    s = symbol(lit)
                    if s < 256:
                        ends()
                        if len(out) + 1 > limit:
                            raise _Broken(BEYOND_WINDOW)
                        out.append(s)
                        continue
                    if s == 256:
                        ends()
                        break
                    if s > 285:
                        raise _Broken(SYMBOL)
                    length = dc.LEN_BASE[s - 257] + take(dc.LEN_EXTRA[s - 257])
                    d = symbol(dist)
                    if d > 29:
                        raise _Broken(SYMBOL)
                    distance = dc.DIST_BASE[d] + take(dc.DIST_EXTRA[d])
                    ends()
                    if distance > len(out):
                        raise _Broken(DISTANCE)
                    if len(out) + length > limit:
                        raise _Broken(BEYOND_WINDOW)
                    if distance >= length:
                        out += out[len(out) - distance:len(out) - distance + length]
                    else:
                        for _ in range(length):
                            out.append(out[-distance])
            if bfinal:
                return dict(status=SEG_FINAL, end=(pos + 7) >> 3, out_bytes=len(out), rule=0, bit=pos), bytes(out)
    except _Broken as e:
        status = SEG_TOO_LONG if e.rule == BEYOND_WINDOW else SEG_BROKEN
        return dict(status=status, end=0, out_bytes=len(out), rule=e.rule, bit=pos if e.bit is None else e.bit), bytes(out)


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


def plan(gz, window=WINDOW, stop_at_empty=True):
    """what mi_inflate_buffer says of the member: dict(result = DONE / NOT_PARALLEL / INVALID, out, rule, at_in, at_out, n_candidates,
    n_segments, n_rounds, sizes).  Only the live chain's candidates are decoded"""
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
        row, data = decode_segment(gz, at, window, stop_at_empty)
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


def _dynamic(hlit, hdist, cl):
    """BFINAL 1, BTYPE 2 and the header up to the code-length code's lengths (cl: symbol -> length, as many of CL_ORDER as needed)"""
    hclen = max([4] + [dc.CL_ORDER.index(s) + 1 for s in cl])
    w = _Bits().put(1, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
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
