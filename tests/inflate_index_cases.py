"""The indexed device inflate's model (csrc/host_inflate_index.h, csrc/mi_inflate_wave.h's span mode), written from RFC
1951 and the format stated in include/makisu_mi.h: a block walk of its own, the index of checkpoints of a member -- index(gz, spacing),
byte for byte what mi_inflate_index_build must give --, its parse, and the decoder of ONE SPAN with the numbered rules --
decode_span(gz, in_bit, end_bit, hist, out_bytes), what inflate_span_kernel must reproduce.  Pure functions of the bytes.  The code
tables, the rule numbers and the Deflate writer are inflate_cases'.

THE SPAN differs from inflate_cases' segment in five ways: it starts at a BIT; an empty stored block does not end it; it ends where a
block's header would begin at end_bit, with exactly out_bytes made -- a header behind end_bit, a BFINAL block in front of it and output
beyond out_bytes are all rule 12, INDEX --; the last span (end_bit 0) ends at its BFINAL block; a match may reach len(hist) bytes
before the span's first byte, into hist."""
import zlib

import deflate_cases as dc
from inflate_cases import (BLOCK_TYPE, CODE, DISTANCE, EOB, INPUT_ENDS, LENGTH_CODE, NO_END_OF_BLOCK, REPEAT, SEG_BROKEN, SEG_ENDS, SEG_FINAL,
                           STORED_LEN, SYMBOL, TOO_MANY_CODES, Deflate, _build, _fixed, gzip_header, host_leg, no_reset, noise, one_stream)

INDEX = 12                                               # kInfIndex: the span does not end where the index says
ENDS_EARLY = 0x100                                       # (the kernel's word to the host) the last span's stream ends before n - 8
MAGIC = b"MIGZIX01"
SPACING, WINDOW = 262144, 32768
REFUSALS = (OK, R_MAGIC, R_SIZES, R_FIRST, R_IN_BIT, R_OUT_AT, R_IN_END, R_OUT_END, R_WIN_BYTES, R_WINDOW, R_MEMBER) = tuple(range(11))


class _Broken(Exception):
    def __init__(self, rule, bit=None):
        self.rule, self.bit = rule, bit


def _walk(gz, in_bit, end_bit, hist, limit, on_block=None):
    """the blocks from bit in_bit -> (row, bytes); on_block(bit, output so far, bfinal) behind every block"""
    n, nbits = len(gz), 8 * len(gz)
    buf = bytearray(hist)
    base = len(buf)
    pos = in_bit

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

    def incomplete(b):
        return b[1] > 0 and not (b[3] == 1 and b[2] == 1)

    try:
        while True:
            if end_bit:
                if pos == end_bit:
                    if len(buf) - base != limit:
                        raise _Broken(INDEX)
                    return dict(status=SEG_ENDS, end=pos >> 3, out_bytes=len(buf) - base, rule=0, bit=pos), bytes(buf[base:])
                if pos > end_bit:
                    raise _Broken(INDEX)
            bfinal, btype = take(1), take(2)
            ends()
            if bfinal and end_bit:
                raise _Broken(INDEX)
            if btype == 3:
                raise _Broken(BLOCK_TYPE)
            if btype == 0:
                take(-pos & 7)
                ln, nln = take(16), take(16)
                ends()
                if ln ^ 0xFFFF != nln:
                    raise _Broken(STORED_LEN)
                byte = pos >> 3
                if byte + ln > n:
                    raise _Broken(INPUT_ENDS, nbits)
                if len(buf) - base + ln > limit:
                    raise _Broken(INDEX)
                buf += gz[byte:byte + ln]
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
                            if len(lens) + rep > hlit + hdist:
                                raise _Broken(REPEAT)
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
                while True:
                    s = symbol(lit)
                    if s < 256:
                        ends()
                        if len(buf) - base + 1 > limit:
                            raise _Broken(INDEX)
                        buf.append(s)
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
                    if distance > len(buf):              # beyond the span's own bytes AND the window in front of them
                        raise _Broken(DISTANCE)
                    if len(buf) - base + length > limit:
                        raise _Broken(INDEX)
                    if distance >= length:
                        src = len(buf) - distance
                        buf += buf[src:src + length]
                    else:
                        for _ in range(length):
                            buf.append(buf[-distance])
            if on_block:
                on_block(pos, len(buf) - base, bfinal)
            if bfinal:
                return dict(status=SEG_FINAL, end=(pos + 7) >> 3, out_bytes=len(buf) - base, rule=0, bit=pos), bytes(buf[base:])
    except _Broken as e:
        return dict(status=SEG_BROKEN, end=0, out_bytes=len(buf) - base, rule=e.rule, bit=pos if e.bit is None else e.bit), bytes(buf[base:])


def decode_span(gz, in_bit, end_bit, hist, out_bytes):
    """the span from bit in_bit -> (row, its bytes).  row: dict(status, end, out_bytes, rule, bit) -- what inflate_span_kernel makes of
    the span: SEG_ENDS / SEG_FINAL with rule 0, or SEG_BROKEN with the rule.  end_bit 0: the last span, which must end at n - 8 (before
    it: rule ENDS_EARLY, behind it: INDEX)"""
    row, out = _walk(bytes(gz), in_bit, end_bit, bytes(hist), out_bytes)
    if row["status"] == SEG_FINAL:
        if row["out_bytes"] != out_bytes:
            row.update(status=SEG_BROKEN, rule=INDEX)
        elif row["end"] != len(gz) - 8:
            row.update(status=SEG_BROKEN, rule=ENDS_EARLY if row["end"] < len(gz) - 8 else INDEX)
    return row, out


def boundaries(gz):
    """the block walk: [(bit behind the block, output behind it, bfinal)], and the member's inflation"""
    gz = bytes(gz)
    found = []
    row, out = _walk(gz, 8 * gzip_header(gz), 0, b"", 1 << 62, lambda bit, o, bfinal: found.append((bit, o, bfinal)))
    assert row["status"] == SEG_FINAL and row["end"] == len(gz) - 8, row
    assert zlib.crc32(out) == int.from_bytes(gz[-8:-4], "little") and len(out) & 0xFFFFFFFF == int.from_bytes(gz[-4:], "little")
    return found, out


def points(gz, spacing=0):
    """the point rule -> ([(in_bit, out_at)], the inflation)"""
    spacing = spacing or SPACING
    found, out = boundaries(gz)
    pts = [(8 * gzip_header(bytes(gz)), 0)]
    for bit, o, bfinal in found:
        if not bfinal and o - pts[-1][1] >= spacing:
            pts.append((bit, o))
    if len(pts) > 1 and pts[-1][1] == len(out):          # a span without output
        pts.pop()
    return pts, out


def index(gz, spacing=0):
    """the member's index of checkpoints, as bytes"""
    gz = bytes(gz)
    pts, out = points(gz, spacing)
    rows, windows = b"", b""
    for k, (bit, o) in enumerate(pts):
        wb = min(WINDOW, o) if k else 0
        rows += bit.to_bytes(8, "little") + o.to_bytes(8, "little") + len(windows).to_bytes(8, "little") + wb.to_bytes(4, "little") + bytes(4)
        windows += out[o - wb:o] + bytes(-wb % 16)
    head = MAGIC + len(gz).to_bytes(8, "little") + len(out).to_bytes(8, "little") + gz[-8:] + gzip_header(gz).to_bytes(8, "little")
    head += len(pts).to_bytes(8, "little") + (spacing or SPACING).to_bytes(8, "little") + len(windows).to_bytes(8, "little")
    return head + rows + windows


def parse(ix):
    """-> dict(n, out_bytes, crc, isize, header, n_points, spacing, windows_bytes, points: [dict(in_bit, out_at, win_at, win_bytes)], windows)"""
    u = lambda at, k=8: int.from_bytes(ix[at:at + k], "little")
    assert ix[:8] == MAGIC
    h = dict(n=u(8), out_bytes=u(16), crc=u(24, 4), isize=u(28, 4), header=u(32), n_points=u(40), spacing=u(48), windows_bytes=u(56))
    h["points"] = [dict(in_bit=u(64 + 32 * k), out_at=u(72 + 32 * k), win_at=u(80 + 32 * k), win_bytes=u(88 + 32 * k, 4)) for k in range(h["n_points"])]
    h["windows"] = ix[64 + 32 * h["n_points"]:]
    return h


def spans(ix):
    """the span table the plan makes of an index: [dict(in_bit, end_bit, out_at, out_bytes, win_at, win_bytes, hist)]"""
    h = parse(ix)
    p = h["points"]
    out = []
    for k, q in enumerate(p):
        nxt = p[k + 1] if k + 1 < len(p) else None
        out.append(dict(in_bit=q["in_bit"], end_bit=nxt["in_bit"] if nxt else 0, out_at=q["out_at"],
                        out_bytes=(nxt["out_at"] if nxt else h["out_bytes"]) - q["out_at"], win_at=q["win_at"], win_bytes=q["win_bytes"],
                        hist=h["windows"][q["win_at"]:q["win_at"] + q["win_bytes"]]))
    return out


def patch(ix, at, value, k=8):
    return ix[:at] + value.to_bytes(k, "little") + ix[at + k:]


def row_at(k, field):
    """the offset of a field of row k in an index"""
    return 64 + 32 * k + {"in_bit": 0, "out_at": 8, "win_at": 16, "win_bytes": 24, "zero": 28}[field]


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
def _m(length, distance):
    ls, _, lx = dc.length_symbol(length)
    ds, _, dx = dc.dist_symbol(distance)
    return (ls, lx, ds, dx)


_PLANTED = None


def planted_member():
    """-> (member, data, what: name -> the output offset of the point whose span shows it).  Written block by block with Deflate: at
    spacing 1 every block with output begins a span, so each block's first tokens are that span's first tokens.  The points lie at
    every bit offset mod 8 (the stored blocks realign to 0, the nine-bit literals 200 shift by one bit each), and the spans hold matches
    wholly inside the window, straddling position 0 (plain and overlapping), overlapping with dist < len from inside the window, at
    distance 32 768 reaching hist[0] (and at distance == out_at reaching hist[0] of a SHORT window), a span that BEGINS with an empty
    stored block (the point lies directly at it; by the point rule no point can lie behind one without output in between) and points
    with out_at < 32 768"""
    global _PLANTED
    if _PLANTED is not None:
        return _PLANTED
    d, what = Deflate(), {}

    def mark(name):
        what[name] = len(d.data)
    d.stored(noise(1000, 301))
    mark("short_window")                                 # out_at 1 000: the window is 1 000 bytes
    mark("inside_window")
    d.fixed([_m(10, 500), _m(258, 1000), 65, EOB])      # wholly inside the window; then distance == out_at + 10: hist[0] of the short window
    mark("short_window_first_byte")
    d.fixed([_m(40, len(d.data)), 66, EOB])              # op 0, distance == out_at: the short window's first byte
    mark("straddle_plain")
    d.fixed(list(noise(10, 302)) + [_m(8, 14), 67, EOB])                # source -4 .. +4
    mark("straddle_overlap")
    d.fixed(list(noise(5, 303)) + [_m(20, 15), _m(200, 7), 68, EOB])    # source -10 .. +10 with dist < len, then one across the ring
    mark("overlap_from_window")
    d.fixed([_m(258, 3), _m(258, 1), _m(100, 300), 69, EOB])            # op 0: source -3, dist 3 < len 258
    for k in range(8):                                   # the points' bit offsets: a block of 18 + 9 k bits
        mark("shift_%d" % k)
        d.fixed([200] * k + [72 + k, EOB])
    d.stored(noise(40000, 304), pad=0b11011)
    mark("far")
    d.fixed([(284, 31, 29, 8191), 70, _m(3, 32768), _m(258, 32768), EOB])     # op 0, distance 32 768: hist[0]; then op 259 and 262
    mark("far_second")
    d.fixed([71, _m(258, 32768), EOB])
    mark("empty_stored_first")
    d.stored(b"", pad=0b101)                             # the span begins with an empty stored block, which does not end it
    d.seg = 0                                            # (the writer's own segment rule does not hold here: matches reach across)
    d.fixed([_m(30, 20000), 73, EOB]).stored(b"")
    d.seg = 0
    d.fixed([_m(9, 9), EOB])                             # (no point in front: the empty block advanced no output ... but the fixed one did)
    mark("last")
    d.dynamic([65, 66, (257, 0, 0, 0), EOB], [0] * 65 + [2, 2] + [0] * 189 + [2, 2], [1], 1)
    gz, data = d.member()
    _PLANTED = (gz, data, what)
    return _PLANTED


def local_binary(n=1 << 20):
    """n bytes of a binary that lies on every machine this runs on: the interpreter's own"""
    import os
    import sys
    with open(os.path.realpath(sys.executable), "rb") as f:
        data = f.read(n)
    if len(data) < n:                                    # (a launcher script: pad with text, the sizes stay)
        data += dc.text(n - len(data), 305)
    return data


def members():
    """name -> (member, data): what the builder and the model must agree on"""
    data = dc.text(60000, 310) + local_binary(400000) + dc.random_bytes(3000, 311) + dc.text(40000, 312)
    out = {}
    for level in (1, 6, 9):
        out["one_stream_%d" % level] = (one_stream(data, level), data)
    out["one_stream_fixed"] = (one_stream(data, 6, zlib.Z_FIXED), data)
    out["no_reset"] = (no_reset(data, 1 << 15), data)
    out["host_leg"] = (host_leg(data, 6, 1 << 17), data)
    rnd = dc.random_bytes(200000, 313)
    out["stored_only"] = (one_stream(rnd, 6), rnd)
    gz, pdata, _ = planted_member()
    out["planted"] = (gz, pdata)
    return out
