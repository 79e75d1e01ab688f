"""The speculative device inflate's model (csrc/mi_inflate_spec.hip, csrc/host_inflate_spec.h), written from RFC 1951 and
the contract stated in include/makisu_mi.h, on top of inflate_cases / inflate_index_cases (the code tables, the rule numbers, the Deflate
writer, the index format): find(gz, piece) -- every piece's candidate --, speculate(gz, cand, k, piece) -- a candidate's row and its ring
entries --, chain, windows, plan and index_of(plan).  Pure functions of the bytes.

THE PIECES.  The deflate stream behind the gzip header (length hdr) is cut into pieces of `piece` member bytes; piece k covers the bits
[8 (hdr + k piece), 8 (hdr + (k + 1) piece)) below 8 (n - 8).  Piece 0's candidate is 8 hdr.  For k >= 1 it is the SMALLEST bit p of the
piece at which a non-final dynamic block header parses -- BFINAL 0, BTYPE 2, the header's rules 3, 4, 5, 6 and 9 and the tables' rule 7
hold -- or NONE.  A header may run past its piece's end, never past the member.

THE SPECULATIVE SPAN from a candidate's bit: blocks are decoded into ENTRIES, one per output position -- a literal is its byte, a byte the
span cannot know is a MARKER 0x8000 + k, "the byte 32 768 - k positions before my first byte"; a match copies entries as they are.  There
is no distance rule.  Before every block header at a bit b > the start: b is its piece's candidate -> the span ENDS there.  A BFINAL
block ends it FINAL (end: the next byte boundary, in bits).  Output beyond the window, or more than 32 x piece literals and matches,
end it TOO_LONG (rules 11 and 13)."""
import zlib

import deflate_cases as dc
import inflate_cases as ic
import inflate_index_cases as xc
from inflate_cases import (BEYOND_WINDOW, BLOCK_TYPE, CODE, EOB, INPUT_ENDS, LENGTH_CODE, NO_END_OF_BLOCK, REPEAT, SEG_BROKEN, SEG_ENDS, SEG_FINAL,
                           SEG_TOO_LONG, STORED_LEN, SYMBOL, TOO_MANY_CODES, Deflate, _build, _fixed, gzip_header, noise)

SYMBOL_CAP = 13                                          # kInfSymbolCap
NONE = 2 ** 64 - 1
PIECE, PIECE_MIN, PIECE_MAX, MAX_PIECES = 65536, 1024, 16777216, 16384
RING = 32768
SYMBOLS_PER_BYTE = 32
DONE, NOT_PARALLEL, INVALID, INTERNAL = "done", "not_parallel", "invalid", "internal"


class _Broken(Exception):
    def __init__(self, rule, bit=None):
        self.rule, self.bit = rule, bit


def pieces(gz, piece_bytes=0):
    """-> (hdr, the piece used, the number of pieces), or None: piece_bytes out of range, or no header"""
    hdr = gzip_header(gz)
    piece = piece_bytes or PIECE
    if hdr is None or len(gz) < hdr + 9 or not PIECE_MIN <= piece <= PIECE_MAX:
        return None
    stream = len(gz) - 8 - hdr
    while -(-stream // piece) > MAX_PIECES:
        piece *= 2
    return hdr, piece, -(-stream // piece)


class _Reader:
    def __init__(self, gz, pos):
        self.gz, self.pos, self.nbits = gz, pos, 8 * len(gz)

    def take(self, k):
        v = (int.from_bytes(self.gz[self.pos >> 3:(self.pos >> 3) + 4], "little") >> (self.pos & 7)) & ((1 << k) - 1)
        self.pos += k
        return v

    def symbol(self, built):
        longest, table = built[3], built[4]
        e = table[(int.from_bytes(self.gz[self.pos >> 3:(self.pos >> 3) + 4], "little") >> (self.pos & 7)) & ((1 << longest) - 1)] if longest else None
        if e is None:
            raise _Broken(SYMBOL)
        self.pos += e[1]
        return e[0]

    def ends(self):
        if self.pos > self.nbits:
            raise _Broken(INPUT_ENDS)


def _incomplete(b):
    return b[1] > 0 and not (b[3] == 1 and b[2] == 1)


def _dynamic_tables(r):
    """the dynamic header behind BTYPE -> (literal/length code, distance code); raises the rule"""
    hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
    r.ends()
    if hlit > 286 or hdist > 30:
        raise _Broken(TOO_MANY_CODES)
    cl = [0] * 19
    for i in range(hclen):
        cl[dc.CL_ORDER[i]] = r.take(3)
    r.ends()
    clb = _build(cl)
    if clb[0] or clb[1] != 0:
        raise _Broken(LENGTH_CODE)
    lens, prev_len = [], 0
    while len(lens) < hlit + hdist:
        s = r.symbol(clb)
        if s < 16:
            lens.append(s)
            prev_len = s
        else:
            if s == 16:
                if not lens:
                    raise _Broken(REPEAT)
                val, rep = prev_len, 3 + r.take(2)
            elif s == 17:
                val, rep = 0, 3 + r.take(3)
            else:
                val, rep = 0, 11 + r.take(7)
            if len(lens) + rep > hlit + hdist:
                raise _Broken(REPEAT)
            lens += [val] * rep
            prev_len = val
        r.ends()
    if lens[256] == 0:
        raise _Broken(NO_END_OF_BLOCK)
    lit, dist = _build(lens[:hlit]), _build(lens[hlit:])
    if lit[0] or _incomplete(lit):
        raise _Broken(CODE)
    if dist[0] or (dist[2] != 0 and _incomplete(dist)):
        raise _Broken(CODE)
    return lit, dist


def parses(gz, p):
    """a non-final dynamic block header parses at bit p -> None, or the rule it breaks (-1: BFINAL or BTYPE are not 0 and 2)"""
    r = _Reader(gz, p)
    if r.take(3) != 4:
        return -1
    try:
        _dynamic_tables(r)
    except _Broken as e:
        return e.rule
    return None


_KRAFT = (0, 64, 32, 16, 8, 4, 2, 1)


def _may_parse(v):
    """the first 74 bits at a position, as an integer: what any header that parses satisfies (only a shortcut of parses())"""
    if v & 7 != 4 or (v >> 3) & 31 > 29 or (v >> 8) & 31 > 29:
        return False
    hclen, k = ((v >> 13) & 15) + 4, 0
    v >>= 17
    for _ in range(hclen):
        k += _KRAFT[v & 7]
        v >>= 3
    return k == 128


def find(gz, piece_bytes=0):
    """every piece's candidate: [bit or NONE]"""
    gz = bytes(gz)
    hdr, piece, n_pieces = pieces(gz, piece_bytes)
    n = len(gz)
    cand = [8 * hdr]
    for k in range(1, n_pieces):
        first, last = 8 * (hdr + k * piece), min(8 * (hdr + (k + 1) * piece), 8 * (n - 8))
        got = NONE
        for byte in range(first >> 3, (last + 7) >> 3):
            v = int.from_bytes(gz[byte:byte + 11], "little")
            for o in range(8):
                p = 8 * byte + o
                if first <= p < last and _may_parse(v >> o) and parses(gz, p) is None:
                    got = p
                    break
            if got != NONE:
                break
        cand.append(got)
    return cand


def speculate(gz, cand, k, piece_bytes=0, window=ic.WINDOW, cap=None):
    """candidate k's speculative span -> (row, entries): row = dict(status, end, out_bytes, rule, bit) with `end` a BIT, entries = one int
    per output position (the ring holds the last 32 768 of them, position p at p & 32 767).  None, None for a candidate of NONE"""
    gz = bytes(gz)
    hdr, piece, n_pieces = pieces(gz, piece_bytes)
    assert len(cand) == n_pieces
    n, start = len(gz), cand[k]
    if start == NONE:
        return None, None
    cap = SYMBOLS_PER_BYTE * piece if cap is None else cap
    stream_end = 8 * (n - 8)
    r = _Reader(gz, start)
    out, symbols = [], 0
    try:
        while True:
            at = r.pos
            if start < at < stream_end:
                pk = (at // 8 - hdr) // piece
                if pk < n_pieces and cand[pk] == at:
                    return dict(status=SEG_ENDS, end=at, out_bytes=len(out), rule=0, bit=at), out
            bfinal, btype = r.take(1), r.take(2)
            r.ends()
            if btype == 3:
                raise _Broken(BLOCK_TYPE)
            if btype == 0:
                r.take(-r.pos & 7)
                ln, nln = r.take(16), r.take(16)
                r.ends()
                if ln ^ 0xFFFF != nln:
                    raise _Broken(STORED_LEN)
                byte = r.pos >> 3
                if byte + ln > n:
                    raise _Broken(INPUT_ENDS, 8 * n)
                if len(out) + ln > window:
                    raise _Broken(BEYOND_WINDOW)
                out += gz[byte:byte + ln]
                r.pos = 8 * (byte + ln)
            else:
                lit, dist = _fixed() if btype == 1 else _dynamic_tables(r)
                while True:
                    s = r.symbol(lit)
                    if s < 256:
                        r.ends()
                        if len(out) + 1 > window:
                            raise _Broken(BEYOND_WINDOW)
                        if symbols + 1 > cap:
                            raise _Broken(SYMBOL_CAP)
                        out.append(s)
                        symbols += 1
                        continue
                    if s == 256:
                        r.ends()
                        break
                    if s > 285:
                        raise _Broken(SYMBOL)
                    length = dc.LEN_BASE[s - 257] + r.take(dc.LEN_EXTRA[s - 257])
                    d = r.symbol(dist)
                    if d > 29:
                        raise _Broken(SYMBOL)
                    distance = dc.DIST_BASE[d] + r.take(dc.DIST_EXTRA[d])
                    r.ends()
                    if len(out) + length > window:
                        raise _Broken(BEYOND_WINDOW)
                    if symbols + 1 > cap:
                        raise _Broken(SYMBOL_CAP)
                    symbols += 1
                    for _ in range(length):
                        p = len(out) - distance
                        out.append(out[p] if p >= 0 else 0x8000 + 32768 + p)
            if bfinal:
                return dict(status=SEG_FINAL, end=(r.pos + 7) // 8 * 8, out_bytes=len(out), rule=0, bit=r.pos), out
    except _Broken as e:
        status = SEG_TOO_LONG if e.rule in (BEYOND_WINDOW, SYMBOL_CAP) else SEG_BROKEN
        return dict(status=status, end=0, out_bytes=len(out), rule=e.rule, bit=r.pos if e.bit is None else e.bit), out


def ring_of(entries):
    """the ring's 32 768 entries behind a span: position p at p & 32 767 (None where no position landed)"""
    ring = [None] * RING
    for p in range(max(0, len(entries) - RING), len(entries)):
        ring[p & (RING - 1)] = entries[p]
    return ring


def chain(gz, cand, rows, piece_bytes=0):
    """the walk from candidate 0 along the rows' ends (rows: per piece, or a function k -> row) -> dict(result, rule, span, at_bit, at_out,
    bit, total, live: [(piece, in_bit, out_at, out_bytes)]).  It trusts nothing: an end that is no candidate, does not advance or lies
    outside the stream is INTERNAL"""
    gz = bytes(gz)
    hdr, piece, n_pieces = pieces(gz, piece_bytes)
    n = len(gz)
    get = rows if callable(rows) else (lambda k: rows[k])
    res = dict(result=INTERNAL, rule=0, span=0, at_bit=0, at_out=0, bit=0, total=0, live=[])
    if cand[0] != 8 * hdr:
        return res
    k, at, stream_end = 0, cand[0], 8 * (n - 8)
    while True:
        row = get(k)
        res.update(span=len(res["live"]), at_bit=at, at_out=res["total"], rule=row["rule"], bit=row["bit"])
        if row["status"] == SEG_BROKEN:
            res["live"].append((k, at, res["total"], row["out_bytes"]))
            res["result"] = INVALID
            return res
        if row["status"] == SEG_TOO_LONG:
            res["live"].append((k, at, res["total"], row["out_bytes"]))
            res["result"] = NOT_PARALLEL
            return res
        if row["status"] not in (SEG_ENDS, SEG_FINAL) or row["end"] <= at or row["end"] > 8 * n or row["out_bytes"] > (NONE >> 1) - res["total"]:
            return res
        res["live"].append((k, at, res["total"], row["out_bytes"]))
        res["total"] += row["out_bytes"]
        if row["status"] == SEG_FINAL:
            res["rule"] = 0
            if row["end"] == stream_end:
                res["result"] = DONE
            elif row["end"] < stream_end:
                res["result"] = NOT_PARALLEL
            else:
                res.update(result=INVALID, rule=INPUT_ENDS, bit=8 * n)
            return res
        if row["end"] >= stream_end:
            return res
        nxt = (row["end"] // 8 - hdr) // piece
        if nxt >= n_pieces or nxt <= k or cand[nxt] != row["end"]:
            return res
        k, at = nxt, row["end"]


def merge(live):
    """the live spans -> the span table: a span without output is merged into the one in front (and so is one with no output in front of
    it): [dict(in_bit, end_bit, out_at, out_bytes, win_at, win_bytes, ring)], the window area's bytes"""
    spans = []
    for k, in_bit, out_at, out_bytes in live:
        if spans and (out_bytes == 0 or out_at == 0):
            if spans[-1]["out_bytes"] == 0:
                spans[-1]["ring"] = k
            spans[-1]["out_bytes"] += out_bytes
        else:
            spans.append(dict(in_bit=in_bit, end_bit=0, out_at=out_at, out_bytes=out_bytes, win_at=0, win_bytes=0, ring=k))
    win_at = 0
    for i, s in enumerate(spans):
        s["end_bit"] = spans[i + 1]["in_bit"] if i + 1 < len(spans) else 0
        if i:
            s["win_bytes"], s["win_at"] = min(RING, s["out_at"]), win_at
            win_at += (s["win_bytes"] + 15) // 16 * 16
    return spans, win_at


def windows(spans, total, entries_of):
    """the window area: span i's window from span i - 1's entries (entries_of(piece) -> its entries), markers resolved through span
    i - 1's window; a marker that reaches before the member's first byte reads as zero"""
    area = bytearray(total)
    prev_w = b""
    for i in range(1, len(spans)):
        p, s = spans[i - 1], spans[i]
        ent = entries_of(p["ring"])
        assert len(ent) == p["out_bytes"]
        w = bytearray(s["win_bytes"])
        for j in range(s["win_bytes"]):
            a = s["out_at"] - s["win_bytes"] + j
            if a >= p["out_at"]:
                e = ent[a - p["out_at"]]
                at = -1 if e < 0x8000 else p["win_bytes"] - 32768 + (e - 0x8000)
                w[j] = e if e < 0x8000 else (prev_w[at] if at >= 0 else 0)
            else:
                w[j] = prev_w[p["win_bytes"] - (p["out_at"] - a)]
        area[s["win_at"]:s["win_at"] + s["win_bytes"]] = w
        prev_w = bytes(w)
    return bytes(area)


def plan(gz, piece_bytes=0, window=ic.WINDOW):
    """what the speculative plan makes of the member: dict(result, rule, span, at_bit, at_out, bit, total, piece, n_pieces, cand, n_found,
    n_live, spans, windows, rows: {piece: row} of the chain's candidates).  Only the chain's candidates are decoded"""
    gz = bytes(gz)
    hdr, piece, n_pieces = pieces(gz, piece_bytes)
    cand = find(gz, piece)
    seen = {}

    def decoded(k):
        if k not in seen:
            seen[k] = speculate(gz, cand, k, piece, window)
        return seen[k]
    res = chain(gz, cand, lambda k: decoded(k)[0], piece)
    res.update(piece=piece, n_pieces=n_pieces, cand=cand, n_found=sum(1 for c in cand if c != NONE), n_live=len(res["live"]), header=hdr,
               spans=[], windows=b"", rows=dict((k, v[0]) for k, v in seen.items()))
    if res["result"] == DONE:
        spans, total = merge(res["live"])
        if max(s["out_bytes"] for s in spans) > window:
            res.update(result=NOT_PARALLEL, rule=BEYOND_WINDOW)
            return res
        res.update(spans=spans, windows=windows(spans, total, lambda k: decoded(k)[1]))
    return res


def index_of(p, gz):
    """a DONE plan as a MIGZIX01 index: the points as planned, the windows as made, the spacing field = the piece used"""
    assert p["result"] == DONE
    rows = b"".join(s["in_bit"].to_bytes(8, "little") + s["out_at"].to_bytes(8, "little") + s["win_at"].to_bytes(8, "little") +
                    s["win_bytes"].to_bytes(4, "little") + bytes(4) for s in p["spans"])
    head = xc.MAGIC + len(gz).to_bytes(8, "little") + p["total"].to_bytes(8, "little") + bytes(gz[-8:]) + p["header"].to_bytes(8, "little")
    head += len(p["spans"]).to_bytes(8, "little") + p["piece"].to_bytes(8, "little") + len(p["windows"]).to_bytes(8, "little")
    return head + rows + p["windows"]


def inflate_by_plan(gz, p):
    """the plan's spans through the indexed inflate's span decoder -> (the bytes, the first refusal (span, rule) or None)"""
    out = bytearray()
    for i, s in enumerate(p["spans"]):
        row, data = xc.decode_span(gz, s["in_bit"], s["end_bit"], p["windows"][s["win_at"]:s["win_at"] + s["win_bytes"]], s["out_bytes"])
        if row["rule"]:
            return bytes(out), (i, row["rule"])
        out += data
    return bytes(out), None


# ---- the planted member ------------------------------------------------------------------------------------------------------------------
PLANTED_PIECE = 1024
_PLANTED = None


def _m(length, distance):
    ls, _, lx = dc.length_symbol(length)
    ds, _, dx = dc.dist_symbol(distance)
    return (ls, lx, ds, dx)


def _dyn(d, tokens, bfinal=0):
    """a dynamic block around the tokens, its code lengths from their counts (Huffman, limit 15); a block without matches has HDIST 1 and
    no distance code"""
    lit, dist = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            lit[t[0]] += 1
            dist[t[2]] += 1
        else:
            lit[t] += 1
    ll, dl = dc.code_lengths(lit, 15), dc.code_lengths(dist, 15)
    hlit = max(257, max(s for s in range(286) if ll[s]) + 1)
    hdist = max([1] + [s + 1 for s in range(30) if dl[s]])
    return d.dynamic(tokens, ll[:hlit], dl[:hdist], bfinal)


def windows_trace(spans, entries_of):
    """which spans' windows hold a byte whose marker resolved to a byte that was itself a marker one span earlier: {span}"""
    seen, prev_from = set(), []
    for i in range(1, len(spans)):
        p, s = spans[i - 1], spans[i]
        ent = entries_of(p["ring"])
        from_marker = []
        for j in range(s["win_bytes"]):
            a = s["out_at"] - s["win_bytes"] + j
            if a >= p["out_at"]:
                e = ent[a - p["out_at"]]
                at = p["win_bytes"] - 32768 + (e - 0x8000)
                from_marker.append(e >= 0x8000)
                if e >= 0x8000 and at >= 0 and prev_from[at]:
                    seen.add(i)
            else:
                from_marker.append(prev_from[p["win_bytes"] - (p["out_at"] - a)])
        prev_from = from_marker
    return seen


def planted_member():
    """-> (member, data, what: name -> the output offset at which the span that shows it begins).  Written block by block with Deflate, for
    pieces of PLANTED_PIECE bytes.  Every span begins with a dynamic block -- a candidate, because stored noise of more than a piece lies in
    front of it and noise does not parse -- and ends behind stored noise; planted_facts() asserts each case on the model"""
    global _PLANTED
    if _PLANTED is not None:
        return _PLANTED
    d, what = Deflate(), {}
    seed = [400]

    def pad(n=1100):
        seed[0] += 1
        d.stored(noise(n, seed[0]))

    def span(name, tokens, fill=1100):
        what[name] = len(d.data)
        _dyn(d, tokens)
        if fill:
            pad(fill)
    pad(1500)                                            # piece 0's span: stored noise
    # candidates at all eight bit offsets: a fixed block of k nine-bit literals in front shifts the next header by k + 2 bits
    for k in range(8):
        d.fixed([200] * k + [EOB])
        span("offset_%d" % ((k + 2) % 8), [70 + k, 66, EOB])
    # matches that reach before the span: wholly in front; then one whose source is those marker entries; straddling the span's first
    # byte, plain and overlapping
    span("in_front", [_m(10, 500), _m(5, 10), 65, _m(12, 8), EOB])
    span("straddle_plain", list(noise(10, 390)) + [_m(8, 14), 67, EOB])
    span("straddle_overlap", list(noise(5, 391)) + [_m(20, 15), _m(200, 7), 68, EOB])
    # a piece with no candidate, and a span through stored blocks over several of them: 40 000 stored bytes are more than the symbol cap
    # of 32 768 would allow if they counted, and they wrap the ring
    span("stored_long", [69, EOB], 0)
    pad(40000)
    # distance 32 768 from the span's first byte: the window's first byte
    span("far", [(284, 31, 29, 8191), 70, _m(3, 32768), _m(258, 32768), EOB])
    # a dead candidate: a stored block whose payload is a complete non-final dynamic header -- byte-aligned, and once behind three bits
    for name, junk in (("dead_aligned", 0), ("dead_odd", 3)):
        t = Deflate()
        if junk:
            t.w.put(7, junk)
        _dyn(t, [65, 66, _m(4, 2), EOB])
        what[name] = len(d.data)
        seed[0] += 1
        d.stored(noise(30, seed[0]) + t.w.bytes() + noise(2200, seed[0] + 50))
        span(name + "_behind", [71, EOB])
    # a marker that resolves through two windows: A begins with markers, B (small) copies A's marker entries, C reads B's window
    a_at = len(d.data)
    span("two_windows_a", [_m(20, 3000), 72, EOB])
    span("two_windows_b", [_m(20, len(d.data) - a_at), 73, EOB])
    span("two_windows_c", [_m(30, 1100 + 21), 74, EOB])
    # spans of exactly 32 767, 32 768 and 32 769 bytes
    for size in (32767, 32768, 32769):
        span("size_%d" % size, [75, EOB], 0)
        pad(size - 1)
    # Huffman output that wraps the ring past its staging: 150 matches of 258 bytes
    span("wrap", [76] + [_m(258, 1)] * 150 + [_m(258, 32768), EOB])
    # a live span without output: a block of its end-of-block code alone, then empty stored blocks over more than a piece
    what["zero_output"] = len(d.data)
    _dyn(d, [EOB])
    for _ in range(230):
        d.stored(b"")
    d.seg = 0                                            # (the writer's segment rule is not this format's: matches reach across)
    # the last span ends on the member's last bit: a final fixed block of as many nine-bit literals as that takes
    span("last", [_m(9, 9), 77, EOB], 0)
    d.fixed([200] * (-(d.w.n + 10) % 8) + [EOB], 1)
    assert d.w.n % 8 == 0
    gz, data = d.member()
    _PLANTED = (gz, data, what)
    return _PLANTED


def planted_facts():
    """every case the planted member is there for, asserted on the model: a case that stops being hit fails here"""
    gz, data, what = planted_member()
    p = plan(gz, PLANTED_PIECE)
    assert p["result"] == DONE and inflate_by_plan(gz, p) == (data, None) and ic.zlib_inflates(gz) == data
    cand, hdr = p["cand"], p["header"]
    live = {at: (k, in_bit, out_bytes) for k, in_bit, at, out_bytes in p["live"]}
    found = [c for c in cand if c != NONE]
    starts = {s["out_at"]: s for s in p["spans"]}
    # candidate positions
    for r in range(8):
        assert live[what["offset_%d" % r]][1] % 8 == r, r
    assert NONE in cand[1:]
    for name in ("dead_aligned", "dead_odd"):
        k_behind = live[what[name + "_behind"]][0]
        dead = [k for k in range(len(cand)) if cand[k] != NONE and k not in {v[0] for v in live.values()} and cand[k] < cand[k_behind]]
        k_dead = max(dead)
        assert cand[k_dead] % 8 == (0 if name == "dead_aligned" else 3), (name, cand[k_dead] % 8)
        in_front = max(v[0] for v in live.values() if v[0] < k_dead)
        assert k_behind - in_front >= 2 and p["rows"][in_front]["end"] == cand[k_behind]    # the chain passes over the dead candidate
        row, _ = speculate(gz, cand, k_dead, PLANTED_PIECE)
        assert row["status"] == SEG_BROKEN, row                                             # it decodes noise
    # matches and markers
    ent = lambda name: speculate(gz, cand, live[what[name]][0], PLANTED_PIECE)[1]
    e = ent("in_front")
    assert e[:10] == [0x8000 + 32768 - 500 + i for i in range(10)] and e[10:15] == e[:5] and e[15] == 65
    e = ent("straddle_plain")
    assert e[10:14] == [0x8000 + 32768 - 4 + i for i in range(4)] and e[14:18] == e[:4]
    e = ent("straddle_overlap")
    assert e[5:15] == [0x8000 + 32768 - 10 + i for i in range(10)] and e[15:20] == e[:5] and e[20:25] == e[5:10]
    e = ent("far")
    assert e[0] == 0x8000 and what["far"] >= 32768 and starts[what["far"]]["win_bytes"] == 32768
    spans = p["spans"]
    i_b = next(i for i, s in enumerate(spans) if s["out_at"] == what["two_windows_b"])
    assert spans[i_b]["out_bytes"] < 32768
    assert i_b + 1 in windows_trace(spans, lambda k: speculate(gz, cand, k, PLANTED_PIECE)[1])
    # span sizes and the ring
    for size in (32767, 32768, 32769):
        assert starts[what["size_%d" % size]]["out_bytes"] == size
    assert starts[what["wrap"]]["out_bytes"] > RING + 512 + 1100 - 1 and len(ent("wrap")) > RING + 512
    # special spans
    k, in_bit, out_bytes = live[what["stored_long"]]
    nxt = min(v[0] for v in live.values() if v[0] > k)
    assert out_bytes > SYMBOLS_PER_BYTE * PLANTED_PIECE and nxt - k >= 30 and all(c == NONE for c in cand[k + 1:nxt])
    zero = [(k, b) for k, b, at, ob in p["live"] if ob == 0]
    assert len(zero) == 1 and p["n_live"] == len(spans) + 1 and all(s["in_bit"] != zero[0][1] for s in spans)     # merged: its start is no point
    assert p["rows"][p["live"][-1][0]]["bit"] == 8 * (len(gz) - 8)
    return p
