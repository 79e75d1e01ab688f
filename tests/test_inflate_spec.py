"""The speculative device inflate's model against zlib and against the C checker, without a GPU: the model's plan -- the
candidates, the chain, the merged spans, the windows resolved from markers -- put through inflate_index_cases.decode_span gives zlib's
bytes on members of every kind; index_of(plan) passes mi_inflate_index_check; the planted member reaches every case it is there for;
and the finder's contract holds on hand-made headers, one per header rule broken."""
import os
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import deflate_cases as dc  # noqa: E402
import inflate_cases as ic  # noqa: E402
import inflate_index_cases as xc  # noqa: E402
import inflate_spec_cases as sc  # noqa: E402


def _members():
    out = dict((name, (gz, data, 4096)) for name, (gz, data) in xc.members().items())        # levels 1, 6, 9, Z_FIXED, no_reset, host_leg, stored_only
    out["planted_index"] = out.pop("planted")[:2] + (1024,)                                  # (the indexed inflate's planted member)
    plain = dc.text(140000, 360) + dc.random_bytes(70000, 361)
    out["device_leg"] = (dc.gzip_member(plain), plain, 2048)
    gz, data, _ = sc.planted_member()
    out["planted"] = (gz, data, sc.PLANTED_PIECE)
    return out


@pytest.mark.parametrize("name", ["one_stream_1", "one_stream_6", "one_stream_9", "one_stream_fixed", "no_reset", "host_leg", "stored_only",
                                  "planted_index", "device_leg", "planted"])
def test_the_plans_spans_give_zlibs_bytes_and_its_index_passes_the_checker(name):
    gz, data, piece = _members()[name]
    assert ic.zlib_inflates(gz) == data
    p = sc.plan(gz, piece)
    assert p["result"] == sc.DONE and p["total"] == len(data), (p["result"], p["rule"])
    assert sc.inflate_by_plan(gz, p) == (data, None)
    ix = sc.index_of(p, gz)
    assert M.inflate_index_check(ix, gz)[0] == 0
    h = xc.parse(ix)
    assert (h["spacing"], h["n_points"], h["out_bytes"]) == (p["piece"], len(p["spans"]), len(data))
    if name in ("no_reset", "host_leg", "one_stream_6", "planted"):
        assert len(p["spans"]) >= 4, len(p["spans"])
    # every window is the output in front of its point, whatever route its bytes took
    for s in p["spans"][1:]:
        assert p["windows"][s["win_at"]:s["win_at"] + s["win_bytes"]] == data[s["out_at"] - s["win_bytes"]:s["out_at"]], s["out_at"]


def test_the_planted_member_reaches_every_case_it_is_there_for():
    p = sc.planted_facts()
    assert p["n_found"] < p["n_pieces"] and p["n_live"] < p["n_found"]                        # pieces without a candidate, and dead candidates


def test_a_stream_of_fixed_blocks_and_two_members_are_not_parallel():
    fixed = ic.one_stream(dc.text(1 << 20, 370), 6, zlib.Z_FIXED)
    p = sc.plan(fixed, 1024)
    assert (p["result"], p["rule"], p["n_found"], p["at_bit"], p["at_out"]) == (sc.NOT_PARALLEL, sc.SYMBOL_CAP, 1, 80, 0)
    one = ic.one_stream(dc.text(30000, 371), 6)
    p = sc.plan(one + one, 1024)
    assert (p["result"], p["rule"]) == (sc.NOT_PARALLEL, 0)
    p = sc.plan(ic.one_stream(bytes(3 << 20), 6), 0, 1 << 20)
    assert (p["result"], p["rule"]) == (sc.NOT_PARALLEL, ic.BEYOND_WINDOW)


def _header(**broken):
    """a non-final dynamic block header that parses, or the same with ONE rule broken, as the bits behind BFINAL: -> ic._Bits"""
    lit = [0] * 65 + [2, 2] + [0] * 189 + [2, 2]                                             # 65, 66, 256, 257: two bits each
    dist = [1]
    if broken.get("code"):
        lit[67] = 2                                                                           # five codes of two bits: over-subscribed
    if broken.get("no_eob"):
        lit[256], lit[258 - 1] = 0, 2
        lit = lit[:257] + [2, 2]                                                              # 256 has no code; 257 and 258 keep the code complete
    run = ic.length_run(lit + dist)
    cnt = [0] * 19
    for s, _ in run:
        cnt[s] += 1
    cl_lens = dc.code_lengths(cnt, 7)
    hlit, hdist = len(lit), len(dist)
    if broken.get("length_code"):
        k = next(s for s in range(19) if cl_lens[s] > 1)
        cl_lens[k] -= 1                                                                       # over-subscribed
    w = ic._Bits().put(broken.get("bfinal", 0), 1).put(broken.get("btype", 2), 2)
    w.put(30 if broken.get("too_many") else hlit - 257, 5).put(hdist - 1, 5)
    need = max(dc.CL_ORDER.index(s) + 1 for s in range(19) if cl_lens[s])
    w.put(max(need, 4) - 4, 4)
    for s in dc.CL_ORDER[:max(need, 4)]:
        w.put(cl_lens[s], 3)
    cl = dc.canonical_codes(cl_lens)
    if broken.get("repeat"):
        run = run[:-1] + [(18, 127)]                                                          # a run that passes HLIT + HDIST
        assert cl_lens[18]
    for s, x in (run[:len(run) // 2] if broken.get("input_ends") else run):
        w.put(cl[s], cl_lens[s]).put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
    return w


@pytest.mark.parametrize("broken,rule", [({}, None), (dict(bfinal=1), -1), (dict(btype=1), -1), (dict(too_many=1), ic.TOO_MANY_CODES),
                                         (dict(length_code=1), ic.LENGTH_CODE), (dict(repeat=1), ic.REPEAT), (dict(no_eob=1), ic.NO_END_OF_BLOCK),
                                         (dict(code=1), ic.CODE), (dict(input_ends=1), ic.INPUT_ENDS)])
def test_the_finders_contract_on_hand_made_headers(broken, rule):
    """a member whose second piece holds stored noise and, at a byte boundary and at an odd bit, the header: it is the piece's candidate
    exactly when it parses"""
    head = _header(**broken).bytes()
    for shift in (0, 3):
        bits = ic._Bits().put(7, shift) if shift else ic._Bits()
        w = _header(**broken)
        bits.put(w.acc, w.n)
        payload = ic.noise(1100, 380) + bits.bytes()
        if not broken.get("input_ends"):
            payload += ic.noise(60, 381)
        gz, _ = ic.Deflate().stored(payload, 1).member()
        if broken.get("input_ends"):
            gz = gz[:-8]                                                                      # the header runs into the member's end (no trailer: the
            gz = gz + b"\xff" * 0                                                             # finder's word on a member cut there)
            gz = gz + bytes(0)
        at = 8 * (10 + 5 + 1100) + shift
        assert sc.parses(gz, at) == rule, (broken, shift, sc.parses(gz, at))
        if not broken.get("input_ends"):
            cand = sc.find(gz, 1024)
            assert len(cand) == 2 and cand[1] == (at if rule is None else sc.NONE), (broken, shift, cand)
    assert head
