"""csrc/host_inflate_spec.h in a stand-alone program of its own (tests/host_inflate_spec/driver.cpp), compiled and run twice: plain, and
under AddressSanitizer + UBSan, in the manner of test_host_inflate_index_driver.py.  The piece rule against the model's; the chain walk
and the span table against the model's on members of every kind; and the walk on rows that CONTRADICT the candidates -- an end that is
no candidate, one that goes backwards, one behind the member, a candidate table with ~0 on the chain: each ends kInfChainInternal and
reads nothing outside the two tables.  Nothing is preloaded and nothing is loaded into python."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inflate_cases as ic  # noqa: E402
import inflate_index_cases as xc  # noqa: E402
import inflate_spec_cases as sc  # noqa: E402

CSRC = os.path.join(ROOT, "makisu_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "host_inflate_spec", "driver.cpp")
CHAIN_DONE, CHAIN_NOT_PARALLEL, CHAIN_CORRUPT, CHAIN_INTERNAL = range(4)
ENDS = {sc.DONE: CHAIN_DONE, sc.NOT_PARALLEL: CHAIN_NOT_PARALLEL, sc.INVALID: CHAIN_CORRUPT, sc.INTERNAL: CHAIN_INTERNAL}
UNWRITTEN = dict(end=sc.NONE, out_bytes=sc.NONE, status=0xFFFFFFFF, rule=0xFFFFFFFF, bit=sc.NONE)      # a row nobody wrote


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("inflate_spec_" + request.param) / "driver"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall"] + flags + ["-I", CSRC, DRIVER, "-o", str(exe)], capture_output=True, text=True)
    if p.returncode != 0:
        if flags and ("asan" in p.stderr or "ubsan" in p.stderr or "sanitize" in p.stderr):
            pytest.skip("the compiler lacks the sanitizer runtime: " + p.stderr[-300:])
        raise AssertionError(p.stderr[-3000:])

    def run(lines):
        q = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=300)
        assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, q.stderr[-3000:]
        out = q.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def _line(gz, piece, cand, rows):
    hdr, piece, n_pieces = sc.pieces(gz, piece)
    words = [len(gz), hdr, piece, n_pieces] + list(cand)
    for r in rows:
        r = r or UNWRITTEN
        words += [r["end"], r["out_bytes"], r["status"], r["rule"], r["bit"]]
    return "C " + " ".join(str(w) for w in words)


def _parse(line):
    f = [int(x) for x in line.split()[1:]]
    head = dict(zip(("end", "rule", "span", "at_bit", "at_out", "bit", "total", "n_live", "windows_bytes", "n_spans"), f[:10]))
    keys = ("in_bit", "end_bit", "out_at", "out_bytes", "win_at", "win_bytes", "ring")
    head["spans"] = [dict(zip(keys, f[10 + 7 * i:17 + 7 * i])) for i in range(head["n_spans"])]
    assert len(f) == 10 + 7 * head["n_spans"]
    return head


@pytest.fixture(scope="module")
def tables():
    """(member, piece, candidates, every candidate's row) of the planted member and two compressed ones"""
    out = []
    text = xc.dc.text(30000, 320) + xc.local_binary(30000)
    for gz, piece in ((sc.planted_member()[0], sc.PLANTED_PIECE), (ic.no_reset(text, 4096), 1024), (ic.host_leg(text, 6, 8192), 2048)):
        cand = sc.find(gz, piece)
        out.append((gz, piece, cand, [sc.speculate(gz, cand, k, piece)[0] for k in range(len(cand))]))
    return out


def test_the_piece_rule_is_the_models(driver):
    cases = [(n, hdr, piece) for n in (19, 100, 1043, 5000, 40000, 1 << 24, (1 << 24) + 19, 1 << 30, 1 << 36) for hdr in (10, 17)
             for piece in (0, 1, 1023, 1024, 4096, 32768, 65536, 16777216, 16777217)]
    out = driver(["P %d %d %d" % c for c in cases])
    for (n, hdr, piece), line in zip(cases, out):
        want = None
        if sc.PIECE_MIN <= (piece or sc.PIECE) <= sc.PIECE_MAX and n >= hdr + 9:
            used = piece or sc.PIECE
            while -(-(n - 8 - hdr) // used) > sc.MAX_PIECES:
                used *= 2
            want = "P 1 %d %d" % (used, -(-(n - 8 - hdr) // used))
        assert line == (want or "P 0"), (n, hdr, piece, line)


def test_the_walk_and_the_span_table_are_the_models(driver, tables):
    out = driver([_line(*t) for t in tables])
    for (gz, piece, cand, rows), line in zip(tables, out):
        got = _parse(line)
        want = sc.chain(gz, cand, rows, piece)
        spans, windows_bytes = sc.merge(want["live"])
        assert want["result"] == sc.DONE and got["end"] == CHAIN_DONE
        assert (got["total"], got["n_live"], got["windows_bytes"]) == (want["total"], len(want["live"]), windows_bytes)
        assert got["spans"] == spans and len(spans) >= 4


def test_rows_that_contradict_the_candidates_end_internal_and_nothing_is_read_outside(driver, tables):
    lines, want = [], []
    for gz, piece, cand, rows in tables:
        live = sc.chain(gz, cand, rows, piece)["live"]
        k1, k2, k3 = live[1][0], live[2][0], live[3][0]
        n = len(gz)

        def case(change_rows=None, change_cand=None):
            r, c = [dict(x) if x else None for x in rows], list(cand)
            for k, ch in (change_rows or {}).items():
                r[k].update(ch)
            for k, v in (change_cand or {}).items():
                c[k] = v
            lines.append(_line(gz, piece, c, r))
            want.append(sc.chain(gz, c, r, piece)["result"])
        case({k1: dict(end=rows[k1]["end"] + 1)})                                 # an end that is no candidate
        case({k2: dict(end=cand[k1])})                                            # an end that goes backwards
        case({k2: dict(end=cand[k2])})                                            # ... that does not advance
        case({k1: dict(end=8 * n + 8)})                                           # an end behind the member
        case({k1: dict(end=8 * (n - 8))})                                         # ... where only the trailer may lie
        case({k1: dict(end=2 ** 63 + 5)})                                         # ... far behind it: a piece number no table has
        case({k1: dict(end=sc.NONE)})
        case(None, {k2: sc.NONE})                                                 # a candidate table with ~0 on the chain
        case(None, {0: sc.NONE})
        case(None, {0: cand[0] + 1})
        case({k3: dict(status=7)})                                                # a status that is none
        case({k3: dict(UNWRITTEN)})                                               # a row nobody wrote
        case({k1: dict(out_bytes=2 ** 64 - 2)})                                   # output that wraps the sum
    out = driver(lines)
    assert all(w == sc.INTERNAL for w in want)
    for line in out:
        got = _parse(line)
        assert got["end"] == CHAIN_INTERNAL and got["spans"] == [], line[:200]


def test_broken_and_too_long_rows_on_the_chain_are_verdicts_dead_ones_are_not_read(driver, tables):
    gz, piece, cand, rows = tables[1]
    live = sc.chain(gz, cand, rows, piece)["live"]
    on_chain = {k for k, _, _, _ in live}
    dead = [k for k in range(len(cand)) if k not in on_chain]
    k2 = live[2][0]
    lines, want = [], []
    for change in (dict(status=ic.SEG_BROKEN, rule=ic.SYMBOL, end=0), dict(status=ic.SEG_TOO_LONG, rule=sc.SYMBOL_CAP, end=0),
                   dict(status=ic.SEG_TOO_LONG, rule=ic.BEYOND_WINDOW, end=0)):
        r = [dict(x) if x else None for x in rows]
        r[k2].update(change)
        for k in dead:                                                           # whatever a dead row says
            r[k] = dict(UNWRITTEN)
        lines.append(_line(gz, piece, cand, r))
        want.append(sc.chain(gz, cand, r, piece))
    for line, w in zip(driver(lines), want):
        got = _parse(line)
        assert (got["end"], got["rule"], got["span"], got["at_bit"], got["at_out"], got["bit"]) == (ENDS[w["result"]], w["rule"], w["span"], w["at_bit"],
                                                                                                     w["at_out"], w["bit"])
        assert got["span"] == 2 and got["n_live"] == 3 and got["spans"] == []
