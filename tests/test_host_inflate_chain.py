"""csrc/host_inflate.h in a stand-alone program of its own (tests/host_inflate/chain_driver.cpp), compiled and run twice: plain, and under
AddressSanitizer + UBSan.  The gzip header with every optional field, cut at every length, against the model's parse; the walk
along the chain over rows made by hand.  Nothing is preloaded and nothing is loaded into python."""
import os
import shutil
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inflate_cases as ic  # noqa: E402

CSRC = os.path.join(ROOT, "makisu_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "host_inflate", "chain_driver.cpp")
DONE, NOT_PARALLEL, CORRUPT, INTERNAL = range(4)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("inflate_chain_" + request.param) / "chain_driver"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall"] + flags + ["-I", CSRC, DRIVER, "-o", str(exe)], capture_output=True, text=True)
    if p.returncode != 0:
        if flags and ("asan" in p.stderr or "ubsan" in p.stderr or "sanitize" in p.stderr):
            pytest.skip("the compiler lacks the sanitizer runtime: " + p.stderr[-300:])
        raise AssertionError(p.stderr[-3000:])

    def run(lines):
        q = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, q.stderr[-3000:]
        out = [[int(x) for x in ln.split()[1:]] for ln in q.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def _header(flg, extra=b"", name=b"", comment=b"", hcrc=True):
    h = bytes((0x1f, 0x8b, 8, flg, 1, 2, 3, 4, 0, 3))
    if flg & 4:
        h += len(extra).to_bytes(2, "little") + extra
    if flg & 8:
        h += name + b"\x00"
    if flg & 16:
        h += comment + b"\x00"
    if flg & 2:
        h += (zlib.crc32(h) & 0xFFFF).to_bytes(2, "little") if hcrc else b"\x00\x00"
    return h


def test_the_header_with_every_optional_field_cut_at_every_length(driver):
    heads = [_header(flg, b"xtra-field", b"name.tar", b"a comment") for flg in range(32)]
    heads += [_header(31, b"", b"", b""), _header(4, bytes(300)), _header(1)]
    # a wrong FHCRC, the reserved flag bits, another method, a wrong magic
    bad = [_header(2, hcrc=False), _header(0x20), _header(0x80), b"\x1f\x8b\x07" + heads[0][3:], b"\x1f\x8c" + heads[0][2:], b"\x1e\x8b" + heads[0][2:]]
    heads += bad
    cases = []
    for h in heads:
        full = h + b"\x03\x00" + bytes(8)
        cases += [full[:k] for k in range(len(full) + 1)]
    got = driver(["H " + (c.hex() or "-") for c in cases])
    accepted = 0
    for c, (ok, length) in zip(cases, got):
        want = ic.gzip_header(c)
        assert (ok, length) == ((1, want) if want is not None else (0, 0)), (c.hex(), ok, length, want)
        accepted += ok
    assert accepted > 100 and len(cases) - accepted > 100
    assert ic.gzip_header(heads[31] + b"\x03\x00") == len(heads[31]) == 10 + 2 + 10 + 9 + 10 + 2      # every field at once
    for h in bad:
        assert ic.gzip_header(h + b"\x03\x00" + bytes(8)) is None, h.hex()


def _chain(n, first, window, cand, rows):
    return "C %d %d %d %d %s %s" % (n, first, window, len(cand), " ".join(map(str, cand)), " ".join(" ".join(map(str, r)) for r in rows))


ENDS, FINAL, BROKEN, TOO_LONG = ic.SEG_ENDS, ic.SEG_FINAL, ic.SEG_BROKEN, ic.SEG_TOO_LONG


def test_the_walk_over_rows_made_by_hand(driver):
    n = 1000                                             # END must lie at 992
    lines = [
        # a dead candidate between two live ones: its row says END at the right place, and nobody asks
        _chain(n, 10, 1 << 20, [10, 300, 500], [(500, 7000, ENDS, 0, 4000), (992, 1, FINAL, 0, 7900), (992, 9000, FINAL, 0, 7930)]),
        # ... and dead rows that are broken, too long or nonsense do not matter either
        _chain(n, 10, 1 << 20, [4, 10, 300, 500, 700], [(0, 0, BROKEN, 1, 40), (500, 7000, ENDS, 0, 4000), (0, 5, TOO_LONG, 11, 0), (992, 9000, FINAL, 0, 7930),
                                                        (2, 99, 77, 99, 1)]),
        # the chain misses n - 8: before it (more members, trailing bytes) and behind it (no room for the trailer)
        _chain(n, 10, 1 << 20, [10, 500], [(500, 7000, ENDS, 0, 4000), (990, 9000, FINAL, 0, 7915)]),
        _chain(n, 10, 1 << 20, [10, 500], [(500, 7000, ENDS, 0, 4000), (993, 9000, FINAL, 0, 7940)]),
        _chain(n, 10, 1 << 20, [10, 500], [(996, 7000, ENDS, 0, 7968), (0, 0, BROKEN, 3, 0)]),
        # a row whose end is not a candidate, one that does not move forward, one behind the member; zero candidates; no first
        _chain(n, 10, 1 << 20, [10, 500], [(499, 7000, ENDS, 0, 3992), (992, 9000, FINAL, 0, 7930)]),
        _chain(n, 10, 1 << 20, [10, 500], [(10, 0, ENDS, 0, 80), (992, 9000, FINAL, 0, 7930)]),
        _chain(n, 10, 1 << 20, [10, 500], [(500, 7000, ENDS, 0, 4000), (1001, 9000, FINAL, 0, 8008)]),
        _chain(n, 10, 1 << 20, [], []),
        _chain(n, 10, 1 << 20, [500], [(992, 9000, FINAL, 0, 7930)]),
        # live segments that break a rule: the distance rule and the window hand the blob to zlib, anything else is corruption
        _chain(n, 10, 1 << 20, [10, 500], [(500, 7000, ENDS, 0, 4000), (0, 12, BROKEN, ic.DISTANCE, 4100)]),
        _chain(n, 10, 1 << 20, [10, 500], [(500, 7000, ENDS, 0, 4000), (0, 1 << 20, TOO_LONG, ic.BEYOND_WINDOW, 4100)]),
        _chain(n, 10, 1 << 20, [10, 500], [(500, 7000, ENDS, 0, 4000), (0, 12, BROKEN, ic.SYMBOL, 4100)]),
        _chain(n, 10, 1 << 20, [10, 500], [(500, 7000, ENDS, 0, 4000), (0, 12, 9, 0, 4100)]),
        # rounds: 4 segments of 400 000 bytes and an empty one under a window of 1 MiB, and one segment that fills it
        _chain(n, 10, 1 << 20, [10, 100, 200, 300, 400], [(100, 400000, ENDS, 0, 0), (200, 400000, ENDS, 0, 0), (300, 400000, ENDS, 0, 0),
                                                          (400, 400000, ENDS, 0, 0), (992, 0, FINAL, 0, 0)]),
        _chain(n, 10, 1 << 20, [10, 100], [(100, 1 << 20, ENDS, 0, 0), (992, 1, FINAL, 0, 0)]),
        # a member too short to hold a trailer at all
        _chain(6, 2, 1 << 20, [2], [(4, 0, FINAL, 0, 30)]),
    ]
    got = driver(lines)
    assert got[0] == [DONE, 0, 500, 7000, 16000, 2, 1, 10, 500]
    assert got[1] == [DONE, 0, 500, 7000, 16000, 2, 1, 10, 500]
    assert got[2][:6] == [NOT_PARALLEL, 0, 500, 7000, 16000, 2]
    assert got[3][:6] == [CORRUPT, ic.INPUT_ENDS, 500, 7000, 16000, 2]
    assert got[4][:6] == [CORRUPT, ic.INPUT_ENDS, 10, 0, 7000, 1]
    assert [g[0] for g in got[5:10]] == [INTERNAL] * 5
    assert got[10][:6] == [NOT_PARALLEL, ic.DISTANCE, 500, 7000, 7000, 2]
    assert got[11][:6] == [NOT_PARALLEL, ic.BEYOND_WINDOW, 500, 7000, 7000, 2]
    assert got[12][:6] == [CORRUPT, ic.SYMBOL, 500, 7000, 7000, 2]
    assert got[13][0] == INTERNAL
    assert got[14][:7] == [DONE, 0, 400, 1600000, 1600000, 5, 2] and ic.rounds([400000] * 4 + [0], 1 << 20) == 2
    assert got[15][:7] == [DONE, 0, 100, 1 << 20, (1 << 20) + 1, 2, 2] and ic.rounds([1 << 20, 1], 1 << 20) == 2
    assert got[16][0] == CORRUPT
