"""csrc/host_inflate_index.h in a stand-alone program of its own (tests/host_inflate_index/driver.cpp), compiled and run twice: plain, and
under AddressSanitizer + UBSan, in the manner of test_host_inflate_chain.py.  The builder over members of every kind (its index against
the model's, its SHA-256 against hashlib's), over members cut at many lengths and with flipped bits; the checker over indexes that
are truncated at every length near a boundary and over indexes with one bit flipped -- whatever it is given, it answers with a
number and reads nothing outside the buffer.  Nothing is preloaded and nothing is loaded into python."""
import hashlib
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inflate_index_cases as xc  # noqa: E402

CSRC = os.path.join(ROOT, "makisu_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "host_inflate_index", "driver.cpp")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("inflate_index_" + request.param) / "driver"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall"] + flags + ["-I", CSRC, DRIVER, "-o", str(exe), "-lz"], capture_output=True, text=True)
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


def _hex(b):
    return bytes(b).hex() or "-"


@pytest.fixture(scope="module")
def small():
    """the planted member and two small compressed ones: (member, data)"""
    gz, data, _ = xc.planted_member()
    text = xc.dc.text(30000, 320) + xc.dc.random_bytes(500, 321)
    return [(gz, data), (xc.no_reset(text, 4096), text), (xc.host_leg(text, 6, 8192), text)]


def test_the_builder_gives_the_models_index_and_hashlibs_digest(driver, small):
    lines, want = [], []
    for gz, data in small:
        for spacing in (1, 4096, 0):
            lines.append("B %d %s" % (spacing, _hex(gz)))
            want.append((xc.index(gz, spacing), data))
    for line, (ix, data) in zip(driver(lines), want):
        f = line.split()
        assert f[:2] == ["B", "1"], line[:200]
        assert int(f[2]) == xc.parse(ix)["n_points"] and int(f[4]) == len(data)
        assert f[5] == hashlib.sha256(data).hexdigest()
        assert bytes.fromhex(f[6]) == ix


def test_the_builder_on_cut_and_flipped_members_refuses_or_builds_and_reads_nothing_else(driver, small):
    gz, data = small[1]
    cases = [gz[:k] for k in list(range(0, 40)) + list(range(len(gz) - 20, len(gz)))] + [gz[:len(gz) // 2]]
    for at in list(range(0, 24)) + list(range(100, len(gz), 97)):
        cases.append(gz[:at] + bytes((gz[at] ^ (1 << (at % 8)),)) + gz[at + 1:])
    out = driver(["B 1 " + _hex(c) for c in cases])
    built = 0
    for c, line in zip(cases, out):
        f = line.split()
        if f[1] == "1":                                  # what it builds it has checked: CRC-32 and ISIZE hold (a flip in MTIME, XFL or OS is no damage)
            built += 1
            assert int(f[4]) == len(data) and f[5] == hashlib.sha256(data).hexdigest(), line[:200]
    assert 0 < built <= 8, built                         # MTIME (4 bytes), XFL, OS -- and nothing that touches the stream or the trailer


def test_the_checker_on_truncated_and_flipped_indexes(driver, small):
    gz, _ = small[0]
    ix = xc.index(gz, 1)
    h = xc.parse(ix)
    rows_end = 64 + 32 * h["n_points"]
    cuts = sorted(set(list(range(0, 130)) + list(range(rows_end - 40, rows_end + 40)) + list(range(len(ix) - 40, len(ix)))))
    lines = ["K %s %s" % (_hex(ix[:k]), _hex(gz)) for k in cuts]
    flips = [(at, bit) for at in range(0, rows_end) for bit in (0, 7)]
    lines += ["K %s %s" % (_hex(ix[:at] + bytes((ix[at] ^ (1 << bit),)) + ix[at + 1:]), _hex(gz)) for at, bit in flips]
    lines += ["K %s -" % _hex(ix), "K %s %s" % (_hex(ix), _hex(gz)), "K - -"]
    out = [int(l.split()[1]) for l in driver(lines)]
    for k, r in zip(cuts, out):
        assert r in (xc.R_MAGIC, xc.R_SIZES) if k < len(ix) else r == 0, (k, r)
    seen = set()
    for (at, bit), r in zip(flips, out[len(cuts):]):
        seen.add(r)                                      # (a number whatever the flip: what no rule of the checker holds -- a point moved by a
                                                         # bit, the spacing -- the spans and the CRC-32 hold at the end of a run)
    seen.discard(0)
    assert seen >= {xc.R_MAGIC, xc.R_SIZES, xc.R_FIRST, xc.R_IN_BIT, xc.R_OUT_AT, xc.R_WIN_BYTES, xc.R_WINDOW, xc.R_MEMBER}, seen
    assert out[-3:] == [0, 0, xc.R_MAGIC]
