"""csrc/host_tarcache.h in a stand-alone program of its own (tests/host_tarcache/driver.cpp), compiled and run twice:
plain, and under AddressSanitizer + UBSan.  Lookups at, before and behind every held block, ranges that straddle a held and an unheld
block, meta bodies of 0, 1, 1 024 and 1 025 bytes, an empty cache, a cursor that is asked backwards -- against a model of a dozen
lines.  Nothing is preloaded and nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "makisu_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "host_tarcache", "driver.cpp")
H, B = 1, 2


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("tarcache_" + request.param) / "driver"
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


def _new(marked):
    return "N %d %s" % (len(marked), " ".join("%d %d" % (b, k) for b, k in marked))


def _held(marked, off, n):
    """the model: held iff n > 0 and every block the range touches is marked; the kind is the first block's"""
    kinds = dict(marked)
    if n == 0:
        return (0, 0)
    touched = range(off // 512, (off + n - 1) // 512 + 1)
    return (1, kinds[touched[0]]) if all(j in kinds for j in touched) else (0, 0)


def _ask(driver, marked, queries):
    got = driver([_new(marked)] + ["L %d %d" % q for q in queries])
    assert got[0] == [len(marked)]
    for (off, n), (held, kind, same, cur) in zip(queries, got[1:]):
        assert (held, kind if held else 0) == _held(marked, off, n), (marked, off, n, held, kind)
        assert same == held and 0 <= cur <= len(marked), (off, n, same, cur)


MARKED = [(0, H), (3, H), (4, B), (5, B), (9, H), (10, H | B), (11, B), (12, B), (40, H), (1000, H), (1001, B), (1 << 33, H)]


def test_lookups_at_before_and_behind_every_held_block(driver):
    queries = []
    for b, _ in MARKED:
        for j in (b - 1, b, b + 1):
            if j >= 0:
                queries += [(512 * j, 512), (512 * j, 1), (512 * j + 511, 1), (512 * j + 100, 412)]
    _ask(driver, MARKED, queries)                                          # ascending: the cursor walks
    _ask(driver, MARKED, queries[::-1])                                    # descending: every lookup is asked backwards
    _ask(driver, MARKED, queries[::7] + queries[3::5] + queries[::-3])     # jumps both ways


def test_ranges_that_straddle_held_and_unheld_blocks(driver):
    queries = [(512 * 3, 1536), (512 * 3, 1537), (512 * 3, 2048), (512 * 2, 1024), (512 * 2 + 511, 2), (512 * 5 + 511, 2), (512 * 9, 2048),
               (512 * 9, 2049), (512 * 8 + 1, 1023), (512 * 12, 513), (512 * 40, 512), (512 * 40, 513), (512 * 39 + 511, 513),
               (512 * 1000, 1024), (512 * 1000 + 7, 1017), (512 * 1000, 1025), (512 * 1001, 512), (512 * (1 << 33), 512), (512 * (1 << 33), 513),
               (512 * (1 << 33) - 1, 2), (512 * ((1 << 33) + 5), 512), ((1 << 64) - 512, 512), ((1 << 64) - 512, 511), (0, 0), (700, 0)]
    queries = [q for q in queries if q[0] + q[1] < 1 << 64] + [((1 << 64) - 512, 512)]     # (the last one wraps: refused)
    got = driver([_new(MARKED)] + ["L %d %d" % q for q in queries])
    for (off, n), (held, kind, same, _) in zip(queries[:-1], got[1:-1]):
        assert (held, kind if held else 0) == _held(MARKED, off, n) and same == held, (off, n, held, kind)
    assert got[-1][0] == 0


def test_meta_bodies_of_0_1_1024_and_1025_bytes(driver):
    """a meta header at block 20 whose two body blocks travelled: the parser asks for the body's `size` bytes at the data offset"""
    marked = [(20, H), (21, B), (22, B), (23 + 4, H)]
    data = 512 * 21
    got = driver([_new(marked)] + ["L %d %d" % (data, n) for n in (0, 1, 512, 513, 1024, 1025)])
    assert [g[0] for g in got[1:]] == [0, 1, 1, 1, 1, 0]                    # size 0 is never asked for; 1 025 bytes need a fetch
    assert all(g[2] == g[0] for g in got[1:])
    # ... and at the archive's end only one body block exists
    got = driver([_new([(20, H), (21, B)]), "L %d 512" % data, "L %d 513" % data])
    assert [g[0] for g in got[1:]] == [1, 0]


def test_an_empty_cache_holds_nothing(driver):
    got = driver([_new([]), "L 0 512", "L 512 1", "L 0 0", "L %d 512" % (512 << 40)])
    assert [g[0] for g in got[1:]] == [0, 0, 0, 0]
    got = driver(["L 0 512"])                                              # no cache was ever made
    assert got == [[0, 0, 0, 0]]


def test_a_cursor_that_is_asked_backwards_and_far_ahead(driver):
    marked = [(2 * k, H) for k in range(500)]
    order = [998, 0, 996, 2, 500, 498, 502, 10, 10, 12, 14, 400, 16, 999, 997, 1, 0]
    _ask(driver, marked, [(512 * j, 512) for j in order])
    got = driver([_new(marked)] + ["L %d 512" % (512 * j) for j in order])
    assert [g[3] for g in got[1:]] == [(j + 1) // 2 for j in order]          # the cursor stands at the first marked block >= the one asked for


def test_what_a_fetch_asks_for(driver):
    T = 512 * 100 + 7
    cases = [((0, 512, T), (0, 1024)), ((512 * 5, 512, T), (512 * 5, 1024)), ((512 * 5, 1025, T), (512 * 5, 1536)),
             ((512 * 5 + 3, 10, T), (512 * 5, 1024)), ((512 * 99, 512, T), (512 * 99, 519)), ((512 * 98, 512, T), (512 * 98, 1024)),
             ((512 * 100, 7, T), (512 * 100, 7)), ((512 * 99, 512, 512 * 100), (512 * 99, 512)), ((512 * 4, 1025, 512 * 100), (512 * 4, 1536))]
    got = driver(["F %d %d %d" % c for c, _ in cases])
    assert [tuple(g) for g in got] == [w for _, w in cases]
