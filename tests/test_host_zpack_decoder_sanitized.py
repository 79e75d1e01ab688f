"""csrc/host_lz4.h under AddressSanitizer and UBSan, in a stand-alone program of its own: the decoder that parses bytes from
elsewhere refuses every row of the malformed table and 200 random byte strings posing as streams, and never reads or writes
outside the buffers it was given -- which are heap allocations of EXACTLY the stored and the chunk's size, so one byte too far
is a report.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import zpack_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "makisu_amd", "csrc")

MAIN = r"""
#include "host_lz4.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// stdin: lines of "<length> <hex of the stored form, - for none>"; stdout: the decoder's rule per line, then the output's hex
int main() {
    static char line[1 << 20];
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long n = 0;
        char* hex = nullptr;
        n = strtoull(line, &hex, 10);
        while (*hex == ' ') ++hex;
        size_t len = 0;
        while (hex[len] && hex[len] != '\n') ++len;
        const size_t stored = hex[0] == '-' ? 0 : len / 2;
        uint8_t* src = (uint8_t*)malloc(stored ? stored : 1);      // exactly as long as the stream (malloc(0) may be NULL)
        uint8_t* dst = (uint8_t*)malloc(n ? n : 1);
        for (size_t i = 0; i < stored; ++i) {
            unsigned v = 0;
            sscanf(hex + 2 * i, "%2x", &v);
            src[i] = (uint8_t)v;
        }
        memset(dst, 0, n ? n : 1);
        const uint32_t rule = mi_host::lz4_block_decode(src, stored, dst, n);
        printf("%u ", rule);
        if (rule == 0)
            for (size_t i = 0; i < n; ++i) printf("%02x", dst[i]);
        printf("\n");
        free(src);
        free(dst);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def decoder(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    tmp = tmp_path_factory.mktemp("lz4_san")
    src = tmp / "main.cpp"
    src.write_text(MAIN)
    exe = tmp / "decode"
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    if p.returncode != 0:
        if "asan" in p.stderr or "ubsan" in p.stderr or "sanitize" in p.stderr:
            pytest.skip("the compiler lacks the sanitizer runtime: " + p.stderr[-300:])
        raise AssertionError(p.stderr[-3000:])
    return str(exe)


def _run(exe, rows):
    text = "".join("%d %s\n" % (n, bytes(s).hex() or "-") for n, s in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    out = [ln.split(" ", 1) for ln in p.stdout.splitlines()]
    assert len(out) == len(rows)
    return [(int(r), bytes.fromhex(h.strip())) for r, h in out]


def test_the_malformed_table_is_refused_without_a_sanitizer_report(decoder):
    rows = [(specs[0]["length"], specs[0]["stream"]) for _, specs, _ in zc.malformed_table()[:7]]
    rows.append((34, zc.GOOD_STREAM))
    got = _run(decoder, rows)
    assert [r for r, _ in got[:7]] == [1, 2, 3, 4, 5, 6, 4]                   # host_lz4.h's rules, in the table's order
    assert got[7] == (0, zc.GOOD_PLAIN)


def test_the_models_blocks_decode_and_random_strings_are_refused_or_decode_inside_their_bounds(decoder):
    rng = np.random.default_rng(83)
    design = open(os.path.join(ROOT, "DESIGN.md"), "rb").read()
    good = [design[:8192], bytes(65536), b"abc" * 1000, b"z" * 13, zc.text_like(4095, 3)]
    rows = [(len(c), zc.compress_chunk(c)) for c in good]
    assert all(len(s) < n for n, s in rows)
    # 200 seeded random byte strings posing as streams, for lengths around what they could produce; and the good streams cut
    # short and with a byte changed
    for i in range(200):
        s = rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8)
        if i % 3 == 0 and len(s):
            s[0] = rng.choice([0x0F, 0xF0, 0xFF, 0x10, 0x44])                  # tokens that reach the extension paths at once
        if i % 5 == 0 and len(s) > 4:
            s[1:4] = 255
        rows.append((int(rng.integers(0, 600)), s.tobytes()))
    for n, s in rows[:5]:
        rows.append((n, s[:len(s) // 2]))
        hurt = bytearray(s)
        hurt[len(s) // 3] ^= 0x80
        rows.append((n, bytes(hurt)))
        rows.append((n - 1, s))
        rows.append((n + 1, s))
    got = _run(decoder, rows)
    for (n, s), (rule, out), c in zip(rows[:5], got[:5], good):
        assert rule == 0 and out == c
    refused = 0
    for (n, s), (rule, out) in zip(rows[5:], got[5:]):
        try:
            want = zc.lz4_block_decode(s, n)                                   # the independent decoder agrees on what is a block
        except ValueError:
            want = None
        assert (rule == 0) == (want is not None), (n, s.hex(), rule)
        if rule == 0:
            assert out == want
        else:
            refused += 1
    assert refused >= 190
