"""csrc/host_huff.h under AddressSanitizer and UBSan, in a stand-alone program of its own (the pattern of
test_host_zpack_decoder_sanitized.py): the decoder that parses entropy forms from elsewhere refuses every row of the malformed
table with the model's rule, decodes the planted forms, and takes seeded damage to good forms without reading or writing outside
the buffers it was given -- heap allocations of EXACTLY the stored and the chunk's size, so one byte too far is a report.
Nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import zentropy_cases as ze
import zpack_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "makisu_amd", "csrc")

MAIN = r"""
#include "host_huff.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// stdin: lines of "<length> <hex of the stored form>"; stdout: zform_decode's rule per line, then the output's hex
int main() {
    static char line[1 << 20];
    while (fgets(line, sizeof line, stdin)) {
        char* hex = nullptr;
        const unsigned long long n = strtoull(line, &hex, 10);
        while (*hex == ' ') ++hex;
        size_t len = 0;
        while (hex[len] && hex[len] != '\n') ++len;
        const size_t stored = len / 2;
        uint8_t* src = (uint8_t*)malloc(stored ? stored : 1);      // exactly as long as the form
        uint8_t* dst = (uint8_t*)malloc(n ? n : 1);
        uint8_t* inner = (uint8_t*)malloc(n ? n : 1);              // what mi_zpack_check gives the decoder: `length` bytes
        for (size_t i = 0; i < stored; ++i) {
            unsigned v = 0;
            sscanf(hex + 2 * i, "%2x", &v);
            src[i] = (uint8_t)v;
        }
        memset(dst, 0, n ? n : 1);
        const uint32_t rule = mi_host::zform_decode(src, stored, dst, n, inner);
        printf("%u ", rule);
        if (rule == 0)
            for (size_t i = 0; i < n; ++i) printf("%02x", dst[i]);
        printf("\n");
        free(src);
        free(dst);
        free(inner);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def decoder(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("needs g++")
    tmp = tmp_path_factory.mktemp("huff_san")
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
    text = "".join("%d %s\n" % (n, bytes(s).hex()) for n, s in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    out = [ln.split(" ", 1) for ln in p.stdout.splitlines()]
    assert len(out) == len(rows)
    return [(int(r), bytes.fromhex(h.strip())) for r, h in out]


def test_the_malformed_table_is_refused_with_the_models_rule_and_without_a_report(decoder):
    table = [(name, specs[0], rule) for name, specs, _, rule in ze.malformed_table() if rule != ze.RULE_PAD]     # (the pad is the caller's)
    got = _run(decoder, [(s["length"], s["stream"]) for _, s, _ in table])
    assert [(name, r) for (name, _, _), (r, _) in zip(table, got)] == [(name, rule) for name, _, rule in table]


def test_the_planted_forms_decode_and_damaged_ones_stay_inside_their_bounds(decoder):
    rng = np.random.default_rng(293)
    cases = [(name, c) for name, c in ze.planted_chunks_h() if len(c) <= 8192]
    good = []
    for level in (1, 2):
        good += [(c, ze.compress_chunk_h(c, level)) for _, c in cases]
    good = [(c, s) for c, s in good if ze.is_form_h(s, len(c))]
    assert {s[1] for _, s in good} == {1, 2} and len(good) >= 8
    good.append((ze.GOOD_PLAIN, ze.GOOD_H))
    good.append((zc.text_like(3000, 5), ze.huff_form(zc.compress_chunk(zc.text_like(3000, 5)), 1, 64)))
    good.append((zc.text_like(3000, 5), ze.huff_form(zc.compress_chunk(zc.text_like(3000, 5)), 1, 1)))
    rows = [(len(c), s) for c, s in good]
    for c, s in good:                                              # cut short, a byte changed in every region, lengths one off
        n = len(c)
        rows.append((n, s[:len(s) // 2]))
        rows.append((n, s[:ze.HEAD + 10]))
        rows.append((n - 1, s))
        rows.append((n + 1, s))
        for _ in range(12):
            hurt = bytearray(s)
            at = int(rng.integers(1, len(s)))
            hurt[at] ^= 1 << int(rng.integers(0, 8))
            rows.append((n, bytes(hurt)))
        hurt = bytearray(s)
        hurt[4:8] = (0xFFFFFFF0).to_bytes(4, "little")            # an inner length far beyond the chunk
        rows.append((n, bytes(hurt)))
    got = _run(decoder, rows)
    for (c, s), (rule, out) in zip(good, got):
        assert rule == 0 and out == c
    refused = 0
    for (n, s), (rule, out) in zip(rows[len(good):], got[len(good):]):
        want_rule, want = ze.chunk_rule(s, n) if len(s) < n else (None, None)
        if want_rule is None:                                      # stored >= length is not a form: mi_zpack_check never decodes it
            continue
        assert rule == want_rule, (n, len(s), rule, want_rule)
        if rule == 0:
            assert out == want
        else:
            refused += 1
    assert refused >= 100
