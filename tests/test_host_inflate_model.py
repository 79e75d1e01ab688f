"""The device inflate's model (tests/inflate_cases.py) against zlib, without a GPU: the same bytes on every input of the GPU tests
where zlib accepts, a refusal or NOT_PARALLEL where zlib refuses; every rule pinned by a stream written by hand; the planted inputs
each hold a dead candidate; a wrong model -- one that does not stop at an empty stored block -- differs; the new prototypes and
the refusals that need no device."""
import ctypes as C
import gzip
import os
import re
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_cases as dc  # noqa: E402
import inflate_cases as ic  # noqa: E402

HEADER = os.path.join(ROOT, "include", "makisu_mi.h")


def _done(gz, data, window=ic.WINDOW):
    p = ic.plan(gz, window)
    assert p["result"] == ic.DONE and p["out"] == data == ic.zlib_inflates(gz), (p["result"], p["rule"])
    assert sum(p["sizes"]) == len(data) and p["n_segments"] == len(p["sizes"]) <= p["n_candidates"]
    return p


def test_the_device_legs_form():
    for n in (0, 1, 13, 65535, 65536, 65537):
        for make in (lambda n: dc.text(n, 51), lambda n: dc.random_bytes(n, 52), lambda n: dc.symbols(n, 4, 53)):
            data = make(n)
            _done(dc.gzip_member(data), data)
    p = _done(dc.gzip_member(dc.text(65537, 51)), dc.text(65537, 51))
    assert p["sizes"][0] == 65536 and p["n_segments"] >= 2
    assert _done(dc.gzip_member(dc.random_bytes(65537, 52)), dc.random_bytes(65537, 52))["n_segments"] == 1      # stored pieces: no marker
    for data in (dc.no_match(), dc.one_distance()):
        _done(dc.gzip_member(data), data)


def test_the_host_legs_form_and_every_block_type():
    mixed = dc.text(100000, 54) + bytes(30000) + dc.random_bytes(40000, 55) + dc.symbols(60000, 7, 56)
    for level in (1, 6, 9):
        p = _done(ic.host_leg(mixed, level, 1 << 16), mixed)
        assert p["sizes"][:3] == [65536] * 3 and p["sizes"][-1] == 0 and p["n_segments"] == 5
    x = dc.text(140000, 63)
    for gz, data in ((ic.one_stream(x[:30000], 6, zlib.Z_FIXED), x[:30000]), (ic.one_stream(x, 0), x),
                     (ic.one_stream(x[:30000], 6, zlib.Z_HUFFMAN_ONLY), x[:30000]), (ic.one_stream(bytes(100000), 6, zlib.Z_RLE), bytes(100000)),
                     (ic.one_stream(ic.repeat_at(32768), 9), ic.repeat_at(32768)), ic.source_at_start(), (gzip.compress(x), x), ic.two_piece()):
        _done(gz, data)
    assert _done(gzip.compress(x), x)["n_candidates"] == 1
    # the edges: a match whose source is the segment's first byte is in source_at_start's stream.  One at distance 32 768 is NOT in
    # repeat_at's: zlib's longest distance is 32 768 - 262, the repeat is literals there and the stream is shorter only because the bytes
    # below 199 code in under eight bits (planted_streams' far_first and far_second hold that match: test_host_inflate_planted.py)
    far = ic.one_stream(ic.repeat_at(32768), 9)
    assert len(far) < len(ic.repeat_at(32768)) - 8 and not any(l[0] == "far" for l in ic.trace(far, 10)[2])
    gz, data = ic.source_at_start()
    assert [r["status"] for _, r in ic.rows(gz)] == [ic.SEG_ENDS, ic.SEG_ENDS, ic.SEG_FINAL] and len(gz) < len(data)


def test_every_planted_input_holds_a_dead_candidate():
    for name, (gz, data) in ic.planted_cases().items():
        p = _done(gz, data)
        assert p["n_candidates"] > p["n_segments"] == 1, name
        rows = ic.rows(gz)
        live = ic.gzip_header(gz)
        dead = [(c, r) for c, r in rows if c != live]
        assert dead and gz[dead[0][0] - 4:dead[0][0]] == ic.MARKER
        if name == "block_end":                          # it sits on a true block boundary and decodes cleanly to END: still dead
            assert dead[0][1]["status"] == ic.SEG_FINAL and dead[0][1]["end"] == len(gz) - 8
        if name == "fname":
            assert dead[0][0] < live


def test_what_is_not_parallel():
    data = dc.text(140000, 64)
    gz = ic.no_reset(data)
    p = ic.plan(gz)
    assert ic.zlib_inflates(gz) == data and (p["result"], p["rule"], p["n_segments"], p["at_out"]) == (ic.NOT_PARALLEL, ic.DISTANCE, 2, 65536)
    z = bytes(1 << 20)
    assert _done(gzip.compress(z), z, 1 << 20)["n_rounds"] == 1
    p = ic.plan(gzip.compress(z + b"\x00"), 1 << 20)
    assert (p["result"], p["rule"]) == (ic.NOT_PARALLEL, ic.BEYOND_WINDOW)
    a = gzip.compress(dc.text(3000, 65))
    p = ic.plan(a + a)
    assert (p["result"], p["rule"], p["n_segments"]) == (ic.NOT_PARALLEL, 0, 1) and ic.zlib_inflates(a + a) is None
    assert ic.plan(a + b"\x00")["result"] == ic.NOT_PARALLEL             # trailing bytes


def test_every_rule_by_a_stream_written_by_hand():
    streams = ic.rule_streams()
    assert sorted(streams) == list(range(1, 11))
    for rule, gz in streams.items():
        row, _ = ic.decode_segment(gz, 10)
        assert (row["status"], row["rule"]) == (ic.SEG_BROKEN, rule) and len(gz) < 40, (rule, row)
        p = ic.plan(gz)
        assert p["result"] == (ic.NOT_PARALLEL if rule == ic.DISTANCE else ic.INVALID) and p["rule"] == rule and p["at_in"] == 10
        assert ic.zlib_inflates(gz) is None, rule
    row, out = ic.decode_segment(gzip.compress(b"abcdef"), 10, limit=5)
    assert (row["status"], row["rule"], out) == (ic.SEG_TOO_LONG, ic.BEYOND_WINDOW, b"abcde")
    # the one incomplete code that is allowed: a single distance code of length 1 -- zlib's own streams of one distance use it
    one = ic.one_stream(b"a" * 600, 9)
    assert _done(one, b"a" * 600)


def test_the_corruption_cases_agree_with_zlib():
    base, data = ic.two_piece()
    assert 1400 < len(base) < 2100 and ic.plan(base)["n_segments"] == 3
    import numpy as np
    rng = np.random.default_rng(66)
    accepted = refused = 0
    for b in sorted(set(int(x) for x in rng.integers(0, 8 * len(base), 256)) | set(range(32, 64)) | set(range(72, 80))):     # ... and MTIME, OS
        m = base[:b >> 3] + bytes((base[b >> 3] ^ 1 << (b & 7),)) + base[(b >> 3) + 1:]
        p, z = ic.plan(m), ic.zlib_inflates(m)
        if p["result"] == ic.DONE:
            assert z == p["out"]
            accepted += 1
        else:
            refused += 1
        if z is None:
            assert p["result"] != ic.DONE
    for k in (1, 9, 10, 18, 19, 200, len(base) - 9, len(base) - 1):
        assert ic.plan(base[:k])["result"] == ic.INVALID and ic.zlib_inflates(base[:k]) is None
    assert accepted > 0 and refused > 200


def test_a_model_that_reads_on_behind_an_empty_stored_block_differs():
    """the wrong decoder finds ONE segment where there are five, and on a blob whose matches cross the flushes it accepts what the
    rule hands to zlib"""
    data = dc.text(140000, 64)
    gz = ic.host_leg(data, 6, 1 << 16)
    right, wrong = ic.plan(gz), ic.plan(gz, stop_at_empty=False)
    assert right["result"] == wrong["result"] == ic.DONE and right["out"] == wrong["out"] == data
    assert right["n_segments"] == 4 and wrong["n_segments"] == 1 and right["sizes"] != wrong["sizes"]
    cross = ic.no_reset(data)
    assert ic.plan(cross)["result"] == ic.NOT_PARALLEL and ic.plan(cross, stop_at_empty=False)["result"] == ic.DONE


def test_the_rounds_for_a_window():
    assert ic.rounds([65536] * 80 + [0], 1 << 20) == 5 and ic.rounds([65536] * 80 + [0]) == 1
    assert ic.rounds([1 << 20, 1], 1 << 20) == 2 and ic.rounds([0], 1 << 20) == 1 and ic.rounds([600000, 600000, 600000], 1 << 20) == 3


def test_the_guard_scenarios_inputs():
    for gz in (ic.cut_in_last_segment(), ic.ends_on_last_bit()):
        p = ic.plan(gz)
        assert len(gz) % 256 == 0 and (p["result"], p["rule"]) == (ic.INVALID, ic.INPUT_ENDS) and ic.zlib_inflates(gz) is None
    gz = ic.ends_on_last_bit()
    row, _ = ic.decode_segment(gz, ic.gzip_header(gz))
    assert row["status"] == ic.SEG_FINAL and row["bit"] == 8 * len(gz)  # the final code's last bit is the member's last


def test_the_new_prototypes_are_exported_and_tagged(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("mi_inflate_buffer", "mi_tar_inflate_ctx"):
        assert re.search(r"^MI_BLOCK\s[^\n;]*\b%s\s*\(" % name, src, flags=re.M), name
        assert hasattr(engine_lib, name)
    assert re.search(r"^#define MI_INFLATE_DONE 0$", src, flags=re.M) and re.search(r"^#define MI_INFLATE_NOT_PARALLEL 1$", src, flags=re.M)
    assert re.search(r"^#define MI_ABI_VERSION 6$", src, flags=re.M)
    import makisu_amd as M
    assert (M.INFLATE_DONE, M.INFLATE_NOT_PARALLEL) == (0, 1) and C.sizeof(M.InflateInfo) == 7 * 8 + 4 * 4 + 2 * 8
    host = open(os.path.join(ROOT, "makisu_amd", "csrc", "host_inflate.h")).read()
    assert "hip" not in re.sub(r"//.*", "", host).lower()                # no HIP header: a stand-alone program includes it
    for k, name in enumerate(("kInfBlockType", "kInfStoredLen", "kInfTooManyCodes", "kInfLengthCode", "kInfRepeat", "kInfNoEndOfBlock", "kInfCode",
                              "kInfSymbol", "kInfInputEnds", "kInfDistance", "kInfWindow"), 1):
        assert re.search(r"\b%s = %d," % (name, k), host), name          # the model's numbers


def test_the_refusals_that_need_no_gpu(engine_lib, tmp_path):
    INVALID = -1
    fake_ctx = C.c_void_p(8)                                             # never touched: every call below is refused before it looks
    n, buf = C.c_uint64(), (C.c_uint8 * 64)()
    assert engine_lib.mi_inflate_buffer(None, buf, 20, buf, 64, C.byref(n), None) == INVALID
    assert engine_lib.mi_inflate_buffer(fake_ctx, buf, 20, buf, 64, None, None) == INVALID
    assert engine_lib.mi_inflate_buffer(fake_ctx, None, 20, buf, 64, C.byref(n), None) == INVALID
    assert engine_lib.mi_inflate_buffer(fake_ctx, buf, 20, None, 64, C.byref(n), None) == INVALID
    err = C.create_string_buffer(256)
    assert engine_lib.mi_tar_inflate_ctx(None, b"/nonexistent", None, None, None, None, None, err, 256) == INVALID
    assert engine_lib.mi_tar_inflate_ctx(fake_ctx, None, None, None, None, None, None, err, 256) == INVALID
    missing = str(tmp_path / "missing.gz").encode()
    assert engine_lib.mi_tar_inflate_ctx(fake_ctx, missing, None, None, None, None, None, err, 256) == -5 and b"open " in err.value       # MI_ERR_IO
