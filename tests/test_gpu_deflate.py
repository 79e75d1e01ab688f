"""GPU tests of the device deflate coder (mi_deflate_buffer): byte for byte against the model of deflate_cases.py
and through zlib's inflate, on the smallest shapes where the kernels can go wrong -- the lengths around a step, a piece and its
two stored blocks, several pieces; zeros (distance 1, the split lengths), text, random bytes, 2 and 16 symbols; the planted
repeats at 32 768 and 32 769; the pieces without a match and with one distance symbol; the pieces whose codes the model reports
as clamped; a (D) form one byte under and one byte over its (S) form; a source at every alignment mod 16.  The counts of
mi_deflate_info and the CRC are held against the model's and zlib's.  The length-limiting device function is also driven alone
through tests/kernel_probe.  Bit for bit: there are no tolerances.

The host source's alignment is what mi_deflate_buffer's caller controls: a window's bytes are copied into pinned memory and lie
on the device at offset 0, every piece at a multiple of 65 536.  The kernels themselves read with unaligned loads
(mi_deflate_wave.h BOUNDS)."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (before the engine: its HIP runtime serves the library and the probe too)
except ImportError:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import deflate_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

PROBE_DIR = os.path.join(ROOT, "tests", "kernel_probe")
PROBE = os.path.join(PROBE_DIR, "libmi_deflate_probe.so")


@pytest.fixture(scope="module")
def engine():
    with M.Engine(device=0) as e:
        yield e


_MODEL = {}


def _model(data):
    """the model's blob and counts, computed once per input"""
    key = (len(data), zlib.crc32(data))
    if key not in _MODEL:
        info = {}
        _MODEL[key] = (dc.deflate_blob(data, info), info)
    return _MODEL[key]


def _check(engine, data):
    want, winfo = _model(data)
    blob, crc, info = engine.deflate_buffer(data)
    assert blob == want, (len(blob), len(want), next((i for i in range(min(len(blob), len(want))) if blob[i] != want[i]), None))
    assert crc == (zlib.crc32(data) & 0xFFFFFFFF)
    for k in ("n_pieces", "n_dynamic", "n_stored", "in_bytes", "out_bytes"):
        assert info[k] == (winfo[k] if data else 0), (k, info, winfo)
    if data:
        assert dc.inflate(blob) == data and info["ms_device"] > 0
    return info


CONTENTS = {"zeros": lambda n: bytes(n), "text": dc.text, "random": dc.random_bytes, "two": lambda n: dc.symbols(n, 2),
            "sixteen": lambda n: dc.symbols(n, 16)}


@pytest.mark.parametrize("n", dc.LENGTHS)
@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_every_length_and_content_is_the_models_blob(engine, content, n):
    info = _check(engine, CONTENTS[content](n))
    if content == "random" and n >= 64:                                  # all pieces stored, a full piece as two blocks
        assert info["n_dynamic"] == 0 and info["out_bytes"] == sum(dc.stored_size(min(65536, n - at)) for at in range(0, n, 65536))
    if content == "zeros" and n >= 63:
        assert info["n_stored"] == (1 if n % 65536 in (1, 5) and n > 65536 else 0)     # (a last piece of 1 or 5 bytes stays stored)


@pytest.mark.parametrize("n", range(255, 268))
def test_zeros_around_the_split_lengths(engine, n):
    """a literal and one match of n - 1 at distance 1: 258 | 256 + 3 | 257 + 3 | 258 + 3 | 258 + 4 ..."""
    assert dc.parse(bytes(n)) == [0] + [(p, 1) for p in dc.split_length(n - 1)]
    _check(engine, bytes(n))


def test_a_repeat_at_32768_is_taken_and_one_at_32769_is_not(engine):
    assert (16, 32768) in dc.parse(dc.planted(32768))
    assert not any(isinstance(it, tuple) and it[1] > 1 for it in dc.parse(dc.planted(32769)))
    _check(engine, dc.planted(32768))
    _check(engine, dc.planted(32769))


def test_no_distance_code_and_a_single_distance_symbol(engine):
    plan = dc.piece_plan(dc.no_match())
    assert plan["dynamic"] and plan["hdist"] == 1 and plan["d_lens"][0] == 0
    assert _check(engine, dc.no_match())["n_dynamic"] == 1
    plan = dc.piece_plan(dc.one_distance())
    assert plan["dynamic"] and plan["n_dist_symbols"] == 1 and sum(plan["d_lens"]) == 1
    assert _check(engine, dc.one_distance())["n_dynamic"] == 1


def test_the_pieces_whose_codes_are_clamped(engine):
    seed, piece = dc.find_ll_clamped(dc.LL_CLAMP_SEED)
    rep = {}
    plan = dc.piece_plan(piece, rep)
    assert seed == dc.LL_CLAMP_SEED and rep["ll_free_depth"] > 15 and max(plan["ll_lens"]) == 15 and plan["dynamic"]
    assert _check(engine, piece)["n_dynamic"] == 1
    seed, piece = dc.find_cl_clamped(dc.CL_CLAMP_SEED)
    plan = dc.piece_plan(piece, rep)
    assert seed == dc.CL_CLAMP_SEED and rep["cl_free_depth"] > 7 and max(plan["cl_lens"]) == 7 and plan["dynamic"]
    assert _check(engine, piece)["n_dynamic"] == 1


@pytest.mark.parametrize("delta", sorted(dc.NEAR_SEEDS))
def test_a_dynamic_form_one_byte_under_and_over_the_stored_form(engine, delta):
    seed, piece = dc.find_near_stored(delta, dc.NEAR_SEEDS[delta])
    plan = dc.piece_plan(piece)
    assert seed == dc.NEAR_SEEDS[delta] and plan["d_size"] - plan["s_size"] == delta
    info = _check(engine, piece)
    assert info["n_dynamic"] == (1 if delta < 0 else 0) and info["out_bytes"] == (plan["d_size"] if delta < 0 else plan["s_size"])


def test_a_source_at_every_alignment_mod_16(engine):
    lib = M.load_library()
    data = dc.text(65536 + 700, 11)
    want, _ = _model(data)
    pool = np.zeros(len(data) + 64, dtype=np.uint8)
    base = (-pool.ctypes.data) % 16
    cap = lib.mi_deflate_bound(len(data))
    out = np.zeros(cap, dtype=np.uint8)
    for a in range(16):
        pool[base + a:base + a + len(data)] = np.frombuffer(data, dtype=np.uint8)
        assert (pool.ctypes.data + base + a) % 16 == a
        n, crc = C.c_uint64(), C.c_uint32()
        assert lib.mi_deflate_buffer(engine._h, pool.ctypes.data + base + a, len(data), out.ctypes.data, cap, C.byref(n), C.byref(crc), None) == 0
        assert out[:n.value].tobytes() == want and crc.value == zlib.crc32(data)


def test_windows_do_not_show_and_the_refusals_leave_the_ctx_usable(engine, monkeypatch):
    lib = M.load_library()
    data = dc.text(2 * 1048576 + 65536 + 9, 12)                          # three windows of 1 MiB: two in flight, then the rest
    monkeypatch.setenv("MI_GZIP_DEVICE_WINDOW_MB", "1")
    a = engine.deflate_buffer(data)
    monkeypatch.delenv("MI_GZIP_DEVICE_WINDOW_MB")
    b = engine.deflate_buffer(data)
    assert a[0] == b[0] and a[1] == b[1] == zlib.crc32(data) and dc.inflate(a[0]) == data
    assert a[2]["n_pieces"] == b[2]["n_pieces"] == 34 and a[2]["out_bytes"] == len(a[0])
    for at in (0, 1048576, 2 * 1048576 + 65536):                         # (the model on the first, a middle and the last piece)
        assert dc.piece_form(data[at:at + 65536]) in a[0]
    n, crc, buf = C.c_uint64(7), C.c_uint32(), (C.c_uint8 * 128)()
    assert lib.mi_deflate_buffer(engine._h, buf, 100, buf, lib.mi_deflate_bound(100) - 1, C.byref(n), C.byref(crc), None) == -7 and n.value == 0
    assert "need room" in lib.mi_last_error(engine._h).decode()
    assert lib.mi_deflate_buffer(engine._h, None, 100, buf, 128, C.byref(n), C.byref(crc), None) == -1
    assert lib.mi_deflate_buffer(engine._h, buf, 100, None, 128, C.byref(n), C.byref(crc), None) == -1
    assert lib.mi_deflate_buffer(engine._h, buf, 100, buf, 128, None, C.byref(crc), None) == -1
    assert lib.mi_deflate_buffer(engine._h, None, 0, buf, 0, C.byref(n), None, None) == 0 and n.value == 0
    _check(engine, dc.text(1000))


# ---- the length-limiting device function alone ------------------------------------------------------------------------------------------
def _build_probe():
    src = os.path.join(PROBE_DIR, "deflate_probe.cpp")
    lib = os.path.join(ROOT, "makisu_amd", "libmakisu_mi.so")
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall",
                               src, "-o", PROBE, "-L", os.path.dirname(lib), "-lmakisu_mi",
                               "-Wl,-rpath,$ORIGIN/../../makisu_amd", "-Wl,--no-undefined"])
    return PROBE


@pytest.fixture(scope="module")
def probe(engine):
    lib = C.CDLL(_build_probe())
    lib.probe_deflate_code_lengths.restype = C.c_int
    lib.probe_deflate_code_lengths.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]

    def run(counts, limit):
        d_counts = torch.from_numpy(np.asarray(counts, dtype=np.uint32).view(np.int32)).cuda()
        d_lens = torch.full((len(counts) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        assert lib.probe_deflate_code_lengths(d_counts.data_ptr(), len(counts), limit, d_lens.data_ptr()) == 0
        out = d_lens.cpu().numpy()
        assert (out[len(counts):] == 0xA5).all()                         # nothing behind the row was written
        return [int(x) for x in out[:len(counts)]]
    return run


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def test_the_device_code_lengths_on_given_counts(probe):
    cases = []
    ll = [0] * dc.N_LITLEN
    for k, c in enumerate(_fib(24)[1:]):
        ll[3 * k + 1] = c
    ll[dc.EOB] = 1
    cases.append((ll, 15))                                               # free depth 23
    cases.append((_fib(12) + [0] * 7, 7))                                # a code-length alphabet, free depth 11
    cases += [(_fib(n), 7) for n in (2, 3, 9, 10, 19)]
    cases += [([0, 0, 9, 0], 15), ([5, 0, 3], 15), ([1] * 286, 15), ([1] * 19, 7), ([1, 1, 2, 4], 15), ([7] * 30, 15), ([0] * 30, 15)]
    rng = np.random.default_rng(21)
    for _ in range(12):
        n = int(rng.integers(2, 287))
        cases.append(([int(x) for x in rng.integers(0, 3, n) * rng.integers(1, 60000, n)], 15))
    for counts, limit in cases:
        rep = {}
        want = dc.code_lengths(counts, limit, rep)
        assert probe(counts, limit) == want, (counts, limit)
        if sum(1 for c in counts if c) >= 2:
            assert dc.kraft_sum(want, limit) == 1 << limit and max(want) <= limit
    rep = {}
    dc.code_lengths(cases[0][0], 15, rep)
    assert rep["free_depth"] > 15
    dc.code_lengths(cases[1][0], 7, rep)
    assert rep["free_depth"] > 7
