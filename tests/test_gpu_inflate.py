"""GPU tests of the device inflate (mi_inflate_buffer): byte for byte against zlib and the model of inflate_cases.py --
the device leg's and the host leg's forms, every block type and the match edges, planted false candidates, the blobs that are not
parallel, corruption against zlib, rounds and alignment, one scenario under MI_GUARD_ALLOC=1 in a process of its own (no positive
control: a deliberate fault has no place here), and the table builder alone through tests/kernel_probe."""
import ctypes as C
import gzip
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
import inflate_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu

PROBE_DIR = os.path.join(ROOT, "tests", "kernel_probe")
PROBE = os.path.join(PROBE_DIR, "libmi_inflate_probe.so")
MODEL_UP_TO = 300000                                    # output bytes the pure-Python model is asked to decode


@pytest.fixture(scope="module")
def engine():
    with M.Engine(device=0) as e:
        yield e


def _check(engine, gz, data, window=ic.WINDOW):
    """DONE with the bytes zlib gives; the counts are the model's where the model is asked"""
    out, info = engine.inflate_buffer(gz)
    assert info["verdict"] == M.INFLATE_DONE and info["fell_back"] == 0, info
    assert out == data, (len(out), len(data), next((i for i in range(min(len(out), len(data))) if out[i] != data[i]), None))
    assert ic.zlib_inflates(gz) == data and (info["in_bytes"], info["out_bytes"]) == (len(gz), len(data))
    if len(data) <= MODEL_UP_TO:
        p = ic.plan(gz, window)
        assert p["result"] == ic.DONE and p["out"] == data
        assert (info["n_candidates"], info["n_segments"], info["n_rounds"]) == (p["n_candidates"], p["n_segments"], p["n_rounds"]), (info, p)
    return info


def _device_leg(engine, data):
    blob, _, _ = engine.deflate_buffer(data)             # (test_gpu_deflate.py holds it against the model's blob)
    return ic.member(blob + b"\x03\x00", data, bytes((0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 255)))


# ---- 1. the device leg's forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["text", "random", "symbols"])
def test_the_device_legs_members_of_every_length(engine, content):
    make = {"text": lambda n: dc.text(n, 51), "random": lambda n: dc.random_bytes(n, 52), "symbols": lambda n: dc.symbols(n, 4, 53)}[content]
    for n in dc.LENGTHS:
        data = make(n)
        info = _check(engine, _device_leg(engine, data), data)
        if content == "random":                          # stored pieces end in no marker: one segment, one wave
            assert info["n_segments"] == 1
        elif n >= 65536:
            assert info["n_segments"] > n // 65536          # every full dynamic piece ends its segment


def test_the_device_legs_edge_pieces(engine):
    for data in (dc.no_match(), dc.one_distance(), dc.one_distance(65536 + 700)):
        gz = _device_leg(engine, data)
        assert gz == dc.gzip_member(data)
        _check(engine, gz, data)


# ---- 2. the host leg's forms ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    return dc.text(100000, 54) + bytes(30000) + dc.random_bytes(40000, 55) + dc.symbols(60000, 7, 56)


@pytest.mark.parametrize("level", [1, 6, 9])
def test_the_host_legs_blocks_of_64k(engine, mixed, level):
    info = _check(engine, ic.host_leg(mixed, level, 1 << 16), mixed)
    assert info["n_segments"] >= 3


def test_the_host_legs_block_of_1m(engine):
    data = b"".join(dc.text(65536, 57 + k % 3) for k in range(16)) + dc.text(4000, 60)
    info = _check(engine, ic.host_leg(data, 6, 1 << 20), data)
    assert info["n_segments"] == 3 <= info["n_candidates"]               # 1 MiB, 4 000 bytes, 03 00


def test_a_real_layer_of_the_host_leg_with_a_block_of_random_bytes(engine, tmp_path):
    """a layer from mi_layer at the default level whose tar is a little above 2 MiB and whose first 1 MiB block is random bytes: the stored
    path of the host leg's sink"""
    root = tmp_path / "root"
    root.mkdir()
    (root / "a_random.bin").write_bytes(dc.random_bytes((1 << 20) + 70000, 61))
    (root / "b_text.txt").write_bytes(b"".join(dc.text(65536, 62 + k % 2) for k in range(15)))
    for p in (root / "a_random.bin", root / "b_text.txt", root):
        os.utime(p, (1700000000, 1700000000))
    ents = M.tree_walk(str(root), str(root), (), M.TREE_SCAN, full=True)
    blobs = {}
    for name, level in (("layer.tar", M.GZIP_OFF), ("layer.gz", M.GZIP_DEFAULT)):
        fd = os.open(str(tmp_path / name), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        l = M.Layer(out_fd=fd, gzip_level=level)
        try:
            for e in ents:
                l.add(e, os.path.join(str(root), e["relpath"].lstrip("/")) if e["kind"] == 1 else None)
            l.finish()
        finally:
            l.close()
            os.close(fd)
        blobs[name] = (tmp_path / name).read_bytes()
    tar = blobs["layer.tar"]
    assert 2 << 20 < len(tar) < (2 << 20) + 100000
    info = _check(engine, blobs["layer.gz"], tar)
    assert info["n_segments"] >= 2


# ---- 3. every block type and the match edges -------------------------------------------------------------------------------------------
def test_every_block_type_and_the_match_edges(engine):
    x = dc.text(200000, 63)
    for gz, data in ((ic.one_stream(x[:30000], 6, zlib.Z_FIXED), x[:30000]),
                     (ic.one_stream(x[:140000], 0), x[:140000]),                          # stored blocks of 65 535
                     (ic.one_stream(x[:30000], 6, zlib.Z_HUFFMAN_ONLY), x[:30000]),
                     (ic.one_stream(bytes(100000), 6, zlib.Z_RLE), bytes(100000)),         # distance 1, length 258
                     # 32 KB of literals and a few short matches: zlib's longest distance is 32 768 - 262, so the repeat 32 768 behind is
                     # written as literals -- distance 32 768 itself is test_gpu_inflate_planted.py's (far_first, far_second)
                     (ic.one_stream(ic.repeat_at(32768), 9), ic.repeat_at(32768)),
                     ic.source_at_start()):
        _check(engine, gz, data)
    info = _check(engine, gzip.compress(x), x)                                            # no marker: one wave
    assert (info["n_candidates"], info["n_segments"]) == (1, 1)


# ---- 4. planted false candidates -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["middle", "block_end", "straddle", "fname"])
def test_planted_false_candidates_are_dead(engine, name):
    gz, data = ic.planted_cases()[name]
    info = _check(engine, gz, data)
    assert info["n_candidates"] > info["n_segments"] == 1


# ---- 5. not parallel -------------------------------------------------------------------------------------------------------------------
def _not_parallel(engine, gz, window=ic.WINDOW):
    out, info = engine.inflate_buffer(gz)
    p = ic.plan(gz, window)
    assert out == b"" and info["verdict"] == M.INFLATE_NOT_PARALLEL and info["out_bytes"] == 0 and p["result"] == ic.NOT_PARALLEL, (info, p)
    assert (info["rule"], info["at_in"], info["at_out"], info["n_segments"]) == (p["rule"], p["at_in"], p["at_out"], p["n_segments"]), (info, p)
    return info


def test_one_stream_flushed_without_reset_is_not_parallel(engine):
    data = dc.text(140000, 64)
    gz = ic.no_reset(data)
    assert ic.zlib_inflates(gz) == data
    info = _not_parallel(engine, gz)
    assert info["rule"] == ic.DISTANCE and info["n_segments"] == 2 and info["at_out"] == 65536 and gz[info["at_in"] - 4:info["at_in"]] == ic.MARKER
    n = C.c_uint64(77)
    buf = np.zeros(len(data), dtype=np.uint8)
    src = np.frombuffer(gz, dtype=np.uint8)
    assert engine._lib.mi_inflate_buffer(engine._h, src.ctypes.data, len(gz), buf.ctypes.data, len(data), C.byref(n), None) == 0 and n.value == 0


def test_a_segment_may_inflate_to_a_window_and_no_more(engine, monkeypatch):
    monkeypatch.setenv("MI_INFLATE_WINDOW_MB", "1")
    z = bytes(1 << 20)
    out, info = engine.inflate_buffer(gzip.compress(z))
    assert out == z and info["verdict"] == M.INFLATE_DONE and info["n_rounds"] == 1
    info = _not_parallel(engine, gzip.compress(z + b"\x00"), 1 << 20)
    assert info["rule"] == ic.BEYOND_WINDOW and info["n_segments"] == 1


def test_two_members_are_not_parallel(engine):
    a = gzip.compress(dc.text(3000, 65))
    info = _not_parallel(engine, a + a)
    assert info["rule"] == 0 and info["n_segments"] == 1


# ---- 6. corruption against zlib --------------------------------------------------------------------------------------------------------
def _mutants():
    base, _ = ic.two_piece()
    n = len(base)
    starts = [c for c, _ in ic.rows(base)]                                # the two pieces and the final block
    assert len(starts) == 3
    rng = np.random.default_rng(66)
    flips = set(int(b) for b in rng.integers(0, 8 * n, 256))
    for s in starts[:2]:
        flips.update(range(8 * s, 8 * s + 43))                            # the block header and the first 40 bits of the dynamic header
    for s in starts[1:]:
        flips.update(range(8 * (s - 6), 8 * s))                           # the empty stored block that ends a piece: header bits, pad, LEN, NLEN
    flips.update(range(8 * starts[2], 8 * starts[2] + 16))                # the final 03 00
    out = [("bit %d" % b, base[:b >> 3] + bytes((base[b >> 3] ^ 1 << (b & 7),)) + base[(b >> 3) + 1:]) for b in sorted(flips)]
    out += [("cut %d" % k, base[:k]) for k in (2, 1, 9, 10, 11, 17, 18, 19, 200, starts[1] - 1, starts[1], starts[1] + 1, n - 9, n - 8, n - 4, n - 1)]
    return base, out


def test_corruption_against_zlib(engine):
    base, mutants = _mutants()
    good = ic.zlib_inflates(base)
    accepted = refused = 0
    for name, m in mutants:
        z = ic.zlib_inflates(m)
        try:
            out, info = engine.inflate_buffer(m)
        except M.MiError as e:
            assert e.code == -1, (name, e)
            assert "input offset" in str(e) or "header" in str(e), (name, e)         # a segment is named, unless there is none yet
            again, _ = engine.inflate_buffer(base)                                   # the ctx stays usable
            assert again == good, name
            refused += 1
            continue
        if info["verdict"] == M.INFLATE_DONE:
            assert z is not None and out == z, name                                  # what the device accepts zlib accepts, same bytes
            accepted += 1
        else:
            assert out == b""
            refused += 1
        if z is None:
            assert info["verdict"] != M.INFLATE_DONE, name
    assert accepted > 0 and refused > 0, (accepted, refused)


def test_the_trailer_and_the_header_fields_nobody_checks(engine):
    base, data = ic.two_piece()
    n = len(base)
    for at in (n - 8, n - 5, n - 4, n - 1):                                          # CRC and ISIZE
        m = base[:at] + bytes((base[at] ^ 0x10,)) + base[at + 1:]
        assert ic.zlib_inflates(m) is None and ic.plan(m)["result"] == ic.INVALID
        with pytest.raises(M.MiError) as ei:
            engine.inflate_buffer(m)
        assert ei.value.code == -1 and "CRC-32" in str(ei.value) and "input offset" in str(ei.value)
    for at in (4, 5, 6, 7, 9):                                                       # MTIME and OS: both sides accept
        m = base[:at] + bytes((base[at] ^ 0x21,)) + base[at + 1:]
        assert ic.zlib_inflates(m) == data
        _check(engine, m, data)


def test_every_rule_by_a_stream_written_by_hand(engine):
    """the device's rule numbers are the model's"""
    good, data = ic.two_piece()
    for rule, gz in ic.rule_streams().items():
        assert ic.zlib_inflates(gz) is None
        if rule == ic.DISTANCE:
            info = _not_parallel(engine, gz)
            assert (info["rule"], info["at_in"], info["at_out"]) == (rule, 10, 0)
            continue
        with pytest.raises(M.MiError) as ei:
            engine.inflate_buffer(gz)
        assert ei.value.code == -1 and "input offset 10 (output offset 0) breaks rule %d at" % rule in str(ei.value), (rule, ei.value)
        assert engine.inflate_buffer(good)[0] == data


# ---- 7. rounds and alignment -----------------------------------------------------------------------------------------------------------
def test_several_rounds_through_both_slots(engine, monkeypatch):
    texts = [dc.text(65536, 67 + k) for k in range(4)]
    data = b"".join(texts[k % 4] for k in range(80))                                 # 5 MiB in 64 KiB pieces
    gz = ic.host_leg(data, 6, 1 << 16)
    out, whole = engine.inflate_buffer(gz)
    assert out == data and whole["n_rounds"] == 1 and whole["n_segments"] == 81
    monkeypatch.setenv("MI_INFLATE_WINDOW_MB", "1")
    out, info = engine.inflate_buffer(gz)
    assert out == data and info["verdict"] == M.INFLATE_DONE
    assert info["n_rounds"] == ic.rounds([65536] * 80 + [0], 1 << 20) == 5 and info["n_segments"] == 81


def test_the_source_at_every_alignment_and_the_capacity(engine):
    gz, data = ic.two_piece()
    lib = engine._lib
    pool = np.zeros(len(gz) + 64, dtype=np.uint8)
    base = (-pool.ctypes.data) % 16
    out = np.zeros(len(data) + 16, dtype=np.uint8)
    n = C.c_uint64()
    for a in range(16):
        pool[base + a:base + a + len(gz)] = np.frombuffer(gz, dtype=np.uint8)
        out[:] = 0xA5
        assert lib.mi_inflate_buffer(engine._h, pool.ctypes.data + base + a, len(gz), out.ctypes.data, len(data), C.byref(n), None) == 0
        assert n.value == len(data) and out[:len(data)].tobytes() == data and (out[len(data):] == 0xA5).all()
    pool[base:base + len(gz)] = np.frombuffer(gz, dtype=np.uint8)
    src = pool.ctypes.data + base
    assert lib.mi_inflate_buffer(engine._h, src, len(gz), out.ctypes.data, len(data) - 1, C.byref(n), None) == -7 and n.value == len(data)
    assert lib.mi_inflate_buffer(engine._h, src, len(gz), None, 0, C.byref(n), None) == -7 and n.value == len(data)
    assert lib.mi_inflate_buffer(engine._h, src, len(gz), None, 5, C.byref(n), None) == -1
    assert lib.mi_inflate_buffer(engine._h, None, len(gz), out.ctypes.data, len(data), C.byref(n), None) == -1
    info = M.InflateInfo()
    assert lib.mi_inflate_buffer(engine._h, src, len(gz), out.ctypes.data, len(data), C.byref(n), C.byref(info)) == 0 and info.n_segments == 3


# ---- 8. under the guard ----------------------------------------------------------------------------------------------------------------
GUARDED = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import makisu_amd as M
import inflate_cases as ic
with M.Engine(device=0) as eng:
    for gz in (ic.cut_in_last_segment(), ic.ends_on_last_bit()):
        assert len(gz) %% 256 == 0                  # the member's last byte is the allocation's last
        p = ic.plan(gz)
        assert p["result"] == ic.INVALID and p["rule"] == ic.INPUT_ENDS, p
        try:
            eng.inflate_buffer(gz)
            raise SystemExit("accepted")
        except M.MiError as e:
            assert e.code == -1 and "rule %%d" %% p["rule"] in str(e) and "input offset %%d " %% p["at_in"] in str(e), (str(e), p)
    gz, data = ic.two_piece()
    gz = ic.with_fname(gz, 256 - len(gz) %% 256)
    out, info = eng.inflate_buffer(gz)
    assert out == data and info["n_segments"] == 3
print("OK")
'''


def test_no_read_leaves_the_member_under_the_guard():
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", GUARDED % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr[-3000:]


# ---- 9. the table builder alone --------------------------------------------------------------------------------------------------------
def _build_probe():
    src = os.path.join(PROBE_DIR, "inflate_probe.cpp")
    lib = os.path.join(ROOT, "makisu_amd", "libmakisu_mi.so")
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall",
                               src, "-o", PROBE, "-L", os.path.dirname(lib), "-lmakisu_mi",
                               "-Wl,-rpath,$ORIGIN/../../makisu_amd", "-Wl,--no-undefined"])
    return PROBE


@pytest.fixture(scope="module")
def probe(engine):
    lib = C.CDLL(_build_probe())
    lib.probe_inflate_table.restype = C.c_int
    lib.probe_inflate_table.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]

    def run(lens, tab_bits, bits, n_bits, max_out=64):
        d_lens = torch.from_numpy(np.asarray(lens, dtype=np.uint8)).cuda()
        d_bits = torch.from_numpy(np.frombuffer(bits + bytes(-len(bits) % 4 + 4), dtype=np.uint8).copy()).cuda()
        d_verdict = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_out = torch.full((max_out + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        assert lib.probe_inflate_table(d_lens.data_ptr(), len(lens), tab_bits, d_bits.data_ptr(), n_bits, d_verdict.data_ptr(), d_out.data_ptr(), max_out) == 0
        v, out = [int(x) for x in d_verdict.cpu().numpy()], d_out.cpu().numpy()
        assert (out[max_out:] == 0x5A5A5A5A).all() and v[5:] == [0x5A5A5A5A] * 3       # nothing behind the rows was written
        return v[:4], [int(x) for x in out[:v[4]]]
    return run


def test_the_table_builder_on_given_lengths(probe):
    fixed = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    fifteen = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15]                  # complete, with codes beyond the primary table
    cases = [("complete", [2, 2, 2, 2], 10), ("complete, mixed", [1, 2, 3, 3], 10), ("over-subscribed", [1, 1, 1], 10),
             ("over-subscribed late", fifteen + [15], 10), ("incomplete", [2, 2, 2], 10), ("a single length-1 code", [0, 1, 0], 10),
             ("all zero", [0] * 30, 8), ("15-bit codes", fifteen, 10), ("15-bit codes, small table", fifteen, 7), ("the fixed code", fixed, 10),
             ("the fixed distances", [5] * 32, 8), ("a code-length code", [3, 3, 3, 3, 3, 3, 3, 3] + [0] * 11, 7)]
    rng = np.random.default_rng(68)
    for name, lens, tab_bits in cases:
        over, left, total, longest, _ = ic._build(lens)
        coded = [s for s, l in enumerate(lens) if l]
        syms = [coded[int(k)] for k in rng.integers(0, len(coded), 40)] + coded[-3:] if coded and not over else []
        bits, n_bits = ic.code_bits(lens, syms) if syms else (bytes(8), 0)
        verdict, out = probe(lens, tab_bits, bits, n_bits)
        if over:
            assert verdict[0] == 1 and out == [], (name, verdict)
            continue
        assert verdict == [0, left, total, longest], (name, verdict)
        assert out == syms, (name, out, syms)
    # a pattern with no symbol: the single code is 0, so a 1 bit decodes to nothing; three codes of length 2 leave 11 free
    for lens, bits, n_bits, want in (([0, 1, 0], b"\x02", 2, [1, 0xFFFF]), ([2, 2, 2], b"\x03", 2, [0xFFFF]), ([0] * 30, b"\x00", 1, [0xFFFF])):
        assert probe(lens, 8, bits, n_bits)[1] == want, lens
