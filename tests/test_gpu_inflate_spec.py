"""GPU tests of the speculative device inflate: the finder, the speculative pass and the window pass each alone through
tests/kernel_probe -- the candidate table, every candidate's row and ring and the window area against the model of inflate_spec_cases.py --,
then mi_inflate_buffer_spec, mi_tar_inflate_ctx_spec and the spec layer add: byte-exact against zlib, the returned index against the
model's, every verdict, and one scenario under MI_GUARD_ALLOC=1 in a process of its own (no positive control: a deliberate fault has no
place here)."""
import ctypes as C
import gzip
import hashlib
import os
import re
import subprocess
import sys
import tarfile
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
import inflate_index_cases as xc  # noqa: E402
import inflate_spec_cases as sc  # noqa: E402
import layer_blob_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

PROBE_DIR = os.path.join(ROOT, "tests", "kernel_probe")
PROBE = os.path.join(PROBE_DIR, "libmi_inflate_spec_probe.so")
NONE = 2 ** 64 - 1


@pytest.fixture(scope="module")
def engine():
    with M.Engine(device=0) as e:
        yield e


def _build_probe():
    src = os.path.join(PROBE_DIR, "inflate_spec_probe.cpp")
    lib = os.path.join(ROOT, "makisu_amd", "libmakisu_mi.so")
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall",
                               src, "-o", PROBE, "-L", os.path.dirname(lib), "-lmakisu_mi",
                               "-Wl,-rpath,$ORIGIN/../../makisu_amd", "-Wl,--no-undefined"])
    return PROBE


def _u64(values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint64).reshape(-1).view(np.int64).copy()).cuda()


class Probe:
    def __init__(self, lib):
        self.lib = lib
        vp, u64 = C.c_void_p, C.c_uint64
        lib.probe_inflate_find.restype = lib.probe_inflate_speculate.restype = lib.probe_inflate_spec_windows.restype = C.c_int
        lib.probe_inflate_find.argtypes = [vp, u64, u64, u64, u64, vp]
        lib.probe_inflate_speculate.argtypes = [vp, u64, u64, u64, u64, vp, u64, u64, vp, vp]
        lib.probe_inflate_spec_windows.argtypes = [vp, u64, vp, u64, vp, u64, vp]

    @staticmethod
    def member(gz):
        return torch.from_numpy(np.frombuffer(bytes(gz) + bytes(4), dtype=np.uint8).copy()).cuda()

    def find(self, gz, piece_bytes):
        hdr, piece, n_pieces = sc.pieces(gz, piece_bytes)
        d_gz = self.member(gz)
        d_cand = torch.full((n_pieces + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        assert self.lib.probe_inflate_find(d_gz.data_ptr(), len(gz), hdr, piece, n_pieces, d_cand.data_ptr()) == 0
        out = d_cand.cpu().numpy().view(np.uint64)
        assert all(int(x) == 0x5A5A5A5A5A5A5A5A for x in out[n_pieces:])                # nothing behind the table
        return [int(x) for x in out[:n_pieces]]

    def speculate(self, gz, piece_bytes, cand, window=ic.WINDOW, cap=None):
        """-> (rows: a dict or None per piece, the rings as an (n_pieces, 32 768) uint16 array, still on the device)"""
        hdr, piece, n_pieces = sc.pieces(gz, piece_bytes)
        cap = sc.SYMBOLS_PER_BYTE * piece if cap is None else cap
        d_gz, d_cand = self.member(gz), _u64(cand)
        d_rings = torch.full((n_pieces + 1, sc.RING), 0x7E7E, dtype=torch.int16, device="cuda")
        d_rows = torch.full((4 * n_pieces + 4,), -1, dtype=torch.int64, device="cuda")
        assert self.lib.probe_inflate_speculate(d_gz.data_ptr(), len(gz), hdr, piece, n_pieces, d_cand.data_ptr(), window, cap, d_rings.data_ptr(),
                                                d_rows.data_ptr()) == 0
        raw = d_rows.cpu().numpy().view(np.uint64)
        assert all(int(x) == NONE for x in raw[4 * n_pieces:])
        assert bool((d_rings[n_pieces] == 0x7E7E).all())                                 # nothing behind the last ring
        rows = []
        for k in range(n_pieces):
            end, out_bytes, word, bit = (int(x) for x in raw[4 * k:4 * k + 4])
            rows.append(None if (end, out_bytes, word, bit) == (NONE,) * 4 else
                        dict(status=word & 0xFFFFFFFF, end=end, out_bytes=out_bytes, rule=word >> 32, bit=bit))
        return rows, d_rings

    def windows(self, d_rings, n_rings, spans, total):
        live = [(s["out_at"], s["out_bytes"], s["win_at"], s["win_bytes"], s["ring"]) for s in spans]
        d_hist = torch.zeros((total + 64,), dtype=torch.uint8, device="cuda")
        d_hist[total:] = 0x5A
        d_bad = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        assert self.lib.probe_inflate_spec_windows(d_rings.data_ptr(), n_rings, _u64(live).data_ptr(), len(live), d_hist.data_ptr(), total,
                                                   d_bad.data_ptr()) == 0
        out = d_hist.cpu().numpy()
        assert bytes(out[total:]) == b"\x5a" * 64
        return bytes(out[:total]), int(d_bad.cpu().numpy().view(np.uint64)[0])


@pytest.fixture(scope="module")
def probe(engine):
    return Probe(C.CDLL(_build_probe()))


@pytest.fixture(scope="module")
def no_reset_stream():
    data = xc.local_binary(300000)
    return ic.no_reset(data, 4096), data


def _shapes(no_reset_stream):
    gz, data = no_reset_stream
    pgz, pdata, _ = sc.planted_member()
    return {"no_reset_1024": (gz, data, 1024), "no_reset_4096": (gz, data, 4096), "planted": (pgz, pdata, sc.PLANTED_PIECE)}


# ---- 1. the three kernels alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["no_reset_1024", "no_reset_4096", "planted"])
def test_the_three_kernels_give_the_models_tables(probe, no_reset_stream, shape):
    gz, data, piece = _shapes(no_reset_stream)[shape]
    want = sc.find(gz, piece)
    cand = probe.find(gz, piece)
    assert cand == want, [(k, a, b) for k, (a, b) in enumerate(zip(cand, want)) if a != b][:5]
    if shape == "no_reset_1024":
        assert len(cand) >= 60 and sum(1 for c in cand if c == NONE) >= 5
    rows, d_rings = probe.speculate(gz, piece, cand)
    rings = d_rings.cpu().numpy().view(np.uint16)
    entries = {}
    for k in range(len(cand)):
        row, ent = sc.speculate(gz, cand, k, piece)
        assert rows[k] == row, (k, rows[k], row)                                          # dead candidates' rows included
        if row is not None and row["status"] in (ic.SEG_ENDS, ic.SEG_FINAL):
            entries[k] = ent
            held = min(sc.RING, len(ent))
            at = np.arange(len(ent) - held, len(ent))
            assert np.array_equal(rings[k][at & (sc.RING - 1)], np.asarray(ent[len(ent) - held:], dtype=np.uint16)), k
    p = sc.plan(gz, piece)
    assert p["result"] == sc.DONE and len(p["spans"]) >= 2
    area, bad = probe.windows(d_rings, len(cand), p["spans"], len(p["windows"]))
    assert bad == NONE and area == p["windows"]
    assert sc.inflate_by_plan(gz, p) == (data, None)


def test_the_window_pass_refuses_a_table_that_does_not_fit(probe, no_reset_stream):
    gz, data = no_reset_stream
    p = sc.plan(gz, 4096)
    cand = p["cand"]
    rows, d_rings = probe.speculate(gz, 4096, cand)
    total = len(p["windows"])
    for k, change in ((2, dict(ring=len(cand))), (3, dict(win_at=total - 16)), (1, dict(out_at=p["spans"][1]["out_at"] + 1)), (2, dict(win_bytes=32769))):
        spans = [dict(s) for s in p["spans"]]
        spans[k].update(change)
        area, bad = probe.windows(d_rings, len(cand), spans, total)
        assert bad in (k, k + 1), (k, change, bad)                                        # the span itself, or the one that reads it


# ---- 2. mi_inflate_buffer_spec ------------------------------------------------------------------------------------------------------------
def _done(engine, gz, data, piece=0):
    out, info, spec, ix = engine.inflate_buffer_spec(gz, piece, want_index=True)
    assert info["verdict"] == M.INFLATE_DONE and info["fell_back"] == 0, (info, spec)
    assert out == data, (len(out), len(data), next((i for i in range(min(len(out), len(data))) if out[i] != data[i]), None))
    p = sc.plan(gz, piece)
    assert (spec["piece_bytes"], spec["n_pieces"], spec["n_found"], spec["n_live"]) == (p["piece"], p["n_pieces"], p["n_found"], p["n_live"]), spec
    assert spec["ring_bytes"] == 65536 * p["n_pieces"] and info["n_segments"] == len(p["spans"])
    assert M.inflate_index_check(ix, gz)[0] == 0
    assert ix == sc.index_of(p, gz)
    again, info2 = engine.inflate_buffer_indexed(gz, ix)
    assert info2["verdict"] == M.INFLATE_DONE and again == data
    return info, spec


def test_every_member_is_zlibs_bytes_and_the_index_is_the_models(engine):
    for name, (gz, data) in xc.members().items():
        assert ic.zlib_inflates(gz) == data
        _done(engine, gz, data, 4096 if name != "planted" else 1024)
    gz, data, _ = sc.planted_member()
    _done(engine, gz, data, sc.PLANTED_PIECE)
    plain = dc.text(140000, 360) + dc.random_bytes(70000, 361)
    _done(engine, dc.gzip_member(plain), plain, 2048)                                     # the device leg's form
    _done(engine, ic.one_stream(b""), b"", 0)


def test_the_capacity_is_known_after_the_plan(engine, no_reset_stream):
    gz, data = no_reset_stream
    src = np.frombuffer(gz, dtype=np.uint8)
    n, info, dst = C.c_uint64(), M.InflateInfo(), np.zeros(16, dtype=np.uint8)
    rc = engine._lib.mi_inflate_buffer_spec(engine._h, src.ctypes.data, src.size, 4096, dst.ctypes.data, 16, C.byref(n), C.byref(info), None, None, None)
    assert rc == -7 and n.value == len(data) and bytes(dst) == bytes(16) and info.ms_write == 0
    for piece in (1, 1023, 16777217):
        with pytest.raises(M.MiError) as e:
            engine.inflate_buffer_spec(gz, piece)
        assert e.value.code == -1


def test_several_rounds_and_a_span_beyond_the_window(engine, monkeypatch):
    monkeypatch.setenv("MI_INFLATE_WINDOW_MB", "1")
    data = xc.local_binary(1 << 20) + dc.text(1 << 20, 334) + xc.local_binary(1 << 20)[::-1]
    gz = ic.one_stream(data, 6)
    out, info, spec = engine.inflate_buffer_spec(gz, 16384)
    assert info["verdict"] == M.INFLATE_DONE and out == data and info["n_rounds"] >= 3, (info, spec)
    zeros = ic.one_stream(bytes(3 << 20), 6)
    p = sc.plan(zeros, 0, 1 << 20)
    assert p["result"] == sc.NOT_PARALLEL and p["rule"] == ic.BEYOND_WINDOW
    out, info, spec = engine.inflate_buffer_spec(zeros)
    assert out == b"" and (info["verdict"], info["rule"], info["at_in"], info["at_out"]) == (M.INFLATE_NOT_PARALLEL, ic.BEYOND_WINDOW, p["at_bit"] // 8,
                                                                                           p["at_out"]), info


def test_fixed_blocks_two_members_and_corruption_get_the_models_verdicts(engine):
    # a stream of fixed blocks has no candidate: the symbol cap ends the one span
    fixed = ic.one_stream(dc.text(1 << 20, 370), 6, zlib.Z_FIXED)
    cand = sc.find(fixed, 1024)
    row, _ = sc.speculate(fixed, cand, 0, 1024)
    assert (row["status"], row["rule"]) == (ic.SEG_TOO_LONG, sc.SYMBOL_CAP)
    out, info, spec = engine.inflate_buffer_spec(fixed, 1024)
    assert out == b"" and (info["verdict"], info["rule"], info["at_in"], info["at_out"]) == (M.INFLATE_NOT_PARALLEL, sc.SYMBOL_CAP, 10, 0), info
    assert spec["n_live"] == 1
    # two members
    one = ic.one_stream(dc.text(30000, 371), 6)
    out, info, spec = engine.inflate_buffer_spec(one + one, 1024)
    assert out == b"" and info["verdict"] == M.INFLATE_NOT_PARALLEL and info["rule"] == 0, info
    assert sc.plan(one + one, 1024)["result"] == sc.NOT_PARALLEL
    # a flipped bit inside a live span: the model's span, rule and bit.  (A flip among a block's symbols only changes bytes -- a Huffman
    # decode finds its way back, and the CRC-32 tells; a flip in BTYPE of the header at which the third span begins makes it block type
    # 3, no candidate any more, in the middle of the second span)
    base = ic.no_reset(dc.text(40000, 372) + xc.local_binary(30000), 4096)
    at = sc.plan(base, 1024)["spans"][2]["in_bit"] + 1
    bad = base[:at // 8] + bytes((base[at // 8] ^ (1 << (at % 8)),)) + base[at // 8 + 1:]
    p = sc.plan(bad, 1024)
    assert (p["span"], p["rule"]) == (1, ic.BLOCK_TYPE)
    assert p["result"] == sc.INVALID and ic.zlib_inflates(bad) is None
    with pytest.raises(M.MiError) as e:
        engine.inflate_buffer_spec(bad, 1024)
    assert e.value.code == -1
    m = re.search(r"span (\d+) at input bit (\d+) \(output offset (\d+)\) breaks rule (\d+) at bit (\d+)", str(e.value))
    assert m and tuple(int(x) for x in m.groups()) == (p["span"], p["at_bit"], p["at_out"], p["rule"], p["bit"]), (str(e.value), p["rule"], p["bit"])


def test_what_only_the_write_pass_can_tell_is_refused_and_nothing_is_delivered(engine):
    # the first match reaches before byte 0: markers nobody can resolve -- rule 10 in the write pass
    early = ic.rule_streams()[ic.DISTANCE]
    p = sc.plan(early, 0)
    assert p["result"] == sc.DONE and sc.inflate_by_plan(early, p)[1] == (0, ic.DISTANCE)
    out, info, spec = engine.inflate_buffer_spec(early)
    assert out == b"" and (info["verdict"], info["rule"]) == (M.INFLATE_INDEX_REFUSED, ic.DISTANCE), info
    # a flipped byte in a stored block: every span ends where it should, the CRC-32 tells
    rnd = dc.random_bytes(200000, 373)
    gz = ic.one_stream(rnd, 6)
    at = len(gz) // 2
    bad = gz[:at] + bytes((gz[at] ^ 0x40,)) + gz[at + 1:]
    p = sc.plan(bad, 4096)
    assert p["result"] == sc.DONE and sc.inflate_by_plan(bad, p)[1] is None
    out, info, spec, ix = engine.inflate_buffer_spec(bad, 4096, want_index=True)
    assert out == b"" and ix is None and (info["verdict"], info["rule"]) == (M.INFLATE_INDEX_REFUSED, 0), info


# ---- 3. mi_tar_inflate_ctx_spec and the layer add --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_tar():
    binary = xc.local_binary(400000)
    return lc.tarfile_tar(tarfile.GNU_FORMAT, extra=[("text-%d" % i, dc.text(50000, 50 + i)) for i in range(2)] +
                          [("bin-%d" % i, binary[i * 200000:(i + 1) * 200000]) for i in range(2)] + [("rnd", dc.random_bytes(70000, 9))])


def test_tar_inflate_spec_gives_what_tar_inflate_gives(engine, tmp_path, small_tar):
    tar, _ = small_tar
    for name, blob in (("foreign", gzip.compress(tar)), ("no_reset", ic.no_reset(tar)), ("plain", tar)):
        p = tmp_path / (name + ".blob")
        p.write_bytes(blob)
        host = M.tar_inflate(str(p), str(tmp_path / "host.tar"))
        dev = engine.tar_inflate_spec(str(p), str(tmp_path / "dev.tar"), 4096, want_index=True)
        assert (tmp_path / "dev.tar").read_bytes() == (tmp_path / "host.tar").read_bytes() == tar
        assert (dev["tar_bytes"], dev["tar_digest"], dev["blob_digest"]) == (host["tar_bytes"], host["tar_digest"], host["blob_digest"])
        if name == "plain":
            assert dev["index"] is None
            continue
        assert dev["info"]["verdict"] == M.INFLATE_DONE and dev["info"]["fell_back"] == 0 and dev["spec"]["n_live"] >= 4, dev
        assert dev["index"] == sc.index_of(sc.plan(blob, 4096), blob)
        assert engine.tar_inflate_indexed(str(p), dev["index"])["tar_digest"] == host["tar_digest"]
    # fixed blocks: not parallel, the host path gives the same
    fixed = ic.one_stream(tar, 6, zlib.Z_FIXED)
    p = tmp_path / "fixed.gz"
    p.write_bytes(fixed)
    host = M.tar_inflate(str(p), str(tmp_path / "host2.tar"))
    dev = engine.tar_inflate_spec(str(p), str(tmp_path / "dev2.tar"), 1024, want_index=True)
    assert dev["info"]["verdict"] == M.INFLATE_NOT_PARALLEL and dev["info"]["fell_back"] == 1 and dev["index"] is None, dev["info"]
    assert (tmp_path / "dev2.tar").read_bytes() == tar and (dev["tar_digest"], dev["blob_digest"]) == (host["tar_digest"], host["blob_digest"])


def test_a_foreign_gzip_becomes_a_batch_without_an_index(engine, tmp_path, small_tar):
    tar, members = small_tar
    blob = gzip.compress(tar)
    with engine.batch() as b:
        ents0, offs0, info0, sha0 = b.add_layer_blob(blob, 5)
        b.run()
        roots0, chunks0 = b.roots().copy(), b.chunks().copy()
    p = tmp_path / "layer.gz"
    p.write_bytes(blob)
    fixed = ic.one_stream(tar, 6, zlib.Z_FIXED)
    for how, source, verdict in (("blob", M.LAYER_SOURCE_SPEC_GZIP, M.INFLATE_DONE), ("path", M.LAYER_SOURCE_SPEC_GZIP, M.INFLATE_DONE),
                                 ("fixed", M.LAYER_SOURCE_DEVICE_GZIP, M.INFLATE_DONE)):
        with engine.batch() as b:
            b.add_bytes(b"in front", 1)
            before = b.counts()
            if how == "path":
                ents, offs, info, sha = b.add_layer_path_spec(str(p), 5, 4096)
            else:
                ents, offs, info, sha = b.add_layer_blob_spec(fixed if how == "fixed" else blob, 5, 1024 if how == "fixed" else 4096)
            assert (ents, offs) == (ents0, offs0) and sha == hashlib.sha256(fixed if how == "fixed" else blob).digest()
            assert (info["source"], info["tar_bytes"], info["n_files"], info["inflate"]["verdict"]) == (source, len(tar), len(members), verdict), info
            assert info["first_file"] == 1 and b.counts()[0] == before[0] + len(members)
            if how != "fixed":
                assert info["spec"]["n_live"] >= 4 and info["inflate"]["fell_back"] == 0
            b.run()
            regs = [e for e in ents if e["kind"] == M.KIND_FILE]
            for e, (_, data) in zip(regs, members):
                assert b.read_file(1 + e["file_index"], 0, len(data)) == data, e["relpath"]
            assert np.array_equal(b.roots()[1:], roots0) and np.array_equal(b.chunks()["sha256"][1:], chunks0["sha256"])


# ---- 4. under the guard allocator ---------------------------------------------------------------------------------------------------------
GUARDED = r'''
import sys
sys.path[:0] = [%(root)r, %(root)r + "/tests"]
import gzip
import makisu_amd as M
import deflate_cases as dc
import inflate_cases as ic
import inflate_spec_cases as sc
gz, data, _ = sc.planted_member()
text = dc.text(300000, 350) + dc.random_bytes(5000, 351)
with M.Engine(device=0) as e:
    for blob, want, piece in ((gz, data, sc.PLANTED_PIECE), (ic.no_reset(text, 1 << 15), text, 1024), (gzip.compress(text), text, 0)):
        out, info, spec = e.inflate_buffer_spec(blob, piece)
        assert info["verdict"] == M.INFLATE_DONE and out == want, (info, spec)
print("OK")
'''


def test_no_access_leaves_the_member_the_rings_or_the_windows_under_the_guard():
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", GUARDED % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr[-3000:]
