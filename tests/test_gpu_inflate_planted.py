"""GPU tests of the device inflate on the planted members of tests/inflate_cases.py (planted_streams: streams written by hand, so that
every branch of csrc/mi_inflate_wave.h's decoder is taken on purpose; tests/test_host_inflate_planted.py holds them against zlib and
says which member is there for which branch): each member through mi_inflate_buffer; every candidate's ROW -- status, end, out_bytes,
rule and bit, dead candidates included -- and the rows from every byte offset of three small members as a start, against
decode_segment, through the size pass alone (tests/kernel_probe); the write pass alone into a buffer with guard bytes around every
segment; the members of thousands of empty segments under both windows; one member as a layer through mi_batch_add_layer_blob."""
import ctypes as C
import hashlib
import os
import sys

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
import inflate_cases as ic  # noqa: E402
import test_gpu_inflate as base  # noqa: E402  (its _check and its probe's build)

pytestmark = pytest.mark.gpu

PLANTED = sorted(ic.planted_streams())
ROW = np.dtype([("end", "<u8"), ("out_bytes", "<u8"), ("status", "<u4"), ("rule", "<u4"), ("bit", "<u8")])
FIELDS = ("status", "end", "out_bytes", "rule", "bit")
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def engine():
    with M.Engine(device=0) as e:
        yield e


@pytest.fixture(scope="module")
def probe(engine):
    lib = C.CDLL(base._build_probe())
    lib.probe_inflate_rows.restype = lib.probe_inflate_write.restype = C.c_int
    lib.probe_inflate_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.probe_inflate_write.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def _up(gz):
    return torch.from_numpy(np.frombuffer(gz, dtype=np.uint8).copy()).cuda()


def _rows(probe, gz, starts, window):
    """the size pass over the starts, one grid: the rows"""
    d_gz, d_starts = _up(gz), torch.tensor(starts, dtype=torch.int64, device="cuda")
    d_rows = torch.full((4 * len(starts) + 4,), -1, dtype=torch.int64, device="cuda")
    assert probe.probe_inflate_rows(d_gz.data_ptr(), len(gz), d_starts.data_ptr(), len(starts), window, d_rows.data_ptr()) == 0
    got = d_rows.cpu().numpy()
    assert (got[4 * len(starts):] == -1).all()           # nothing behind the rows was written
    return got[:4 * len(starts)].view(ROW)


def _same_rows(probe, gz, starts, window, what):
    got = _rows(probe, gz, starts, window)
    differ = []
    for k, start in enumerate(starts):
        want = ic.decode_segment(gz, start, window)[0]
        if any(int(got[k][f]) != want[f] for f in FIELDS):
            differ.append((start, {f: int(got[k][f]) for f in FIELDS}, want))
    assert not differ, (what, len(differ), differ[:5])
    return got


# ---- 1. every planted member through the whole call ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLANTED)
def test_a_planted_member_inflates(engine, name):
    gz, data, _ = ic.planted_streams()[name]
    info = base._check(engine, gz, data)
    p = ic.plan(gz)                                      # (the counts of the member of 1 MiB too, which _check leaves to zlib)
    assert (info["n_candidates"], info["n_segments"], info["n_rounds"]) == (p["n_candidates"], p["n_segments"], p["n_rounds"]), (info, p)


# ---- 2. the rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLANTED)
def test_every_candidates_row_is_the_models(probe, name):
    gz = ic.planted_streams()[name][0]
    starts = ic.candidates(gz, ic.gzip_header(gz))
    got = _same_rows(probe, gz, starts, ic.WINDOW, name)
    if name == "dead_headers":
        assert [int(r["rule"]) for r in got[1:]] == [ic.NO_END_OF_BLOCK] * 3


def test_the_rows_from_every_byte_offset_are_the_models(probe):
    """some thousands of one-wave decodes of what is mostly garbage -- this code's normal case --, one grid a member; the window is
    64 KiB, so that BEYOND_WINDOW is among the rows"""
    statuses = set()
    for what, gz in (("two_piece", ic.two_piece()[0]), ("lengths", ic.planted_streams()["lengths"][0]), ("long_run", ic.planted_streams()["long_run"][0])):
        got = _same_rows(probe, gz, list(range(len(gz))), 65536, what)
        statuses |= set(int(s) for s in got["status"])
    assert statuses == {ic.SEG_ENDS, ic.SEG_FINAL, ic.SEG_BROKEN, ic.SEG_TOO_LONG}


# ---- 3. the write pass alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLANTED)
def test_the_write_pass_writes_its_segments_and_nothing_else(probe, name):
    """every candidate whose decode ends well, dead ones too, into one buffer: GUARD spare bytes in front of, between and behind the
    segments, the offsets through every alignment mod 16"""
    gz = ic.planted_streams()[name][0]
    segs, at = [], GUARD
    for k, c in enumerate(ic.candidates(gz, ic.gzip_header(gz))):
        row, data = ic.decode_segment(gz, c)
        if row["status"] in (ic.SEG_ENDS, ic.SEG_FINAL):
            at += (PLANTED.index(name) + k - at) % 16     # (most members are one segment: the member's number moves the first one)
            segs.append((c, at, data))
            at += len(data) + GUARD
    total = at
    table = torch.tensor([v for c, a, data in segs for v in (c, a, len(data))], dtype=torch.int64, device="cuda")
    d_gz, d_out = _up(gz), torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    d_bad = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    assert probe.probe_inflate_write(d_gz.data_ptr(), len(gz), table.data_ptr(), len(segs), total, d_out.data_ptr(), d_bad.data_ptr()) == 0
    assert d_bad.cpu().tolist() == [-1, -1]
    out = d_out.cpu().numpy()
    spare = np.ones(total, dtype=bool)
    for c, a, data in segs:
        assert out[a:a + len(data)].tobytes() == data, (name, c, a % 16, next(i for i in range(len(data)) if out[a + i] != data[i]))
        spare[a:a + len(data)] = False
    assert (out[spare] == FILL).all(), (name, np.flatnonzero(spare & (out != FILL))[:8])


def test_the_write_pass_says_which_segment_ended_otherwise(probe):
    """a table that states one byte too few for its second segment: that segment is named, its bytes stay inside what the table states"""
    gz = ic.planted_streams()["tile_edges"][0]
    rows = [(c, ic.decode_segment(gz, c)) for c in ic.candidates(gz, 10)[:3]]
    table, at = [], GUARD
    for k, (c, (row, data)) in enumerate(rows):
        table += [c, at, len(data) - (k == 1)]
        at += len(data) + GUARD
    d_out, d_bad = torch.full((at,), FILL, dtype=torch.uint8, device="cuda"), torch.full((1,), -1, dtype=torch.int64, device="cuda")
    d_gz, d_table = _up(gz), torch.tensor(table, dtype=torch.int64, device="cuda")
    assert probe.probe_inflate_write(d_gz.data_ptr(), len(gz), d_table.data_ptr(), 3, at, d_out.data_ptr(), d_bad.data_ptr()) == 0
    assert d_bad.cpu().tolist() == [1]
    out = d_out.cpu().numpy()
    for k, (c, (row, data)) in enumerate(rows):
        a, n = table[3 * k + 1], table[3 * k + 2]
        assert (out[a - GUARD:a] == FILL).all() and (out[a + n:a + n + GUARD - 1] == FILL).all()
        if k != 1:
            assert out[a:a + n].tobytes() == data


# ---- 4. thousands of empty segments, under both windows --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["empty_segments", "empty_segments_between"])
def test_empty_segments_at_a_rounds_edge(engine, monkeypatch, name):
    gz, data, _ = ic.planted_streams()[name]
    monkeypatch.setenv("MI_INFLATE_WINDOW_MB", "1")
    out, info = engine.inflate_buffer(gz)
    p = ic.plan(gz, 1 << 20)
    assert out == data and info["verdict"] == M.INFLATE_DONE
    assert (info["n_candidates"], info["n_segments"], info["n_rounds"]) == (p["n_candidates"], p["n_segments"], p["n_rounds"]), (info, p)
    assert info["n_segments"] == ic.N_EMPTY + 1 and info["n_rounds"] == (2 if data else 1)


# ---- 5. as a layer ---------------------------------------------------------------------------------------------------------------------
def test_distance_32768_as_a_layer(engine):
    """the same decode once more, into a batch's arena (mi_inflater_run_device)"""
    blob, tar, content = ic.far_layer()
    assert ic.zlib_inflates(blob) == tar and ("far", 0) in ic.trace(blob, 10)[2]
    with engine.batch() as b:
        ents, offs, info, sha = b.add_layer_blob(blob)
        assert sha == hashlib.sha256(blob).digest() and (info["tar_bytes"], info["n_files"], info["source"]) == (len(tar), 1, M.LAYER_SOURCE_DEVICE_GZIP), info
        assert info["inflate"]["verdict"] == M.INFLATE_DONE and info["inflate"]["fell_back"] == 0 and info["inflate"]["n_segments"] == 1
        regs = [e for e in ents if e["kind"] == M.KIND_FILE]
        assert [e["size"] for e in regs] == [len(content)] and offs == [512]
        b.run()
        assert b.read_file(regs[0]["file_index"], 0, len(content)) == content
        assert b.read_back().tobytes() == content
