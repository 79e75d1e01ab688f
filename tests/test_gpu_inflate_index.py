"""GPU tests of the indexed device inflate: inflate_span_kernel alone through tests/kernel_probe -- every span's bytes and
end against the model of inflate_index_cases.py, on the planted member and on 1 MB of a local binary at spacing 1 --, then
mi_inflate_buffer_indexed, mi_tar_inflate_ctx_indexed and mi_batch_add_layer_blob_indexed on members no unindexed call can take in
parallel, the rounds under a small window, every way an index is refused (always a verdict, never MI_ERR_INVALID), and one scenario
under MI_GUARD_ALLOC=1 in a process of its own (no positive control: a deliberate fault has no place here)."""
import ctypes as C
import gzip
import hashlib
import os
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
import layer_blob_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

PROBE_DIR = os.path.join(ROOT, "tests", "kernel_probe")
PROBE = os.path.join(PROBE_DIR, "libmi_inflate_index_probe.so")
NONE = 2 ** 64 - 1


@pytest.fixture(scope="module")
def engine():
    with M.Engine(device=0) as e:
        yield e


def _build_probe():
    src = os.path.join(PROBE_DIR, "inflate_index_probe.cpp")
    lib = os.path.join(ROOT, "makisu_amd", "libmakisu_mi.so")
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall",
                               src, "-o", PROBE, "-L", os.path.dirname(lib), "-lmakisu_mi",
                               "-Wl,-rpath,$ORIGIN/../../makisu_amd", "-Wl,--no-undefined"])
    return PROBE


@pytest.fixture(scope="module")
def probe(engine):
    lib = C.CDLL(_build_probe())
    lib.probe_inflate_spans.restype = C.c_int
    lib.probe_inflate_spans.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                        C.c_void_p]

    def run(gz, table, round_bytes, windows):
        """the spans of `table` (six words each) -> (the round's bytes, the bad word, {span: (rule, bit)} of the refused ones)"""
        d_gz = torch.from_numpy(np.frombuffer(bytes(gz) + bytes(4), dtype=np.uint8).copy()).cuda()
        d_span = torch.from_numpy(np.asarray(table, dtype=np.uint64).reshape(-1).view(np.int64).copy()).cuda()
        d_out = torch.full((round_bytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        d_hist = torch.from_numpy(np.frombuffer(bytes(windows) + bytes(16), dtype=np.uint8).copy()).cuda()
        d_bad = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        d_verdict = torch.full((2 * len(table),), -1, dtype=torch.int64, device="cuda")
        assert lib.probe_inflate_spans(d_gz.data_ptr(), len(gz), d_span.data_ptr(), len(table), round_bytes, d_out.data_ptr(), d_hist.data_ptr(),
                                       len(windows), d_bad.data_ptr(), d_verdict.data_ptr()) == 0
        out = d_out.cpu().numpy()
        assert bytes(out[round_bytes:]) == b"\x5a" * 64                 # nothing behind the round
        v = d_verdict.cpu().numpy().view(np.uint64).reshape(-1, 2)
        refused = {}
        for k in range(len(table)):
            if int(v[k, 0]) != NONE:
                assert int(v[k, 0]) & 0xFFFFFFFF == k
                refused[k] = (int(v[k, 0]) >> 32, int(v[k, 1]))
        return bytes(out[:round_bytes]), int(d_bad.cpu().numpy().view(np.uint64)[0]), refused
    return run


def _table(spans):
    return [(s["in_bit"], s["end_bit"], s["out_at"], s["out_bytes"], s["win_at"], s["win_bytes"]) for s in spans]


# ---- 1. the span decoder alone ----------------------------------------------------------------------------------------------------------
def test_every_span_of_the_planted_member_is_the_models(probe):
    gz, data, what = xc.planted_member()
    ix = xc.index(gz, 1)
    spans, windows = xc.spans(ix), xc.parse(ix)["windows"]
    assert {s["in_bit"] % 8 for s in spans} == set(range(8)) and len(spans) >= 20
    out, bad, refused = probe(gz, _table(spans), len(data), windows)
    assert bad == NONE and not refused
    for s in spans:
        row, want = xc.decode_span(gz, s["in_bit"], s["end_bit"], s["hist"], s["out_bytes"])
        assert row["rule"] == 0 and out[s["out_at"]:s["out_at"] + s["out_bytes"]] == want, s["out_at"]
    assert out == data
    # the same spans in another order and at other offsets of a larger round: nothing of one span depends on another
    order = list(reversed(range(len(spans))))
    at, table = 7, []
    for k in order:
        s = spans[k]
        table.append((s["in_bit"], s["end_bit"], at, s["out_bytes"], s["win_at"], s["win_bytes"]))
        at += s["out_bytes"] + 3
    out, bad, refused = probe(gz, table, at, windows)
    assert bad == NONE and not refused
    for row, k in zip(table, order):
        assert out[row[2]:row[2] + row[3]] == data[spans[k]["out_at"]:spans[k]["out_at"] + spans[k]["out_bytes"]], k


def test_every_span_of_a_megabyte_of_a_binary_is_the_models(probe):
    data = xc.local_binary(1 << 20)
    gz = ic.one_stream(data, 6)
    ix = xc.index(gz, 1)
    assert M.inflate_index_build(gz, 1)[0] == ix
    spans, windows = xc.spans(ix), xc.parse(ix)["windows"]
    assert len(spans) >= 8 and max(s["out_bytes"] for s in spans) < 400000
    out, bad, refused = probe(gz, _table(spans), len(data), windows)
    assert bad == NONE and not refused
    for s in spans:
        assert out[s["out_at"]:s["out_at"] + s["out_bytes"]] == data[s["out_at"]:s["out_at"] + s["out_bytes"]], s["out_at"]
    row, want = xc.decode_span(gz, spans[3]["in_bit"], spans[3]["end_bit"], spans[3]["hist"], spans[3]["out_bytes"])
    assert row["rule"] == 0 and want == out[spans[3]["out_at"]:spans[3]["out_at"] + spans[3]["out_bytes"]]


def test_a_span_that_is_not_what_the_table_says_is_refused_with_the_models_rule(probe):
    gz, data, what = xc.planted_member()
    ix = xc.index(gz, 1)
    spans, windows = xc.spans(ix), xc.parse(ix)["windows"]
    by_out = {s["out_at"]: k for k, s in enumerate(spans)}
    k_far, k_short = by_out[what["far"]], by_out[what["short_window_first_byte"]]
    cases = []                                           # (span, what changes)
    for k in (1, 4, k_far):
        s = spans[k]
        cases += [(k, dict(in_bit=s["in_bit"] + 1)), (k, dict(out_bytes=s["out_bytes"] + 1)), (k, dict(out_bytes=s["out_bytes"] - 1))]
        if s["end_bit"]:
            cases += [(k, dict(end_bit=s["end_bit"] + 1)), (k, dict(end_bit=s["end_bit"] - 1)), (k, dict(end_bit=0))]
    cases += [(len(spans) - 1, dict(end_bit=spans[-1]["in_bit"] + 40))]
    # a window one byte shorter than the span's first match needs: the window's last bytes stay the last
    for k in (k_far, k_short):
        s = spans[k]
        cases.append((k, dict(win_at=s["win_at"] + 16, win_bytes=s["win_bytes"] - 16, hist=s["hist"][16:])))
    table, want = [], []
    at = 0
    for k, change in cases:
        s = dict(spans[k], **change)
        row, _ = xc.decode_span(gz, s["in_bit"], s["end_bit"], s["hist"], s["out_bytes"])
        table.append((s["in_bit"], s["end_bit"], at, s["out_bytes"], s["win_at"], s["win_bytes"]))
        want.append(row)
        at += s["out_bytes"] + 8
    out, bad, refused = probe(gz, table, at, windows)
    for j, ((k, change), row) in enumerate(zip(cases, want)):
        assert row["rule"] != 0, (k, change)
        assert j in refused and refused[j][0] == row["rule"], (k, change, row, refused.get(j))
    assert want[-1]["rule"] == want[-2]["rule"] == ic.DISTANCE and {r["rule"] for r in want} >= {xc.INDEX, ic.DISTANCE}
    assert bad == 0
    # a table that points outside the member, the round or the window area is refused before a byte is decoded
    s = spans[2]
    table = [(8 * len(gz), 0, 0, 10, 0, 0), (s["in_bit"], s["end_bit"], 5, s["out_bytes"], s["win_at"], s["win_bytes"]),
             (s["in_bit"], s["end_bit"], 0, s["out_bytes"], len(windows) - 8, 16), (s["in_bit"], s["end_bit"], 0, s["out_bytes"], 0, 32769),
             (s["in_bit"], s["in_bit"], 0, s["out_bytes"], s["win_at"], s["win_bytes"])]
    out, bad, refused = probe(gz, table, s["out_bytes"] + 4, windows)
    assert bad == 0 and sorted(refused) == list(range(5)) and {r for r, _ in refused.values()} == {xc.INDEX}
    assert out == b"\x5a" * (s["out_bytes"] + 4)


# ---- 2. mi_inflate_buffer_indexed --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    return dc.text(150000, 330) + xc.local_binary(500000) + dc.random_bytes(40000, 331) + dc.text(100000, 332)


def _done(engine, gz, data, spacing=65536):
    ix, built = M.inflate_index_build(gz, spacing)
    out, info = engine.inflate_buffer_indexed(gz, ix)
    assert info["verdict"] == M.INFLATE_DONE and info["fell_back"] == 0 and info["index_refusal"] == 0, info
    assert out == data, (len(out), len(data), next((i for i in range(min(len(out), len(data))) if out[i] != data[i]), None))
    assert (info["in_bytes"], info["out_bytes"], info["n_segments"]) == (len(gz), len(data), built["n_points"])
    return info


def test_members_no_unindexed_call_takes_in_parallel(engine, mixed):
    rnd = dc.random_bytes(300000, 333)
    forms = {"foreign": gzip.compress(mixed, 6), "no_reset": ic.no_reset(mixed, 1 << 16), "host_leg": ic.host_leg(mixed, 6, 1 << 18),
             "stored_only": ic.one_stream(rnd, 6)}
    for name, gz in forms.items():
        data = rnd if name == "stored_only" else mixed
        info = _done(engine, gz, data)
        assert info["n_segments"] >= 4, (name, info)
        plain, unindexed = engine.inflate_buffer(gz)
        if name == "no_reset":                           # matches across the flushes: without the index zlib takes it
            assert unindexed["verdict"] == M.INFLATE_NOT_PARALLEL and plain == b""
        else:
            assert unindexed["verdict"] == M.INFLATE_DONE and plain == data
            if name in ("foreign", "stored_only"):
                assert unindexed["n_segments"] == 1 < info["n_segments"]
    gz, data, _ = xc.planted_member()
    _done(engine, gz, data, 1)
    empty = ic.one_stream(b"")
    _done(engine, empty, b"", 1)


def test_the_capacity_is_known_from_the_index(engine, mixed):
    gz = gzip.compress(mixed, 6)
    ix, _ = M.inflate_index_build(gz, 0)
    src, idx = np.frombuffer(gz, dtype=np.uint8), np.frombuffer(ix, dtype=np.uint8)
    n, info, dst = C.c_uint64(), M.InflateInfo(), np.zeros(16, dtype=np.uint8)
    rc = engine._lib.mi_inflate_buffer_indexed(engine._h, src.ctypes.data, src.size, idx.ctypes.data, idx.size, dst.ctypes.data, 16, C.byref(n), C.byref(info))
    assert rc == -7 and n.value == len(mixed) and bytes(dst) == bytes(16)


def test_several_rounds_under_a_window_of_one_megabyte(engine, monkeypatch):
    monkeypatch.setenv("MI_INFLATE_WINDOW_MB", "1")
    data = xc.local_binary(1 << 20) + dc.text(1 << 20, 334) + xc.local_binary(1 << 20)[::-1]
    gz = ic.one_stream(data, 6)
    info = _done(engine, gz, data, 0)
    assert info["n_rounds"] >= 3 and info["n_segments"] >= 6, info
    # a span beyond the window: no span is split, zlib takes the member
    ix, built = M.inflate_index_build(gz, 2 << 20)
    assert built["n_points"] == 2
    out, info = engine.inflate_buffer_indexed(gz, ix)
    assert out == b"" and info["verdict"] == M.INFLATE_NOT_PARALLEL and info["rule"] == ic.BEYOND_WINDOW and info["at_out"] == 0, info


# ---- 3. the index is only ever a hint ----------------------------------------------------------------------------------------------------
def _first_refusal(gz, ix):
    """the model's word on an index the checker lets through: the first span that does not decode as its row says"""
    for k, s in enumerate(xc.spans(ix)):
        row, _ = xc.decode_span(gz, s["in_bit"], s["end_bit"], s["hist"], s["out_bytes"])
        if row["rule"]:
            return k, s, row["rule"]
    return None


def _refused(engine, gz, ix, want=None):
    out, info = engine.inflate_buffer_indexed(gz, ix)                    # (no MiError: a refusal is a verdict)
    assert out == b"" and info["verdict"] == M.INFLATE_INDEX_REFUSED and info["out_bytes"] in (0, xc.parse(ix)["out_bytes"]), info
    if want is not None:
        k, s, rule = want
        assert (info["at_in"], info["at_out"], info["rule"]) == (s["in_bit"] // 8, s["out_at"], rule), (info, k, rule)
    return info


def short_window_member():
    """a member zlib refuses: 1 000 stored bytes, then a match at distance 1 500 -- beyond the window of the point behind the stored
    block, which is the stream's own start -- and an index of it made by hand, which the checker lets through"""
    d = ic.Deflate().stored(ic.noise(600, 340)).stored(ic.noise(1000, 341)).fixed([(257, 7 - 7, *dc.dist_symbol(1500)[::2]), 65, ic.EOB], 1)
    full, data = d.member()
    stream = full[10 + 605:-8]
    pretend = data[600:]
    gz = ic.member(stream, pretend)
    assert ic.zlib_inflates(gz) is None
    windows = pretend[:1000] + bytes(-1000 % 16)
    row = lambda bit, o, at, wb: bit.to_bytes(8, "little") + o.to_bytes(8, "little") + at.to_bytes(8, "little") + wb.to_bytes(4, "little") + bytes(4)
    head = xc.MAGIC + len(gz).to_bytes(8, "little") + len(pretend).to_bytes(8, "little") + gz[-8:] + (10).to_bytes(8, "little")
    head += (2).to_bytes(8, "little") + (1).to_bytes(8, "little") + len(windows).to_bytes(8, "little")
    return gz, head + row(80, 0, 0, 0) + row(80 + 8 * 1005, 1000, 0, 1000) + windows


def test_an_index_that_is_wrong_is_refused_with_the_span_and_the_rule(engine, mixed):
    gz, data, what = xc.planted_member()
    ix = xc.index(gz, 1)
    h = xc.parse(ix)
    by_out = {p["out_at"]: k for k, p in enumerate(h["points"])}
    # in_bit off by one: the span in front of it does not end where the index says
    k = by_out[what["straddle_plain"]]
    bad = xc.patch(ix, xc.row_at(k, "in_bit"), h["points"][k]["in_bit"] + 1)
    assert M.inflate_index_check(bad, gz)[0] == 0
    want = _first_refusal(gz, bad)
    assert want[0] == k - 1 and want[2] == xc.INDEX
    _refused(engine, gz, bad, want)
    # a wrong out_at (behind a full window, so that win_bytes stays right)
    k = by_out[what["far_second"]]
    bad = xc.patch(ix, xc.row_at(k, "out_at"), h["points"][k]["out_at"] + 1)
    assert M.inflate_index_check(bad, gz)[0] == 0
    want = _first_refusal(gz, bad)
    assert want[0] == k - 1 and want[2] == xc.INDEX
    _refused(engine, gz, bad, want)
    # a flipped window byte that a match reads (hist[0] of the span at distance 32 768): every span ends where it should, the CRC-32 tells
    k = by_out[what["far"]]
    at = 64 + 32 * h["n_points"] + h["points"][k]["win_at"]
    bad = ix[:at] + bytes((ix[at] ^ 0x40,)) + ix[at + 1:]
    assert M.inflate_index_check(bad, gz)[0] == 0 and _first_refusal(gz, bad) is None
    info = _refused(engine, gz, bad)
    assert info["rule"] == 0
    # a distance beyond a short window
    sgz, six = short_window_member()
    assert M.inflate_index_check(six, sgz)[0] == 0
    want = _first_refusal(sgz, six)
    assert want[0] == 1 and want[2] == ic.DISTANCE
    _refused(engine, sgz, six, want)
    # an index of another member: the checker's word, before anything goes up
    other = gzip.compress(mixed, 6)
    info = _refused(engine, other, ix)
    assert info["index_refusal"] == xc.R_MEMBER and info["rule"] == 0
    info = _refused(engine, gz, ix[:-1])
    assert info["index_refusal"] == xc.R_SIZES


def test_a_corrupt_blob_with_its_stale_index_goes_to_zlib(engine, mixed, tmp_path):
    gz = gzip.compress(mixed, 6)
    ix, _ = M.inflate_index_build(gz, 65536)
    at = len(gz) // 2
    bad = gz[:at] + bytes((gz[at] ^ 0x08,)) + gz[at + 1:]
    assert ic.zlib_inflates(bad) is None and M.inflate_index_check(ix, bad)[0] == 0
    _refused(engine, bad, ix)
    p = tmp_path / "bad.gz"
    p.write_bytes(bad)
    with pytest.raises(M.MiError) as host:
        M.tar_inflate(str(p), str(tmp_path / "host.tar"))
    with pytest.raises(M.MiError) as dev:
        engine.tar_inflate_indexed(str(p), ix, str(tmp_path / "dev.tar"))
    assert dev.value.code == host.value.code == -1
    tail = lambda e: str(e.value).split(str(p) + ": ", 1)[1]
    assert tail(dev) == tail(host) and "corrupt" in tail(host)                      # the fallback's zlib error, word for word
    assert (tmp_path / "dev.tar").exists() == (tmp_path / "host.tar").exists()        # what mi_tar_inflate leaves of a corrupt blob, no more


# ---- 4. mi_tar_inflate_ctx_indexed and the layer add -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_tar():
    """about 650 KB that zlib cuts into nine blocks or more: text, 400 KB of a binary, random bytes"""
    binary = xc.local_binary(400000)
    return lc.tarfile_tar(tarfile.GNU_FORMAT, extra=[("text-%d" % i, dc.text(50000, 50 + i)) for i in range(2)] +
                          [("bin-%d" % i, binary[i * 200000:(i + 1) * 200000]) for i in range(2)] + [("rnd", dc.random_bytes(70000, 9))])


def test_tar_inflate_indexed_gives_what_tar_inflate_gives(engine, tmp_path, small_tar):
    tar, _ = small_tar
    for name, blob in (("foreign", gzip.compress(tar)), ("no_reset", ic.no_reset(tar))):
        p = tmp_path / (name + ".gz")
        p.write_bytes(blob)
        ix, built = M.inflate_index_build(blob, 32768, want_digest=True)
        host = M.tar_inflate(str(p), str(tmp_path / "host.tar"))
        dev = engine.tar_inflate_indexed(str(p), ix, str(tmp_path / "dev.tar"))
        assert dev["info"]["verdict"] == M.INFLATE_DONE and dev["info"]["fell_back"] == 0 and dev["info"]["n_segments"] == built["n_points"] >= 4
        assert (tmp_path / "dev.tar").read_bytes() == (tmp_path / "host.tar").read_bytes() == tar
        assert (dev["tar_bytes"], dev["tar_digest"], dev["blob_digest"]) == (host["tar_bytes"], host["tar_digest"], host["blob_digest"])
        assert built["tar_digest"] == host["tar_digest"]                 # the first pull's digest comes out of the builder's pass
        assert engine.tar_inflate_indexed(str(p), ix)["tar_digest"] == host["tar_digest"]      # digests only
        # a refused index: the partial output is gone and the host path gives the same
        k = built["n_points"] - 1
        bad = xc.patch(ix, xc.row_at(k, "in_bit"), xc.parse(ix)["points"][k]["in_bit"] + 1)
        dev = engine.tar_inflate_indexed(str(p), bad, str(tmp_path / "dev2.tar"))
        assert dev["info"]["verdict"] == M.INFLATE_INDEX_REFUSED and dev["info"]["fell_back"] == 2, dev["info"]
        assert (tmp_path / "dev2.tar").read_bytes() == tar and dev["tar_digest"] == host["tar_digest"]


def _rows(b):
    return b.files().copy(), b.chunks().copy(), b.roots().copy()


def _same_rows(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a[0]) == len(b[0]) and len(a[1]) == len(b[1])


def test_a_foreign_gzip_becomes_a_batch_through_its_index(engine, tmp_path, small_tar):
    tar, members = small_tar
    blob = gzip.compress(tar)
    ix, built = M.inflate_index_build(blob, 32768)
    with engine.batch() as b:
        ents0, offs0, info0, sha0 = b.add_layer_blob(blob, 5)
        b.run()
        rows0 = _rows(b)
    assert info0["source"] == M.LAYER_SOURCE_DEVICE_GZIP
    k = built["n_points"] // 2
    stale = xc.patch(ix, xc.row_at(k, "in_bit"), xc.parse(ix)["points"][k]["in_bit"] + 1)
    p = tmp_path / "layer.gz"
    p.write_bytes(blob)
    for how, index, source, fell_back in (("blob", ix, M.LAYER_SOURCE_INDEXED_GZIP, 0), ("path", ix, M.LAYER_SOURCE_INDEXED_GZIP, 0),
                                          ("blob", stale, M.LAYER_SOURCE_DEVICE_GZIP, 2), ("blob", ix[:100], M.LAYER_SOURCE_DEVICE_GZIP, 2)):
        with engine.batch() as b:
            b.add_bytes(b"in front", 1)
            before = b.counts()
            ents, offs, info, sha = b.add_layer_blob_indexed(blob, index, 5) if how == "blob" else b.add_layer_path_indexed(str(p), index, 5)
            assert (ents, offs, sha) == (ents0, offs0, sha0) and sha == hashlib.sha256(blob).digest()
            assert (info["source"], info["inflate"]["fell_back"], info["tar_bytes"], info["n_files"]) == (source, fell_back, len(tar), len(members)), info
            assert info["inflate"]["verdict"] == M.INFLATE_DONE and info["first_file"] == 1 and b.counts()[0] == before[0] + len(members)
            if source == M.LAYER_SOURCE_INDEXED_GZIP:
                assert info["inflate"]["n_segments"] == built["n_points"] >= 4
            b.run()
            regs = [e for e in ents if e["kind"] == M.KIND_FILE]
            for e, (_, data) in zip(regs, members):
                assert b.read_file(1 + e["file_index"], 0, len(data)) == data, e["relpath"]
            files, chunks, roots = _rows(b)
            assert np.array_equal(roots[1:], rows0[2]) and np.array_equal(chunks["sha256"][1:], rows0[1]["sha256"])
    # a blob that is corrupt AND carries a stale index: the inflater's error, and the batch is what it was
    at = len(blob) // 2
    corrupt = blob[:at] + bytes((blob[at] ^ 0x08,)) + blob[at + 1:]
    with engine.batch() as b:
        b.add_bytes(b"in front", 1)
        with pytest.raises(M.MiError) as e:
            b.add_layer_blob_indexed(corrupt, ix, 5)
        assert e.value.code == -1 and b.counts()[0] == 1
        b.run()
        assert b.read_file(0, 0, 8) == b"in front"


# ---- 5. under the guard allocator --------------------------------------------------------------------------------------------------------
GUARDED = r'''
import sys
sys.path[:0] = [%(root)r, %(root)r + "/tests"]
import gzip
import makisu_amd as M
import deflate_cases as dc
import inflate_cases as ic
import inflate_index_cases as xc
gz, data, _ = xc.planted_member()
text = dc.text(300000, 350) + dc.random_bytes(5000, 351)
with M.Engine(device=0) as e:
    for blob, want, spacing in ((gz, data, 1), (ic.no_reset(text, 1 << 15), text, 16384), (gzip.compress(text), text, 0)):
        ix, _ = M.inflate_index_build(blob, spacing)
        out, info = e.inflate_buffer_indexed(blob, ix)
        assert info["verdict"] == M.INFLATE_DONE and out == want, info
print("OK")
'''


def test_no_read_leaves_the_member_or_the_windows_under_the_guard():
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", GUARDED % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr[-3000:]
