"""GPU tests of the layer-blob add (mi_batch_add_layer_blob): the header pass alone through tests/kernel_probe against the
model of layer_blob_cases.py; plain tars of every builder into a batch against mi_tar_open on the same bytes and against a twin batch
fed the members by add_bytes; the sources (device-leg gzip, host-leg gzip, foreign gzip inside and beyond what one wave inflates, plain);
rounds; position in the batch; the index and a zpack downstream; failures that leave the batch as it was; refusals; one scenario under
MI_GUARD_ALLOC=1 in a process of its own.  Every comparison is exact."""
import base64
import ctypes as C
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys
import tarfile

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
import layer_blob_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

PROBE_DIR = os.path.join(ROOT, "tests", "kernel_probe")
PROBE = os.path.join(PROBE_DIR, "libmi_tar_probe.so")
H, B = lc.HEADER, lc.BODY


@pytest.fixture(scope="module")
def engine():
    with M.Engine(device=0) as e:
        yield e


# ---- 1. the marking alone ---------------------------------------------------------------------------------------------------------------
def _build_probe():
    src = os.path.join(PROBE_DIR, "tar_probe.cpp")
    lib = os.path.join(ROOT, "makisu_amd", "libmakisu_mi.so")
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall",
                               src, "-o", PROBE, "-L", os.path.dirname(lib), "-lmakisu_mi",
                               "-Wl,-rpath,$ORIGIN/../../makisu_amd", "-Wl,--no-undefined"])
    return PROBE


@pytest.fixture(scope="module")
def probe(engine):
    lib = C.CDLL(_build_probe())
    lib.probe_tar_scan.restype = C.c_int
    lib.probe_tar_scan.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]

    def run(buf):
        """the buffer as it is -> [(block, kind)], the dense bytes"""
        d = torch.from_numpy(np.frombuffer(bytes(buf) + b"\x00", dtype=np.uint8).copy()).cuda()[:len(buf)]
        cap = len(buf) // 512 + 1
        n, blocks, kinds, dense = C.c_uint64(~0 & (2 ** 64 - 1)), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8), np.zeros(cap * 512, np.uint8)
        assert lib.probe_tar_scan(d.data_ptr(), len(buf), C.byref(n), blocks.ctypes.data, kinds.ctypes.data, dense.ctypes.data, cap) == 0
        k = n.value
        assert k <= cap
        return [(int(b), int(t)) for b, t in zip(blocks[:k], kinds[:k])], dense[:512 * k].tobytes()
    return run


def _probe_agrees(probe, buf):
    want = lc.marked_blocks(buf)
    got, dense = probe(buf)
    assert got == want, (len(buf), got[:8], want[:8])
    assert dense == b"".join(buf[512 * j:512 * j + 512] for j, _ in want)
    return want


def _sprinkled(n_blocks, seed, extra_tail=0):
    """n_blocks blocks of noise with headers every few blocks, meta headers among them, and headers on the plan tile's edge"""
    rng = np.random.default_rng(seed)
    blocks = [rng.integers(0, 256, 512, dtype=np.uint8).tobytes() for _ in range(n_blocks)]
    for j in range(0, n_blocks, 5):
        blocks[j] = lc.raw_header("m%d" % j, j, typeflag=b"xgLK0"[j % 7 % 5:j % 7 % 5 + 1])
    for j in (2046, 2047, 2048, n_blocks - 1):
        if 0 <= j < n_blocks:
            blocks[j] = lc.raw_header("edge%d" % j, 1, typeflag=b"x" if j % 2 else b"0")
    return b"".join(blocks) + rng.integers(0, 256, extra_tail, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("n_blocks", [1, 2, 2047, 2048, 2049])
def test_the_marking_at_the_plan_tiles_edge(probe, n_blocks):
    want = _probe_agrees(probe, _sprinkled(n_blocks, n_blocks))
    assert any(k & B for _, k in want) or n_blocks == 1


def test_the_marking_leaves_a_trailing_piece_alone(probe):
    for tail in (1, 511):
        buf = _sprinkled(9, 7, extra_tail=tail)
        assert _probe_agrees(probe, buf) == lc.marked_blocks(buf[:512 * 9])
        # a whole header in front of the piece, and a piece that would be a header's beginning
        buf = lc.raw_header("a", 0) + lc.raw_header("b", 0)[:tail]
        assert _probe_agrees(probe, buf) == [(0, H)]
    assert probe(lc.raw_header("a", 0)[:511]) == ([], b"") and probe(b"\x01") == ([], b"")


def test_the_marking_with_no_header_and_with_nothing_but_headers(probe):
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, 512 * 300, dtype=np.uint8).tobytes()
    assert _probe_agrees(probe, noise) == [] and _probe_agrees(probe, bytes(512 * 64)) == []
    headers = b"".join(lc.raw_header("h%d" % j, j) for j in range(300))
    assert _probe_agrees(probe, headers) == [(j, H) for j in range(300)]
    metas = b"".join(lc.raw_header("h%d" % j, j, typeflag=b"L") for j in range(40))
    assert _probe_agrees(probe, metas) == [(0, H)] + [(j, H | B) for j in range(1, 40)]


def test_the_marking_of_a_meta_header_in_the_last_blocks(probe):
    data = b"\x07" * 512
    x = lc.raw_header("PaxHeaders/x", 700, typeflag=b"x")
    assert _probe_agrees(probe, data * 3 + x) == [(3, H)]
    assert _probe_agrees(probe, data * 3 + x + data) == [(3, H), (4, B)]
    assert _probe_agrees(probe, data * 3 + x + data * 2) == [(3, H), (4, B), (5, B)]
    assert _probe_agrees(probe, data * 3 + x + data * 3) == [(3, H), (4, B), (5, B)]


def test_the_marking_of_hand_made_headers_and_of_a_tar_inside_a_tar(probe):
    hand, members = lc.hand_made_tar()
    want = _probe_agrees(probe, hand)
    assert sum(1 for _, k in want if k & H) == len(members) + 1           # every member's header and the g header
    assert lc.marked_blocks(hand, header=lc.is_header_forgets_signed) != want and lc.marked_blocks_no_body(hand) != want
    for form, (field, signed) in lc.CHECKSUM_FORMS.items():
        blk = lc.raw_header(b"n\xff\xfe\x80" if signed else b"name", 3, chksum=field, signed=signed)
        flipped = bytearray(blk)
        flipped[153 if form in ("usual", "signed sum", "NULs behind", "spaces behind") else 155] ^= 1
        assert _probe_agrees(probe, blk + bytes(flipped) + blk) == [(0, H), (2, H)], form
    many_high = bytearray(b"\xff" * 512)                                   # a negative base-256 field against the signed sum
    many_high[148:156] = b"\xff" * 7 + b"\x08"
    assert _probe_agrees(probe, bytes(many_high)) == [(0, H)]
    nested, _ = lc.nested_tar()
    assert len(_probe_agrees(probe, nested)) > 2


# ---- 2. plain tars into a batch ---------------------------------------------------------------------------------------------------------
def _rows(b):
    return b.files().copy(), b.chunks().copy(), b.roots().copy()


def _same_rows(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a[0]) == len(b[0]) and len(a[1]) == len(b[1])


def _twin(engine, parts):
    """a batch fed (data, tag) by add_bytes in this order, run: its rows"""
    with engine.batch() as b:
        for data, tag in parts:
            b.add_bytes(data, tag)
        b.run()
        return _rows(b)


def _host_listing(tmp_path, tar):
    p = tmp_path / ("t%d.tar" % len(list(tmp_path.iterdir())))
    p.write_bytes(tar)
    return M.tar_entries(str(p))


def _chain(tar):
    """the live chain, walked here: (headers on it, meta bodies beyond what travels, ended on a zero block?)"""
    off, live, big, size_override = 0, 0, 0, None
    while off + 512 <= len(tar):
        blk = tar[off:off + 512]
        if blk == bytes(512):
            return live, big, True
        live += 1
        size, t = lc.number(blk[124:136]), blk[156:157]
        if t in (b"x", b"g", b"L", b"K"):
            big += size > 512 * lc.META_INLINE
            m = re.search(rb"\d+ size=(\d+)\n", tar[off + 512:off + 512 + size]) if t == b"x" else None
            size_override = int(m.group(1)) if m else None
            off += 512 + (size + 511) // 512 * 512
            continue
        if size_override is not None:
            size, size_override = size_override, None
        off += 512 + (0 if t in (b"1", b"2", b"3", b"4", b"5", b"6") else (size + 511) // 512 * 512)
    return live, big, False


def _add_and_check(engine, tmp_path, blob, tar, members, source, tag_base=0):
    host = _host_listing(tmp_path, tar)
    with engine.batch() as b:
        ents, offs, info, sha = b.add_layer_blob(blob, tag_base)
        assert ents == host and offs == [e["data_offset"] for e in host]
        assert sha == hashlib.sha256(blob).digest()
        assert (info["tar_bytes"], info["arena_at"], info["first_file"], info["source"]) == (len(tar), 0, 0, source), info
        assert (info["n_files"], info["n_entries"]) == (len(members), len(host)) and b.counts()[0] == len(members)
        live, big, marker = _chain(tar)
        assert info["n_live"] == live and info["n_marked"] >= info["n_live"], (info, live)
        assert info["n_marked"] == len(lc.marked_blocks(tar))
        assert info["n_fetched"] == big + (1 if marker else 0), (info, big, marker)
        regs = [e for e in ents if e["kind"] == M.KIND_FILE]
        assert [e["file_index"] for e in regs] == list(range(len(members))) and [e["size"] for e in regs] == [len(d) for _, d in members]
        if not members:                                                   # (an archive without a regular member: nothing to run)
            return info, None
        b.run()
        for e, (_, data) in zip(regs, members):
            assert b.read_file(e["file_index"], 0, len(data)) == data, e["relpath"]
        rows = _rows(b)
        assert _same_rows(rows, _twin(engine, [(d, tag_base + i) for i, (_, d) in enumerate(members)]))
        assert b.read_back().tobytes() == b"".join(d for _, d in members)
    return info, rows


BUILDERS = {
    "ustar": lambda: lc.tarfile_tar(tarfile.USTAR_FORMAT),
    "gnu": lambda: lc.tarfile_tar(tarfile.GNU_FORMAT, extra=[(lc.long_name(1023), b"inline"), (lc.long_name(1025), b"fetched")]),
    "pax": lambda: lc.tarfile_tar(tarfile.PAX_FORMAT, extra=[(lc.long_name(900), b"inline"), (lc.long_name(1100), b"fetched"), (lc.long_name(2000), b"too")]),
    "no end marker": lambda: lc.tarfile_tar(tarfile.USTAR_FORMAT, end_marker=False),
    "hand made": lc.hand_made_tar,
    "nested": lc.nested_tar,
    "pax size override": lc.pax_size_override,
    "empty archive": lambda: (lc.END, []),
    "nothing at all": lambda: (b"", []),
}


@pytest.mark.parametrize("builder", sorted(BUILDERS))
def test_a_plain_tar_becomes_a_batch(engine, tmp_path, builder):
    tar, members = BUILDERS[builder]()
    info, _ = _add_and_check(engine, tmp_path, tar, tar, members, M.LAYER_SOURCE_TAR, tag_base=1000)
    fetched = {"gnu": 2, "pax": 3, "no end marker": 0, "nothing at all": 0}.get(builder, 1)
    assert info["n_fetched"] == fetched, info                            # the bodies beyond 1 024 bytes and the end marker's one
    if builder == "nested":
        assert info["n_marked"] > info["n_live"]
    elif builder != "hand made":
        assert info["n_marked"] == info["n_live"] + {"gnu": 4, "pax": 6, "pax size override": 1}.get(builder, 0)   # + the BODY blocks


def test_add_layer_path_maps_the_file(engine, tmp_path):
    tar, members = lc.tarfile_tar(tarfile.GNU_FORMAT)
    p = tmp_path / "layer.tar"
    p.write_bytes(tar)
    with engine.batch() as b:
        ents, _, info, sha = b.add_layer_path(str(p), 5)
        assert ents == M.tar_entries(str(p)) and sha == hashlib.sha256(tar).digest() and info["n_files"] == len(members)
        b.run()
        assert _same_rows(_rows(b), _twin(engine, [(d, 5 + i) for i, (_, d) in enumerate(members)]))
        with pytest.raises(M.MiError) as ei:
            engine.batch().add_layer_path(str(tmp_path / "missing"))
        assert ei.value.code == -5 and "missing" in str(ei.value)


# ---- 3. the sources ---------------------------------------------------------------------------------------------------------------------
def _device_leg(engine, data):
    blob, _, _ = engine.deflate_buffer(data)
    return ic.member(blob + b"\x03\x00", data, bytes((0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 255)))


@pytest.fixture(scope="module")
def big_tar():
    """about 300 KB; the member `rep` repeats itself at a distance that reaches across a 65 536-byte flush"""
    rep = lc.content(20000, 99)
    return lc.tarfile_tar(tarfile.GNU_FORMAT, extra=[("big-%d" % i, lc.content(50000, 50 + i)) for i in range(3)] + [("rep", rep * 4)])


def test_every_source_gives_the_same_batch(engine, tmp_path, big_tar):
    tar, members = big_tar
    assert 280000 < len(tar) < 340000
    forms = [("plain", tar, M.LAYER_SOURCE_TAR), ("device leg", _device_leg(engine, tar), M.LAYER_SOURCE_DEVICE_GZIP),
             ("host leg", ic.host_leg(tar, block=1 << 16), M.LAYER_SOURCE_DEVICE_GZIP),
             ("foreign, one stream", gzip.compress(tar), M.LAYER_SOURCE_DEVICE_GZIP),      # no marker: one wave inflates it, up to the window
             ("foreign, not parallel", ic.no_reset(tar), M.LAYER_SOURCE_ZLIB)]
    rows = None
    for name, blob, source in forms:
        info, r = _add_and_check(engine, tmp_path, blob, tar, members, source)
        inf = info["inflate"]
        if source == M.LAYER_SOURCE_DEVICE_GZIP:
            assert inf["verdict"] == M.INFLATE_DONE and inf["fell_back"] == 0 and inf["out_bytes"] == len(tar) and inf["in_bytes"] == len(blob), (name, inf)
            assert (inf["n_segments"] == 1) == (name == "foreign, one stream"), (name, inf)
        elif source == M.LAYER_SOURCE_ZLIB:
            assert inf["verdict"] == M.INFLATE_NOT_PARALLEL and inf["fell_back"] == 1 and ic.zlib_inflates(blob) == tar, (name, inf)
        assert rows is None or _same_rows(rows, r), name
        rows = r


def test_a_foreign_gzip_beyond_the_window_goes_through_zlib(engine, tmp_path, monkeypatch):
    monkeypatch.setenv("MI_INFLATE_WINDOW_MB", "1")
    tar, members = lc.tarfile_tar(tarfile.USTAR_FORMAT, extra=[("big-%d" % i, lc.content(300000, 60 + i)) for i in range(4)])
    assert len(tar) > 1 << 20
    info, _ = _add_and_check(engine, tmp_path, gzip.compress(tar), tar, members, M.LAYER_SOURCE_ZLIB)
    assert info["inflate"]["rule"] == ic.BEYOND_WINDOW


def test_the_references_go_written_layer_blob(engine, tmp_path):
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "sha256_reference_fixtures.json")))["vectors"][0]
    assert vec["name"] == "alpine_layer_blob"
    blob = base64.b64decode(vec["file_b64"])
    p = tmp_path / "test_layer.tar"
    p.write_bytes(blob)
    host = M.tar_entries(str(p))                                         # mi_tar_open_ex on the blob: through zlib
    tar = ic.zlib_inflates(blob)
    with engine.batch() as b:
        ents, offs, info, sha = b.add_layer_blob(blob)
        assert ents == host and len(host) > 0 and sha == hashlib.sha256(blob).digest() and info["tar_bytes"] == len(tar)
        assert info["source"] in (M.LAYER_SOURCE_DEVICE_GZIP, M.LAYER_SOURCE_ZLIB)
        b.run()
        for e in ents:
            if e["kind"] == M.KIND_FILE:
                assert b.read_file(e["file_index"], 0, e["size"]) == tar[e["data_offset"]:e["data_offset"] + e["size"]]


# ---- 4. rounds --------------------------------------------------------------------------------------------------------------------------
def test_rounds_through_both_slots_write_the_same_bytes(engine, tmp_path, monkeypatch):
    tar, members = lc.tarfile_tar(tarfile.USTAR_FORMAT, extra=[("big-%d" % i, lc.content(500000 + 1111 * i, 70 + i)) for i in range(5)])
    assert 2.4 * (1 << 20) < len(tar) < 2.8 * (1 << 20)
    blob = ic.host_leg(tar)                                              # a segment a MiB, none aligned to anything: the members' sizes are odd
    info, rows = _add_and_check(engine, tmp_path, blob, tar, members, M.LAYER_SOURCE_DEVICE_GZIP)
    assert info["inflate"]["n_rounds"] == 1
    monkeypatch.setenv("MI_INFLATE_WINDOW_MB", "1")
    info1, rows1 = _add_and_check(engine, tmp_path, blob, tar, members, M.LAYER_SOURCE_DEVICE_GZIP)
    assert info1["inflate"]["n_rounds"] >= 3 and info1["inflate"]["n_segments"] == info["inflate"]["n_segments"]
    assert _same_rows(rows, rows1)
    # the device leg's segments end wherever a piece ends: rounds that begin at odd output offsets
    body = tar.rstrip(b"\x00")                                           # (without the end marker and the record's padding)
    tar2 = body + bytes(-len(body) % 512) + lc.member("odd", b"o" * 77) + lc.END
    blob2 = _device_leg(engine, tar2)
    info2, _ = _add_and_check(engine, tmp_path, blob2, tar2, members + [(b"odd", b"o" * 77)], M.LAYER_SOURCE_DEVICE_GZIP)
    assert info2["inflate"]["n_rounds"] >= 3


# ---- 5. position ------------------------------------------------------------------------------------------------------------------------
def test_a_layer_behind_files_in_front_of_files_and_two_layers(engine, tmp_path, big_tar):
    tar, members = big_tar
    tar2, members2 = lc.hand_made_tar()
    first, last = [lc.content(3000, 201), lc.content(100, 202), lc.content(70001, 203)], [lc.content(5, 204), lc.content(66000, 205)]
    with engine.batch() as b:
        for i, d in enumerate(first):
            b.add_bytes(d, 10 + i)
        ents, _, info, _ = b.add_layer_blob(ic.host_leg(tar, block=1 << 16), tag_base=100)
        assert info["first_file"] == 3 and info["arena_at"] > 0 and info["arena_at"] % 256 == 0
        b.add_bytes(last[0], 20)
        ents2, _, info2, _ = b.add_layer_blob(tar2, tag_base=500)
        assert info2["first_file"] == 3 + len(members) + 1 and info2["arena_at"] >= info["arena_at"] + len(tar) and info2["arena_at"] % 256 == 0
        b.add_bytes(last[1], 21)
        assert b.counts()[0] == 3 + len(members) + 1 + len(members2) + 1
        b.run()
        for e, (_, d) in zip([e for e in ents2 if e["kind"] == M.KIND_FILE], members2):
            assert b.read_file(info2["first_file"] + e["file_index"], 0, len(d)) == d
        parts = [(d, 10 + i) for i, d in enumerate(first)] + [(d, 100 + i) for i, (_, d) in enumerate(members)] + [(last[0], 20)]
        parts += [(d, 500 + i) for i, (_, d) in enumerate(members2)] + [(last[1], 21)]
        assert _same_rows(_rows(b), _twin(engine, parts))
        assert [int(t) for t in b.files()["user_tag"]] == [t for _, t in parts]


# ---- 6. downstream ----------------------------------------------------------------------------------------------------------------------
def test_the_index_and_a_zpack_see_an_ordinary_batch(engine, big_tar):
    tar, members = big_tar
    got = []
    for layer in (True, False):
        with engine.batch() as b, M.ChunkIndex(engine) as ix:
            if layer:
                b.add_layer_blob(_device_leg(engine, tar))
            else:
                for i, (_, d) in enumerate(members):
                    b.add_bytes(d, i)
            b.run()
            known, n_new, n_known = ix.add_batch(b)
            with b.zpack(verify=True) as z:
                got.append((known.copy(), n_new, n_known, z.entries().copy(), z.read()))
    a, t = got
    assert np.array_equal(a[0], t[0]) and a[1:3] == t[1:3] and a[1] > 0
    assert np.array_equal(a[3], t[3]) and a[4] == t[4]


# ---- 7. failure leaves the batch as it was ----------------------------------------------------------------------------------------------
def _tar_error(tmp_path, tar):
    p = tmp_path / ("bad%d.tar" % len(list(tmp_path.iterdir())))
    p.write_bytes(tar)
    with pytest.raises(M.MiError) as ei:
        M.tar_entries(str(p))
    return str(ei.value).split(str(p) + ": ", 1)[1]


def _fails_and_leaves_the_batch(engine, blob, text, code=-1):
    first = [lc.content(3000, 301), lc.content(70001, 302)]
    with engine.batch() as b:
        b.add_bytes(first[0], 1)
        counts = b.counts()
        with pytest.raises(M.MiError) as ei:
            b.add_layer_blob(blob, 7)
        assert ei.value.code == code and text in str(ei.value), (str(ei.value), text)
        assert b.counts() == counts
        b.add_bytes(first[1], 2)
        b.run()
        assert _same_rows(_rows(b), _twin(engine, [(first[0], 1), (first[1], 2)]))
        assert b.read_back().tobytes() == first[0] + first[1]
    return str(ei.value)


def test_a_tar_error_is_the_parsers_and_leaves_the_batch(engine, tmp_path):
    tar, _ = lc.tarfile_tar(tarfile.USTAR_FORMAT)
    third = [m.offset for m in tarfile.open(fileobj=__import__("io").BytesIO(tar)).getmembers()][3]
    bad = bytearray(tar)
    bad[third + 5] ^= 1                                                   # a header on the chain whose checksum is wrong now
    text = _tar_error(tmp_path, bytes(bad))
    assert text == "bad tar header checksum at offset %d" % third
    for blob in (bytes(bad), ic.host_leg(bytes(bad))):
        _fails_and_leaves_the_batch(engine, blob, "mi_batch_add_layer_blob: " + text)
    cut = tar[:len(tar) - 10240 - 4096]                                   # the last member runs past the end
    text = _tar_error(tmp_path, cut)
    assert "runs past the end of the archive" in text
    for blob in (cut, _device_leg(engine, cut)):
        _fails_and_leaves_the_batch(engine, blob, "mi_batch_add_layer_blob: " + text)
    text = _tar_error(tmp_path, tar[:1024 + 100])                         # a last block of 100 bytes
    _fails_and_leaves_the_batch(engine, tar[:1024 + 100], "mi_batch_add_layer_blob: " + text)


def test_a_corrupt_gzip_is_the_inflaters_and_leaves_the_batch(engine, big_tar):
    tar, _ = big_tar
    good = ic.host_leg(tar, block=1 << 16)
    crc = bytearray(good)
    crc[-8] ^= 1                                                          # a wrong trailer CRC: found on the device, behind the last round
    flipped = bytearray(good)
    flipped[len(good) // 2] ^= 0x10                                       # a byte of a live segment
    for blob, words in ((bytes(crc), "the trailer states"), (bytes(flipped), None)):
        assert ic.zlib_inflates(blob) is None
        said = None                                                       # what mi_inflate_buffer says of the same blob
        try:
            _, inf = engine.inflate_buffer(blob)
            assert inf["verdict"] == M.INFLATE_NOT_PARALLEL and words is None      # (the flip may hand the blob to zlib, which refuses it)
        except M.MiError as e:
            assert e.code == -1
            said = str(e).split("mi_inflate_buffer: ", 1)[1]
            assert "corrupt gzip stream" in said and (words is None or words in said)
        got = _fails_and_leaves_the_batch(engine, blob, "corrupt gzip stream")
        assert said is None or got.split("mi_batch_add_layer_blob: ", 1)[1] == said
    broken = bytearray(ic.no_reset(tar))                                  # not parallel AND corrupt: zlib says so
    broken[len(broken) // 2] ^= 0x10
    if ic.zlib_inflates(bytes(broken)) is None:
        _fails_and_leaves_the_batch(engine, bytes(broken), "corrupt gzip stream")


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    tar, _ = lc.hand_made_tar()
    with engine.batch() as b:
        b.add_bytes(b"abc", 0)
        b.run()
        rows = _rows(b)
        with pytest.raises(M.MiError) as ei:
            b.add_layer_blob(tar)
        assert ei.value.code == -6 and "batch already ran; begin a new batch" in str(ei.value)
        assert _same_rows(_rows(b), rows)
        h = C.c_void_p(1)
        assert engine._lib.mi_batch_add_layer_blob(b._h, None, 0, 0, C.byref(h), None, None) == -1 and h.value is None
        assert engine._lib.mi_batch_add_layer_path(b._h, None, 0, None, None, None) == -1
    assert engine._lib.mi_batch_add_layer_blob(None, tar, len(tar), 0, None, None, None) == -1
    # a group head is not reachable through the ABI by itself (mi_batch_group_begin is hidden and no public call hands the handle's
    # batch out), so the group refusal runs in no test -- as mi_batch_pack_chunks' (tests/test_gpu_chunk_pack.py); DESIGN.md 4.21 says so
    src = open(os.path.join(ROOT, "makisu_amd", "csrc", "mi_layerblob.hip")).read()
    assert 'if (b->group) return fail(c, MI_ERR_INVALID, "mi_batch_add_layer_blob: a batch group has one arena per GPU' in src


# ---- 9. under the guard -----------------------------------------------------------------------------------------------------------------
GUARDED = r'''
import sys, tarfile
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import makisu_amd as M
import inflate_cases as ic
import layer_blob_cases as lc
tar, members = lc.tarfile_tar(tarfile.GNU_FORMAT, extra=[(lc.long_name(1025), b"fetched")])
tar += b"\x01" * 7                                   # behind the end marker: 512 k + 7 bytes, the last block is no block
assert len(tar) %% 512 == 7
with M.Engine(device=0) as eng:
    roots = None
    for blob in (tar, ic.host_leg(tar, block=1 << 16)):
        with eng.batch() as b:
            ents, offs, info, sha = b.add_layer_blob(blob)
            assert info["tar_bytes"] == len(tar) and info["n_files"] == len(members) and info["n_fetched"] == 2, info
            b.run()
            assert b.read_back().tobytes() == b"".join(d for _, d in members)
            r = b.roots().copy()
            assert roots is None or np.array_equal(roots, r)
            roots = r
print("OK")
'''


def test_no_read_leaves_the_tar_under_the_guard():
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", GUARDED % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr[-3000:]
