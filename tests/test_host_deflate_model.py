"""The device deflate leg without a GPU: the model of deflate_cases.py against zlib's inflate on every input the
GPU tests use, a few short forms pinned byte for byte by hand, the length-limiting rule on counts that need it, the split rule,
wrong models that must differ, the new prototypes, mi_deflate_bound, and the refusals that need no device."""
import ctypes as C
import os
import re
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import deflate_cases as dc  # noqa: E402

HEADER = os.path.join(ROOT, "include", "makisu_mi.h")


def _inputs():
    out = []
    for n in dc.LENGTHS:
        out += [("zeros-%d" % n, bytes(n)), ("text-%d" % n, dc.text(n)), ("random-%d" % n, dc.random_bytes(n)),
                ("two-%d" % n, dc.symbols(n, 2)), ("sixteen-%d" % n, dc.symbols(n, 16))]
    out += [("zeros-%d" % n, bytes(n)) for n in range(255, 268)]
    out += [("planted-32768", dc.planted(32768)), ("planted-32769", dc.planted(32769)), ("no-match", dc.no_match()),
            ("one-distance", dc.one_distance()), ("ll-clamped", dc.copies_piece(dc.LL_CLAMP_SEED)), ("cl-clamped", dc.records_piece(dc.CL_CLAMP_SEED))]
    out += [("near%+d" % d, dc.near_piece(s)) for d, s in dc.NEAR_SEEDS.items()]
    return out


INPUTS = _inputs()


@pytest.mark.parametrize("name,data", INPUTS, ids=[n for n, _ in INPUTS])
def test_the_models_blob_inflates_to_the_input_and_fits_the_bound(name, data):
    info = {}
    blob = dc.deflate_blob(data, info)
    assert dc.inflate(blob) == data
    assert len(blob) <= dc.deflate_bound(len(data)) and info["out_bytes"] == len(blob) and info["n_pieces"] == (len(data) + 65535) // 65536
    assert info["n_dynamic"] + info["n_stored"] == info["n_pieces"]
    if name.startswith("random-") and len(data) >= 64:                   # all pieces stored, a full piece as two blocks
        assert info["n_dynamic"] == 0 and len(blob) == sum(dc.stored_size(min(65536, len(data) - at)) for at in range(0, len(data), 65536))


def test_short_forms_pinned_by_hand():
    assert dc.deflate_blob(b"") == b""
    # one byte, 13 zeros: (D) is no smaller, so one stored block -- 00, LEN, ~LEN, the bytes
    assert dc.deflate_blob(b"a") == bytes.fromhex("00 0100 feff 61")
    assert dc.deflate_blob(bytes(13)) == bytes.fromhex("00 0d00 f2ff") + bytes(13)
    # "ab" * 40, a two-symbol piece: literals a, b, then one match of 78 at distance 2.  HLIT 278 (the length symbol 277, 67..82,
    # is the last), HDIST 2 (distance symbol 1, the only one: length 1); a, b, end-of-block and 277 take two bits each.  The first
    # byte: BFINAL 0, BTYPE 10, then HLIT - 257 = 21 = 10101 from bit 3 on: 0xAC.  Kept: the model must not move
    blob = dc.deflate_blob(b"ab" * 40)
    assert blob == bytes.fromhex("acc1810c0000008030d6f28748a21d5f010000ffff")
    plan = dc.piece_plan(b"ab" * 40)
    assert plan["items"] == [97, 98, (78, 2)] and (plan["hlit"], plan["hdist"]) == (278, 2)
    assert [plan["ll_lens"][s] for s in (97, 98, 256, 277)] == [2, 2, 2, 2] and plan["d_lens"][:2] == [0, 1]
    assert blob[-4:] == b"\x00\x00\xff\xff" and plan["d_size"] == 21 < plan["s_size"] == 85
    # a full piece of random bytes: 65 535 + 1
    r = dc.random_bytes(65536)
    assert dc.deflate_blob(r) == b"\x00\xff\xff\x00\x00" + r[:65535] + b"\x00\x01\x00\xfe\xff" + r[65535:]


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def _complete(lens, limit):
    return dc.kraft_sum(lens, limit) == 1 << limit and max(lens) <= limit


def test_the_length_limiting_rule_on_counts_that_need_it():
    counts = [0] * dc.N_LITLEN
    for k, c in enumerate(_fib(24)[1:]):                                 # 1 (the end-of-block symbol's), 1, 2, 3, 5, ...
        counts[3 * k + 1] = c
    counts[dc.EOB] = 1
    rep = {}
    lens = dc.code_lengths(counts, 15, rep)
    assert rep["free_depth"] > 15 and _complete(lens, 15)
    assert [bool(l) for l in lens] == [bool(c) for c in counts]
    # heavier symbols never get longer codes
    order = sorted((c, s) for s, c in enumerate(counts) if c)
    assert all(lens[a[1]] >= lens[b[1]] for a, b in zip(order, order[1:]))
    cl = [0] * dc.N_CL
    for k, c in enumerate(_fib(12)):
        cl[k] = c
    lens = dc.code_lengths(cl, 7, rep)
    assert rep["free_depth"] > 7 and _complete(lens, 7)
    # a code that needs no limit is Huffman's, complete by itself; two symbols are one bit each; one symbol is one bit
    assert dc.code_lengths([5, 0, 3], 15) == [1, 0, 1] and dc.code_lengths([0, 9], 15) == [0, 1] and dc.code_lengths([0, 0], 7) == [0, 0]
    assert dc.code_lengths([1, 1, 2, 4], 15) == [3, 3, 2, 1]
    # step 5 at work: 300 equal counts do not exist in deflate, but 19 under a limit of 5 do -- clamped, grown, then completed
    for n in range(2, 20):
        for limit in (5, 7):
            assert _complete(dc.code_lengths(_fib(n), limit), limit), (n, limit)
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(2, 286))
        c = [int(x) for x in rng.integers(0, 3, n) * rng.integers(1, 60000, n)]
        if sum(1 for x in c if x) >= 2:
            assert _complete(dc.code_lengths(c, 15), 15)
            c19 = c[:19]
            if sum(1 for x in c19 if x) >= 2:
                assert _complete(dc.code_lengths(c19, 7), 7)


def test_the_split_rule():
    want = {258: [258], 259: [256, 3], 260: [257, 3], 261: [258, 3], 262: [258, 4], 516: [258, 258], 517: [258, 256, 3], 3: [3], 4: [4],
            65536: [258] * 254 + [4], 65535: [258] * 254 + [3], 65534: [258] * 253 + [257, 3]}
    for length, parts in want.items():
        assert dc.split_length(length) == parts, length
    for length in range(3, 2000):
        parts = dc.split_length(length)
        assert sum(parts) == length and all(3 <= p <= 258 for p in parts)
    # zeros: a literal, then distance 1 in those parts
    for n in range(255, 268):
        assert dc.parse(bytes(n)) == [0] + [(p, 1) for p in dc.split_length(n - 1)]


def test_the_clamped_and_the_near_pieces_are_what_the_searches_report():
    seed, piece = dc.find_ll_clamped(dc.LL_CLAMP_SEED)
    rep = {}
    plan = dc.piece_plan(piece, rep)
    assert seed == dc.LL_CLAMP_SEED and rep["ll_free_depth"] > 15 and max(plan["ll_lens"]) == 15 and plan["dynamic"] and _complete(plan["ll_lens"], 15)
    seed, piece = dc.find_cl_clamped(dc.CL_CLAMP_SEED)
    plan = dc.piece_plan(piece, rep)
    assert seed == dc.CL_CLAMP_SEED and rep["cl_free_depth"] > 7 and max(plan["cl_lens"]) == 7 and plan["dynamic"] and _complete(plan["cl_lens"], 7)
    for delta, s in dc.NEAR_SEEDS.items():
        seed, piece = dc.find_near_stored(delta, s)
        plan = dc.piece_plan(piece)
        assert seed == s and plan["d_size"] - plan["s_size"] == delta and plan["dynamic"] == (delta < 0)
        assert len(dc.deflate_blob(piece)) == min(plan["d_size"] if delta < 0 else plan["s_size"], plan["s_size"])
    # the special distance codes: none at all, and one of length 1
    plan = dc.piece_plan(dc.no_match())
    assert plan["dynamic"] and plan["n_dist_symbols"] == 0 and plan["hdist"] == 1 and plan["d_lens"][0] == 0
    plan = dc.piece_plan(dc.one_distance())
    assert plan["dynamic"] and plan["n_dist_symbols"] == 1 and plan["d_lens"][0] == 1 and sum(plan["d_lens"]) == 1
    # the planted repeats: taken at 32 768, refused at 32 769
    assert (16, 32768) in dc.parse(dc.planted(32768))
    assert all(d <= 32768 for it in dc.parse(dc.planted(32769)) if isinstance(it, tuple) for d in [it[1]])
    assert not any(isinstance(it, tuple) and it[1] > 1 for it in dc.parse(dc.planted(32769)))


def _zlib_takes(blob, data):
    try:
        return dc.inflate(blob) == data
    except (zlib.error, AssertionError):
        return False


def test_wrong_models_differ_on_these_inputs():
    # distances to 32 769 allowed: the planted repeat is taken -- another parse, and one deflate has no distance symbol for
    p = dc.planted(32769)
    wrong = dc.parse(p, max_dist=32769)
    assert (16, 32769) in wrong and wrong != dc.parse(p)
    with pytest.raises(AssertionError):
        dc.deflate_blob(p, max_dist=32769)
    # an incomplete code left (step 5 missing): other bytes on the clamped pieces, and zlib refuses them
    for piece in (dc.copies_piece(dc.LL_CLAMP_SEED), dc.records_piece(dc.CL_CLAMP_SEED)):
        wrong = dc.deflate_blob(piece, complete=False)
        assert wrong != dc.deflate_blob(piece) and not _zlib_takes(wrong, piece)
    # a remainder of 2: 258 + 2 for a match of 260
    def bad_split(length):
        return [258] * (length // 258) + ([length % 258] if length % 258 else [])
    z = bytes(261)
    assert 2 in bad_split(260)
    with pytest.raises((AssertionError, TypeError)):
        dc.deflate_blob(z, split=bad_split)                              # (the model's own tables have no symbol for 2)


def test_the_new_prototypes_are_exported_and_tagged(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("mi_deflate_bound", "mi_deflate_buffer", "mi_layer_set_gzip_ctx"):
        assert re.search(r"^MI_BLOCK\s[^\n;]*\b%s\s*\(" % name, src, flags=re.M), name
        assert hasattr(engine_lib, name)
    assert re.search(r"^#define MI_MEMFS_GZIP_DEVICE 0x40u", src, flags=re.M) and re.search(r"^#define MI_ABI_VERSION 6$", src, flags=re.M)
    import makisu_amd as M
    assert M.MEMFS_GZIP_DEVICE == 0x40 and C.sizeof(M.DeflateInfo) == 48


def test_the_bound_is_monotone_and_enough_for_every_model_output(engine_lib):
    last = 0
    for n in list(range(0, 300)) + [65534, 65535, 65536, 65537, 131071, 131072, 131073, 3 * 65536 + 5, 1 << 30, (1 << 40) + 1]:
        b = engine_lib.mi_deflate_bound(n)
        assert b == dc.deflate_bound(n) and b >= last and b >= n
        last = b
    for _, data in INPUTS:
        if len(data) <= 65537:
            assert len(dc.deflate_blob(data)) <= engine_lib.mi_deflate_bound(len(data))
    assert engine_lib.mi_deflate_bound(65536) == dc.stored_size(65536) == 65546


def test_the_refusals_that_need_no_gpu(engine_lib, tmp_path):
    import makisu_amd as M
    INVALID, STATE = -1, -6
    fake_ctx = C.c_void_p(8)                                             # never touched: every call below is refused before it looks
    n, crc, buf = C.c_uint64(), C.c_uint32(), (C.c_uint8 * 64)()
    assert engine_lib.mi_deflate_buffer(None, buf, 1, buf, 64, C.byref(n), C.byref(crc), None) == INVALID
    assert engine_lib.mi_layer_set_gzip_ctx(None, fake_ctx) == INVALID
    for level in (M.GZIP_OFF, 0):
        l = M.Layer(gzip_level=level)
        try:
            assert engine_lib.mi_layer_set_gzip_ctx(l._h, None) == INVALID
            assert engine_lib.mi_layer_set_gzip_ctx(l._h, fake_ctx) == INVALID           # nothing to code
            assert "no gzip leg" in engine_lib.mi_layer_error(l._h).decode()
        finally:
            l.close()
    l = M.Layer(gzip_level=M.GZIP_DEFAULT)
    try:
        l.add({"relpath": "/d", "kind": 0, "mode": 0o40755, "mtime_sec": 1})
        assert engine_lib.mi_layer_set_gzip_ctx(l._h, fake_ctx) == STATE                 # after the first add
        assert l.finish()["gzip_bytes"] > 20                             # the refused call changed nothing: zlib's leg wrote the blob
    finally:
        l.close()
    # the commit option with ctx == NULL: MI_ERR_STATE before anything is walked; no effect at MI_GZIP_OFF
    root = tmp_path / "root"
    root.mkdir()
    (root / "f").write_bytes(b"x" * 100)
    with M.MemFS(str(root)) as fs:
        fs.set_options(gzip_device=True)
        with pytest.raises(M.MiError) as ei:
            fs.commit_layer(must_scan=True, gzip_level=M.GZIP_DEFAULT)
        assert ei.value.code == STATE and "MI_MEMFS_GZIP_DEVICE" in str(ei.value)
        assert not any(e["relpath"].endswith("f") for e in fs.entries())  # nothing was walked
        res = fs.commit_layer(must_scan=True, gzip_level=M.GZIP_OFF)
        assert res is not None and res["n_entries"] >= 1
    with M.MemFS(str(root)) as fs, M.MemFS(str(root)) as plain:          # ... and the same layer as without the option
        fs.set_options(gzip_device=True)
        a, b = fs.commit_layer(must_scan=True, gzip_level=M.GZIP_OFF), plain.commit_layer(must_scan=True, gzip_level=M.GZIP_OFF)
        assert a["tar_digest"] == b["tar_digest"] and a["tar_bytes"] == b["tar_bytes"]
