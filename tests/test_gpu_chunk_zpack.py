"""GPU tests of the compressed packs (mi_pack_compress, mi_zpack_*, mi_packset_add_zblob, mi_packset_add_zpack): every blob and
every entry array the device produces is compared byte for byte with the model of zpack_cases.py, every set fed from a compressed
pack is compared with the plain pack -- planted chunks whose sequence lists are known by construction (literal runs, match
lengths, offsets and steps at every edge), the raw rule on both sides of its threshold, the scan's block edges, the round trip
through a batch, everything that is refused, and the bounds under the guard allocator.  Bit for bit: there are no tolerances."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import pack_cases as pc  # noqa: E402
import restore_cases as rc  # noqa: E402
import zpack_cases as zc  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_zentries(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]), np.asarray(want[f]))
                                         for f in ("digest", "offset", "chunk_index", "length", "stored"))


def _pack_of_chunks(engine, chunks, alg=pc.SHA256):
    """distinct chunks -> a Pack that holds them in this order (through a set: mi_packset_pack takes any length)"""
    entries, blob = zc.pack_of(chunks, alg)
    with engine.packset() as s:
        s.add_blob(blob, entries, verify=True)
        p = s.pack(np.ascontiguousarray(entries["digest"]), verify=True)
    assert pc.same_entries(p.entries(), entries) and p.bytes() == blob
    return p, entries, blob


def _compress_and_compare(engine, pack, alg, verify=True):
    """pack.compress() against the model, mi_zpack_check, and both ways back into a set against the plain pack;
    -> (zentries, zblob)"""
    entries, blob = pack.entries().copy(), pack.bytes()
    want_e, want_b = zc.model_compress(entries, blob)
    with pack.compress(verify=verify) as z:
        got_e, got_b, info = z.entries().copy(), z.read(), z.info
        assert _same_zentries(got_e, want_e), [(k, int(got_e["stored"][k]), int(want_e["stored"][k])) for k in range(len(want_e))
                                              if got_e["stored"][k] != want_e["stored"][k] or got_e["offset"][k] != want_e["offset"][k]][:10]
        assert got_b == want_b, next(i for i in range(len(want_b)) if i >= len(got_b) or got_b[i] != want_b[i])
        assert (info.n_entries, info.blob_bytes, info.chunk_bytes, info.stored_bytes, info.n_raw, info.alg, info.verified) == \
            (len(want_e), len(want_b), int(want_e["length"].sum()), int(want_e["stored"].sum()),
             int((want_e["stored"] == want_e["length"]).sum()), alg, int(verify))
        assert len(z) == len(want_e) and z.read(0, 0) == b""
        if len(want_e):
            assert info.ms_encode > 0 and info.ms_compact > 0 and (info.ms_verify > 0) == verify
            assert (0 < info.ms_decode < info.ms_verify) == verify
            assert z.read(16, len(want_b) - 16) == want_b[16:]
        assert pack.bytes() == blob and pc.same_entries(pack.entries(), entries)           # the input is unchanged
        assert M.zpack_check(got_b, got_e, alg=alg) is None
        dig = np.ascontiguousarray(entries["digest"])
        distinct = len({bytes(d) for d in dig})
        for feed in ("zblob", "zpack"):
            with engine.packset() as s:
                if feed == "zblob":
                    s.add_zblob(got_b, got_e, verify=True)
                else:
                    s.add_zpack(z, verify=True)
                si = s.info
                assert (si.n_packs, si.n_entries, si.n_digests) == (1, len(want_e), distinct)
                assert si.blob_bytes == sum(pc.round16(int(k)) for k in entries["length"])
                if len(want_e) and distinct == len(want_e):
                    with s.pack(dig, entries["length"].astype(np.uint32), verify=True) as back:
                        assert back.bytes() == blob
        assert z.read() == want_b                                                             # ... and so is the zpack
    return got_e, got_b


# ---- 1. planted chunks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", [pc.SHA256, pc.BLAKE2S])
def test_planted_chunks_code_to_the_models_bytes_and_decode_to_their_own(alg):
    cases = zc.planted_chunks()
    chunks = [c for _, c, _ in cases]
    # what the planting guarantees, held against the model here (tests/test_host_chunk_zpack.py holds the rest)
    for name, chunk, want in cases:
        if want is not None and len(chunk) >= zc.MIN_CHUNK:
            assert zc.parse(chunk) == want, name
    stored = {name: len(zc.compress_chunk(c)) for name, c, _ in cases}
    assert stored["block of 141 for 150"] == 150 and stored["block of 141 for 151"] == 141
    assert stored["zeros"] == 267 and stored["random 65536"] == 65536 and stored["text 13"] == 13
    with M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0) as e:
        p, entries, blob = _pack_of_chunks(e, chunks, alg)
        with p:
            got_e, _ = _compress_and_compare(e, p, alg)
        for (name, chunk, want), en in zip(cases, got_e):
            assert (int(en["stored"]) < len(chunk)) == (stored[name] < len(chunk)), name
        # the same chunks in reverse order: another layout, the same stored forms
        p2, _, _ = _pack_of_chunks(e, chunks[::-1], alg)
        with p2:
            rev_e, _ = _compress_and_compare(e, p2, alg, verify=False)
        assert rev_e["stored"].tolist() == got_e["stored"].tolist()[::-1]


def test_a_chunk_of_200000_bytes_and_the_offset_limit():
    """the same 8 bytes 65 535 apart are a match, 65 536 apart they stay literals; positions beyond 2^17.  A table of 4 096
    slots forgets a position long before 65 535 others have gone in, so the bytes in between are ONE match (a period of 200:
    its positions beyond the step do not go into the table) and the sources lie just in front of it"""
    rng = np.random.default_rng(92)
    n = 200_000
    for _ in range(50):
        a = zc.filler(rng, n)
        zc.plant(a, 65_800, 66_000, 65_482)                        # ends at 131 482
        zc.plant(a, 65_950, 65_950 + 65_535, 8)                    # lane 3 of the next step: found, offset 65 535
        zc.plant(a, 65_970, 65_970 + 65_536, 8)                    # 13 bytes on: one too far, stays literals
        want = [(66_000, 200, 65_482), (3, 65_535, 8), (n - 131_493, None, None)]
        if zc.parse(a) == want:
            break
    else:
        raise AssertionError("no filler")
    chunk = bytes(a)
    assert chunk[65_970:65_978] == chunk[131_506:131_514] and len(zc.compress_chunk(chunk)) < n - (n >> 4)
    with M.Engine(max_size=262144) as e:
        p, _, _ = _pack_of_chunks(e, [chunk, chunk[:70_007]])
        with p:
            got_e, _ = _compress_and_compare(e, p, pc.SHA256)
        assert int(got_e["stored"][0]) < n and int(got_e["stored"][1]) == 70_007


# ---- 2. pack shapes ----------------------------------------------------------------------------------------------------------------
def test_pack_shapes_at_the_scans_block_edges_and_every_residue_at_the_blobs_end():
    rng = np.random.default_rng(93)
    pool = rng.integers(0, 256, (4097, 16), dtype=np.uint8)
    assert len({bytes(x) for x in pool}) == 4097
    with M.Engine() as e:
        for n in (0, 1, 2047, 2048, 2049, 4097):
            if n == 0:
                with e.packset() as s, s.pack(np.zeros((0, 32), dtype=np.uint8)) as p:
                    _compress_and_compare(e, p, pc.SHA256)
                continue
            # mostly raw 16-byte chunks; every 100th a chunk that is coded, so that offsets and sizes differ along the scan
            chunks = [bytes(pool[i]) if i % 100 else zc.text_like(200 + i, i) for i in range(n)]
            p, _, _ = _pack_of_chunks(e, chunks)
            with p:
                got_e, _ = _compress_and_compare(e, p, pc.SHA256, verify=(n != 2048))
            assert (got_e["stored"] < got_e["length"]).sum() == (n + 99) // 100
        # the blob's end: a last entry whose stored size is 0, 1 and 15 mod 16
        for mod in (0, 1, 15):
            tail = zc.tail_chunk(rng, (mod + 5) % 16, mod)
            p, _, _ = _pack_of_chunks(e, [bytes(pool[0]), zc.text_like(999, mod), tail])
            with p:
                got_e, got_b = _compress_and_compare(e, p, pc.SHA256)
            assert int(got_e["stored"][-1]) % 16 == mod and int(got_e["stored"][-1]) < len(tail)
            assert len(got_b) == int(got_e["offset"][-1]) + pc.round16(int(got_e["stored"][-1]))


@pytest.mark.parametrize("alg", [pc.SHA256, pc.BLAKE2S])
def test_a_batchs_pack_with_repeated_digests_and_1100_one_byte_chunks(alg):
    """more than 1 024 entries in one 16 KiB tile of the gather; digests that repeat (a set keeps each once)"""
    rng = np.random.default_rng(94)
    with M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0) as e, e.batch() as b:
        for i in range(1100):
            b.add_bytes(bytes([int(rng.integers(0, 256))]), i)
        block = zc.text_like(40_000, 5)
        b.add_bytes(block + block + zc.text_like(9000, 6), 2000)
        b.run()
        chunks = b.chunks()
        name = "sha256"
        assert len(chunks) > 1100 and len({bytes(d) for d in chunks[name]}) < len(chunks) - 800
        with b.pack(verify=True) as p:
            assert len(p) == len(chunks)
            got_e, _ = _compress_and_compare(e, p, alg)
        assert got_e["stored"][:1100].tolist() == [1] * 1100 and (got_e["stored"][1100:] < got_e["length"][1100:]).any()


# ---- 3. the round trip ---------------------------------------------------------------------------------------------------------------
def test_batch_to_pack_to_zpack_to_set_to_recipes_gives_every_file_back():
    rng = np.random.default_rng(95)
    design = open(os.path.join(ROOT, "DESIGN.md"), "rb").read()
    files = [design[:300_000], rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes(), b"", design[1000:90_000] + bytes(50_000),
             bytes([7]), zc.text_like(123_457, 1)]
    with M.Engine() as e, e.batch() as b:
        for i, f in enumerate(files):
            b.add_bytes(f, i)
        b.run()
        chunks = b.chunks().copy()
        rows = pc.rows_of(chunks)
        recipes = [rc.recipe_of(rows, files, f) for f in range(len(files))]
        with b.pack(verify=True) as p:
            entries, blob = p.entries().copy(), p.bytes()
            with p.compress(verify=True) as z:
                zentries, zblob = z.entries().copy(), z.read()
                assert z.info.verified == 1 and z.info.stored_bytes < z.info.chunk_bytes * 0.8 and 0 < z.info.n_raw < len(z)
                want = zc.model_compress(entries, blob)
                assert _same_zentries(zentries, want[0]) and zblob == want[1]
                with e.packset() as s, e.batch() as r:                               # device to device
                    s.add_zpack(z, verify=True)
                    r.add_recipes(s, recipes, verify=True)
                    r.run()
                    assert [r.read_file(i, 0, len(f)) if f else b"" for i, f in enumerate(files)] == files
        # the pulling side, on an engine of its own, from host memory
        assert M.zpack_check(zblob, zentries) is None
        plain_e, plain_b = zc.model_expand(zentries, zblob)
        assert plain_b == blob and pc.same_entries(plain_e, entries)
    with M.Engine() as puller, puller.packset() as s, puller.batch() as r:
        s.add_zblob(zblob, zentries, verify=True)
        st = r.add_recipes(s, recipes, verify=True)
        assert st.n_files == len(files) and st.bytes == sum(len(f) for f in files)
        r.run()
        assert [r.read_file(i, 0, len(f)) if f else b"" for i, f in enumerate(files)] == files
        assert np.array_equal(r.chunks()["sha256"], chunks["sha256"])
        # a sub-pack cut from the set by digest, compressed again
        dig = np.ascontiguousarray(chunks["sha256"][::3])
        with s.pack(dig, verify=True) as sub:
            _compress_and_compare(puller, sub, pc.SHA256)


# ---- 4. what is refused ---------------------------------------------------------------------------------------------------------------
def _raises(code, call, *needles):
    with pytest.raises(M.MiError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)
    return ei.value


def test_the_malformed_table_is_refused_and_the_set_stays_as_it_was():
    rng = np.random.default_rng(96)
    held = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in (100, 17, 3000)]
    h_entries, h_blob = zc.pack_of(held)
    probe = np.ascontiguousarray(np.concatenate([h_entries["digest"], np.frombuffer(zc.sha(zc.GOOD_PLAIN), dtype=np.uint8).reshape(1, 32)]))
    table = zc.malformed_zpacks()
    assert len(table) == 24
    with M.Engine() as e, e.packset() as s:
        s.add_blob(h_blob, h_entries, verify=True)
        info0 = {k: v for k, v in s.info.as_dict().items() if not k.startswith("ms_")}
        for name, entries, blob, bad in table:
            assert M.zpack_check(blob, entries) == bad, name
            for verify in (False, True):
                err = _raises(-1, lambda: s.add_zblob(blob, entries, verify=verify), "entry %d " % bad)
                assert err.first_bad == bad, name
            assert {k: v for k, v in s.info.as_dict().items() if not k.startswith("ms_")} == info0, name
            got = s.missing(probe)                                   # the table: what it held it holds, and nothing of the refused pack
            assert got[0].tolist() == [1, 1, 1, 0], name
        # the rule is named
        by_name = {name: (en, bl) for name, en, bl, _ in table}
        for name, words in (("offset 0", "offset of 0"), ("offset one beyond the bytes produced", "beyond the bytes produced"),
                            ("literal run one byte past the stored span", "literal run"), ("output one byte short", "short of"),
                            ("match one byte past length", "passes the chunk's length"), ("non-zero pad", "pad byte")):
            _raises(-1, lambda: s.add_zblob(by_name[name][1], by_name[name][0]), words)
        # a good zpack goes in
        good_e, good_b = zc.build_zpack([zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN)])
        s.add_zblob(good_b, good_e, verify=True)
        assert s.missing(probe)[0].tolist() == [1, 1, 1, 1]
        with s.pack(probe[3:]) as p:
            assert p.bytes()[:34] == zc.GOOD_PLAIN and p.bytes()[34:] == bytes(14)
        # unknown flags, 2^32 entries, NULL arguments, a zpack of another engine, a ctx that still has a zpack
        L, bad = e._lib, C.c_uint64()
        assert L.mi_packset_add_zblob(s._h, good_b, len(good_b), good_e.ctypes.data, 1, 0x2, C.byref(bad)) == -1 and b"unknown flags" in L.mi_last_error(e._h)
        assert L.mi_packset_add_zblob(s._h, good_b, len(good_b), good_e.ctypes.data, 1 << 32, 0, C.byref(bad)) == -1 and b"2^32" in L.mi_last_error(e._h)
        assert L.mi_packset_add_zblob(s._h, None, 16, good_e.ctypes.data, 1, 0, None) == -1
        assert L.mi_packset_add_zblob(None, good_b, len(good_b), good_e.ctypes.data, 1, 0, None) == -1
        assert L.mi_packset_add_zpack(s._h, None, 0) == -1
        out = C.c_void_p(5)
        assert L.mi_pack_compress(None, 0, C.byref(out)) == -1 and out.value is None
        with s.pack(probe) as p:
            assert L.mi_pack_compress(p._h, 0x2, C.byref(out)) == -1 and b"unknown flags" in L.mi_last_error(e._h)
            z = p.compress()
        with M.Engine() as other, other.packset() as s2:
            _raises(-1, lambda: s2.add_zpack(z), "another ctx")
        s.close()
        assert L.mi_ctx_destroy(e._h) == -6 and b"still alive" in L.mi_last_error(e._h)
        assert len(z) == 4 and M.zpack_check(z.read(), z.entries()) is None                   # it outlives the pack and the set
        z.close()


@pytest.mark.parametrize("alg", [pc.SHA256, pc.BLAKE2S])
def test_a_stream_that_decodes_cleanly_to_wrong_bytes_is_caught_by_the_digests_only(alg):
    rng = np.random.default_rng(97)
    chunks = [zc.text_like(5000, 1), rng.integers(0, 256, 900, dtype=np.uint8).tobytes(), zc.text_like(7001, 2)]
    entries, blob = zc.pack_of(chunks, alg)
    zentries, zblob = zc.model_compress(entries, blob)
    assert int(zentries["stored"][2]) < 7001
    # one literal of entry 2 changed: the stream is as sound as before, the bytes are not the digest's
    run = zc.parse(chunks[2])[0][0]
    first_lit = 1 + (0 if run < 15 else (run - 15) // 255 + 1)
    wrong = bytearray(zblob)
    wrong[int(zentries["offset"][2]) + first_lit] ^= 0x20
    wrong = bytes(wrong)
    plain_wrong = zc.model_expand(zentries, wrong)[1]
    assert plain_wrong != blob and len(plain_wrong) == len(blob)
    assert M.zpack_check(wrong, zentries, alg=alg) == 2 and M.zpack_check(zblob, zentries, alg=alg) is None
    recipe = [(np.ascontiguousarray(entries["digest"]), entries["length"].astype(np.uint32))]
    with M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0) as e:
        with e.packset() as s:
            err = _raises(-1, lambda: s.add_zblob(wrong, zentries, verify=True), "entry 2 ", "does not hash")
            assert err.first_bad == 2 and s.info.n_digests == 0
            s.add_zblob(wrong, zentries)                                                    # without the flag it gets past ...
            with s.pack(recipe[0][0]) as p:
                assert p.bytes() == plain_wrong
            with e.batch() as r:                                                            # ... and the recipes' check is the last net
                _raises(-5, lambda: r.add_recipes(s, recipe, verify=True), "row 2 ")
        with e.packset() as s, e.batch() as r:
            s.add_zblob(zblob, zentries, verify=True)
            r.add_recipes(s, recipe, verify=True)
            r.run()
            assert r.read_back().tobytes() == b"".join(chunks)


# ---- 5. the bounds, checked by the hardware --------------------------------------------------------------------------------------------
# The bounds, from the code (csrc/mi_zpack.hip): the encoder reads src[pos .. pos + 3] with pos <= n - 12 and match bytes below
# n - 5; the gather reads aligned 16-byte units inside [src, src + round16(stored)) of the input pack (a raw chunk) or of a
# scratch span; the decoder compares every index into the stored form with `stored` before the load, reads the pad
# [stored, round16(stored)) -- to the compressed blob's last byte when the last entry ends on its last unit, and not beyond --
# and writes [dst, dst + round16(length)): to the plain blob's last byte.  So a pack whose last chunk ends on its blob's last
# unit, with lengths 1, 15 and 0 mod 16, and a compressed blob whose last entry is LZ-coded and ends on its last unit, are read
# and written to their last bytes.  Under MI_GUARD_ALLOC=1 every device allocation ends on an unmapped page
# (tests/test_gpu_overread.py).  No positive control: a deliberate fault has no place on a shared box.
GUARD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import makisu_amd as M
import pack_cases as pc
import zpack_cases as zc
rng = np.random.default_rng(98)
with M.Engine() as e:
    for mod in (1, 15, 0):
        last = zc.tail_chunk(rng, mod, 0)                         # coded, and its stored form ends on a 16-byte boundary
        raw_last = rng.integers(0, 256, 32 + mod, dtype=np.uint8).tobytes()
        for chunks in ([zc.text_like(300, mod), b"\x05", last], [zc.text_like(77, mod), last, raw_last]):
            entries, blob = zc.pack_of(chunks)
            assert int(entries["offset"][-1]) + pc.round16(len(chunks[-1])) == len(blob) and len(chunks[-1]) %% 16 == mod
            want_e, want_b = zc.model_compress(entries, blob)
            with e.packset() as s:
                s.add_blob(blob, entries, verify=True)
                with s.pack(np.ascontiguousarray(entries["digest"])) as p:
                    with p.compress(verify=True) as z:
                        got_e, got_b = z.entries().copy(), z.read()
                        assert got_b == want_b and got_e["stored"].tolist() == want_e["stored"].tolist()
                        if chunks[-1] is last:
                            assert int(got_e["stored"][-1]) %% 16 == 0 and int(got_e["stored"][-1]) < len(last)
                            assert int(got_e["offset"][-1]) + int(got_e["stored"][-1]) == len(got_b)
                        with e.packset() as s2:
                            s2.add_zpack(z, verify=True)
                            with s2.pack(np.ascontiguousarray(entries["digest"])) as back:
                                assert back.bytes() == blob
            with e.packset() as s3:
                s3.add_zblob(want_b, want_e, verify=True)
                with s3.pack(np.ascontiguousarray(entries["digest"])) as back:
                    assert back.bytes() == blob
print("OK")
"""


def test_no_load_or_store_leaves_the_spans_the_design_states(tmp_path):
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", GUARD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout[-1500:] + p.stderr[-3000:]
