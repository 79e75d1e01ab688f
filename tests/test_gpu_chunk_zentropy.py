"""GPU tests of the zpack entropy stage (MI_ZPACK_ENTROPY, form H): mi_pack_compress with the flag is compared
byte for byte with the model of zentropy_cases.py at both levels, the census with the model's, and a zpack of all four forms goes
through every reader -- mi_packset_add_zpack / _zblob, mi_zset_add_zblob with VERIFY, mi_zset_zpack and mi_zset_prune (which move
spans verbatim) and mi_batch_add_zrecipes at odd destination residues.  Every row of the malformed table is refused by the device
with the entry and the rule the model names, and leaves its set or batch as it was.  Without a form H every output is what the
existing models give.  Bit for bit: there are no tolerances."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import pack_cases as pc  # noqa: E402
import zentropy_cases as ze  # noqa: E402
import zpack2_cases as z2  # noqa: E402
import zpack_cases as zc  # noqa: E402

pytestmark = pytest.mark.gpu

RULE_WORDS = {2: "a match offset beyond the bytes produced so far", 6: "short of the chunk's length", 7: "a pad byte behind the stored span",
              8: "an entropy form with a bad header", 9: "an entropy form whose code lengths", 10: "an entropy form whose stream sizes",
              11: "an entropy form with a stream that ends early"}


def _same_zentries(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]), np.asarray(want[f]))
                                         for f in ("digest", "offset", "chunk_index", "length", "stored"))


def _raises(code, call, *needles):
    with pytest.raises(M.MiError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)
    return ei.value


def _pack_of_chunks(engine, chunks):
    entries, blob = zc.pack_of(chunks)
    with engine.packset() as s:
        s.add_blob(blob, entries, verify=True)
        p = s.pack(np.ascontiguousarray(entries["digest"]), verify=True)
    assert pc.same_entries(p.entries(), entries) and p.bytes() == blob
    return p, entries, blob


def _forms(f):
    return [[int(f.n[i]), int(f.stored[i])] for i in range(4)]


@pytest.fixture(scope="module")
def planted():
    """the planted chunks and what the model stores for them at both levels, computed once"""
    cases = ze.planted_chunks_h()
    chunks = [c for _, c in cases]
    entries, blob = zc.pack_of(chunks)
    want = dict((level, ze.model_compress_h(entries, blob, level)) for level in (1, 2))
    return cases, chunks, entries, blob, want


# ---- 1. the coder against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2])
def test_compress_with_the_stage_is_the_models_bytes_and_every_reader_takes_them(planted, level):
    cases, chunks, entries, blob, want = planted
    want_e, want_b = want[level]
    census = ze.count_forms(want_e, want_b)
    assert all(n > 0 for n, _ in census), census                    # all four forms occur
    names = [name for name, _ in cases]
    form = dict((name, ze.form_of(want_b[int(en["offset"]):int(en["offset"]) + int(en["stored"])], int(en["length"]))) for name, en in zip(names, want_e))
    assert form["text 65537"] == 1 and form["text 65536"] == 2 and form["four symbols"] == 3 and form["sixteen symbols"] == 3
    assert all(form["random %d" % n] == 0 for n in ze.H_LENGTHS) and form["zeros"] == 2
    with M.Engine(max_size=262144) as e:
        p, _, _ = _pack_of_chunks(e, chunks)
        with p, p.compress(verify=True, level=level, entropy=True) as z:
            got_e, got_b, info = z.entries().copy(), z.read(), z.info
            assert _same_zentries(got_e, want_e), [(names[k], int(got_e["stored"][k]), int(want_e["stored"][k])) for k in range(len(want_e))
                                                  if got_e["stored"][k] != want_e["stored"][k] or got_e["offset"][k] != want_e["offset"][k]][:10]
            assert got_b == want_b, next(i for i in range(len(want_b)) if i >= len(got_b) or got_b[i] != want_b[i])
            assert (info.n_entries, info.blob_bytes, info.stored_bytes, info.n_raw, info.verified) == \
                (len(want_e), len(want_b), int(want_e["stored"].sum()), census[0][0], 1)
            assert _forms(z.count_forms()) == census
            assert M.zpack_check(got_b, got_e) is None
            assert p.bytes() == blob                                # the input is unchanged
            dig, lens = np.ascontiguousarray(entries["digest"]), entries["length"].astype(np.uint32)
            for feed in ("zblob", "zpack"):                         # into a plain set: decoded, hashed, the plain pack again
                with e.packset() as s:
                    if feed == "zblob":
                        s.add_zblob(got_b, got_e, verify=True)
                    else:
                        s.add_zpack(z, verify=True)
                    with s.pack(dig, lens, verify=True) as back:
                        assert back.bytes() == blob
            # the same pack without VERIFY and without the flag: the flag alone makes the difference
            with p.compress(level=level, entropy=True) as z2_:
                assert z2_.read() == want_b and z2_.info.verified == 0
            with p.compress(level=level) as plain:
                base_e, base_b = (zc.model_compress if level == 1 else z2.model_compress2)(entries, blob)
                assert plain.read() == base_b and _same_zentries(plain.entries(), base_e)
                f = _forms(plain.count_forms())
                assert f[2] == f[3] == [0, 0] and f[0][0] + f[1][0] == len(chunks)


# ---- 2. a mixed zpack through the compressed set: add, cut, prune, restore -------------------------------------------------------------
def test_a_set_of_all_four_forms_is_cut_pruned_and_restored(planted):
    cases, chunks, entries, blob, want = planted
    want_e, want_b = want[1]
    keep = [k for k, c in enumerate(chunks) if len(c) <= 8192]      # small rows: files of many rows stay quick
    small = [chunks[k] for k in keep]
    s_entries, s_blob = zc.pack_of(small)
    se, sb = ze.model_compress_h(s_entries, s_blob, 1)
    census = ze.count_forms(se, sb)
    assert all(n > 0 for n, _ in census)
    dig = np.ascontiguousarray(se["digest"])
    lens = se["length"].astype(np.uint32)
    rng = np.random.default_rng(294)
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(sb, se, verify=True)                           # MI_ZSET_VERIFY unwraps, decodes and hashes
        assert _forms(zs.count_forms()) == census
        # the cut moves spans verbatim: it IS cut-plain-and-recompress with the same flags
        order = rng.permutation(len(small))
        sub = [small[k] for k in order[:9]]
        sub_entries, sub_blob = zc.pack_of(sub)
        cut_e, cut_b = ze.model_compress_h(sub_entries, sub_blob, 1)
        with zs.zpack(dig[order[:9]], lens[order[:9]], verify=True) as z:
            assert z.read() == cut_b and np.array_equal(z.entries()["stored"], cut_e["stored"]) and np.array_equal(z.entries()["offset"], cut_e["offset"])
            assert _forms(z.count_forms()) == ze.count_forms(cut_e, cut_b)
        # the restore: every form inside one file, destinations at odd residues (a 13-byte row first, a front of 1 001 bytes)
        front = rng.integers(1, 256, 1001, dtype=np.uint8).tobytes()
        files = [[int(k) for k in order], [int(k) for k in order[::-1]], [int(order[0])]]
        shortest = int(np.argmin(lens))
        files[0].insert(0, shortest)
        recipes = [(dig[f], lens[f]) for f in files]
        bodies = [b"".join(small[k] for k in f) for f in files]
        assert {ze.form_of(sb[int(se["offset"][k]):int(se["offset"][k]) + int(se["stored"][k])], int(lens[k])) for k in files[0]} == {0, 1, 2, 3}
        with e.batch() as b:
            b.add_bytes(front, 7)
            st = b.add_zrecipes(zs, recipes, verify=True)
            assert (st.n_files, st.n_rows, st.bytes) == (3, sum(len(f) for f in files), sum(len(x) for x in bodies))
            b.run()
            for i, x in enumerate([front] + bodies):
                assert b.read_file(i, 0, len(x)) == x, i
            with e.batch() as host_fed:
                for i, x in enumerate([front] + bodies):
                    host_fed.add_bytes(x, i)
                host_fed.run()
                assert np.array_equal(host_fed.files()["chunk_root"], b.files()["chunk_root"])
        # the prune: the survivors' spans stay verbatim
        kept = order[: len(small) // 2]
        zs.prune(dig[kept], keep=True, min_live_permille=1000)
        with zs.zpack(dig[np.sort(kept)], verify=True) as z:
            got_e, got_b = z.entries(), z.read()
            for k, en in zip(np.sort(kept), got_e):
                a, w = int(en["offset"]), int(se["offset"][k])
                assert int(en["stored"]) == int(se["stored"][k]) and got_b[a:a + int(en["stored"])] == sb[w:w + int(se["stored"][k])]
        assert sum(n for n, _ in _forms(zs.count_forms())) == len(kept) == zs.info.n_digests


def test_a_hand_built_zpack_with_one_two_and_sixty_four_streams_decodes():
    chunks = [zc.text_like(3000, 5) + bytes([65 + i]) * i for i in range(4)]                # distinct chunks, one stream count each
    specs = [zc._entry(ze.huff_form(zc.compress_chunk(c), 1, s), len(c), c) for c, s in zip(chunks, (1, 2, 33, 64))]
    entries, blob = zc.build_zpack(specs)
    assert M.zpack_check(blob, entries) is None and ze.first_refused(entries, blob) is None
    with M.Engine() as e, e.packset() as s, e.zset() as zs, e.batch() as b:
        s.add_zblob(blob, entries, verify=True)
        zs.add_zblob(blob, entries, verify=True)
        b.add_zrecipes(zs, [(np.ascontiguousarray(entries["digest"]), entries["length"].astype(np.uint32))], verify=True)
        b.run()
        assert b.read_file(0, 0, sum(len(c) for c in chunks)) == b"".join(chunks)


# ---- 3. the malformed table on the device ------------------------------------------------------------------------------------------------
def test_the_device_names_the_entry_and_the_rule_the_model_names_and_changes_nothing():
    table = ze.malformed_zpacks()
    good_e, good_b = ze.good_zpack()
    with M.Engine(max_size=262144) as e, e.packset() as ps, e.batch() as b:
        b.add_bytes(b"front" * 50, 1)
        ps_info = ps.info.as_dict()
        for name, entries, blob, bad, rule in table:
            assert M.zpack_check(blob, entries) == bad and ze.first_refused(entries, blob) == (bad, rule), name
            word = RULE_WORDS[rule]
            err = _raises(-1, lambda: ps.add_zblob(blob, entries), "entry %d " % bad, "does not decode: ", word)
            assert err.first_bad == bad, name
            assert {k: v for k, v in ps.info.as_dict().items() if not k.startswith("ms_")} == {k: v for k, v in ps_info.items() if not k.startswith("ms_")}
            with e.zset() as zs:
                before = {k: v for k, v in zs.info.as_dict().items() if not k.startswith("ms_")}
                err = _raises(-1, lambda: zs.add_zblob(blob, entries, verify=True), "entry %d " % bad, word)
                assert err.first_bad == bad and {k: v for k, v in zs.info.as_dict().items() if not k.startswith("ms_")} == before, name
                zs.add_zblob(blob, entries)                          # an unverified set takes it: nothing is decoded at add time
                recipe = (np.ascontiguousarray(entries["digest"]), entries["length"].astype(np.uint32))
                counts = b.counts()
                for verify in (False, True):
                    _raises(-1, lambda: b.add_zrecipes(zs, [recipe], verify=verify), "file 0, row %d " % bad, word)
                assert b.counts() == counts, name
        with e.zset() as zs:                                          # ... and a good restore into the same batch afterwards
            zs.add_zblob(good_b, good_e, verify=True)
            b.add_zrecipes(zs, [(np.ascontiguousarray(good_e["digest"]), good_e["length"].astype(np.uint32))], verify=True)
        b.run()
        want = zc.GOOD_PLAIN + ze.GOOD_PLAIN + bytes(range(40)) + ze.GOOD_PLAIN2
        assert b.read_file(1, 0, len(want)) == want


# ---- 4. where the flag is refused, and what a set of form H refuses -------------------------------------------------------------------------
def test_the_flag_is_taken_by_compress_and_recode_and_refused_where_it_is_out_of_scope(planted):
    cases, chunks, entries, blob, want = planted
    small = [c for c in chunks if len(c) <= 8192]
    s_entries, s_blob = zc.pack_of(small)
    se, sb = ze.model_compress_h(s_entries, s_blob, 1)
    assert M.ZPACK_ENTROPY == 0x20
    with M.Engine() as e:
        L = e._lib
        p, _, _ = _pack_of_chunks(e, small)
        out = C.c_void_p()
        with p:
            for flags in (0x2, 0x8, 0x10, 0x40, 0x20 | 0x2, 0x80000000):
                assert L.mi_pack_compress(p._h, flags, C.byref(out)) == -1 and b"unknown flags" in L.mi_last_error(e._h)
            for flags in (0x20, 0x21, 0x24, 0x25):
                assert L.mi_pack_compress(p._h, flags, C.byref(out)) == 0
                L.mi_zpack_free(out)
        with e.batch() as b:                                          # the commit's side codes at level 1: the flag is out of scope there
            b.add_bytes(b"".join(small), 0)
            b.run()
            assert L.mi_batch_zpack_chunks(b._h, None, 0, 0x20, C.byref(out)) == -1 and b"unknown flags" in L.mi_last_error(e._h)
        with e.zset() as zs:                                          # the recode takes it too (test_gpu_chunk_zrecode_entropy.py)
            info = M.RecodeInfo()
            zs.add_zblob(sb, se, verify=True)
            for flags in (0x20 | 0x2, 0x20 | 0x8, 0x20 | 0x40, 0x80000020):
                assert L.mi_zset_recode(zs._h, flags, 0, C.byref(info)) == -1 and b"unknown flags" in L.mi_last_error(e._h)
            for flags in (0x20, 0x20 | M.ZPACK_LEVEL2, 0x21, 0x25):
                assert L.mi_zset_recode(zs._h, flags, 0, C.byref(info)) == 0 and info.n_undecodable == 0
        assert L.mi_zpack_count_forms(None, None) == -1 and L.mi_zset_count_forms(None, None) == -1


# ---- 5. no form H: every output is what it was --------------------------------------------------------------------------------------------
def test_without_a_form_h_every_call_gives_what_the_existing_models_give():
    cases = [c for c in zc.planted_chunks() if len(c[1]) <= 4095][:40]
    chunks = [c for _, c, _ in cases]
    entries, blob = zc.pack_of(chunks)
    want_e, want_b = zc.model_compress(entries, blob)
    want2_e, want2_b = z2.model_compress2(entries, blob)
    dig, lens = np.ascontiguousarray(entries["digest"]), entries["length"].astype(np.uint32)
    with M.Engine() as e:
        p, _, _ = _pack_of_chunks(e, chunks)
        with p:
            for level, (we, wb) in ((1, (want_e, want_b)), (2, (want2_e, want2_b))):
                with p.compress(verify=True, level=level) as z:
                    assert z.read() == wb and _same_zentries(z.entries(), we)
                    f = _forms(z.count_forms())
                    assert f[2] == f[3] == [0, 0]
                    assert f[0] == [int((we["stored"] == we["length"]).sum()), int(we["stored"][we["stored"] == we["length"]].sum())]
                    assert f[1][1] == int(we["stored"][we["stored"] < we["length"]].sum())
                    with e.packset() as s:
                        s.add_zpack(z, verify=True)
                        with s.pack(dig, lens, verify=True) as back:
                            assert back.bytes() == blob
        with e.zset() as zs, e.batch() as b:
            zs.add_zblob(want_b, want_e, verify=True)
            assert _forms(zs.count_forms())[2:] == [[0, 0], [0, 0]]
            with zs.zpack(dig, lens, verify=True) as z:
                assert z.read() == want_b
            b.add_zrecipes(zs, [(dig, lens)], verify=True)
            b.run()
            assert b.read_file(0, 0, len(b"".join(chunks))) == b"".join(chunks)
            info = zs.recode(level=2, verify=True)                    # a set without form H recodes as ever
            assert info.n_digests == len(chunks) and info.stored_after <= info.stored_before
            with zs.zpack(dig, lens, verify=True) as z:
                got = z.entries()
                assert np.array_equal(got["stored"], np.minimum(want_e["stored"], want2_e["stored"]))
