"""GPU tests of the compressed pack sets (mi_zset_*, mi_zset_zpack, mi_batch_add_zrecipes): a zpack cut out of stored forms is
compared byte for byte with what the existing path makes by decoding, cutting plain and coding again, and with the model of
zset_cases.py; files decoded straight into the arena are compared with restore_cases' model and with the existing restore --
every destination residue, raw and coded rows side by side, the second grid trip, malformed streams, everything that is
refused, and the bounds under the guard allocator.  Bit for bit: there are no tolerances."""
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
import fetch_cases as fc  # noqa: E402
import pack_cases as pc  # noqa: E402
import restore_cases as rc  # noqa: E402
import zpack_cases as zc  # noqa: E402
import zset_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu
ALGS = [pc.SHA256, pc.BLAKE2S]
NAME = "sha256"                                       # the digest column of Batch.chunks(), whichever algorithm filled it


def _engine(alg, **kw):
    return M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0, **kw)


def _same_zentries(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]), np.asarray(want[f]))
                                         for f in ("digest", "offset", "chunk_index", "length", "stored"))


def _counts(info):
    return {k: v for k, v in info.as_dict().items() if not k.startswith("ms_")}


def _raises(code, call, *needles):
    with pytest.raises(M.MiError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)
    return ei.value


def _cut_and_compare(zset, zpacks, request, lengths=None, verify=True):
    """zset.zpack(request) against the model; -> (entries, blob)"""
    want_e, want_b = qc.model_cut(zpacks, request)
    with zset.zpack(request, lengths, verify=verify) as z:
        got_e, got_b, info = z.entries().copy(), z.read(), z.info
    assert _same_zentries(got_e, want_e), [k for k in range(min(len(got_e), len(want_e))) if got_e[k] != want_e[k]][:10]
    assert got_b == want_b, next(i for i in range(max(len(want_b), len(got_b))) if i >= min(len(got_b), len(want_b)) or got_b[i] != want_b[i])
    assert (info.n_entries, info.blob_bytes, info.chunk_bytes, info.stored_bytes, info.n_raw, info.verified) == \
        (len(want_e), len(want_b), int(want_e["length"].sum()), int(want_e["stored"].sum()),
         int((want_e["stored"] == want_e["length"]).sum()), int(verify))
    assert info.ms_encode == 0 and (info.ms_compact > 0) == (len(want_e) > 0)
    return got_e, got_b


# ---- 1. the cut commutes with the coder ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    return [c for _, c, _ in zc.planted_chunks()]


@pytest.mark.parametrize("alg", ALGS)
def test_the_cut_equals_decoding_cutting_plain_and_coding_again(planted, alg):
    chunks = planted
    dig = qc.digests_of(chunks, alg)
    groups = [list(range(0, 20)), list(range(20, 40)) + [3], list(range(40, len(chunks)))]        # chunk 3 lies in two packs
    plain = [zc.pack_of([chunks[k] for k in g], alg) for g in groups]
    zpacks = [zc.model_compress(*p) for p in plain]
    request, _ = fc.tripled_request(np.random.default_rng(101), dig)
    with _engine(alg) as e, e.zset() as zs, e.packset() as ps, e.zset() as dirty:
        for (pe, pb), (ze, zb) in zip(plain, zpacks):
            ps.add_blob(pb, pe, verify=True)
            zs.add_zblob(zb, ze, verify=True)
            dirty.add_zblob(qc.with_pads(ze, zb, 0xA5), ze)                   # unverified: pads of 0xA5 behind raw and coded entries
        zi = zs.info
        assert (zi.n_packs, zi.n_entries, zi.n_digests, zi.alg) == (3, len(chunks) + 1, len(chunks), alg)
        assert zi.blob_bytes == sum(len(zb) for _, zb in zpacks)
        store = qc.stored_store(zpacks)
        assert zi.stored_bytes == sum(len(s) for _, s in store.values()) and zi.chunk_bytes == sum(len(c) for c in chunks)
        got_e, got_b = _cut_and_compare(zs, zpacks, request)
        with ps.pack(request) as p, p.compress() as z:                         # the existing path: cut plain, parse again
            assert z.read() == got_b and _same_zentries(z.entries(), got_e)
        with dirty.zpack(request) as z:
            assert z.read() == got_b and _same_zentries(z.entries(), got_e)
        assert M.zpack_check(got_b, got_e, alg=alg) is None


def test_a_cut_zpack_feeds_both_kinds_of_set_and_outlives_its_set(planted):
    chunks = planted[:30]
    _, _, ze, zb = qc.zpack_of(chunks)
    dig = qc.digests_of(chunks)
    request = np.ascontiguousarray(dig[::-1][::2])
    with M.Engine() as e:
        zs = e.zset()
        zs.add_zblob(zb, ze, verify=True)
        z = zs.zpack(request, verify=True)
        zs.close()
        want_e, want_b = qc.model_cut([(ze, zb)], request)
        assert z.read() == want_b and _same_zentries(z.entries(), want_e)
        with e.packset() as ps, e.zset() as zs2:
            ps.add_zpack(z, verify=True)
            zs2.add_zpack(z, verify=True)
            assert ps.info.n_digests == zs2.info.n_digests == len(request)
            with zs2.zpack(request[::-1]) as back, ps.pack(request[::-1]) as p, p.compress() as again:
                assert back.read() == again.read()
        z.close()


# ---- 2. the scan's edges ------------------------------------------------------------------------------------------------------------
def test_requests_at_the_scans_block_edges_and_every_residue_at_the_blobs_end():
    rng = np.random.default_rng(102)
    pool = rng.integers(0, 256, (2049, 16), dtype=np.uint8)
    assert len({bytes(x) for x in pool}) == 2049
    # mostly raw 16-byte chunks; every 100th a chunk that is coded, so that offsets and sizes differ along the scan
    chunks = [bytes(pool[i]) if i % 100 else zc.text_like(200 + i, i) for i in range(2049)]
    tails = [zc.tail_chunk(rng, (mod + 5) % 16, mod) for mod in (1, 15, 0)]
    _, _, ze, zb = qc.zpack_of(chunks + tails)
    dig = qc.digests_of(chunks + tails)
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze, verify=True)
        for n in (0, 1, 2047, 2048, 2049):
            order = rng.permutation(2049)[:n]
            got_e, _ = _cut_and_compare(zs, [(ze, zb)], dig[order], verify=(n != 2048))
            assert len(got_e) == n
        for t, mod in enumerate((1, 15, 0)):
            got_e, got_b = _cut_and_compare(zs, [(ze, zb)], dig[[5, 100, 2049 + t]])
            assert int(got_e["stored"][-1]) % 16 == mod and int(got_e["stored"][-1]) < len(tails[t])
            assert len(got_b) == int(got_e["offset"][-1]) + pc.round16(int(got_e["stored"][-1]))


# ---- 3. the fused restore: every residue, raw and coded side by side ------------------------------------------------------------------
@pytest.fixture(scope="module")
def residue_case():
    rows = qc.restore_rows()
    chunks, files = qc.residue_files(rows)
    plain_e, plain_b, ze, zb = qc.zpack_of(chunks)
    recipes = [qc.recipe(chunks, f) for f in files]
    want = rc.model_restore([(plain_e, plain_b)], recipes)
    assert want == [b"".join(chunks[k] for k in f) for f in files]
    return chunks, files, ze, zb, recipes, want


def test_rows_at_every_destination_residue_land_byte_for_byte_and_nothing_else_is_written(residue_case):
    chunks, files, ze, zb, recipes, want = residue_case
    rng = np.random.default_rng(103)
    front = rng.integers(1, 256, 1001, dtype=np.uint8).tobytes()             # ends 233 bytes into a 256-byte slot
    behind = rng.integers(1, 256, 777, dtype=np.uint8).tobytes()
    with M.Engine() as e, e.zset() as zs, e.batch() as b:
        zs.add_zblob(zb, ze, verify=True)
        b.add_bytes(front, 100)
        st = b.add_zrecipes(zs, recipes, tags=list(range(len(files))), verify=True)
        b.add_bytes(behind, 200)
        assert (st.n_files, st.n_rows, st.bytes, st.n_joined_units) == (len(files), sum(len(f) for f in files), sum(len(x) for x in want), 0)
        assert st.ms_assemble > 0 and st.ms_verify > 0
        b.run()
        everything = [front] + want + [behind]
        for i, x in enumerate(everything):
            assert b.read_file(i, 0, len(x)) == x, i
        fr = b.files()
        assert fr["size"].tolist() == [len(x) for x in everything] and fr["user_tag"].tolist() == [100] + list(range(len(files))) + [200]
        with e.batch() as plain:                                               # the rows and roots of the same bytes, host-fed
            for i, x in enumerate(everything):
                plain.add_bytes(x, i)
            plain.run()
            assert np.array_equal(plain.files()["chunk_root"], fr["chunk_root"])
            assert np.array_equal(plain.chunks()[NAME], b.chunks()[NAME])


# ---- 4. the second grid trip -------------------------------------------------------------------------------------------------------------
def test_65600_rows_of_1_to_16_bytes_take_the_second_grid_trip():
    rng = np.random.default_rng(104)
    pool = {bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in range(1, 17) for _ in range(40)}
    pool |= {bytes([v]) * n for v in (3, 200) for n in (13, 14, 15, 16)}      # coded: 13 bytes and more of one value
    chunks = sorted(pool)
    _, _, ze, zb = qc.zpack_of(chunks)
    assert (ze["stored"] < ze["length"]).sum() == 8
    dig = qc.digests_of(chunks)
    pick = rng.integers(0, len(chunks), 65600)
    cuts = [0, 1, 30000, 65536, 65600]                                          # four files
    recipes = [qc.recipe(chunks, pick[a:b], dig=dig) for a, b in zip(cuts, cuts[1:])]
    want = [b"".join(chunks[k] for k in pick[a:b]) for a, b in zip(cuts, cuts[1:])]
    assert 400_000 < sum(len(x) for x in want) < 700_000
    with M.Engine() as e, e.zset() as zs, e.batch() as b:
        zs.add_zblob(zb, ze)
        st = b.add_zrecipes(zs, recipes, verify=True)
        assert st.n_rows == 65600
        b.run()
        for i, x in enumerate(want):
            assert b.read_file(i, 0, len(x)) == x, i


# ---- 5. equivalence with the existing path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("hint", [0, 600])
def test_a_zset_restores_what_a_plain_set_restores(alg, hint):
    """batch -> pack -> zpack, then (i) plain set -> add_recipes and (ii) zset -> add_zrecipes: the same bytes, the same rows.
    More than 1 024 entries: a table of 1 024 slots (hint 0) and one of 2 048 (hint 600) both grow during the add."""
    rng = np.random.default_rng(105)
    design = open(os.path.join(ROOT, "DESIGN.md"), "rb").read()
    files = [design[:150_000], rng.integers(0, 256, 60_000, dtype=np.uint8).tobytes(), b"", design[1000:40_000] + bytes(20_000), bytes([7])]
    host = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (10, 3000, 999)]
    with _engine(alg, mask_bits=6, min_size=64, max_size=1024) as e, e.batch() as b0:
        for i, f in enumerate(files):
            b0.add_bytes(f, i)
        b0.run()
        chunks = b0.chunks().copy()
        rows = pc.rows_of(chunks)
        recipes = [rc.recipe_of(rows, files, f, alg) for f in range(len(files))]
        with b0.pack(verify=True) as p, p.compress(verify=True) as z:
            assert len(z) > 1100 and 0 < z.info.n_raw < len(z)
            zentries, zblob = z.entries().copy(), z.read()
            with e.packset(hint) as ps, e.zset(hint) as zs, e.batch() as b1, e.batch() as b2:
                ps.add_zpack(z, verify=True)
                zs.add_zpack(z, verify=True)
                assert zs.info.n_digests == ps.info.n_digests == len({bytes(d) for d in chunks[NAME]}) > 1024
                assert zs.info.n_entries == len(z) and zs.info.blob_bytes == z.info.blob_bytes
                for b, add, s in ((b1, b1.add_recipes, ps), (b2, b2.add_zrecipes, zs)):
                    b.add_bytes(host[0], 50)
                    add(s, recipes[:2], tags=[0, 1], verify=True)
                    b.add_bytes(host[1], 51)
                    add(s, recipes[2:], tags=[2, 3, 4])
                    b.add_bytes(host[2], 52)
                    b.run()
                want = [host[0], files[0], files[1], host[1], files[2], files[3], files[4], host[2]]
                for i, x in enumerate(want):
                    assert b2.read_file(i, 0, len(x)) == x if x else True, i
                assert b1.read_back().tobytes() == b2.read_back().tobytes()
                assert np.array_equal(b1.files()["chunk_root"], b2.files()["chunk_root"]) and np.array_equal(b1.files()["size"], b2.files()["size"])
                assert np.array_equal(b1.chunks()[NAME], b2.chunks()[NAME]) and np.array_equal(b1.chunks()["length"], b2.chunks()["length"])
                # the cut, next to the existing path, over every third chunk
                dig = np.ascontiguousarray(chunks[NAME][::3])
                with zs.zpack(dig, verify=True) as cut, ps.pack(dig) as sub, sub.compress() as again:
                    assert cut.read() == again.read() and _same_zentries(cut.entries(), again.entries())
        # the pulling side, on an engine of its own, from host memory
    with _engine(alg, mask_bits=6, min_size=64, max_size=1024) as puller, puller.zset(hint) as zs, puller.batch() as r:
        zs.add_zblob(zblob, zentries, verify=True)
        r.add_zrecipes(zs, recipes, verify=True)
        r.run()
        assert [r.read_file(i, 0, len(f)) if f else b"" for i, f in enumerate(files)] == files
        assert np.array_equal(r.chunks()[NAME], chunks[NAME])


# ---- 6. malformed streams --------------------------------------------------------------------------------------------------------------
STRUCTURAL = ("stored > length", "stored == 0", "overlap", "off-grid offset")


def test_the_malformed_table_passes_an_unverified_add_and_is_refused_by_the_restore():
    table = zc.malformed_zpacks()
    good_e, good_b = zc.build_zpack([zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN)])
    rng = np.random.default_rng(106)
    front = rng.integers(1, 256, 300, dtype=np.uint8).tobytes()
    with M.Engine() as e, e.packset() as ps, e.batch() as b:
        b.add_bytes(front, 9)
        n_good = 0
        for name, entries, blob, bad in table:
            assert M.zpack_check(blob, entries) == bad, name
            structural = name.split(",")[0] in STRUCTURAL
            with e.zset() as zs:
                info0 = _counts(zs.info)
                for verify in (True,) + ((False,) if structural else ()):            # a structural violation is refused always
                    err = _raises(-1, lambda: zs.add_zblob(blob, entries, verify=verify), "entry %d " % bad)
                    assert err.first_bad == bad, name
                    assert _counts(zs.info) == info0, name
                if structural:
                    continue
                zs.add_zblob(blob, entries)                                          # no stream is decoded at add time
                assert zs.info.n_entries == len(entries)
                if len({bytes(d) for d in entries["digest"]}) < len(entries):
                    continue                                                          # (the good entry's form was first: it won)
                # the rule, in the words the existing device path refuses the same input with
                said = str(_raises(-1, lambda: ps.add_zblob(blob, entries), "entry %d " % bad))
                rule = said.split("does not decode: ")[1]
                recipe = (np.ascontiguousarray(entries["digest"]), entries["length"].astype(np.uint32))
                before = b.counts()
                for verify in (False, True):
                    err = _raises(-1, lambda: b.add_zrecipes(zs, [recipe], verify=verify), "file 0, row %d " % bad, rule)
                    assert entries["digest"][bad].tobytes().hex() in str(err), name
                assert b.counts() == before, name
                if name.startswith("non-zero pad"):                                   # the cut writes zero pads: what it makes is sound
                    with zs.zpack(recipe[0], verify=True) as z:
                        assert M.zpack_check(z.read(), z.entries()) is None
                else:
                    _raises(-5, lambda: zs.zpack(recipe[0], verify=True), "row %d " % bad)
                with zs.zpack(recipe[0]) as z:                                        # an unverified cut moves what it holds
                    assert len(z) == len(entries)
            with e.zset() as zs:                                                      # a following good restore into the same batch
                zs.add_zblob(good_b, good_e, verify=True)
                b.add_zrecipes(zs, [(good_e["digest"], good_e["length"])], verify=True)
                n_good += 1
        assert n_good >= 12
        b.run()
        assert b.read_file(0, 0, len(front)) == front
        for i in range(n_good):
            assert b.read_file(1 + i, 0, 34) == zc.GOOD_PLAIN, i


@pytest.mark.parametrize("alg", ALGS)
def test_a_stream_that_decodes_cleanly_to_wrong_bytes_is_caught_by_the_three_flags_only(alg):
    rng = np.random.default_rng(107)
    chunks = [zc.text_like(5000, 1), rng.integers(0, 256, 900, dtype=np.uint8).tobytes(), zc.text_like(7001, 2)]
    entries, blob, zentries, zblob = qc.zpack_of(chunks, alg)
    assert int(zentries["stored"][2]) < 7001
    run = zc.parse(chunks[2])[0][0]                                          # one literal of entry 2 changed: as sound as before
    wrong = bytearray(zblob)
    wrong[int(zentries["offset"][2]) + 1 + (0 if run < 15 else (run - 15) // 255 + 1)] ^= 0x20
    wrong = bytes(wrong)
    plain_wrong = zc.model_expand(zentries, wrong)[1]
    assert plain_wrong != blob and M.zpack_check(wrong, zentries, alg=alg) == 2
    recipe = [(np.ascontiguousarray(entries["digest"]), entries["length"].astype(np.uint32))]
    with _engine(alg) as e, e.zset() as zs:
        err = _raises(-1, lambda: zs.add_zblob(wrong, zentries, verify=True), "entry 2 ", "does not hash")
        assert err.first_bad == 2 and zs.info.n_digests == 0 and zs.info.n_packs == 0
        zs.add_zblob(wrong, zentries)                                        # without the flag it gets past ...
        with zs.zpack(recipe[0][0]) as z:
            assert z.read() == wrong
        with e.batch() as r:                                                 # ... an unflagged restore too
            r.add_zrecipes(zs, recipe)
            r.run()
            assert r.read_file(0, 0, len(b"".join(chunks))) == b"".join(plain_wrong[int(o):int(o) + int(n)] for o, n in zip(entries["offset"], entries["length"]))
        err = _raises(-5, lambda: zs.zpack(recipe[0][0][::-1], verify=True), "row 0 ", "hash to the requested digest")
        assert err.first_bad == 0
        with e.batch() as r:
            _raises(-5, lambda: r.add_zrecipes(zs, recipe, verify=True), "row 2 ")
            assert r.counts() == (0, 0, 0)


# ---- 7. what is refused leaves things as they were ----------------------------------------------------------------------------------
def test_what_is_refused_leaves_set_and_batch_as_they_were(planted):
    chunks = planted[:12]
    _, _, ze, zb = qc.zpack_of(chunks)
    dig = qc.digests_of(chunks)
    lens = np.array([len(c) for c in chunks], dtype=np.uint32)
    alien = np.frombuffer(zc.sha(b"not held"), dtype=np.uint8).reshape(1, 32)
    with M.Engine() as e, e.zset() as zs, e.batch() as b:
        zs.add_zblob(zb, ze, verify=True)
        info0 = _counts(zs.info)
        b.add_bytes(b"first", 1)
        L, bad, out = e._lib, C.c_uint64(), C.c_void_p(5)
        req = np.ascontiguousarray(np.concatenate([dig[:5], alien, dig[5:], alien]))
        err = _raises(-1, lambda: zs.zpack(req), "row 5", alien.tobytes().hex())
        assert err.first_bad == 5
        zero = lens.copy()
        zero[[4, 7]] = 0
        assert _raises(-1, lambda: zs.zpack(dig, zero), "row 4", "length 0").first_bad == 4
        other = lens.copy()
        other[[6, 9]] += 1
        assert _raises(-1, lambda: zs.zpack(dig, other), "row 6", dig[6].tobytes().hex(), "states %d" % other[6]).first_bad == 6
        _raises(-1, lambda: b.add_zrecipes(zs, [(req, np.concatenate([lens[:5], [9], lens[5:], [9]]).astype(np.uint32))]), "file 0, row 5 ", "does not hold")
        _raises(-1, lambda: b.add_zrecipes(zs, [(dig[:3], lens[:3]), (dig, zero)]), "file 1, row 4 ", "length 0")
        _raises(-1, lambda: b.add_zrecipes(zs, [(dig, other)]), "file 0, row 6 ", "states %d" % other[6])
        assert L.mi_zset_zpack(zs._h, dig.ctypes.data, None, len(dig), 0x2, C.byref(out), C.byref(bad)) == -1 and out.value is None
        assert b"unknown flags" in L.mi_last_error(e._h)
        assert L.mi_zset_zpack(zs._h, dig.ctypes.data, None, 1 << 32, 0, C.byref(out), C.byref(bad)) == -1 and b"2^32" in L.mi_last_error(e._h)
        assert L.mi_zset_add_zblob(zs._h, zb, len(zb), ze.ctypes.data, len(ze), 0x2, C.byref(bad)) == -1 and b"unknown flags" in L.mi_last_error(e._h)
        assert L.mi_batch_add_zrecipes(b._h, zs._h, 1, None, None, None, None, 0x2, None) == -1
        assert _counts(zs.info) == info0 and b.counts()[0] == 1
        with M.Engine() as other_e, other_e.batch() as ob, other_e.zset() as ozs:      # a set, a zpack of another ctx
            _raises(-1, lambda: ob.add_zrecipes(zs, [(dig, lens)]), "another ctx")
            with zs.zpack(dig) as z:
                _raises(-1, lambda: ozs.add_zpack(z), "another ctx")
        b.add_zrecipes(zs, [(dig, lens)], verify=True)                                 # and the batch takes a good restore
        b.run()
        assert b.read_file(1, 0, int(lens.sum())) == b"".join(chunks)
        _raises(-6, lambda: b.add_zrecipes(zs, [(dig, lens)]), "already ran")
        # the same digest with another length: the add fails, the set is unusable and says why from every call
        liar = ze[:1].copy()
        liar["length"] += 1
        assert _raises(-1, lambda: zs.add_zblob(zb[:zc.round16(int(ze["stored"][0]))], liar), "another length").first_bad == 0
        def restore_from_it():
            with e.batch() as t:
                t.add_zrecipes(zs, [(dig, lens)])
        for call in (lambda: zs.info, lambda: zs.zpack(dig), lambda: zs.add_zblob(zb, ze), restore_from_it):
            _raises(-6, call, "unusable since", "another length")
        # mi_ctx_destroy while a zset or a cut zpack lives
        with e.zset() as zs2:
            zs2.add_zblob(zb, ze)
            z = zs2.zpack(dig[:2])
        zs.close()
        b.free()
        assert L.mi_ctx_destroy(e._h) == -6 and b"still alive" in L.mi_last_error(e._h)
        assert len(z) == 2
        z.close()
        keep = e.zset()
        assert L.mi_ctx_destroy(e._h) == -6 and b"still alive" in L.mi_last_error(e._h)
        keep.close()


# ---- 7b. the table itself: a conflict inside one add, two stored forms of one chunk, growth through export and re-insert -------------
def test_one_digest_with_two_lengths_in_one_add_is_a_conflict_and_with_two_stored_forms_is_not():
    """Two entries of 16 and 17 bytes under one digest, into a fresh set, verify off (digests are opaque).  Both rows probe in
    one launch: one claims the slot, the other meets its own tag there and is the conflict the verify kernel reports -- which of
    the two compare-and-swaps comes first is the hardware's, so the row named is either, with its own length.  One digest and
    one length stored raw and then coded is no conflict: the set keeps the form it had."""
    _, _, ze, zb = qc.zpack_of([bytes(range(16)), bytes(range(17))])
    ze = ze.copy()
    ze["digest"][1] = ze["digest"][0]
    twice = bytes([9]) * 40
    coded = zc.compress_chunk(twice)
    assert len(coded) < 40
    raw_form, coded_form = zc.build_zpack([zc._entry(twice, 40, twice)]), zc.build_zpack([zc._entry(coded, 40, twice)])
    with M.Engine() as e:
        with e.zset() as zs:
            err = _raises(-1, lambda: zs.add_zblob(zb, ze), "another length", "unusable from here on")
            assert err.first_bad in (0, 1) and "entry %d (%d bytes)" % (err.first_bad, 16 + err.first_bad) in str(err), str(err)
            _raises(-6, lambda: zs.info, "unusable since", "another length")
        with e.zset() as zs, e.batch() as b:
            for en, bl in (raw_form, coded_form):
                zs.add_zblob(bl, en)
            d, ln, st = zs.entries()
            assert (len(d), int(ln[0]), int(st[0])) == (1, 40, 40) and zs.info.n_packs == 2
            b.add_zrecipes(zs, [qc.recipe([twice], [0])], verify=True)
            b.run()
            assert b.read_file(0, 0, 40) == twice


def test_a_zset_grows_through_export_and_re_insert():
    """A fresh set has 1 024 slots and stays under half full: 513 entries grow it empty, 513 more grow it through the export of
    what it holds and their re-insert.  Every digest is found afterwards, by the want list and by a restore."""
    data = np.random.default_rng(110).integers(0, 256, 1026 * 16, dtype=np.uint8).tobytes()
    chunks = [data[16 * i:16 * i + 16] for i in range(1026)]
    dig = qc.digests_of(chunks)
    assert len({bytes(d) for d in dig}) == 1026
    with M.Engine() as e, e.zset() as zs, e.batch() as b:
        for k in (0, 513):
            _, _, ze, zb = qc.zpack_of(chunks[k:k + 513])
            zs.add_zblob(zb, ze)
        assert (zs.info.n_digests, zs.info.n_entries, zs.info.n_packs) == (1026, 1026, 2)
        held, want, info = zs.missing(dig)
        assert held.all() and len(want) == 0 and info.n_want == 0
        pick = [0, 512, 1025]                                    # the first, the 513th and the last
        b.add_zrecipes(zs, [qc.recipe(chunks, pick, dig=dig)], verify=True)
        b.run()
        assert b.read_file(0, 0, 48) == b"".join(chunks[k] for k in pick)


# ---- 8. keys that collide ---------------------------------------------------------------------------------------------------------------
def test_digests_that_share_their_first_eight_bytes_resolve_to_their_own_chunks():
    rng = np.random.default_rng(108)
    lens = [100, 100, 37, 64, 1, 250, 16, 90]                    # entries 0..2 collide; 0 and 1 have equal lengths
    chunks = [zc.text_like(k, k) if k in (250, 90) else rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]
    # verify is off: digests are opaque.  The table of a fresh set has 1 024 slots, slot = first 8 bytes (little endian) & 1023:
    # three digests with one tag walk to slots t, t + 1, t + 2; their neighbours are AT HOME in t + 1, t + 2, t + 3 and t - 1
    tag = 0x1122334455667000 | 0x2FF
    dig = np.zeros((len(lens), 32), dtype=np.uint8)
    for k in range(len(lens)):
        dig[k, 8:] = rng.integers(0, 256, 24, dtype=np.uint8)
    for k, t in enumerate([tag, tag, tag, tag + 1, tag + 2, tag + 3, tag - 1, 0]):             # (tag 0 is stored as 1: the last entry)
        dig[k, :8] = np.frombuffer(int(t).to_bytes(8, "little"), dtype=np.uint8)
    _, _, ze, zb = qc.zpack_of(chunks, digests=dig)
    assert (ze["stored"] < ze["length"]).sum() == 2
    order = [2, 0, 7, 1, 3, 6, 5, 4, 1, 2, 0]
    with M.Engine() as e, e.zset() as zs, e.batch() as b:
        zs.add_zblob(zb, ze)
        assert zs.info.n_digests == len(lens)
        b.add_zrecipes(zs, [qc.recipe(chunks, order, dig=dig)] + [qc.recipe(chunks, [k], dig=dig) for k in range(len(lens))])
        b.run()
        assert b.read_file(0, 0, sum(lens[k] for k in order)) == b"".join(chunks[k] for k in order)
        for k in range(len(lens)):
            assert b.read_file(1 + k, 0, lens[k]) == chunks[k], k
        _cut_and_compare(zs, [(ze, zb)], dig[order], verify=False)


# ---- 9. the bounds, checked by the hardware --------------------------------------------------------------------------------------------
# The bounds, from the code (csrc/mi_zset.hip): the cut reads aligned 16-byte units inside [src, src + round16(stored)) -- to the
# set blob's last byte when the entry ends on its last unit, and not beyond -- and writes the new blob to its last byte; the
# fused restore reads [src, src + round16(stored)) (the pad check reaches the unit's end) and writes [dst, dst + length): to the
# last byte of the arena that is in use when the row is the last file's last.  Under MI_GUARD_ALLOC=1 every device allocation
# ends on an unmapped page (tests/test_gpu_overread.py).  No positive control: a deliberate fault has no place on a shared box.
GUARD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import makisu_amd as M
import pack_cases as pc
import zpack_cases as zc
import zset_cases as qc
rng = np.random.default_rng(109)
coded_last = zc.tail_chunk(rng, 6, 1)                                 # stored = 1 mod 16, coded
raw_last = rng.integers(0, 256, 33, dtype=np.uint8).tobytes()         # stored = length = 1 mod 16, raw
with M.Engine() as e:
    for last in (coded_last, raw_last):
        chunks = [zc.text_like(300, 3), b"\x05", zc.text_like(999, 4), last]
        _, _, ze, zb = qc.zpack_of(chunks)
        assert int(ze["stored"][-1]) %% 16 == 1 and (int(ze["stored"][-1]) < len(last)) == (last is coded_last)
        assert int(ze["offset"][-1]) + pc.round16(int(ze["stored"][-1])) == len(zb)
        dig = qc.digests_of(chunks)
        with e.zset() as zs:
            zs.add_zblob(zb, ze, verify=True)
            request = dig[[1, 0, 3]]                                  # the cut's last entry ends on the set blob's last unit
            want_e, want_b = qc.model_cut([(ze, zb)], request)
            with zs.zpack(request, verify=True) as z:
                assert z.read() == want_b and z.entries()["stored"].tolist() == want_e["stored"].tolist()
                with e.zset() as zs2:
                    zs2.add_zpack(z, verify=True)
                    with zs2.zpack(request[::-1]) as back:
                        assert back.read() == qc.model_cut([(ze, zb)], request[::-1])[1]
            with e.batch() as b:                                      # the last file's last row ends on the arena's last byte in use
                b.add_zrecipes(zs, [qc.recipe(chunks, [3, 1]), qc.recipe(chunks, [2, 1, 0, 3])], verify=True)
                b.run()
                assert b.read_file(0, 0, len(last) + 1) == last + chunks[1]
                assert b.read_file(1, 0, 1300 + len(last)) == chunks[2] + chunks[1] + chunks[0] + last
print("OK")
"""


def test_no_load_or_store_of_the_cut_or_the_restore_leaves_its_span(tmp_path):
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", GUARD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout[-1500:] + p.stderr[-3000:]
