"""GPU tests of the two cuts that serve a compressed set to a plainer reader (mi_zset_zpack_unwrapped, mi_zset_pack; DESIGN.md
4.17): both are compared byte for byte, blob and entries, with the models of zserve_cases.py AND with the composition of existing
calls that gives the same bytes -- ZSet.zpack of a twin set fed the same packs coded without the stage; PackSet.pack of a plain set
fed the same zblobs -- on all four forms, on a request with repeats, without a form H, over 69 637 rows around every tile boundary
and on both trips of the one-wave-a-row kernels, over the malformed tables in an unverified set, after prune and recode, and under
BLAKE2s.  What the host test proves about these inputs (tests/test_host_chunk_zserve.py) is relied on here.  Bit for bit: there are
no tolerances."""
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
import fetch_cases as fc  # noqa: E402
import pack_cases as pc  # noqa: E402
import zentropy_cases as ze  # noqa: E402
import zentropy_rows_cases as zr  # noqa: E402
import zpack_cases as zc  # noqa: E402
import zserve_cases as zs  # noqa: E402

pytestmark = pytest.mark.gpu

RULE_WORDS = {1: "a match offset of 0", 2: "a match offset beyond the bytes produced so far", 3: "a literal run that leaves the stored span",
              4: "cut off by the span's end", 5: "output that passes the chunk's length", 6: "short of the chunk's length",
              7: "a pad byte behind the stored span", 8: "an entropy form with a bad header", 9: "an entropy form whose code lengths",
              10: "an entropy form whose stream sizes", 11: "an entropy form with a stream that ends early"}
ZFIELDS = ("digest", "offset", "chunk_index", "length", "stored")
PFIELDS = ("digest", "offset", "chunk_index", "length")


def _engine(alg, **kw):
    return M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0, **kw)


def _same(got, want, fields):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]), np.asarray(want[f])) for f in fields)


def _raises(code, call, *needles):
    with pytest.raises(M.MiError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)
    return ei.value


def _state(zset):
    """what the set answers: info (without the last add's times), usage, entries in digest order, the census"""
    d, ln, st = zset.entries()
    order = np.lexsort(d.T[::-1])
    f = zset.count_forms()
    return ({k: v for k, v in zset.info.as_dict().items() if not k.startswith("ms_")}, zset.usage().as_dict(), d[order].tobytes(),
            ln[order].tobytes(), st[order].tobytes(), [int(v) for v in f.n] + [int(v) for v in f.stored])


def _first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def _unwrapped_is(zset, request, lengths, verify, want_e, want_b):
    with zset.zpack_unwrapped(request, lengths, verify=verify) as z:
        got_e, got_b, info, forms = z.entries().copy(), z.read(), z.info, z.count_forms()
    assert _same(got_e, want_e, ZFIELDS), [k for k in range(min(len(got_e), len(want_e))) if got_e[k] != want_e[k]][:10]
    assert got_b == want_b, _first_diff(got_b, want_b)
    assert (info.n_entries, info.blob_bytes, info.chunk_bytes, info.stored_bytes, info.n_raw, info.verified) == \
        (len(want_e), len(want_b), int(want_e["length"].sum()), int(want_e["stored"].sum()), int((want_e["stored"] == want_e["length"]).sum()),
         int(verify))
    assert info.ms_encode == 0 and (info.ms_compact > 0) == (len(want_e) > 0)
    assert [int(forms.n[2]), int(forms.n[3]), int(forms.stored[2]), int(forms.stored[3])] == [0, 0, 0, 0]
    return got_e, got_b


def _pack_is(zset, request, lengths, verify, want_e, want_b):
    with zset.pack(request, lengths, verify=verify) as p:
        got_e, got_b, info = p.entries().copy(), p.bytes(), p.info
    assert _same(got_e, want_e, PFIELDS) and not np.asarray(got_e["reserved"]).any(), [k for k in range(min(len(got_e), len(want_e))) if got_e[k] != want_e[k]][:10]
    assert got_b == want_b, _first_diff(got_b, want_b)
    assert (info.n_entries, info.blob_bytes, info.verified) == (len(want_e), len(want_b), int(verify))
    return got_e, got_b


@pytest.fixture(scope="module")
def planted():
    """the planted chunks as a plain pack; with the stage (h) and without it (u) what the model stores at both levels"""
    chunks = [c for _, c in ze.planted_chunks_h()]
    entries, blob = zc.pack_of(chunks)
    h = dict((level, ze.model_compress_h(entries, blob, level)) for level in (1, 2))
    return chunks, entries, blob, h


def _compressed(engine, entries, blob, levels, entropy):
    """the plain pack through mi_pack_compress at the levels, in that order -> [(zentries, zblob)]"""
    out = []
    with engine.packset() as s:
        s.add_blob(blob, entries, verify=True)
        with s.pack(np.ascontiguousarray(entries["digest"]), verify=True) as p:
            for level in levels:
                with p.compress(verify=True, level=level, entropy=entropy) as z:
                    out.append((z.entries().copy(), z.read()))
    return out


# ---- 1. all four forms against the models and against the compositions ----------------------------------------------------------------
@pytest.mark.parametrize("levels", [(1, 2), (2, 1)])
def test_both_cuts_of_all_four_forms_are_the_models_and_the_compositions_bytes(planted, levels):
    chunks, entries, blob, h = planted
    dig = np.ascontiguousarray(entries["digest"])
    rng = np.random.default_rng(1701)
    request, src = fc.tripled_request(rng, dig)
    lengths = entries["length"].astype(np.uint32)[src]
    with M.Engine(max_size=262144) as e:
        with_h = _compressed(e, entries, blob, levels, True)
        without = _compressed(e, entries, blob, levels, False)
        for (ge, gb), level in zip(with_h, levels):                 # the coder is the model's (test_gpu_chunk_zentropy.py): the store is too
            assert gb == h[level][1] and _same(ge, h[level][0], ZFIELDS)
        store = {}
        for ze_, zb_ in with_h:
            zs.store_add(store, ze_, zb_)
        assert all(n > 0 for n in zs.forms_in(store, request))
        want_ue, want_ub = zs.model_zpack_unwrapped(store, request)
        want_pe, want_pb = zs.model_pack(store, request, pc.SHA256)
        with e.zset() as zset, e.zset() as twin, e.packset() as plain:
            for ze_, zb_ in with_h:
                zset.add_zblob(zb_, ze_, verify=True)
                plain.add_zblob(zb_, ze_, verify=True)
            for ze_, zb_ in without:
                twin.add_zblob(zb_, ze_, verify=True)
            before = _state(zset)
            assert before[-1][2] > 0 and before[-1][3] > 0           # the set holds both kinds of form H
            with twin.zpack(request, lengths, verify=True) as z:     # the composition: the same chunks coded WITHOUT the stage, cut verbatim
                assert z.read() == want_ub and _same(z.entries(), want_ue, ZFIELDS)
            with plain.pack(request, lengths, verify=True) as p:     # the composition: decode into a plain set, cut plain
                assert p.bytes() == want_pb and _same(p.entries(), want_pe, PFIELDS)
            for verify in (False, True):
                for ln in (None, lengths):
                    got_e, got_b = _unwrapped_is(zset, request, ln, verify, want_ue, want_ub)
                    pack_e, pack_b = _pack_is(zset, request, ln, verify, want_pe, want_pb)
            assert _state(zset) == before
            # the results feed on: a reader without the stage, the host checks
            assert M.zpack_check(got_b, got_e) is None and M.pack_check(pack_b, pack_e) is None
            with e.zset() as fresh:
                fresh.add_zblob(got_b, got_e, verify=True)
                f = fresh.count_forms()
                assert int(f.n[2]) == int(f.n[3]) == 0 and int(f.n[0]) + int(f.n[1]) == len(chunks)
                with fresh.pack(dig, verify=True) as p:
                    assert p.bytes() == blob and pc.same_entries(p.entries(), entries)
            with e.packset() as ps:                                  # everything that takes a pack takes the plain cut
                with zset.pack(dig, verify=True) as p:
                    ps.add_pack(p, verify=True)
                    with p.compress(verify=True, level=levels[0], entropy=True) as z:
                        first = with_h[0]
                        assert z.read() == first[1] and _same(z.entries(), first[0], ZFIELDS)


# ---- 2. no form H held ------------------------------------------------------------------------------------------------------------------
def test_without_a_form_h_the_unwrapped_cut_is_the_verbatim_cut():
    chunks = [c for _, c, _ in zc.planted_chunks() if len(c) <= 4095][:40]
    entries, blob = zc.pack_of(chunks)
    want_e, want_b = zc.model_compress(entries, blob)
    dig = np.ascontiguousarray(entries["digest"])
    request, src = fc.tripled_request(np.random.default_rng(1702), dig)
    lengths = entries["length"].astype(np.uint32)[src]
    store = zs.store_add({}, want_e, want_b)
    assert zs.forms_in(store, request)[2:] == [0, 0]
    with M.Engine() as e, e.zset() as zset, e.packset() as plain:
        zset.add_zblob(want_b, want_e, verify=True)
        plain.add_zblob(want_b, want_e, verify=True)
        before = _state(zset)
        for verify in (False, True):
            with zset.zpack(request, lengths, verify=verify) as z:
                cut_e, cut_b = z.entries().copy(), z.read()
            got_e, got_b = _unwrapped_is(zset, request, lengths, verify, cut_e, cut_b)
            with plain.pack(request, lengths, verify=verify) as p:
                _pack_is(zset, request, lengths, verify, p.entries().copy(), p.bytes())
        want_e, want_b = zs.model_zpack_unwrapped(store, request)
        assert _same(got_e, want_e, ZFIELDS) and got_b == want_b
        assert _state(zset) == before


# ---- 3. many rows: every tile boundary, both trips of the wave kernels ------------------------------------------------------------------
def test_both_cuts_of_69637_rows_are_the_models_every_row():
    r = zr.many_rows()
    n_h, both, second = zs.many_rows_conditions(r.is_h, zr.N_ROWS)
    assert (zr.N_ROWS, n_h) == (69637, 6243) and both == 34 and second >= 1
    want_pe = r.entries
    with M.Engine() as e, e.zset(entries_hint=zr.N_ROWS) as zset:
        zset.add_zblob(r.zblob, r.zentries)
        f = zset.count_forms()
        assert int(f.n[2]) + int(f.n[3]) == n_h
        with zset.zpack_unwrapped(r.digests, r.lens32) as z:
            got_e, got_b, info = z.entries(), z.read(), z.info
            assert got_b == r.zb1, _first_diff(got_b, r.zb1)
            assert np.array_equal(got_e["stored"], r.ze1["stored"]) and np.array_equal(got_e["offset"], r.ze1["offset"])
            assert np.array_equal(got_e["chunk_index"], np.arange(zr.N_ROWS)) and np.array_equal(got_e["digest"], r.digests)
            assert np.array_equal(got_e["length"], r.ze1["length"]) and info.stored_bytes == int(r.ze1["stored"].sum())
            assert info.n_raw == int((r.ze1["stored"] == r.ze1["length"]).sum())
        with zset.pack(r.digests, r.lens32, verify=True) as p:
            got_e, got_b = p.entries(), p.bytes()
            assert got_b == r.blob, _first_diff(got_b, r.blob)
            assert np.array_equal(got_e["offset"], want_pe["offset"]) and np.array_equal(got_e["length"], want_pe["length"])
            assert np.array_equal(got_e["chunk_index"], np.arange(zr.N_ROWS)) and np.array_equal(got_e["digest"], r.digests)


# ---- 4. the malformed tables in an unverified set -----------------------------------------------------------------------------------------
STRUCTURAL = ("stored > length", "stored == 0", "overlap", "off-grid offset")


def test_a_row_that_does_not_decode_is_named_with_its_rule_and_nothing_changes():
    table = [(name, en, bl) for name, en, bl, _, _ in ze.malformed_zpacks()]
    table += [(name, en, bl) for name, en, bl, _ in zc.malformed_zpacks() if name.split(",")[0] not in STRUCTURAL]
    good_e, good_b = ze.good_zpack()
    n_unwrap = n_moved = 0
    with M.Engine(max_size=262144) as e:
        for name, entries, blob in table:
            if len({bytes(d) for d in entries["digest"]}) < len(entries):
                continue                                             # (the good entry's form was first: it won)
            store = zs.store_add({}, entries, blob)
            dig = np.ascontiguousarray(entries["digest"])
            row, rule = zs.first_refused(store, dig, zs.decode_rule)
            assert (row, rule) == ze.first_refused(entries, blob), name
            with e.zset() as zset:
                zset.add_zblob(blob, entries)                        # unverified: nothing is decoded at add time
                zset.add_zblob(good_b, good_e, verify=True)
                before = _state(zset)
                hexd = entries["digest"][row].tobytes().hex()
                for verify in (False, True):
                    err = _raises(-1, lambda: zset.pack(dig, verify=verify), "mi_zset_pack: row %d " % row, hexd, "does not decode: ", RULE_WORDS[rule])
                    assert err.first_bad == row, name
                unwrap = zs.first_refused(store, dig, zs.unwrap_rule)
                if unwrap:
                    assert unwrap == (row, rule) and rule >= 7, name
                    for verify in (False, True):
                        err = _raises(-1, lambda: zset.zpack_unwrapped(dig, verify=verify), "mi_zset_zpack_unwrapped: row %d " % row, hexd,
                                      "does not decode: ", RULE_WORDS[rule])
                        assert err.first_bad == row, name
                    n_unwrap += 1
                else:                                                # a bad LZ4 block, bare or inside form H: moved, as zpack moves it
                    want_e, want_b = zs.model_zpack_unwrapped(store, dig)
                    with zset.zpack_unwrapped(dig) as z:
                        assert z.read() == want_b and _same(z.entries(), want_e, ZFIELDS), name
                    if rule == 7:                                    # the cut writes zero pads: what it makes is sound
                        with zset.zpack_unwrapped(dig, verify=True) as z:
                            assert M.zpack_check(z.read(), z.entries()) is None
                    else:
                        err = _raises(-5, lambda: zset.zpack_unwrapped(dig, verify=True), "row %d " % row, RULE_WORDS[rule])
                        assert err.first_bad == row, name
                    n_moved += 1
                assert _state(zset) == before, name
                # a good cut of the good digests from the same set afterwards (a digest the malformed pack holds too kept ITS form)
                gd = np.ascontiguousarray(good_e["digest"][[k for k in range(len(good_e)) if good_e["digest"][k].tobytes() not in store]])
                gstore = zs.store_add({}, good_e, good_b)
                assert len(gd) >= 1
                _unwrapped_is(zset, gd, None, True, *zs.model_zpack_unwrapped(gstore, gd))
                _pack_is(zset, gd, None, True, *zs.model_pack(gstore, gd, pc.SHA256))
    assert n_unwrap >= 40 and n_moved >= 12


# ---- 5. the interface's refusals ------------------------------------------------------------------------------------------------------------
def test_what_the_interface_refuses_and_what_the_results_outlive(planted):
    chunks, entries, blob, h = planted
    keep = [k for k, c in enumerate(chunks) if len(c) <= 8192]
    small = [chunks[k] for k in keep]
    s_entries, s_blob = zc.pack_of(small)
    se, sb = ze.model_compress_h(s_entries, s_blob, 1)
    store = zs.store_add({}, se, sb)
    dig = np.ascontiguousarray(se["digest"])
    lens = se["length"].astype(np.uint32)
    alien = np.frombuffer(zc.sha(b"not held"), dtype=np.uint8).reshape(1, 32)
    with M.Engine() as e, e.zset() as zset:
        zset.add_zblob(sb, se, verify=True)
        L, bad, out = e._lib, C.c_uint64(), C.c_void_p(5)
        before = _state(zset)
        req = np.ascontiguousarray(np.concatenate([dig[:5], alien, dig[5:], alien]))
        zero, other = lens.copy(), lens.copy()
        zero[[4, 7]] = 0
        other[[6, 9]] += 1
        for name, cut, flag in (("mi_zset_zpack_unwrapped", zset.zpack_unwrapped, 0x1), ("mi_zset_pack", zset.pack, 0x1)):
            err = _raises(-1, lambda: cut(req), name + ": row 5", "does not hold digest", alien.tobytes().hex())
            assert err.first_bad == 5
            assert _raises(-1, lambda: cut(dig, zero), name + ": row 4", "length 0").first_bad == 4
            err = _raises(-1, lambda: cut(dig, other), name + ": row 6", dig[6].tobytes().hex(), "with %d bytes" % lens[6], "states %d" % other[6])
            assert err.first_bad == 6
            fn = getattr(L, name)
            for flags in (0x2, 0x4, 0x20, 0x80000000, 0x3):
                out.value = 5
                assert fn(zset._h, dig.ctypes.data, None, len(dig), flags, C.byref(out), C.byref(bad)) == -1 and out.value is None
                assert b"unknown flags" in L.mi_last_error(e._h)
            assert fn(zset._h, dig.ctypes.data, None, 1 << 32, 0, C.byref(out), C.byref(bad)) == -1 and b"2^32" in L.mi_last_error(e._h)
            assert fn(None, dig.ctypes.data, None, 1, 0, C.byref(out), C.byref(bad)) == -1
            assert fn(zset._h, None, None, 1, 0, C.byref(out), C.byref(bad)) == -1 and fn(zset._h, dig.ctypes.data, None, 1, 0, None, None) == -1
            with cut(dig[:0]) as nothing:                            # n = 0: the empty result
                assert len(nothing) == 0 and nothing.info.blob_bytes == 0
            with cut(dig[:0], verify=True) as nothing:
                assert len(nothing) == 0
        assert _state(zset) == before
        # a set of another engine: the result is that engine's child
        with M.Engine() as other_e, other_e.zset() as ozs:
            ozs.add_zblob(sb, se)
            z, p = ozs.zpack_unwrapped(dig[:3]), ozs.pack(dig[:3])
            with e.zset() as mine:
                _raises(-1, lambda: mine.add_zpack(z), "another ctx")
            ozs.close()                                              # the results own copies: they survive mi_zset_free
            assert z.read() == zs.model_zpack_unwrapped(store, dig[:3])[1] and p.bytes() == zs.model_pack(store, dig[:3])[1]
            assert other_e._lib.mi_ctx_destroy(other_e._h) == -6 and b"still alive" in other_e._lib.mi_last_error(other_e._h)
            z.close()
            assert other_e._lib.mi_ctx_destroy(other_e._h) == -6 and b"still alive" in other_e._lib.mi_last_error(other_e._h)
            p.close()
        # a sticky set: the same digest with another length
        liar = se[:1].copy()
        liar["length"] += 1
        _raises(-1, lambda: zset.add_zblob(sb[:zc.round16(int(se["stored"][0]))], liar), "another length")
        for cut in (zset.zpack_unwrapped, zset.pack):
            _raises(-6, lambda: cut(dig), "unusable since", "another length")
            _raises(-6, lambda: cut(dig[:0]), "unusable since")


# ---- 6. after the store's own operations ---------------------------------------------------------------------------------------------------
def test_both_cuts_of_a_pruned_and_recoded_set_are_the_models(planted):
    chunks, entries, blob, h = planted
    keep = [k for k, c in enumerate(chunks) if len(c) <= 8192]
    small = [chunks[k] for k in keep]
    s_entries, s_blob = zc.pack_of(small)
    se, sb = zc.model_compress(s_entries, s_blob)                    # level 1, no stage: the recode brings form H in
    dig = np.ascontiguousarray(se["digest"])
    by_digest = dict((s_entries["digest"][k].tobytes(), small[k]) for k in range(len(small)))
    rng = np.random.default_rng(1706)
    order = rng.permutation(len(small))
    stay, gone = order[: len(small) // 2], order[len(small) // 2:]
    with M.Engine() as e, e.zset() as zset:
        zset.add_zblob(sb, se, verify=True)
        info = zset.prune(dig[stay], keep=True, min_live_permille=500)
        assert info.as_dict() and zset.info.n_digests == len(stay)
        zset.recode(level=2, verify=True, entropy=True)
        f = zset.count_forms()
        assert int(f.n[2]) + int(f.n[3]) > 0                         # the recode made form H
        request, _ = fc.tripled_request(rng, dig[stay])
        with zset.zpack(request, verify=True) as z:                  # what the set holds now, moved verbatim: the models' store
            store = zs.store_add({}, z.entries(), z.read())
        assert zs.forms_in(store, request)[2] + zs.forms_in(store, request)[3] == int(f.n[2]) + int(f.n[3])
        before = _state(zset)
        _unwrapped_is(zset, request, None, True, *zs.model_zpack_unwrapped(store, request))
        got_e, got_b = _pack_is(zset, request, None, True, *zs.model_pack(store, request, pc.SHA256))
        for k in range(len(got_e)):                                  # ... which are the chunks that went in
            a = int(got_e["offset"][k])
            assert got_b[a:a + int(got_e["length"][k])] == by_digest[got_e["digest"][k].tobytes()]
        for cut in (zset.zpack_unwrapped, zset.pack):
            err = _raises(-1, lambda: cut(np.ascontiguousarray(np.concatenate([dig[stay[:2]], dig[gone[:1]]]))), "row 2", "does not hold digest")
            assert err.first_bad == 2
        assert _state(zset) == before


# ---- 7. BLAKE2s -------------------------------------------------------------------------------------------------------------------------------
def test_both_cuts_verify_under_blake2s_and_a_sound_form_under_another_digest_is_caught_by_verify_only(planted):
    chunks = planted[0]
    entries, blob = zc.pack_of(chunks, pc.BLAKE2S)
    dig = np.ascontiguousarray(entries["digest"])
    request, src = fc.tripled_request(np.random.default_rng(1701), dig)
    with _engine(pc.BLAKE2S, max_size=262144) as e:
        assert e.chunk_digest == M.DIGEST_BLAKE2S
        with_h = _compressed(e, entries, blob, (1, 2), True)
        store = {}
        with e.zset() as zset:
            for ze_, zb_ in with_h:
                zset.add_zblob(zb_, ze_, verify=True)
                zs.store_add(store, ze_, zb_)
            assert all(n > 0 for n in zs.forms_in(store, request))
            _unwrapped_is(zset, request, None, True, *zs.model_zpack_unwrapped(store, request))
            _pack_is(zset, request, None, True, *zs.model_pack(store, request, pc.BLAKE2S))
        for name, wentries, wblob, bad in zr.wrong_digest_zpacks(pc.BLAKE2S):
            wstore = zs.store_add({}, wentries, wblob)
            wd = np.ascontiguousarray(wentries["digest"])
            with e.zset() as zset:
                zset.add_zblob(wblob, wentries)
                before = _state(zset)
                _unwrapped_is(zset, wd, None, False, *zs.model_zpack_unwrapped(wstore, wd))
                _pack_is(zset, wd, None, False, *zs.model_pack(wstore, wd))
                err = _raises(-5, lambda: zset.zpack_unwrapped(wd, verify=True), "row %d " % bad, "hash to the requested digest")
                assert err.first_bad == bad, name
                err = _raises(-5, lambda: zset.pack(wd, verify=True), "row %d " % bad, "hash to the requested digest")
                assert err.first_bad == bad, name
                assert _state(zset) == before
