"""The models of tests/zserve_cases.py and the inputs of tests/test_gpu_chunk_zserve.py without a GPU: one tiny case of each of
the four forms pinned by hand, the purity condition of the unwrapped cut proved on the planted chunks at both levels, and every
condition the GPU cases rely on proved from the models alone.  The first test fails without the feature: the library exports
neither call.  Bit for bit: there are no tolerances."""
import os
import re
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


def test_the_library_and_the_header_have_both_calls_beside_mi_zset_zpack():
    lib = M.load_library()
    assert lib.mi_abi_version() == 6
    head = open(os.path.join(ROOT, "include", "makisu_mi.h")).read()
    for name, out, flag in (("mi_zset_zpack_unwrapped", "mi_zpack", "MI_ZPACK_VERIFY"), ("mi_zset_pack", "mi_pack", "MI_SUBPACK_VERIFY")):
        assert hasattr(lib, name), name
        decl = re.search(r"MI_BLOCK int\s+%s\(const mi_zset\* s, const uint8_t\* digests, const uint32_t\* lengths, uint64_t n,\s*"
                         r"uint32_t flags /\* %s only \*/, %s\*\* out, uint64_t\* first_bad\);" % (name, flag, out), head)
        assert decl, name
        assert head.index("MI_BLOCK int  mi_zset_zpack(") < decl.start()
    assert callable(M.ZSet.zpack_unwrapped) and callable(M.ZSet.pack)


# ---- 1. the four forms, by hand ----------------------------------------------------------------------------------------------------------
def test_one_tiny_case_of_each_form_is_what_the_hand_says():
    raw = bytes(range(40))
    entries, blob = ze.good_zpack()                                 # LZ4, H over LZ4, raw, H over raw
    store = zs.store_add({}, entries, blob)
    dig = np.ascontiguousarray(entries["digest"])
    assert zs.forms_in(store, dig) == [1, 1, 1, 1]
    # the unwrapped cut: the LZ4 block as it is; the inner block of GOOD_H, which is zpack_cases' level-1 block of the 2 000
    # bytes; the raw chunk; the plain bytes of GOOD_H2 as a raw entry
    want_forms = [zc.GOOD_STREAM, ze.GOOD_INNER, raw, ze.GOOD_PLAIN2]
    assert [len(f) for f in want_forms] == [31, len(zc.compress_chunk(ze.GOOD_PLAIN)), 40, 1024]
    ue, ub = zs.model_zpack_unwrapped(store, dig)
    at = 0
    for k, f in enumerate(want_forms):
        assert (int(ue["offset"][k]), int(ue["stored"][k]), int(ue["length"][k]), int(ue["chunk_index"][k])) == (at, len(f), int(entries["length"][k]), k)
        assert ub[at:at + len(f)] == f and not any(ub[at + len(f):at + zc.round16(len(f))])
        at += zc.round16(len(f))
    assert len(ub) == at == 32 + zc.round16(len(ze.GOOD_INNER)) + 48 + 1024
    assert ze.count_forms(ue, ub)[2:] == [[0, 0], [0, 0]] and ze.count_forms(ue, ub)[0][0] == 2
    assert M.zpack_check(ub, ue) is None
    # the plain cut: the four chunks, each on the 16-byte grid
    pe, pb = zs.model_pack(store, dig, pc.SHA256)
    plains = [zc.GOOD_PLAIN, ze.GOOD_PLAIN, raw, ze.GOOD_PLAIN2]
    assert list(pe["length"]) == [34, 2000, 40, 1024] and list(pe["offset"]) == [0, 48, 48 + 2000, 48 + 2000 + 48]
    assert pb == b"".join(p + bytes(-len(p) % 16) for p in plains)
    assert M.pack_check(pb, pe) is None
    # repeats: the order of first occurrence, chunk_index the row of it
    req = dig[[2, 2, 0, 3, 0, 1]]
    ue, _ = zs.model_zpack_unwrapped(store, req)
    pe, _ = zs.model_pack(store, req)
    assert list(ue["chunk_index"]) == list(pe["chunk_index"]) == [0, 2, 3, 5] and list(ue["stored"]) == [40, 31, 1024, len(ze.GOOD_INNER)]


# ---- 2. purity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2])
def test_the_unwrapped_form_of_a_coded_chunk_is_the_form_under_the_stage(level):
    """the stage wraps a chunk's FINISHED stored form: taking it off gives what a coder without the stage stores"""
    met = set()
    for name, c in ze.planted_chunks_h():
        stored = ze.compress_chunk_h(c, level)
        met.add(ze.form_of(stored, len(c)))
        assert zs.unwrapped_form(stored, len(c)) == ze.under_form(c, level), name
        assert zs.unwrap_rule(stored, len(c)) == 0 == zs.decode_rule(stored, len(c)), name
    assert met == {0, 1, 2, 3}


# ---- 3. what the GPU cases rely on --------------------------------------------------------------------------------------------------------
def test_case_one_request_holds_all_four_forms_and_repeats():
    chunks = [c for _, c in ze.planted_chunks_h()]
    entries, blob = zc.pack_of(chunks)
    store = {}
    for level in (1, 2):
        zs.store_add(store, *ze.model_compress_h(entries, blob, level))
    assert len(store) == len(chunks) == len({bytes(d) for d in entries["digest"]})
    req, src = fc.tripled_request(np.random.default_rng(1701), np.ascontiguousarray(entries["digest"]))
    assert len(req) == 3 * len(chunks) and all(n > 0 for n in zs.forms_in(store, req))
    ue, ub = zs.model_zpack_unwrapped(store, req)
    pe, pb = zs.model_pack(store, req, pc.SHA256)
    assert len(ue) == len(pe) == len(chunks) and list(ue["chunk_index"]) == list(pe["chunk_index"])
    assert list(ue["chunk_index"]) != list(range(len(chunks)))                              # the order of first occurrence is not the rows'
    assert M.zpack_check(ub, ue) is None and M.pack_check(pb, pe) is None
    # purity over the whole request: the cut of a twin set fed the level-1 forms WITHOUT the stage
    twin = zs.store_add({}, *zc.model_compress(entries, blob))
    te, tb = zs.model_zpack_unwrapped(twin, req)
    assert tb == ub and all(np.array_equal(te[f], ue[f]) for f in ("digest", "offset", "chunk_index", "length", "stored"))
    # a kind-1 row's scratch span in the plain cut: inner lengths that are no multiples of 64
    inner = [len(zs.unwrapped_form(s, n)) for s, n, _ in store.values() if ze.form_of(s, n) == 2]
    assert inner and any(v % 64 for v in inner)


def test_the_many_rows_request_has_form_h_at_every_tile_boundary_and_on_the_second_trip():
    r = zr.many_rows()
    n_h, both, second = zs.many_rows_conditions(r.is_h, zr.N_ROWS)
    assert zr.N_ROWS == 69637 and n_h == 6243
    assert both == zr.N_ROWS // zs.PLAN_TILE == 34
    assert second >= 1 and zr.N_ROWS > zs.WAVE_GRID
    assert {int(f) for f in r.forms[zs.WAVE_GRID:]} == {0, 1, 2, 3}                          # the plain cut's second trip meets every branch
    # the model of the unwrapped cut over every row once IS the level-1 zpack without the stage, which zentropy_rows_cases holds
    store = zs.store_add({}, r.zentries, r.zblob)
    ue, ub = zs.model_zpack_unwrapped(store, r.digests)
    assert ub == r.zb1 and np.array_equal(ue["stored"], r.ze1["stored"]) and np.array_equal(ue["offset"], r.ze1["offset"])
    assert np.array_equal(ue["chunk_index"], np.arange(zr.N_ROWS))


def test_the_malformed_tables_rows_are_refused_by_the_models_as_the_cases_expect():
    for name, entries, blob, bad, rule in ze.malformed_zpacks():
        store = zs.store_add({}, entries, blob)
        dig = np.ascontiguousarray(entries["digest"])
        assert ze.first_refused(entries, blob) == (bad, rule), name
        assert zs.first_refused(store, dig, zs.decode_rule) == (bad, rule), name
        got = zs.first_refused(store, dig, zs.unwrap_rule)
        assert got == ((bad, rule) if rule >= 7 else None), name                             # the inner block is moved, not decoded
    seen = set()
    for name, entries, blob, bad in zc.malformed_zpacks():
        if M.zpack_check(blob, entries) != bad or len({bytes(d) for d in entries["digest"]}) < len(entries):
            continue
        try:
            store = zs.store_add({}, entries, blob)
        except Exception:
            continue
        if any(len(s) == 0 or len(s) > n for s, n, _ in store.values()):
            continue                                                                          # structural: no set takes it
        got = zs.first_refused(store, np.ascontiguousarray(entries["digest"]), zs.decode_rule)
        if got is None:
            continue
        assert got[0] == bad, name
        assert zs.first_refused(store, np.ascontiguousarray(entries["digest"]), zs.unwrap_rule) is None, name      # no form H: moved verbatim
        seen.add(got[1])
    assert seen >= {1, 2, 3, 4, 5, 6, 7}
