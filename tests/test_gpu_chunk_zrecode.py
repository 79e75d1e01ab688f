"""GPU tests of recoding a compressed pack set in place (mi_zset_recode): after every call the set is held against the model of
zrecode_cases.py -- the held forms, mi_zset_info, mi_zset_usage and every counter of mi_recode_info -- through public calls
only: mi_zset_entries, the cut of all digests (mi_zset_zpack), mi_zset_get_info, mi_zset_get_usage and mi_batch_add_zrecipes.
Bit for bit: there are no tolerances."""
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
import zpack_cases as zc  # noqa: E402
import zpack2_cases as z2  # noqa: E402
import zprune_cases as pr  # noqa: E402
import zrecode_cases as rc  # noqa: E402
import zset_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu
ALGS = [pc.SHA256, pc.BLAKE2S]
NAMES, CHUNKS = rc.planted()
SMALLER, SAME, LARGER, RAW_AT_1 = rc.classes()
assert SMALLER and SAME and RAW_AT_1, "the planted chunks hold both classes, and raw forms that level 2 codes"
STRUCTURAL = ("stored > length", "stored == 0", "overlap", "off-grid offset")


def _engine(alg=pc.SHA256, **kw):
    return M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0, **kw)


def _raises(code, call, *needles):
    with pytest.raises(M.MiError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)
    return ei.value


def _counts(info):
    return {k: v for k, v in info.as_dict().items() if not k.startswith("ms_")}


def _cut(zs, request):
    with zs.zpack(request) as z:
        return z.entries().copy(), z.read()


def _state(zs, request):
    """everything the public calls say about a set"""
    d, ln, st = zs.entries()
    e, b = _cut(zs, request)
    return ({bytes(d[i]): (int(ln[i]), int(st[i])) for i in range(len(d))}, e.tobytes(), b, zs.usage().as_dict(), _counts(zs.info))


def _holds_the_model(zs, store, request):
    """info, usage, the entries and the cut of `request` (distinct digests) against the model"""
    want = store.info()
    got = zs.info.as_dict()
    assert {k: got[k] for k in want} == want
    assert zs.usage().as_dict() == store.usage()
    d, ln, st = zs.entries()
    assert {bytes(d[i]): (int(ln[i]), int(st[i])) for i in range(len(d))} == {k: (v[0], v[2]) for k, v in store.held.items()}
    got_e, got_b = _cut(zs, request)
    want_e, want_b = store.cut(request)
    assert all(np.array_equal(got_e[f], want_e[f]) for f in ("digest", "offset", "chunk_index", "length", "stored"))
    assert got_b == want_b


def _recode_and_compare(zs, store, request, level, verify=False):
    before = zs.usage()
    info = zs.recode(level=level, verify=verify)
    want = store.recode(level, verify=verify)
    assert _counts(info) == want, (_counts(info), want)
    after = zs.usage()
    assert after.live_bytes == info.live_after
    assert after.resident_bytes == before.resident_bytes - info.freed_bytes + (pr.alloc(info.new_blob_bytes) if info.n_recoded else 0)
    assert info.ms_decode > 0 and info.ms_encode > 0 and (info.ms_rebuild > 0) == (info.n_recoded > 0) and (info.ms_verify > 0) == verify
    _holds_the_model(zs, store, request)
    return info


def _restores(e, zs, chunks, dig, order, verify=True):
    with e.batch() as b:
        b.add_zrecipes(zs, [qc.recipe(chunks, order, dig=dig)], verify=verify)
        b.run()
        want = b"".join(chunks[k] for k in order)
        assert b.read_file(0, 0, len(want)) == want


def _three_zpacks():
    """the planted chunks in three groups: random ones only (nothing level 2 can do: that blob must stay), and two mixed"""
    a = [i for i in SAME if NAMES[i].startswith("random")]
    rest = [i for i in range(len(CHUNKS)) if i not in a]
    b, c = rest[0::2], rest[1::2]
    assert a and all(set(g) & set(SMALLER) and set(g) & set(SAME) for g in (b, c))
    return a, b, c


def _set_at(zs, store, groups, level, alg, verify=True):
    for g in groups:
        ze, zb = rc.zpack_at([CHUNKS[i] for i in g], level, alg)
        zs.add_zblob(zb, ze, verify=verify)
        store.add(ze, zb)


# ---- 1, 2, 3, 11. level 1 to level 2: the smaller form, the restore, the second call ---------------------------------------------------
@pytest.mark.parametrize("alg,verify", [(pc.SHA256, False), (pc.SHA256, True), (pc.BLAKE2S, True)])
def test_level_1_to_level_2_holds_the_smaller_form_restores_and_is_idempotent(alg, verify):
    groups = _three_zpacks()
    dig = qc.digests_of(CHUNKS, alg)
    store = rc.Store()
    with _engine(alg) as e, e.zset() as zs:
        _set_at(zs, store, groups, 1, alg)
        _holds_the_model(zs, store, dig)
        info = _recode_and_compare(zs, store, dig, 2, verify)
        for i, c in enumerate(CHUNKS):                                           # the smaller of the two levels' forms
            assert store.held[bytes(dig[i])][2] == min(len(rc.coded(c, 1)), len(rc.coded(c, 2)))
        assert (info.n_recoded, info.n_raw_recoded, info.n_undecodable) == (len(SMALLER), len(RAW_AT_1), 0)
        assert (info.n_blobs_rewritten, info.n_blobs_freed, info.n_rounds) == (2, 2, 1) and zs.usage().n_blobs == 2
        assert info.stored_after < info.stored_before and info.live_after <= info.live_before
        # 2: every chunk's original bytes
        _restores(e, zs, CHUNKS, dig, list(range(len(CHUNKS))) + SMALLER[::-1])
        # 3: a second call at the same level changes nothing
        state = _state(zs, dig)
        again = _recode_and_compare(zs, store, dig, 2, verify)
        assert again.n_recoded == 0 and again.n_blobs_rewritten == 0 and again.stored_after == info.stored_after
        assert _state(zs, dig) == state


# ---- 4. the reverse: nothing level 1 makes is smaller ----------------------------------------------------------------------------------
def test_level_2_forms_recoded_at_level_1_are_kept_verbatim():
    groups = _three_zpacks()
    dig = qc.digests_of(CHUNKS)
    keeps = [i for i, c in enumerate(CHUNKS) if len(rc.coded(c, 1)) >= len(rc.coded(c, 2))]
    assert len(keeps) == len(CHUNKS) - len(LARGER)
    store = rc.Store()
    with _engine() as e, e.zset() as zs:
        _set_at(zs, store, groups, 2, pc.SHA256)
        before = _cut(zs, dig[keeps])
        state = _state(zs, dig)
        info = _recode_and_compare(zs, store, dig, 1)
        assert info.n_recoded == len(LARGER)
        got = _cut(zs, dig[keeps])
        assert got[0].tobytes() == before[0].tobytes() and got[1] == before[1]
        if not LARGER:
            assert _state(zs, dig) == state


# ---- 5. raw in: what mi_pack_compress makes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2])
def test_a_set_of_raw_entries_holds_the_coders_forms_afterwards(level):
    dig = qc.digests_of(CHUNKS)
    ze, zb = rc.raw_zpack(CHUNKS)
    assert all(ze["stored"] == ze["length"])
    store = rc.Store()
    with _engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze, verify=True)
        store.add(ze, zb)
        info = _recode_and_compare(zs, store, dig, level)
        want_e, want_b = rc.zpack_at(CHUNKS, level)                              # model_compress / model_compress2
        got_e, got_b = _cut(zs, dig)
        assert got_b == want_b and all(np.array_equal(got_e[f], want_e[f]) for f in ("digest", "offset", "length", "stored"))
        assert info.n_recoded == info.n_raw_recoded == int((want_e["stored"] < want_e["length"]).sum())
        for i, c in enumerate(CHUNKS):                                           # 1 and 12 bytes, and what does not compress
            if len(c) < 13 or NAMES[i].startswith("random"):
                assert store.held[bytes(dig[i])][2] == len(c), NAMES[i]
        assert {1, 12} <= {len(c) for c in CHUNKS}
        _restores(e, zs, CHUNKS, dig, range(len(CHUNKS)))


# ---- 6. rounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("verify", [False, True])
def test_the_result_does_not_depend_on_the_rounds(verify):
    groups = _three_zpacks()
    dig = qc.digests_of(CHUNKS)
    scratch = 40000
    states = []
    for bound in (0, scratch):
        store = rc.Store()
        with _engine() as e, e.zset() as zs:
            _set_at(zs, store, groups, 1, pc.SHA256)
            assert store.min_rounds(scratch) >= 3 and any(rc.need(v[0], v[2]) > scratch for v in store.held.values())
            info = zs.recode(level=2, verify=verify, scratch_bytes=bound)
            assert info.n_rounds >= store.min_rounds(bound) and (bound or info.n_rounds == 1)
            assert info.n_recoded == len(SMALLER)
            d, ln, st = zs.entries()
            states.append(({bytes(d[i]): (int(ln[i]), int(st[i])) for i in range(len(d))}, _cut(zs, dig)[1], zs.usage().as_dict(), _counts(zs.info)))
            _restores(e, zs, CHUNKS, dig, range(len(CHUNKS)))
    assert states[0] == states[1]


# ---- 7. composition with the prune -----------------------------------------------------------------------------------------------------
def test_prune_then_recode_and_recode_then_prune_hold_the_same_forms():
    groups = _three_zpacks()
    dig = qc.digests_of(CHUNKS)
    keep = np.ascontiguousarray(dig[0::2])
    got = []
    for first in ("prune", "recode"):
        store = rc.Store()
        with _engine() as e, e.zset() as zs:
            _set_at(zs, store, groups, 1, pc.SHA256)
            for step in ((first, "recode" if first == "prune" else "prune")):
                if step == "prune":
                    zs.prune(keep, keep=True, min_live_permille=1000)
                    store.prune(keep, keep=True, permille=1000)
                else:
                    zs.recode(level=2)
                    store.recode(2)
                _holds_the_model(zs, store, keep)
            d, ln, st = zs.entries()
            got.append(({bytes(d[i]): (int(ln[i]), int(st[i])) for i in range(len(d))}, _cut(zs, keep)[1]))
            _restores(e, zs, CHUNKS, dig, range(0, len(CHUNKS), 2))
    assert got[0] == got[1] and len(got[0][0]) == len(keep)


# ---- 8. unverified entries ------------------------------------------------------------------------------------------------------------
def _malformed_among_good():
    """one zpack: good entries (level-1 forms, some of which level 2 makes smaller) with every malformed stream of the table that
    passes the structural check between them, each under a digest of its own -> (entries, blob, good chunk numbers, bad rows)"""
    rng = np.random.default_rng(301)
    good = SMALLER[:6] + SAME[:6]
    specs, bad = [], []
    malformed = [t[1][t[2]] for t in zc.malformed_table() if t[0] not in STRUCTURAL]
    for k, i in enumerate(good):
        specs.append(zc._entry(rc.coded(CHUNKS[i], 1), len(CHUNKS[i]), CHUNKS[i]))
        if k < len(malformed):
            bad.append(len(specs))
            specs.append(dict(malformed[k], offset=None))
    assert len(bad) == len(malformed) == 8
    ze, zb = zc.build_zpack(specs)
    ze["digest"][bad] = rng.integers(0, 256, (len(bad), 32), dtype=np.uint8)
    return ze, zb, good, bad


def test_undecodable_entries_are_counted_and_kept_and_verify_refuses_them():
    ze, zb, good, bad = _malformed_among_good()
    every = np.ascontiguousarray(ze["digest"])
    store = rc.Store()
    with _engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze)
        store.add(ze, zb)
        info = _recode_and_compare(zs, store, every, 2)
        assert info.n_undecodable == len(bad) and info.n_recoded == 6 and info.n_blobs_rewritten == 1
        got_e, got_b = _cut(zs, np.ascontiguousarray(ze["digest"][bad]))         # their stored bytes, verbatim (the cut zeroes pads)
        for k, row in enumerate(bad):
            at, n = int(got_e["offset"][k]), int(ze["stored"][row])
            assert int(got_e["stored"][k]) == n and got_b[at:at + n] == zb[int(ze["offset"][row]):int(ze["offset"][row]) + n]
        _restores(e, zs, CHUNKS, qc.digests_of(CHUNKS), good)
        with e.batch() as b:                                                     # readers refuse them exactly as before
            _raises(-1, lambda: b.add_zrecipes(zs, [(np.ascontiguousarray(ze["digest"][bad[:1]]), ze["length"][bad[:1]].astype(np.uint32))]),
                    "does not decode")
    with _engine() as e, e.zset() as zs:                                         # VERIFY, on a fresh such set
        zs.add_zblob(zb, ze)
        state = _state(zs, every)
        err = _raises(-5, lambda: zs.recode(level=2, verify=True), "%d of %d entries" % (len(bad), len(ze)), "unchanged")
        assert any(bytes(ze["digest"][row]).hex() in str(err) for row in bad)
        assert _state(zs, every) == state


# ---- 9. a form that decodes but does not hash ----------------------------------------------------------------------------------------------
def test_a_form_under_another_digest_is_recoded_and_verify_names_it():
    picks = SMALLER[:4] + SAME[:4]
    chunks = [CHUNKS[i] for i in picks]
    ze, zb = rc.zpack_at(chunks, 1)
    ze["digest"][1] = np.frombuffer(zc.sha(b"another 32 bytes"), dtype=np.uint8)
    every = np.ascontiguousarray(ze["digest"])
    store = rc.Store()
    with _engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze)
        store.add(ze, zb)
        info = _recode_and_compare(zs, store, every, 2)
        assert info.n_recoded == 4 and info.n_undecodable == 0
        assert store.held[bytes(every[1])][2] == len(rc.coded(chunks[1], 2))     # recoded like any other
    with _engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze)
        state = _state(zs, every)
        _raises(-5, lambda: zs.recode(level=2, verify=True), "1 of 8 entries", bytes(every[1]).hex(), "hash to another digest", "unchanged")
        assert _state(zs, every) == state


# ---- 10. the scrub -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_verify_at_the_level_held_is_a_scrub(alg):
    groups = _three_zpacks()
    dig = qc.digests_of(CHUNKS, alg)
    store = rc.Store()
    with _engine(alg) as e, e.zset() as zs:
        _set_at(zs, store, groups, 1, alg)
        state = _state(zs, dig)
        info = _recode_and_compare(zs, store, dig, 1, verify=True)
        assert info.n_recoded == 0 and info.n_blobs_rewritten == 0 and info.ms_verify > 0 and info.new_blob_bytes == 0
        assert _state(zs, dig) == state


# ---- 12. arguments ---------------------------------------------------------------------------------------------------------------------------
def test_arguments_an_empty_set_and_a_set_in_its_failed_state():
    chunks = [CHUNKS[i] for i in SMALLER[:3]]
    ze, zb = rc.zpack_at(chunks, 1)
    dig = np.ascontiguousarray(ze["digest"])
    with _engine() as e, e.zset() as zs:
        L = e._lib
        info = M.RecodeInfo()
        info.n_rounds = 9
        assert L.mi_zset_recode(None, 0, 0, C.byref(info)) == -1 and info.n_rounds == 0
        got = zs.recode(level=2, verify=True)                                    # an empty set: zeros
        assert _counts(got) == dict.fromkeys(_counts(got), 0) and got.ms_verify == 0
        zs.add_zblob(zb, ze, verify=True)
        state = _state(zs, dig)
        for flags in (0x2, 0x8, 0x10 | M.ZPACK_LEVEL2, 0x80000000):
            assert L.mi_zset_recode(zs._h, flags, 0, C.byref(info)) == -1 and b"unknown flags" in L.mi_last_error(e._h)
        assert L.mi_zset_recode(zs._h, M.ZPACK_LEVEL2 | M.ZSET_RECODE_VERIFY, 0, None) == 0          # info may be NULL
        assert zs.info.stored_bytes < state[4]["stored_bytes"]
        liar = ze[:1].copy()
        liar["length"] += 1
        _raises(-1, lambda: zs.add_zblob(zb[:zc.round16(int(ze["stored"][0]))], liar), "another length")
        _raises(-6, lambda: zs.recode(level=2), "mi_zset_recode", "unusable since", "another length")
