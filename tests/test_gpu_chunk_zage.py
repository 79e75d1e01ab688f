"""GPU tests of a compressed pack set that ages (mi_zset_set_epoch, _get_epoch, _touch, _stamps, _age_census, _expire; DESIGN.md
4.18).  After every step the set is held against the model of zage_cases.py -- every stamp, mi_touch_info, the census bins, every
counter of mi_prune_info -- against a TWIN set that never ages (what exists does not change) and, for an expiry, against a twin
that is pruned with the victims as a list.  Bit for bit: there are no tolerances.  The malformed inputs are argument errors
refused on the host."""
import ctypes as C
import functools
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
import store_rows_cases as sr  # noqa: E402
import zage_cases as ag  # noqa: E402
import zpack_cases as zc  # noqa: E402
import zprune_cases as pr  # noqa: E402
import zrecode_cases as rc  # noqa: E402
import zset_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu
ALGS = [pc.SHA256, pc.BLAKE2S]
NOT_AGEING = "does not age"


def _engine(alg, **kw):
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


def _cut(zs, request, verify=False):
    with zs.zpack(request, verify=verify) as z:
        return z.entries().copy().tobytes(), z.read()


def _entries(zs):
    d, ln, st = zs.entries()
    return {bytes(d[i]): (int(ln[i]), int(st[i])) for i in range(len(d))}


def _holds_the_model(zs, store):
    """info, usage, the entries and the clock against the model"""
    want = store.info()
    got = zs.info.as_dict()
    assert {k: got[k] for k in want} == want
    assert zs.usage().as_dict() == store.usage()
    assert _entries(zs) == {k: (v[0], v[2]) for k, v in store.held.items()}
    assert zs.epoch == (store.ageing, store.epoch, store.stamp_bytes())


def _stamps_follow(zs, store, universe, seed):
    """stamps over every digest ever added and the strangers, in a permuted order with repeats, against the model"""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.permutation(len(universe)), rng.integers(0, len(universe), 64)])
    request = np.ascontiguousarray(universe[rows])
    assert zs.stamps(request).tolist() == store.stamps(request)


def _tiny(lo, hi):
    """distinct chunks of 8..12 bytes, store_rows_cases' tiny rows: always stored as they are"""
    return [((k * sr.ODD) % (1 << 64)).to_bytes(8, "little") + bytes([0x51, 0x52, 0x53, 0x54][:k % 5]) for k in range(lo, hi)]


STRANGERS = np.frombuffer(b"".join(zc.sha(b"never held %d" % i) for i in range(5)), dtype=np.uint8).reshape(-1, 32)


# ---- 1. off means off -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_off_means_off(alg):
    rng = np.random.default_rng(1811)
    chunks = [zc.text_like(500 + 30 * i, i) if i % 2 else rng.integers(0, 256, 40 + i, dtype=np.uint8).tobytes() for i in range(10)]
    chunks += [sr.planted_chunk(5), sr.planted_chunk(13)]                       # level 1 keeps them raw, level 2 codes them
    _, _, ze, zb = qc.zpack_of(chunks, alg)
    dig = qc.digests_of(chunks, alg)
    store = rc.Store()                                                          # THE EXISTING MODELS: zprune_cases, zrecode_cases
    bounds = np.array([1, 2], dtype=np.uint32)
    with _engine(alg) as e, e.zset() as zs:
        zs.add_zblob(zb, ze, verify=True)
        store.add(ze, zb)
        for _ in range(2):
            for call in (lambda: zs.touch(dig[:3]), lambda: zs.stamps(dig[:3]), lambda: zs.age_census(bounds), lambda: zs.expire(0), lambda: zs.expire(1, 500)):
                _raises(-6, call, NOT_AGEING)
            assert zs.epoch == (False, 0, 0)
            info = zs.prune(dig[[0, 3]], keep=False, min_live_permille=1000)
            assert _counts(info) == store.prune(dig[[0, 3]], keep=False, permille=1000) and info.n_dropped in (2, 0)
            info = zs.recode(level=2, verify=True)
            assert _counts(info) == store.recode(2, verify=True)
            want = store.info()
            assert {k: zs.info.as_dict()[k] for k in want} == want and zs.usage().as_dict() == store.usage()
        assert store.info()["n_digests"] == 10


# ---- 2. stamps follow the model through every rebuild ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _growing_packs(alg):
    """three_fates() plus 1 100 tiny chunks and three chunks only level 2 codes, in three zpacks; the third brings five of the
    first one's tiny chunks again -> (chunks, digests, [(zentries, zblob)] * 3, [chunk numbers] * 3)"""
    a, b, c, _ = pr.three_fates()
    tiny = _tiny(0, 1100)
    l2 = [sr.planted_chunk(k) for k in (5, 13, 21)]
    chunks = a + b + c + tiny + l2
    na, nb, ncc = len(a), len(b), len(c)
    t0 = na + nb + ncc
    parts = [list(range(na)) + list(range(t0, t0 + 400)),
             list(range(na, na + nb)) + list(range(t0 + 400, t0 + 800)),
             list(range(na + nb, t0)) + list(range(t0 + 800, t0 + 1100)) + list(range(t0, t0 + 5)) + list(range(t0 + 1100, t0 + 1103))]
    assert len(set(chunks)) == len(chunks)
    packs = [qc.zpack_of([chunks[k] for k in part], alg)[2:] for part in parts]
    return chunks, qc.digests_of(chunks, alg), packs, parts


@pytest.mark.parametrize("alg", ALGS)
def test_stamps_follow_the_model_through_every_rebuild(alg):
    chunks, dig, packs, parts = _growing_packs(alg)
    universe = np.ascontiguousarray(np.concatenate([dig, STRANGERS]))
    a, b, c, stay = pr.three_fates()
    store = ag.Store()
    with _engine(alg) as e, e.zset() as zs, e.zset() as twin:                   # (an entries hint of 0: 1 024 slots)
        zs.set_epoch(1)                                                         # on an empty set
        store.set_epoch(1)
        _holds_the_model(zs, store)
        slots = []
        for epoch, pack in zip((1, 2, 3), packs):
            zs.set_epoch(epoch)
            store.set_epoch(epoch)
            zs.add_zblob(pack[1], pack[0], verify=True)
            twin.add_zblob(pack[1], pack[0], verify=True)
            store.add(*pack)
            _holds_the_model(zs, store)
            _stamps_follow(zs, store, universe, 100 + epoch)
            slots.append(zs.usage().table_slots)
        assert slots == [1024, 2048, 4096]                                      # the table grew twice, the stamps with it
        t0 = len(a) + len(b) + len(c)
        assert zs.stamps(dig[[t0, t0 + 4, t0 + 5]]).tolist() == [3, 3, 1]        # a re-add refreshes
        assert twin.usage().as_dict() == zs.usage().as_dict() and twin.epoch == (False, 0, 0)
        # a touch with repeats and strangers
        zs.set_epoch(4)
        store.set_epoch(4)
        touched = np.ascontiguousarray(np.concatenate([dig[[1, 1, len(a) + 2, t0 + 7, 1, t0 + 900]], STRANGERS[[0, 0, 3]], dig[[t0 + 7]]]))
        before = (zs.info.as_dict(), zs.usage().as_dict(), _entries(zs), zs.count_forms().as_dict())
        info = zs.touch(touched)
        assert _counts(info) == store.touch(touched) == {"n_rows": 10, "n_unknown": 3, "n_refreshed": 4} and info.ms_touch > 0
        assert (zs.info.as_dict(), zs.usage().as_dict(), _entries(zs), zs.count_forms().as_dict()) == before      # nothing but stamps
        _stamps_follow(zs, store, universe, 104)
        assert _counts(zs.touch(touched)) == {"n_rows": 10, "n_unknown": 3, "n_refreshed": 0}
        assert _counts(zs.touch(np.zeros((0, 32), dtype=np.uint8))) == {"n_rows": 0, "n_unknown": 0, "n_refreshed": 0}
        # a list prune with compaction: a dies, b keeps half, c loses its large chunks, every third tiny chunk goes
        goes = list(range(len(a))) + [len(a) + k for k in range(len(b)) if k not in stay] + list(range(len(a) + len(b), t0 - 1)) + \
            list(range(t0, t0 + 1100, 3))
        request = np.ascontiguousarray(np.concatenate([dig[goes], STRANGERS[:2], dig[goes[:3]]]))
        info = zs.prune(request, keep=False, min_live_permille=1000)
        tinfo = twin.prune(request, keep=False, min_live_permille=1000)
        want = store.prune(request, keep=False, permille=1000)
        assert _counts(info) == want and info.n_blobs_compacted >= 2 and info.n_dropped == len(goes)
        assert _counts(tinfo) == dict(want, peak_extra_bytes=want["peak_extra_bytes"] - ag.alloc(4 * store.slots))
        _holds_the_model(zs, store)
        _stamps_follow(zs, store, universe, 105)
        # a level-2 recode, then a level-1 recode with the entropy stage: the stamps stay with their digests
        info = zs.recode(level=2, verify=True)
        tinfo = twin.recode(level=2, verify=True)
        want = store.recode(2, verify=True)
        assert _counts(info) == want and info.n_recoded >= 3
        assert _counts(tinfo) == dict(want, peak_extra_bytes=want["peak_extra_bytes"] - ag.alloc(4 * store.slots))
        _holds_the_model(zs, store)
        _stamps_follow(zs, store, universe, 106)
        info = zs.recode(level=1, verify=True, entropy=True)
        tinfo = twin.recode(level=1, verify=True, entropy=True)
        assert info.n_recoded >= 1                                              # (the entropy stage has no Store model: the twin is the reference)
        assert _counts(info) == dict(_counts(tinfo), peak_extra_bytes=tinfo.peak_extra_bytes + ag.alloc(4 * zs.usage().table_slots))
        assert _entries(zs) == _entries(twin) and zs.usage().as_dict() == twin.usage().as_dict()
        assert zs.epoch == (True, 4, ag.alloc(4 * zs.usage().table_slots))
        _stamps_follow(zs, store, universe, 107)
        survivors = np.ascontiguousarray(dig[[k for k in range(len(chunks)) if bytes(dig[k]) in store.held]])
        assert _cut(zs, survivors, verify=True) == _cut(twin, survivors, verify=True)


# ---- 3. expiry is the list prune -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fates(alg):
    a, b, c, stay = pr.three_fates()
    chunks = a + b + c
    return chunks, qc.digests_of(chunks, alg), [qc.zpack_of(part, alg)[2:] for part in (a, b, c)], [len(a) + k for k in stay]


def _aged_pair(e, alg, n_sets=2):
    """sets of one engine and their models, fed the same zpacks (epochs 1, 2, 3; ageing begins AFTER the first add) and the same
    touch at epoch 4: stamps 1 (a), 2 (half of b), 3 (c) and 4 (the other half of b)"""
    chunks, dig, packs, used = _fates(alg)
    sets = [e.zset() for _ in range(n_sets)]
    stores = [ag.Store() for _ in range(n_sets)]
    for zs, store in zip(sets, stores):
        for epoch, pack in zip((1, 2, 3), packs):
            if epoch > 1:
                zs.set_epoch(epoch)
                store.set_epoch(epoch)
            zs.add_zblob(pack[1], pack[0], verify=True)
            store.add(*pack)
            if epoch == 1:
                zs.set_epoch(1)                                                 # everything already held is stamped
                store.set_epoch(1)
        zs.set_epoch(4)
        store.set_epoch(4)
        assert _counts(zs.touch(dig[used])) == store.touch(dig[used])
        assert zs.stamps(dig).tolist() == store.stamps(dig)
    return sets, stores


@pytest.mark.parametrize("permille", [0, 600, 1000])
@pytest.mark.parametrize("alg", ALGS)
def test_expiry_is_the_list_prune(alg, permille):
    chunks, dig, _, _ = _fates(alg)
    with _engine(alg) as e:
        for min_epoch in (2, 3, 4):                                             # each value that changes the victim set; 4 is the epoch
            (zs, zt), (store, twin) = _aged_pair(e, alg)
            with zs, zt, e.index() as idx:
                stamps = zt.stamps(dig)
                victims = np.flatnonzero(stamps < min_epoch)
                stays = [k for k in range(len(chunks)) if k not in set(victims.tolist())]
                assert len(victims) and len(stays)
                survivors = np.ascontiguousarray(dig[stays[::-1] + stays[:2]])
                cut_before = _cut(zs, survivors, verify=True)
                assert idx.load(dig.tobytes()) == len(dig)
                info = zs.expire(min_epoch, permille)
                tinfo = zt.prune(dig[victims], keep=False, min_live_permille=permille)
                got, other = _counts(info), _counts(tinfo)
                assert got == store.expire(min_epoch, permille) and other == twin.prune(dig[victims], keep=False, permille=permille)
                assert (got.pop("n_rows"), other.pop("n_rows"), got["n_dropped"]) == (0, len(victims), len(victims))
                assert got.pop("peak_extra_bytes") == other.pop("peak_extra_bytes") - pr.alloc(32 * len(victims)) + pr.alloc(0)
                assert got == other
                _holds_the_model(zs, store)
                assert zs.usage().as_dict() == zt.usage().as_dict() and _entries(zs) == _entries(zt)
                assert _cut(zs, survivors, verify=True) == _cut(zt, survivors, verify=True) == cut_before
                assert zs.stamps(dig).tolist() == zt.stamps(dig).tolist() == store.stamps(dig)         # survivors keep their stamps
                with e.batch() as b:
                    b.add_zrecipes(zs, [qc.recipe(chunks, stays + stays[::-1], dig=dig)], verify=True)
                    b.run()
                    want = b"".join(chunks[k] for k in stays + stays[::-1])
                    assert b.read_file(0, 0, len(want)) == want
                assert _raises(-1, lambda: zs.zpack(dig[[stays[0], int(victims[0])]]), "row 1", "does not hold").first_bad == 1
                idx.retain(zs)                                                  # the index's half: no list here either
                blob = idx.export()
                assert {blob[i:i + 32] for i in range(0, len(blob), 32)} == {bytes(dig[k]) for k in stays} and len(idx) == len(stays)


# ---- 4. the census ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_the_census_is_the_models_and_says_what_an_expiry_will_drop(alg):
    with _engine(alg) as e:
        (zs,), (store,) = _aged_pair(e, alg, 1)
        with zs:
            for bounds in ([3], [1], [5], [2, 3, 4], [1, 2, 4], list(range(1, 256)), list(range(0, 255)), [0, 4, 0xFFFFFFFF]):
                bins = [b.as_dict() for b in zs.age_census(bounds)]
                assert bins == store.census(bounds), bounds
                assert len(bins) == len(bounds) + 1 and sum(b["live_bytes"] for b in bins) == zs.usage().live_bytes
                assert sum(b["n_digests"] for b in bins) == zs.info.n_digests
            assert [b.n_digests for b in zs.age_census([2, 3, 4])] == [3, 4, 6, 4]
            for min_epoch in (2, 3, 4):                                         # bounds = [E]: bin 0 is what expire(E) drops
                b0 = zs.age_census([min_epoch])[0]
                info = zs.expire(min_epoch, 0)
                assert (b0.n_digests, b0.stored_bytes, b0.chunk_bytes) == (info.n_dropped, info.dropped_stored_bytes, info.dropped_chunk_bytes)
                assert _counts(info) == store.expire(min_epoch, 0) and info.n_dropped > 0
                assert zs.age_census([min_epoch])[0].as_dict() == dict.fromkeys(["n_digests", "stored_bytes", "live_bytes", "chunk_bytes"], 0)
            assert zs.info.n_digests == 4


# ---- 5. what is refused leaves everything as it was ------------------------------------------------------------------------------------
def test_what_is_refused_leaves_everything_as_it_was():
    alg = pc.SHA256
    chunks, dig, packs, _ = _fates(alg)
    with _engine(alg) as e:
        (zs,), (store,) = _aged_pair(e, alg, 1)
        with zs:
            L = e._lib

            def state():
                return _counts(zs.info), zs.usage().as_dict(), _entries(zs), zs.stamps(dig).tolist(), zs.epoch

            s0 = state()
            _raises(-1, lambda: zs.set_epoch(3), "behind")                      # the clock never goes back
            _raises(-1, lambda: zs.set_epoch(0xFFFFFFFF), "reserved")
            zs.set_epoch(4)                                                     # equal: a no-op
            _raises(-1, lambda: zs.expire(5), "above the set's epoch")
            _raises(-1, lambda: zs.expire(4, 1001), "1000")
            for bounds in ([2, 2], [3, 2], [1, 2, 2, 5], list(range(256))):
                _raises(-1, lambda: zs.age_census(bounds), "bounds" if len(bounds) > 255 else "ascend")
            bins = (M.AgeBin * 4)()
            one = np.array([1], dtype=np.uint32)
            assert L.mi_zset_age_census(zs._h, one.ctypes.data, 0, C.addressof(bins)) == -1 and b"1 to 255" in L.mi_last_error(e._h)
            assert L.mi_zset_age_census(zs._h, None, 1, C.addressof(bins)) == -1 and L.mi_zset_age_census(zs._h, one.ctypes.data, 1, None) == -1
            ti, out = M.TouchInfo(), np.zeros(4, dtype=np.uint32)
            assert L.mi_zset_touch(zs._h, None, 1, C.byref(ti)) == -1 and L.mi_zset_stamps(zs._h, None, 1, out.ctypes.data) == -1
            assert L.mi_zset_stamps(zs._h, dig.ctypes.data, 1, None) == -1
            assert L.mi_zset_touch(zs._h, dig.ctypes.data, 1 << 32, C.byref(ti)) == -1 and b"2^32" in L.mi_last_error(e._h)
            assert L.mi_zset_stamps(zs._h, dig.ctypes.data, 1 << 32, out.ctypes.data) == -1 and b"2^32" in L.mi_last_error(e._h)
            assert L.mi_zset_touch(zs._h, None, 0, C.byref(ti)) == 0 and L.mi_zset_stamps(zs._h, None, 0, None) == 0
            assert state() == s0
            # nothing older: nothing dropped, no rebuild
            slots = zs.usage().table_slots
            info = zs.expire(1, 1000)
            assert _counts(info) == store.expire(1, 1000) and (info.n_dropped, info.n_blobs_freed, info.ms_rebuild) == (0, 0, 0)
            assert state() == s0 and zs.usage().table_slots == slots
            # the same digest with another length: the set is unusable, and every new call says why
            ze, zb = packs[0]
            liar = ze[:1].copy()
            liar["length"] += 1
            _raises(-1, lambda: zs.add_zblob(zb[:zc.round16(int(ze["stored"][0]))], liar), "another length")
            for call in (lambda: zs.set_epoch(9), lambda: zs.epoch, lambda: zs.touch(dig[:1]), lambda: zs.stamps(dig[:1]),
                         lambda: zs.age_census([1]), lambda: zs.expire(1)):
                _raises(-6, call, "unusable since", "another length")


# ---- 6. beyond the first trip of the grid-stride kernels -------------------------------------------------------------------------------
def _tiny_zpack(first8, seed):
    """rows of 8..12 bytes under crafted digests whose first eight bytes are `first8`: each row is one 16-byte unit of the blob,
    stored as it is (store_rows_cases' tiny rows) -> (digests, zentries, zblob)"""
    n = len(first8)
    k = np.asarray(first8, dtype=np.uint64)
    dig = np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
    dig[:, :8] = k.astype("<u8").view(np.uint8).reshape(n, 8)
    lengths = (8 + k % 5).astype(np.uint32)
    blob = np.zeros((n, 16), dtype=np.uint8)
    blob[:, :8] = (k * np.uint64(sr.ODD)).astype("<u8").view(np.uint8).reshape(n, 8)
    for i in range(4):
        blob[(k % 5) > i, 8 + i] = 0x51 + i
    ze = sr.entries_of(zc.ZENTRY_DTYPE, dig, np.arange(n, dtype=np.uint64) * 16, np.arange(n), lengths, lengths)
    return dig, ze, blob.tobytes()


def test_beyond_the_first_trip_of_the_grid_stride_kernels():
    """270 000 digests in three zpacks at three epochs: the table ends at 2^20 slots -- above the 524 288 one pass of 2 048 x 256
    threads covers -- after three growths; a digest's home is its first eight bytes & (slots - 1), so the third zpack's lie on
    both sides of slot 524 288"""
    per, half = 90000, 1 << 19
    firsts = [np.arange(1, per + 1), np.arange(100001, 100001 + per), np.arange(half - per // 2, half + per // 2)]
    packs = [_tiny_zpack(f, 1860 + i) for i, f in enumerate(firsts)]
    lens = [p[1]["length"].astype(np.int64) for p in packs]
    near = np.arange(per // 2 - 1250, per // 2 + 1250)                          # the third zpack's homes 524 288 - 1 250 .. + 1 250
    sample = np.ascontiguousarray(np.concatenate([packs[0][0][:1250], packs[1][0][-1250:], packs[2][0][near]]))
    want_stamps = [1] * 1250 + [2] * 1250 + [3] * 2500
    assert len(sample) == 5000 and firsts[2][near[0]] < half <= firsts[2][near[-1]]
    with M.Engine() as e, e.zset() as zs:
        zs.set_epoch(1)
        for epoch, (dig, ze, zb) in zip((1, 2, 3), packs):
            zs.set_epoch(epoch)
            zs.add_zblob(zb, ze)
        assert zs.usage().table_slots == 1 << 20 and zs.info.n_digests == 3 * per and zs.epoch == (True, 3, ag.alloc(4 << 20))
        bins = zs.age_census([1, 2, 3])
        assert [b.as_dict() for b in bins] == [dict.fromkeys(["n_digests", "stored_bytes", "live_bytes", "chunk_bytes"], 0)] + \
            [{"n_digests": per, "stored_bytes": int(n.sum()), "live_bytes": 16 * per, "chunk_bytes": int(n.sum())} for n in lens]
        assert zs.stamps(sample).tolist() == want_stamps
        info = zs.expire(2, 0)                                                  # the oldest epoch's digests, exactly
        assert (info.n_rows, info.n_unknown, info.n_dropped, info.dropped_stored_bytes, info.n_blobs_freed) == (0, 0, per, int(lens[0].sum()), 1)
        assert zs.usage().table_slots == 1 << 19 and zs.info.n_digests == 2 * per
        assert zs.stamps(sample).tolist() == [ag.NONE] * 1250 + want_stamps[1250:]
        held, _, _ = zs.missing(sample)
        assert held.tolist() == [0] * 1250 + [1] * 3750
        zs.set_epoch(4)
        assert _counts(zs.touch(sample)) == {"n_rows": 5000, "n_unknown": 1250, "n_refreshed": 3750}
        assert [b.n_digests for b in zs.age_census([3, 4])] == [per - 1250, per - 2500, 3750]
