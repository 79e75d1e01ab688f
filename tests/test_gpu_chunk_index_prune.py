"""GPU tests of the chunk index's query, prune and retain calls (mi_index_query, mi_index_query_batch, mi_index_prune,
mi_index_retain_zset).  After every prune the index is held against the model of index_cases.py: its count, its
export (whose own cursor-against-count check runs), a query over every digest the test ever used, and mi_index_prune_info field
for field -- slots_after and peak_extra_bytes included.  The indexes are fed through mi_index_import, which takes arbitrary
digests, unless a batch is named.  Bit for bit: there are no tolerances.

No kernel of these calls runs grid-stride under a capped grid (one thread a row or slot, the grid grows with the request), so
there is no large case."""
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
import index_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu
ALGS = [0, M.FLAG_CHUNK_BLAKE2S]
NONE = np.zeros((0, 32), dtype=np.uint8)


def _counts(info):
    return {k: getattr(info, k) for k in ic.INFO_FIELDS}


def _export_set(idx):
    blob = idx.export()
    out = [blob[i:i + 32] for i in range(0, len(blob), 32)]
    assert len(set(out)) == len(out)
    return set(out)


def _holds_the_model(idx, model, universe):
    """count, export and a query over every digest ever used, against the model"""
    assert len(idx) == len(model.held)
    assert _export_set(idx) == model.held
    assert idx.query(universe).tolist() == model.query(universe)
    u, n_held = np.ascontiguousarray(universe, dtype=np.uint8), C.c_uint64()
    assert idx._lib.mi_index_query(idx._h, u.ctypes.data, len(u), None, C.byref(n_held)) == 0 and n_held.value == sum(model.query(universe))


def _prune_and_compare(idx, model, digests, keep, universe):
    info = idx.prune(digests, keep=keep)
    want = model.prune(digests, keep=keep)
    assert _counts(info) == want, (_counts(info), want)
    assert (info.ms_rebuild > 0) == (info.rebuilt == 1) and (info.ms_mark > 0 or info.slots_before == 0)
    _holds_the_model(idx, model, universe)
    return info


def _fed(e, digests, hint=0):
    """an index and its model that hold `digests`, through mi_index_import"""
    idx, model = e.index(hint), ic.Index(hint)
    assert idx.load(np.ascontiguousarray(digests).tobytes()) == model.add(digests)
    return idx, model


# ---- 1. a random third, with strangers and repeats, in both modes and under both algorithms ----------------------------------------
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("flags", ALGS)
def test_a_random_third_with_strangers_and_repeats(flags, keep):
    rng = np.random.default_rng(1301)
    dig = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
    strangers = rng.integers(0, 256, (100, 32), dtype=np.uint8)
    third = dig[rng.choice(3000, 1000, replace=False)]
    request = np.concatenate([third, strangers])
    request = np.concatenate([request, request[rng.choice(len(request), 200, replace=False)]])
    request = np.ascontiguousarray(request[rng.permutation(len(request))])
    universe = np.ascontiguousarray(np.concatenate([dig, strangers]))
    with M.Engine(flags=flags) as e:
        idx, model = _fed(e, dig)
        with idx:
            _holds_the_model(idx, model, universe)
            info = _prune_and_compare(idx, model, request, keep, universe)
            assert (info.n_rows, info.n_before, info.n_dropped, info.n_after) == (1300, 3000, 2000 if keep else 1000, 1000 if keep else 2000)
            assert info.n_unknown >= 100 and (info.slots_before, info.slots_after) == (8192, 2048 if keep else 4096)
            assert idx.query(strangers).tolist() == [0] * 100                 # a prune never adds: a never-held digest in a KEEP list too
            # a dropped digest is one that was never added: the import takes the dropped ones again and nothing else
            assert idx.load(dig.tobytes()) == model.add(dig) == info.n_dropped
            _holds_the_model(idx, model, universe)


# ---- 2. shrink, regrow, nothing to drop ----------------------------------------------------------------------------------------------------
def test_keep_nothing_shrinks_an_import_regrows_and_nothing_to_drop_touches_nothing():
    rng = np.random.default_rng(1302)
    dig = rng.integers(0, 256, (5000, 32), dtype=np.uint8)
    strangers = rng.integers(0, 256, (7, 32), dtype=np.uint8)
    universe = np.ascontiguousarray(np.concatenate([dig, strangers]))
    with M.Engine() as e:
        idx, model = _fed(e, dig[:3000])
        with idx:
            info = _prune_and_compare(idx, model, NONE, True, universe)                     # KEEP nothing
            assert (info.n_dropped, info.n_after, info.slots_before, info.slots_after, info.rebuilt) == (3000, 0, 8192, 1024, 1)
            assert len(idx) == 0 and idx.export() == b""
            assert idx.load(dig.tobytes()) == model.add(dig) == 5000                        # shrink, then regrow
            _holds_the_model(idx, model, universe)
            for request in (NONE, strangers, np.ascontiguousarray(strangers[[0, 0, 3]])):  # DROP of nothing, of unknown digests only
                info = _prune_and_compare(idx, model, request, False, universe)
                assert (info.rebuilt, info.n_dropped, info.n_unknown, info.n_after) == (0, 0, len(request), 5000)
                assert info.slots_before == info.slots_after == 16384 and info.ms_rebuild == 0
            info = _prune_and_compare(idx, model, universe, True, universe)                 # KEEP of everything: nothing to drop either
            assert (info.rebuilt, info.n_unknown, info.slots_after) == (0, 7, 16384)


# ---- 3. chains: an in-place delete would hide the survivors behind the hole -----------------------------------------------------------
CHAINS = {"a": lambda rng: ic.same_first8(5, rng), "b": lambda rng: ic.same_home(6, rng), "c": lambda rng: ic.last_slot(4, rng)}


@pytest.mark.parametrize("which", sorted(CHAINS))
def test_the_survivors_of_a_chain_are_found_behind_what_was_dropped(which):
    """Which member of a chain sits first is the probe's race, so EVERY member is dropped in turn from a fresh index -- the first
    of the chain and the middle ones are among them -- and then all but each one in turn -- all but the last among them.  An
    implementation that clears slots in place leaves a hole in front of a survivor: its query and its import would miss it."""
    rng = np.random.default_rng(1303)
    chain = CHAINS[which](rng)
    k = len(chain)
    assert all(len({ic.home(d, s) for d in chain}) == 1 for s in (1024, 65536)) and len(set(ic.keys(chain))) == k
    assert len({ic.tag_of(d) for d in chain}) == (1 if which == "a" else k)
    if which == "c":
        assert all(ic.home(d, 1024) == 1023 for d in chain)
    others = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    everything = np.ascontiguousarray(np.concatenate([chain, others]))
    with M.Engine() as e:
        for victims in [[i] for i in range(k)] + [[j for j in range(k) if j != i] for i in range(k)]:
            idx, model = _fed(e, everything)
            with idx:
                rest = [j for j in range(k) if j not in victims]
                info = _prune_and_compare(idx, model, np.ascontiguousarray(chain[victims]), False, everything)
                assert (info.n_dropped, info.n_after, info.slots_after) == (len(victims), 500 + len(rest), 1024)
                assert idx.query(chain).tolist() == [0 if j in victims else 1 for j in range(k)]
                assert idx.load(np.ascontiguousarray(everything[[j for j in range(len(everything)) if j not in victims]]).tobytes()) == 0
                assert idx.load(np.ascontiguousarray(chain[victims[:1]]).tobytes()) == 1
                assert len(idx) == 500 + len(rest) + 1


# ---- 4. both digests stored under tag 1 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gone", [0, 1])
def test_a_zero_tag_and_tag_one_are_told_apart(gone):
    rng = np.random.default_rng(1304)
    pair = ic.zero_and_one(rng)
    assert ic.tag_of(pair[0]) == ic.tag_of(pair[1]) == 1 and bytes(pair[0][:8]) != bytes(pair[1][:8])
    everything = np.ascontiguousarray(np.concatenate([pair, rng.integers(0, 256, (50, 32), dtype=np.uint8)]))
    with M.Engine() as e:
        idx, model = _fed(e, everything)
        with idx:
            assert idx.query(pair).tolist() == [1, 1]
            _prune_and_compare(idx, model, pair[[gone]], False, everything)
            assert idx.query(pair).tolist() == [0 if j == gone else 1 for j in range(2)]
            _prune_and_compare(idx, model, pair[[1 - gone]], True, everything)              # KEEP the other one alone
            assert len(idx) == 1 and idx.query(pair).tolist() == [0 if j == gone else 1 for j in range(2)]


# ---- 5, 6. a real batch ----------------------------------------------------------------------------------------------------------------------
def _batch(e):
    """24 synthetic files of 64 KiB, two of them identical: a few hundred chunks with in-batch repeats"""
    b = e.batch()
    b.add_synthetic([65536] * 24, list(range(23)) + [5], seed=0x1305)
    b.run()
    ch = b.chunks()
    dig = np.ascontiguousarray(ch["sha256"])
    assert 100 <= len(dig) <= 2000 and (ch["dup_of"] >= 0).sum() > 0
    return b, dig, ch["dup_of"] < 0


def test_query_batch_is_add_batch_without_the_adding_and_a_pruned_digest_is_new_again():
    with M.Engine() as e:
        b, dig, first = _batch(e)
        with b, e.index() as idx, e.index() as copy:
            model = ic.Index()
            distinct = ic.keys(dig[first])
            assert idx.query_batch(b).tolist() == [0] * len(dig) and len(idx) == 0          # an in-batch repeat of a digest it lacks: 0
            known, n_new, _ = idx.add_batch(b)
            assert n_new == model.add(dig) == len(distinct) and known.tolist() == [0] * len(dig)
            exported = _export_set(idx)
            assert copy.load(idx.export()) == len(distinct)
            assert idx.query_batch(b).tolist() == copy.add_batch(b)[0].tolist() == [1] * len(dig)
            assert len(idx) == len(distinct) and _export_set(idx) == exported == set(distinct)
            gone = distinct[::2]                                                             # every other distinct chunk digest
            info = _prune_and_compare(idx, model, ic.rows(gone), False, dig)
            assert info.n_dropped == len(gone)
            stayed = [0 if k in set(gone) else 1 for k in ic.keys(dig)]
            assert 0 < sum(stayed) < len(dig)
            assert idx.query_batch(b).tolist() == stayed and len(idx) == len(distinct) - len(gone)
            known, n_new, n_known = idx.add_batch(b)
            assert known.tolist() == stayed and n_new == model.add(dig) == len(gone) and n_known == sum(stayed)
            _holds_the_model(idx, model, dig)
            assert _export_set(idx) == set(distinct)


def test_retain_keeps_what_the_set_holds_and_no_list_crosses_the_host():
    rng = np.random.default_rng(1306)
    foreign = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    with M.Engine() as e, M.Engine() as e2:
        b, dig, first = _batch(e)
        universe = np.ascontiguousarray(np.concatenate([dig, foreign]))
        with b, e.zset() as zs, e.index() as idx, e2.index() as other:
            with b.zpack(first) as z:
                zs.add_zpack(z)
            distinct = ic.keys(dig[first])
            model = ic.Index()
            assert idx.add_batch(b)[1] == model.add(dig) == len(distinct)
            assert idx.load(foreign.tobytes()) == model.add(foreign) == 300
            third = distinct[::3]
            assert zs.prune(ic.rows(third), keep=False).n_dropped == len(third)
            in_set = set(ic.keys(zs.entries()[0]))
            assert in_set == set(distinct) - set(third)
            info = idx.retain(zs)
            want = model.retain(in_set)
            assert _counts(info) == want, (_counts(info), want)
            assert (info.n_rows, info.n_unknown, info.n_dropped, info.rebuilt) == (0, 0, 300 + len(third), 1)
            _holds_the_model(idx, model, universe)
            assert _export_set(idx) == in_set and idx.query(foreign).tolist() == [0] * 300
            info = idx.retain(zs)                                                            # a second one drops nothing
            assert _counts(info) == model.retain(in_set) and (info.rebuilt, info.n_dropped, info.n_after) == (0, 0, len(in_set))
            _holds_the_model(idx, model, universe)
            # an index of another ctx than the set's, and a batch of another ctx than the index's
            assert other.load(universe.tobytes()) == len(set(ic.keys(universe)))
            before = _export_set(other)
            pinfo = M.IndexPruneInfo()
            assert e._lib.mi_index_retain_zset(other._h, zs._h, C.byref(pinfo)) == -1 and pinfo.n_before == 0
            assert e._lib.mi_index_query_batch(other._h, b._h, None, 0, None) == -1
            assert len(other) == len(before) and _export_set(other) == before
            # an empty index has nothing to ask the set
            with e.index() as empty:
                info = empty.retain(zs)
                assert _counts(info) == ic.Index().retain(in_set) and len(empty) == 0


# ---- 7. what is refused ------------------------------------------------------------------------------------------------------------------------
def test_what_is_refused_leaves_the_index_as_it_was():
    rng = np.random.default_rng(1307)
    dig = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    with M.Engine() as e:
        idx, model = _fed(e, dig)
        with idx, e.batch() as b:
            L = e._lib
            before = _export_set(idx)
            info, n, held = M.IndexPruneInfo(), C.c_uint64(9), np.zeros(64, dtype=np.uint8)
            for flags in (0, 3, 4, 0x11):                                                    # neither, both, an unknown bit
                assert L.mi_index_prune(idx._h, dig.ctypes.data, 1, flags, C.byref(info)) == -1 and b"exactly one" in L.mi_last_error(e._h)
            assert L.mi_index_prune(idx._h, None, 1, M.INDEX_PRUNE_DROP, C.byref(info)) == -1
            assert L.mi_index_prune(idx._h, dig.ctypes.data, 1 << 32, M.INDEX_PRUNE_KEEP, None) == -1 and b"2^32" in L.mi_last_error(e._h)
            assert L.mi_index_query(idx._h, None, 1, held.ctypes.data, C.byref(n)) == -1 and n.value == 0
            assert L.mi_index_query(idx._h, dig.ctypes.data, 1 << 32, None, None) == -1 and b"2^32" in L.mi_last_error(e._h)
            assert L.mi_index_query(idx._h, None, 0, None, None) == 0                        # n = 0 is fine
            assert L.mi_index_query(idx._h, dig.ctypes.data, 40, None, C.byref(n)) == 0 and n.value == 40      # held may be NULL
            b.add_synthetic([65536] * 2, [1, 2], seed=0x1307)
            assert L.mi_index_query_batch(idx._h, b._h, held.ctypes.data, 64, C.byref(n)) == -6                # it has not run
            b.run()
            n_chunks = b.counts()[1]
            assert 1 < n_chunks <= 64
            assert L.mi_index_query_batch(idx._h, b._h, held.ctypes.data, n_chunks - 1, C.byref(n)) == -7      # one short
            assert L.mi_index_query_batch(idx._h, b._h, held.ctypes.data, n_chunks, C.byref(n)) == 0 and n.value == 0
            assert L.mi_index_query_batch(idx._h, b._h, None, 0, C.byref(n)) == 0                              # no flags wanted: no cap needed
            assert len(idx) == 40 and _export_set(idx) == before
            _holds_the_model(idx, model, dig)


def test_a_set_in_its_failed_state_is_refused_and_the_index_stays():
    import zpack_cases as zc
    import zset_cases as qc
    rng = np.random.default_rng(1308)
    chunks = [rng.integers(0, 256, 50 + i, dtype=np.uint8).tobytes() for i in range(6)]
    _, _, ze, zb = qc.zpack_of(chunks)
    dig = qc.digests_of(chunks)
    with M.Engine() as e, e.zset() as zs:
        idx, model = _fed(e, dig)
        with idx:
            zs.add_zblob(zb, ze)
            liar = ze[:1].copy()
            liar["length"] += 1
            with pytest.raises(M.MiError):
                zs.add_zblob(zb[:zc.round16(int(ze["stored"][0]))], liar)
            with pytest.raises(M.MiError) as ei:
                idx.retain(zs)
            assert ei.value.code == -6 and "unusable since" in str(ei.value)
            _holds_the_model(idx, model, dig)
