"""GPU tests of pruning a compressed pack set in place (mi_zset_prune, mi_zset_get_usage, mi_zset_entries): after every prune
the set is held against the model of zprune_cases.py -- the held set, mi_zset_info, mi_zset_usage and every counter of
mi_prune_info -- and against ITSELF before the call: the cut of a request over the survivors is byte for byte the cut taken
before, the files restored from it are the originals, a dropped digest is one that was never added.  Bit for bit: there are no
tolerances."""
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
import zpack_cases as zc  # noqa: E402
import zprune_cases as pr  # noqa: E402
import zset_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu
ALGS = [pc.SHA256, pc.BLAKE2S]
PAD_RULE = "a pad byte behind the stored span that is not zero"


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


def _holds_the_model(zs, store):
    """info, usage and the entries against the model"""
    want = store.info()
    got = zs.info.as_dict()
    assert {k: got[k] for k in want} == want
    assert zs.usage().as_dict() == store.usage()
    d, ln, st = zs.entries()
    assert {bytes(d[i]): (int(ln[i]), int(st[i])) for i in range(len(d))} == {k: (v[0], v[2]) for k, v in store.held.items()}


def _restores(e, zs, chunks, dig, order, verify):
    with e.batch() as b:
        b.add_zrecipes(zs, [qc.recipe(chunks, order, dig=dig)], verify=verify)
        b.run()
        want = b"".join(chunks[k] for k in order)
        assert b.read_file(0, 0, len(want)) == want


def _prune_and_compare(zs, store, digests, keep, permille):
    before = zs.usage()
    info = zs.prune(digests, keep=keep, min_live_permille=permille)
    want = store.prune(digests, keep=keep, permille=permille)
    assert _counts(info) == want, (_counts(info), want)
    after = zs.usage()
    new_blob = pr.alloc(info.moved_bytes) if info.moved_bytes else 0
    assert after.resident_bytes == before.resident_bytes - info.freed_bytes + new_blob
    assert info.ms_mark > 0 and (info.ms_move > 0) == (info.moved_bytes > 0) and (info.ms_rebuild > 0) == (info.n_dropped > 0)
    _holds_the_model(zs, store)
    return info


# ---- 1. three zpacks, three fates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("permille", [0, 600, 1000])
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("alg", ALGS)
def test_three_zpacks_three_fates(alg, keep, permille):
    a, b, c, stay = pr.three_fates()
    chunks = a + b + c
    dig = qc.digests_of(chunks, alg)
    nb0 = len(a)
    stays = [nb0 + k for k in stay] + list(range(nb0 + len(b), len(chunks)))
    goes = [k for k in range(len(chunks)) if k not in stays]
    stranger = np.frombuffer(zc.sha(b"never held"), dtype=np.uint8).reshape(1, 32)
    named = stays if keep else goes
    request = np.ascontiguousarray(np.concatenate([dig[named], stranger, dig[named[:2]]]))
    survivors = np.ascontiguousarray(dig[stays[::-1] + stays[:3]])
    store = pr.Store()
    with _engine(alg) as e, e.zset() as zs:
        for part in (a, b, c):
            _, _, ze, zb = qc.zpack_of(part, alg)
            zs.add_zblob(zb, ze, verify=True)
            store.add(ze, zb)
        _holds_the_model(zs, store)
        cut_before = _cut(zs, survivors, verify=True)
        live_before = zs.usage().live_bytes
        info = _prune_and_compare(zs, store, request, keep, permille)
        assert (info.n_rows, info.n_unknown, info.n_dropped) == (len(named) + 3, 1, len(goes))
        assert (info.n_blobs_freed, info.n_blobs_compacted) == ((2, 1) if permille else (1, 0))
        assert zs.usage().n_blobs == 2 and zs.usage().live_bytes < live_before
        assert _cut(zs, survivors, verify=True) == cut_before
        held, want_rows, _ = zs.missing(dig)
        assert held.tolist() == store.missing(dig) == [1 if k in stays else 0 for k in range(len(chunks))]
        assert want_rows.tolist() == goes
        _restores(e, zs, chunks, dig, stays + stays[::-1], verify=True)
        # a dropped digest is one that was never added
        assert _raises(-1, lambda: zs.zpack(dig[[stays[0], goes[1]]]), "row 1", "does not hold").first_bad == 1
        with e.batch() as t:
            _raises(-1, lambda: t.add_zrecipes(zs, [qc.recipe(chunks, [stays[0], goes[0]], dig=dig)]), "row 1 ", "does not hold")
        if permille == 1000:
            # the memory claim, from the sizes: the new table + the moved bytes + the call's scratch, below the live bytes that
            # the cut-and-re-add path allocates twice (the zpack's blob and the new set's copy)
            assert info.peak_extra_bytes < 2 * zs.usage().live_bytes


# ---- 2. the first form wins, and stays ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_the_first_form_wins_and_stays(alg):
    rng = np.random.default_rng(202)
    twice = bytes([9]) * 40
    coded = zc.compress_chunk(twice)
    f1, f2 = bytes(zc.filler(rng, 200)), bytes(zc.filler(rng, 300))
    p1 = zc.build_zpack([zc._entry(twice, 40, twice), zc._entry(f1, 200, f1), zc._entry(f2, 300, f2)], alg)
    p2 = zc.build_zpack([zc._entry(coded, 40, twice), zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN)], alg)
    chunks = [twice, f1, f2, zc.GOOD_PLAIN]
    dig = qc.digests_of(chunks, alg)
    store = pr.Store()
    with _engine(alg) as e, e.zset() as zs:
        for z in (p1, p2):
            zs.add_zblob(z[1], z[0])
            store.add(*z)
        _holds_the_model(zs, store)
        cut_before = _cut(zs, dig[[3, 0]])
        # p1 keeps 48 of 560 bytes; p2's coded form of `twice` lost and was never live, so p2 keeps 32 of 48: both are compacted,
        # into ONE new blob
        info = _prune_and_compare(zs, store, dig[[1, 2]], False, 1000)
        assert (info.n_blobs_compacted, info.moved_bytes, info.n_blobs_freed) == (2, 80, 2) and zs.usage().n_blobs == 1
        assert store.held[bytes(dig[0])][2] == 40                               # the raw form, still
        assert _cut(zs, dig[[3, 0]]) == cut_before
        _restores(e, zs, chunks, dig, [0, 3, 0], verify=True)
        info = _prune_and_compare(zs, store, dig[[0]], False, 1000)             # the compaction blob is a blob: compacted in its turn
        assert (info.n_dropped, info.n_blobs_freed, info.freed_bytes, info.moved_bytes) == (1, 1, pr.alloc(80), 32)
        zs.add_zblob(p2[1], p2[0])                                              # the digest comes back in the form this add brings
        store.add(*p2)
        _holds_the_model(zs, store)
        assert store.held[bytes(dig[0])][2] == len(coded) < 40
        _restores(e, zs, chunks, dig, [0, 3], verify=True)


# ---- 3. digests that share their first eight bytes ----------------------------------------------------------------------------------
def test_digests_that_share_their_first_eight_bytes_survive_the_rebuild():
    rng = np.random.default_rng(203)
    lens = [100, 100, 37, 64, 64, 250, 16, 90, 33]                # entries 0..2 share a tag, 3 and 4 share another
    chunks = [zc.text_like(k, i) if k in (250, 90) else rng.integers(0, 256, k, dtype=np.uint8).tobytes() for i, k in enumerate(lens)]
    # verify is off: digests are opaque.  Slot = first 8 bytes (little endian) & 1023: the triple walks to t, t + 1, t + 2, its
    # neighbours are AT HOME in t + 1, t + 2, t + 3; the pair sits in u, u + 1 with a neighbour at home in u + 1
    tag, pair = 0x1122334455667000 | 0x2FF, 0x0807060504030000 | 0x155
    dig = np.zeros((len(lens), 32), dtype=np.uint8)
    for k in range(len(lens)):
        dig[k, 8:] = rng.integers(0, 256, 24, dtype=np.uint8)
    for k, t in enumerate([tag, tag, tag, pair, pair, tag + 1, tag + 2, tag + 3, pair + 1]):
        dig[k, :8] = np.frombuffer(int(t).to_bytes(8, "little"), dtype=np.uint8)
    _, _, ze, zb = qc.zpack_of(chunks, digests=dig)
    assert (ze["stored"] < ze["length"]).sum() == 2
    store = pr.Store()
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze)
        store.add(ze, zb)
        # which of the triple sits in the middle of the chain is the probe's race: drop each of the three in turn from a fresh set
        for gone in (1, 0, 2):
            with e.zset() as zt:
                zt.add_zblob(zb, ze)
                st = pr.Store()
                st.add(ze, zb)
                _prune_and_compare(zt, st, dig[[gone, 3]], False, 1000)
                rest = [k for k in range(len(lens)) if k not in (gone, 3)]
                _restores(e, zt, chunks, dig, rest + rest[::-1], verify=False)
                for k in rest:
                    _restores(e, zt, chunks, dig, [k], verify=False)
                held, _, _ = zt.missing(dig)
                assert held.tolist() == [0 if k in (gone, 3) else 1 for k in range(len(lens))]
                _raises(-1, lambda: zt.zpack(dig[[gone]]), "does not hold")
        _holds_the_model(zs, store)


# ---- 4. scan and tile edges in the move ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_scan_and_tile_edges_in_the_move(n):
    chunks, dig, ze, zb, cand = pr.edge_store()
    stays = cand[:n]
    layout, total = pr.edge_layout(ze, stays)
    store = pr.Store()
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze)
        store.add(ze, zb)
        request = np.ascontiguousarray(dig[stays])
        cut_before = _cut(zs, request)
        info = _prune_and_compare(zs, store, request, True, 1000)
        assert (info.n_blobs_compacted, info.moved_bytes, info.n_dropped, info.n_blobs_freed) == (1, total, len(chunks) - n, 1)
        assert zs.usage().table_slots == (4096 if n <= 2048 else 8192)
        assert _cut(zs, request) == cut_before
        _restores(e, zs, chunks, dig, stays[::-1], verify=False)


# ---- 5. shrink and regrow ---------------------------------------------------------------------------------------------------------------
def test_shrink_and_regrow():
    rng = np.random.default_rng(205)
    pool = rng.integers(0, 256, (3000, 16), dtype=np.uint8)
    chunks = [bytes(x) for x in pool]
    assert len(set(chunks)) == 3000
    _, _, ze, zb = qc.zpack_of(chunks)
    dig = qc.digests_of(chunks)
    keep = list(range(7, 3000, 300))
    assert len(keep) == 10
    store = pr.Store()
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze)
        store.add(ze, zb)
        assert zs.usage().table_slots == 8192
        _prune_and_compare(zs, store, dig[keep], True, 0)
        assert zs.usage().table_slots == 1024 and zs.usage().n_blobs == 1 and zs.info.n_digests == 10
        _restores(e, zs, chunks, dig, keep, verify=True)
        zs.add_zblob(zb, ze)                                                  # the ten are held already: the first form stays where it is
        store.add(ze, zb)
        _holds_the_model(zs, store)
        assert zs.usage().table_slots == 8192 and zs.usage().n_blobs == 2 and zs.info.n_digests == 3000
        _restores(e, zs, chunks, dig, list(range(2999, -1, -1)), verify=True)
        info = _prune_and_compare(zs, store, np.zeros((0, 32), dtype=np.uint8), True, 500)     # KEEP nothing
        assert (info.n_dropped, info.n_blobs_freed, info.moved_bytes) == (3000, 2, 0)
        u = zs.usage()
        assert (u.n_blobs, u.resident_bytes, u.live_bytes, u.table_slots) == (0, 0, 0, 1024) and zs.info.n_digests == 0
        held, _, _ = zs.missing(dig[:5])
        assert held.tolist() == [0] * 5
        zs.add_zblob(zb, ze, verify=True)                                     # and an emptied set is a set
        _restores(e, zs, chunks, dig, [0, 2999], verify=True)


# ---- 6. verbatim pads -------------------------------------------------------------------------------------------------------------------
def test_a_moved_span_keeps_its_pad_and_the_restore_refuses_it_as_before():
    rng = np.random.default_rng(206)
    f1, f2 = bytes(zc.filler(rng, 100)), bytes(zc.filler(rng, 200))
    ze, zb = zc.build_zpack([zc._entry(f1, 100, f1), zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN, pad=0x5A), zc._entry(f2, 200, f2)])
    assert M.zpack_check(zb, ze) == 1
    chunks = [f1, zc.GOOD_PLAIN, f2]
    dig = np.ascontiguousarray(ze["digest"])
    store = pr.Store()
    with M.Engine() as e, e.zset() as zs, e.batch() as b:
        zs.add_zblob(zb, ze)
        store.add(ze, zb)
        said = str(_raises(-1, lambda: b.add_zrecipes(zs, [qc.recipe(chunks, [0, 1], dig=dig)]), "file 0, row 1 ", PAD_RULE))
        info = _prune_and_compare(zs, store, dig[[0]], False, 1000)            # 32 + 208 live of 352: compacted
        assert (info.n_blobs_compacted, info.moved_bytes) == (1, 240)
        assert str(_raises(-1, lambda: b.add_zrecipes(zs, [qc.recipe(chunks, [2, 1], dig=dig)]), "file 0, row 1 ", PAD_RULE)).split("digest")[1] == \
            said.split("digest")[1]
        assert b.counts() == (0, 0, 0)
        _restores(e, zs, chunks, dig, [2, 2], verify=True)                     # its neighbour came along whole
        with zs.zpack(dig[[1, 2]]) as z:                                       # the cut zeroes the pad, as before
            assert M.zpack_check(z.read(), z.entries()) is None


# ---- 7. unknown digests, repeats, nothing to drop, what is refused ---------------------------------------------------------------------------
def test_unknown_digests_repeats_nothing_to_drop_and_what_is_refused():
    rng = np.random.default_rng(207)
    chunks = [zc.text_like(400 + 10 * i, i) if i % 2 else rng.integers(0, 256, 50 + i, dtype=np.uint8).tobytes() for i in range(12)]
    _, _, ze, zb = qc.zpack_of(chunks)
    dig = qc.digests_of(chunks)
    strangers = np.frombuffer(b"".join(zc.sha(b"stranger %d" % i) for i in range(3)), dtype=np.uint8).reshape(-1, 32)
    store = pr.Store()
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze, verify=True)
        store.add(ze, zb)
        L = e._lib
        # nothing to drop, in both modes: every digest kept (with repeats and strangers); only strangers dropped
        everything = np.ascontiguousarray(np.concatenate([dig, strangers, dig[:4], strangers[:1]]))
        cut_before = _cut(zs, dig)
        for request, keep, unknown in ((everything, True, 4), (np.ascontiguousarray(strangers[[0, 1, 1, 2]]), False, 4),
                                       (np.zeros((0, 32), dtype=np.uint8), False, 0)):
            u0 = zs.usage().as_dict()
            info = _prune_and_compare(zs, store, request, keep, 1000)
            assert (info.n_rows, info.n_unknown, info.n_dropped, info.n_blobs_freed, info.moved_bytes) == (len(request), unknown, 0, 0, 0)
            assert zs.usage().as_dict() == u0 and _cut(zs, dig) == cut_before
        # repeats and strangers where something goes, in both modes
        info = _prune_and_compare(zs, store, np.ascontiguousarray(np.concatenate([dig[[3, 3, 5]], strangers[:2], dig[[3]]])), False, 0)
        assert (info.n_rows, info.n_unknown, info.n_dropped) == (6, 2, 2)
        info = _prune_and_compare(zs, store, np.ascontiguousarray(np.concatenate([dig[[3, 0, 1, 1, 2]], strangers, dig[[0]]])), True, 0)
        assert (info.n_rows, info.n_unknown, info.n_dropped, zs.info.n_digests) == (9, 4, 7, 3)        # (3 went before: a stranger now)
        _restores(e, zs, chunks, dig, [2, 1, 0], verify=True)
        # what is refused
        u0, i0 = zs.usage().as_dict(), _counts(zs.info)
        pinfo = M.PruneInfo()
        for flags in (0, 3, 4, 0x11):
            assert L.mi_zset_prune(zs._h, dig.ctypes.data, 1, flags, 0, C.byref(pinfo)) == -1 and b"exactly one" in L.mi_last_error(e._h)
        assert L.mi_zset_prune(zs._h, dig.ctypes.data, 1, M.ZSET_PRUNE_DROP, 1001, C.byref(pinfo)) == -1 and b"1000" in L.mi_last_error(e._h)
        assert L.mi_zset_prune(zs._h, None, 1, M.ZSET_PRUNE_DROP, 0, None) == -1
        assert L.mi_zset_prune(zs._h, dig.ctypes.data, 1 << 32, M.ZSET_PRUNE_DROP, 0, None) == -1 and b"2^32" in L.mi_last_error(e._h)
        n = C.c_uint64()
        assert L.mi_zset_entries(zs._h, None, None, None, 2, C.byref(n)) == -1 and n.value == 3
        assert zs.usage().as_dict() == u0 and _counts(zs.info) == i0
        # the same digest with another length: the set is unusable and says why from the new calls too
        liar = ze[:1].copy()
        liar["length"] += 1
        _raises(-1, lambda: zs.add_zblob(zb[:zc.round16(int(ze["stored"][0]))], liar), "another length")
        for call in (lambda: zs.prune(dig[:1], keep=False), zs.usage, zs.entries):
            _raises(-6, call, "unusable since", "another length")


# ---- 8. what was made before a prune ---------------------------------------------------------------------------------------------------------
def test_a_cut_zpack_and_a_restored_batch_made_before_a_prune_read_the_same_after_it():
    rng = np.random.default_rng(208)
    chunks = [zc.text_like(900 + i, i) if i % 3 else rng.integers(0, 256, 100 + i, dtype=np.uint8).tobytes() for i in range(20)]
    _, _, ze, zb = qc.zpack_of(chunks)
    dig = qc.digests_of(chunks)
    order = [4, 19, 0, 7, 4]
    with M.Engine() as e, e.zset() as zs, e.batch() as b:
        zs.add_zblob(zb, ze, verify=True)
        z = zs.zpack(dig[order], verify=True)
        z_bytes, z_entries = z.read(), z.entries().copy().tobytes()
        b.add_zrecipes(zs, [qc.recipe(chunks, order)], verify=True)
        b.run()
        want = b"".join(chunks[k] for k in order)
        info = zs.prune(dig[[19, 7]], keep=True, min_live_permille=1000)      # 4 and 0 go; 19 and 7 move; the old blob is freed
        assert (info.n_dropped, info.n_blobs_freed, info.n_blobs_compacted) == (18, 1, 1)
        assert z.read() == z_bytes and z.entries().tobytes() == z_entries
        assert b.read_file(0, 0, len(want)) == want
        zs.prune(np.zeros((0, 32), dtype=np.uint8), keep=True)
        assert zs.usage().n_blobs == 0
        assert z.read() == z_bytes and b.read_file(0, 0, len(want)) == want
        with e.zset() as zs2:                                                  # and the zpack still feeds a set
            zs2.add_zpack(z, verify=True)
            assert zs2.info.n_digests == 4
        z.close()


# ---- 9. the bounds, checked by the hardware ------------------------------------------------------------------------------------------------
# The bounds, from the code (csrc/mi_zprune.hip): the move reads aligned 16-byte units inside [src, src + round16(stored)) -- to
# the source blob's last byte when the span ends on its last unit, and not beyond -- and writes the new blob to its last byte.
# Under MI_GUARD_ALLOC=1 every device allocation ends on an unmapped page and a freed one is never mapped again
# (tests/test_gpu_overread.py): a slot that still pointed into a freed blob would fault the cut and the restore that follow.
# No positive control: a deliberate fault has no place on a shared box.
GUARD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import makisu_amd as M
import zpack_cases as zc
import zprune_cases as pr
import zset_cases as qc
rng = np.random.default_rng(209)
for last in (zc.tail_chunk(rng, 6, 1), rng.integers(0, 256, 33, dtype=np.uint8).tobytes()):     # stored = 1 (mod 16): coded, raw
    chunks = [zc.text_like(300, 3), b"\x05", zc.text_like(999, 4), rng.integers(0, 256, 700, dtype=np.uint8).tobytes(), last]
    dig = pr.crafted_digests(len(chunks), rng)              # slot order = entry order: the last entry's span is the last that moves
    _, _, ze, zb = qc.zpack_of(chunks, digests=dig)
    assert int(ze["stored"][-1]) %% 16 == 1 and int(ze["offset"][-1]) + zc.round16(int(ze["stored"][-1])) == len(zb)
    stays = [1, 2, 4]
    layout, total = pr.edge_layout(ze, stays)
    assert layout[-1][0] == 4 and layout[-1][1] + layout[-1][2] == total
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze)
        with zs.zpack(dig[stays]) as z:
            before = (z.read(), z.entries().tobytes())
        info = zs.prune(dig[[0, 3]], keep=False, min_live_permille=1000)
        assert (info.n_dropped, info.n_blobs_compacted, info.moved_bytes, info.n_blobs_freed) == (2, 1, total, 1)
        u = zs.usage()
        assert (u.n_blobs, u.resident_bytes, u.live_bytes) == (1, pr.alloc(total), total)
        with zs.zpack(dig[stays]) as z:
            assert (z.read(), z.entries().tobytes()) == before
        with e.batch() as b:
            b.add_zrecipes(zs, [qc.recipe(chunks, [4, 1, 2, 4], dig=dig)])
            b.run()
            want = last + chunks[1] + chunks[2] + last
            assert b.read_file(0, 0, len(want)) == want
        info = zs.prune(dig[[4]], keep=True, min_live_permille=1000)           # a compaction blob compacted in its turn
        assert (info.n_dropped, info.n_blobs_compacted, info.moved_bytes) == (2, 1, layout[-1][2])
        with e.batch() as b:
            b.add_zrecipes(zs, [qc.recipe(chunks, [4], dig=dig)])
            b.run()
            assert b.read_file(0, 0, len(last)) == last
print("OK")
"""


def test_no_load_or_store_of_the_move_leaves_its_span_and_no_slot_points_into_a_freed_blob(tmp_path):
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", GUARD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout[-1500:] + p.stderr[-3000:]
