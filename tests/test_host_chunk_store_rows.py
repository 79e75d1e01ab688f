"""No GPU: every condition tests/test_gpu_chunk_store_rows.py and tests/test_gpu_chunk_store_rows_batch.py rest on, proven from
the models of store_rows_cases.py alone -- the constants against the sources, the census per form and per plan round, the pairs
(j, WAVE_GRID + j), the tile population, distinct digests, the batch's cut and tails -- the numpy layouts held against the
row-by-row models of the other case files on inputs small enough for those, the two WRONG models (a plan without its carry, a
second trip on a table nobody cleared) shown to differ from the right ones, and the host decoder over all three compressed
models of the million rows."""
import os
import re
import sys
import time

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
import store_rows_cases as sr  # noqa: E402
import zbatch_cases as bc  # noqa: E402
import zentropy_cases as ze  # noqa: E402
import zpack2_cases as z2  # noqa: E402
import zpack_cases as zc  # noqa: E402
import zset_cases as qc  # noqa: E402

CSRC = os.path.join(ROOT, "makisu_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _same(got, want, fields):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]), np.asarray(want[f])) for f in fields)


PLAIN = ("digest", "offset", "chunk_index", "length", "reserved")
CODED = ("digest", "offset", "chunk_index", "length", "stored")


@pytest.fixture(scope="module")
def rows():
    t = time.time()
    r = sr.million_rows()
    print("the model of %d rows, %d of them planted: %.1f s" % (sr.N_ROWS, len(r.planted), time.time() - t))
    for m in sr.MODELS:
        print("  %s: census %r" % (m, r.models[m].census))
    yield r
    sr.clear_caches()


@pytest.fixture(scope="module")
def batch():
    t = time.time()
    b = sr.batch_files()
    stored, coded, needed = sr.batch_stored()
    print("the batch of %d chunks in %d files: %.1f s; %d coded rows, %d random chunks needed the per-chunk model"
          % (b.n, len(b.files), time.time() - t, len(coded), needed))
    yield b
    sr.clear_caches()


# ---- the constants ------------------------------------------------------------------------------------------------------------------------
def test_the_thresholds_are_the_sources():
    plan = _source("mi_plan.h")
    assert re.search(r"kPlanBlock\s*=\s*256\s*;", plan) and re.search(r"kPlanPer\s*=\s*8\s*;", plan)
    assert sr.PLAN_TILE == 256 * 8 and sr.PLAN_ROUND == 256 * sr.PLAN_TILE == 524288
    for name in ("mi_zpack.hip", "mi_zrecode.hip"):
        assert re.search(r"wave_grid\s*\(u64 n\)[^;]*1u\s*<<\s*20", _source(name)), name
    assert sr.WAVE_GRID == 1 << 20 == 2 * sr.PLAN_ROUND and sr.N_ROWS == sr.WAVE_GRID + 300
    blocks = (sr.N_ROWS + sr.PLAN_TILE - 1) // sr.PLAN_TILE
    assert blocks == 513 and [min(256, blocks - b0) for b0 in range(0, blocks, 256)] == [256, 256, 1]           # three rounds
    # a compressed set of N_ROWS digests: SlotTable keeps cap >= 2 * count, a power of two -- 4 194 304 slots, 8 rounds of the
    # plan over slots, and a sweep grid of 2 048 workgroups * 256 threads that goes round 8 times
    cap = 1024
    while cap < 2 * sr.N_ROWS:
        cap *= 2
    assert cap == 4194304 and cap // sr.PLAN_TILE // 256 == 8
    assert [((n + sr.PLAN_TILE - 1) // sr.PLAN_TILE, (n - 1) % sr.PLAN_TILE + 1) for n in sr.EDGE_SIZES] == [(256, 2048), (257, 1), (258, 77)]


# ---- the million rows -----------------------------------------------------------------------------------------------------------------------
def test_the_rows_are_tiny_distinct_and_fill_every_tile(rows):
    r = rows
    assert r.n == len(r.entries) == sr.N_ROWS
    tiny = ~r.is_planted
    assert r.lengths[tiny].min() == 8 and r.lengths[tiny].max() == 12 < zc.MIN_CHUNK and r.lengths[r.planted].min() >= zc.MIN_CHUNK
    assert len(np.unique(r.digests.view("V32"))) == sr.N_ROWS                                # all digests distinct
    keys = np.frombuffer(r.blob, dtype=np.uint8).reshape(-1, 16)[(r.offsets[tiny] // 16).astype(np.int64), :8].copy().view("<u8").reshape(-1)
    assert len(np.unique(keys)) == int(tiny.sum())                                            # ... because the 8 bytes are a bijection
    assert M.pack_check(r.blob, r.entries) is None                                           # grid, zero pads, digests: the host's checker
    # every tile no planted row reaches into (the last apart) holds exactly 1 024 entries, the LDS limit of gather_tile /
    # restore_tile; a planted row lies in every 4 099th row's tile, so some 800 of the 1 100 tiles are such
    for name, offsets, sizes, total in [("plain", r.offsets, r.lengths, len(r.blob))] + \
            [(m, r.models[m].offsets, r.models[m].stored, len(r.models[m].zblob)) for m in sr.MODELS]:
        pop = sr.tile_population(offsets, total)
        lo = offsets[r.planted].astype(np.int64)
        hi = lo + sr.round16(sizes[r.planted].astype(np.int64)) - 1
        assert (hi - lo < sr.GATHER_TILE).all()                      # a planted span reaches into two tiles at the most
        touched = np.zeros(len(pop), dtype=bool)
        touched[lo // sr.GATHER_TILE] = touched[hi // sr.GATHER_TILE] = touched[-1] = True
        pure = np.flatnonzero(~touched)
        assert len(pure) > 700 and (pop[pure] == 1024).all() and pop.max() == 1024, (name, len(pure), pop.max())


def test_the_planted_rows_are_where_the_kernels_turn(rows):
    p = set(rows.planted.tolist())
    want = list(range(300)) + list(range(sr.WAVE_GRID, sr.WAVE_GRID + 300)) + [2046, 2047, 2048, 2049, sr.N_ROWS - 1]
    want += [sr.PLAN_ROUND + d for d in (-2, -1, 0, 1)] + [2 * sr.PLAN_ROUND + d for d in (-2, -1, 0, 1)] + list(range(0, sr.N_ROWS, 4099))
    assert p == set(want) and set(sr.BOUNDARY_ROWS) <= p
    assert len(p) < 1000                                              # the per-chunk models' share of the fixture's time


def test_the_census_per_form_round_and_trip(rows):
    r = rows
    f = r.models["l1h"].forms
    trip2 = f[sr.WAVE_GRID:sr.WAVE_GRID + sr.TRIP]
    assert sorted(set(trip2.tolist())) == [0, 1, 2, 3], np.bincount(trip2, minlength=4)       # all four forms on the second trip
    both_lz4 = [j for j in range(sr.TRIP) if f[j] == 1 and f[sr.WAVE_GRID + j] == 1]
    both_h = [j for j in range(sr.TRIP) if f[j] >= 2 and f[sr.WAVE_GRID + j] >= 2]
    assert len(both_lz4) >= 50 and len(both_h) >= 20, (len(both_lz4), len(both_h))
    per_round = [np.bincount(f[a:a + sr.PLAN_ROUND], minlength=4).tolist() for a in range(0, sr.N_ROWS, sr.PLAN_ROUND)]
    print("forms per plan round (raw, lz4, h over lz4, h over raw):", per_round, "; second trip:", np.bincount(trip2, minlength=4).tolist(),
          "; pairs lz4 %d, h %d" % (len(both_lz4), len(both_h)))
    assert len(per_round) == 3 and [sum(x) for x in per_round] == [sr.PLAN_ROUND, sr.PLAN_ROUND, sr.TRIP]
    assert all(x[2] > 0 and x[3] > 0 and x[1] > 0 for x in per_round), per_round            # form H (and LZ4) in each of the three rounds
    s1, s2 = r.models["l1"].stored, r.models["l2"].stored
    smaller = np.flatnonzero(s2 < s1)
    print("level 2 smaller than level 1 on %d rows, larger on %d; per round %r" % (len(smaller), int((s2 > s1).sum()),
                                                                                     np.bincount(smaller // sr.PLAN_ROUND, minlength=3).tolist()))
    assert len(smaller) >= 50 and (np.bincount(smaller // sr.PLAN_ROUND, minlength=3) > 0).all()
    assert (r.models["l1"].forms < 2).all() and (r.models["l2"].forms < 2).all()
    for m in sr.MODELS:                                               # the census the GPU tests hold mi_zforms against, from the model's own counter
        lo = sr.sliced(r, 2100)
        assert lo.models[m].census == ze.count_forms(lo.models[m].zentries, lo.models[m].zblob), m


def test_the_numpy_layouts_are_the_row_by_row_models_on_a_slice(rows):
    """2 100 rows -- rows 0..299 and 2 046..2 049 planted -- through zpack_cases.pack_of and the three model_compress functions"""
    s = sr.sliced(rows, 2100)
    chunks = [s.chunk(k) for k in range(s.n)]
    entries, blob = zc.pack_of(chunks)
    assert _same(s.entries, entries, PLAIN) and s.blob == blob
    for m, model in (("l1", zc.model_compress), ("l2", z2.model_compress2), ("l1h", lambda e, b: ze.model_compress_h(e, b, 1))):
        want_e, want_b = model(entries, blob)
        assert _same(s.models[m].zentries, want_e, CODED) and s.models[m].zblob == want_b, m
    # the planted rows' forms decode to their chunks by the decoder written from the format
    z = rows.models["l1h"]
    for k in rows.planted[::7].tolist() + [sr.WAVE_GRID + 1, sr.N_ROWS - 1]:
        o = int(z.offsets[k])
        assert ze.expand_chunk(z.zblob[o:o + int(z.stored[k])], int(rows.lengths[k])) == rows.chunk(k), k


def test_the_host_decoder_accepts_all_three_models(rows):
    for m in sr.MODELS:
        z = rows.models[m]
        assert M.zpack_check(z.zblob, z.zentries) is None, m
        assert len(z.zblob) % 16 == 0 and int(z.zentries["stored"].astype(np.uint64).sum()) == sum(c[1] for c in z.census)
    for n in sr.EDGE_SIZES:
        s = sr.sliced(rows, n)
        assert s.n == n == len(s.entries) and M.pack_check(s.blob, s.entries) is None
        assert M.zpack_check(s.models["l1h"].zblob, s.models["l1h"].zentries) is None, n


def test_blake2s_rows_are_the_same_bytes_under_other_digests(rows):
    b = sr.sliced(sr.million_rows(pc.BLAKE2S), sr.EDGE_SIZES[2])
    s = sr.sliced(rows, sr.EDGE_SIZES[2])
    assert b.blob == s.blob and not (b.digests == s.digests).all(axis=1).any()
    assert M.pack_check(b.blob, b.entries, alg=pc.BLAKE2S) is None and M.pack_check(b.blob, b.entries) == 0
    assert M.zpack_check(b.models["l1h"].zblob, b.models["l1h"].zentries, alg=pc.BLAKE2S) is None
    assert b.models["l1h"].zblob == s.models["l1h"].zblob


# ---- the wrong models ---------------------------------------------------------------------------------------------------------------------
def test_a_layout_without_the_carry_differs_at_every_planted_row_behind_the_first_round(rows):
    for sizes in (rows.lengths, rows.models["l1"].stored, rows.models["l1h"].stored):
        right, _ = sr.layout(sizes)
        wrong = sr.layout_without_carry(sizes)
        assert (wrong[:sr.PLAN_ROUND] == right[:sr.PLAN_ROUND]).all() and (wrong[sr.PLAN_ROUND:] != right[sr.PLAN_ROUND:]).all()
        assert wrong[sr.PLAN_ROUND] == 0 and wrong[2 * sr.PLAN_ROUND] == 0
        behind = [k for k in rows.planted.tolist() if k >= sr.PLAN_ROUND]
        assert len(behind) > 400 and all(wrong[k] != right[k] for k in behind)
        assert all((wrong[k] != right[k]) == (k >= sr.PLAN_ROUND) for k in sr.BOUNDARY_ROWS)
    for n in sr.EDGE_SIZES[1:]:                                       # ... and at the edge sizes: the rows of the second round land on row 0's bytes
        assert sr.layout_without_carry(rows.lengths[:n])[sr.PLAN_ROUND] == 0 < sr.layout(rows.lengths[:n])[0][sr.PLAN_ROUND]


def test_a_second_trip_on_a_table_nobody_cleared_codes_other_bytes(rows):
    r = rows
    _, chunks, forms = sr.planted()
    at = {int(k): i for i, k in enumerate(r.planted)}
    f = r.models["l1"].forms
    pairs = [j for j in range(sr.TRIP) if f[j] == 1 and f[sr.WAVE_GRID + j] == 1]
    differ = []
    for j in pairs:
        first, second = chunks[at[j]], chunks[at[sr.WAVE_GRID + j]]
        wrong = sr.second_trip_with_dirty_table(first, second)
        # the wrong form is a sound block of the same chunk (a stale candidate counts only if its 4 bytes are equal): a
        # verify pass that decodes and hashes cannot tell, only the byte compare with the model can
        assert ze.expand_chunk(wrong, len(second)) == second, j
        if wrong != forms["l1"][at[sr.WAVE_GRID + j]]:
            differ.append(j)
    print("a dirty table changes the form of %d of %d second-trip rows" % (len(differ), len(pairs)))
    assert len(differ) >= 1
    # the optional table changes nothing for a caller that does not pass one, and a clean one IS the default
    c = chunks[at[sr.WAVE_GRID]]
    assert zc.parse(c) == zc.parse(c, np.zeros(zc.TABLE, dtype=np.int64))


# ---- requests, cuts ----------------------------------------------------------------------------------------------------------------------------
def test_first_occurrences_and_gather_are_fetch_cases_rules(rows):
    s = sr.sliced(rows, 700)
    rng = np.random.default_rng(5)
    ids = rng.integers(0, s.n, 1500)
    store = {bytes(s.digests[k]): s.chunk(k) for k in range(s.n)}
    want_e, want_b = fc.model_subpack(store, s.digests[ids], alg=pc.SHA256)
    first = sr.first_occurrences(ids)
    off, blob = sr.gather(s.blob, s.offsets, s.lengths, ids[first])
    assert blob == want_b and np.array_equal(first, want_e["chunk_index"]) and np.array_equal(off, want_e["offset"])
    # ... and the compressed cut: zset_cases.model_cut over the level-1 model
    z = s.models["l1"]
    cut_e, cut_b = qc.model_cut([(z.zentries, z.zblob)], s.digests[ids])
    zoff, zblob = sr.gather(z.zblob, z.offsets, z.stored, ids[first])
    assert zblob == cut_b and np.array_equal(zoff, cut_e["offset"]) and np.array_equal(z.stored[ids[first]], cut_e["stored"])
    held = sr.pseudo_random_half(s.n)
    h, want_rows, info = fc.model_missing({bytes(s.digests[k]): s.chunk(k) for k in np.flatnonzero(held)}, s.digests[ids], s.lens32[ids])
    assert np.array_equal(want_rows, first[~held[ids[first]]]) and info["want_bytes"] == int(s.lens32[ids[first]][~held[ids[first]]].sum())


@pytest.mark.parametrize("permille", [0, 600])
def test_the_prune_and_recode_models_are_zprune_cases_and_zrecode_cases_on_a_slice(rows, permille):
    import zprune_cases as pr
    import zrecode_cases as zrc
    import zrecode_h_cases as zh
    s = sr.sliced(rows, 3000)
    z = s.models["l1h"]
    kept = sr.pseudo_random_half(s.n, 11)
    request = np.concatenate([s.digests[kept], s.digests[kept][:5], np.full((3, 32), 0xEE, dtype=np.uint8)])
    for second in (False, True):                                      # the first prune, and the identical one behind it
        store = pr.Store()
        store.add(z.zentries, z.zblob)
        held = np.ones(s.n, dtype=bool)
        blob_bytes, cap, table = len(z.zblob), 8192, None
        if second:
            first = store.prune(request, keep=True, permille=permille)
            held, blob_bytes, cap, table = kept, first["moved_bytes"] or blob_bytes, 4096, store.usage()["table_bytes"]
        want = store.prune(request, keep=True, permille=permille)
        info, usage = sr.model_prune(z.stored[held], s.lengths[held], kept[held], len(request), 3, cap, blob_bytes, permille, table)
        assert info == want and usage == store.usage(), (second, info, want, usage, store.usage())
    # the recodes: every digest's size afterwards is min(level 1, level 2), and level 1 with the stage is the l1h model itself
    a, b, h = s.models["l1"], s.models["l2"], s.models["l1h"]
    store = zrc.Store()
    store.add(a.zentries, a.zblob)
    info = store.recode(2)
    assert info["n_recoded"] == int((b.stored < a.stored).sum()) > 0 and info["stored_after"] == int(np.minimum(a.stored, b.stored).sum())
    want_e, want_b = store.cut(s.digests)
    got_e, got_b = sr.zpack_of_rows(s, np.minimum(a.stored, b.stored), [a, b], (b.stored < a.stored).astype(np.int64))
    assert _same(got_e, want_e, CODED) and got_b == want_b
    forms, replaced, bad = zh.recode_forms(zh.forms_of(a.zentries, a.zblob), s.lengths.tolist(), 1, True)
    assert (replaced, bad) == (int((h.stored < a.stored).sum()), 0) and forms == zh.forms_of(h.zentries, h.zblob)


def test_crafted_digests_put_every_row_at_home_in_row_order(rows):
    """what the recodes in row order rest on: csrc/mi_slot_table.h probes from tag & (cap - 1), tag = the first 8 bytes"""
    assert re.search(r"slot\s*=\s*tag\s*&\s*mask", _source("mi_slot_table.h"))
    dig = sr.crafted_digests(sr.N_ROWS)
    tags = dig[:, :8].copy().view("<u8").reshape(-1)
    home = tags & np.uint64(4194304 - 1)
    assert (tags != 0).all() and np.array_equal(home, np.arange(1, sr.N_ROWS + 1, dtype=np.uint64))      # distinct, ascending: no collision
    # ... so list row k is row k, and the recode's waves meet these pairs of coded rows on their two trips
    f1, fh = rows.models["l1"].forms, rows.models["l1h"].forms
    assert sum(1 for j in range(sr.TRIP) if f1[j] == 1 and f1[sr.WAVE_GRID + j] == 1) >= 50
    assert sum(1 for j in range(sr.TRIP) if fh[j] >= 2 and fh[sr.WAVE_GRID + j] >= 2) >= 20
    # under the chunks' own digests the rows behind 2^20 are whatever hashes there (probing apart, which moves a row by a few
    # slots): a handful of planted rows at the most, and no pairs
    order = np.argsort(rows.digests[:, :8].copy().view("<u8").reshape(-1) & np.uint64(4194304 - 1), kind="stable")
    there = int(rows.is_planted[order[sr.WAVE_GRID - 8:]].sum())
    print("planted rows among the last 308 list rows under the chunks' own digests: %d" % there)
    assert there < 20


def test_the_permuted_request_has_its_repeats_and_strangers(rows):
    ids, digests, lengths = sr.permuted_request(rows)
    assert len(ids) == sr.N_ROWS + 2000 and (ids >= sr.N_ROWS).sum() == 1000
    assert len(np.unique(ids[ids < sr.N_ROWS])) == sr.N_ROWS
    assert len(np.unique(np.concatenate([rows.digests, digests[ids >= sr.N_ROWS]]).view("V32"))) == sr.N_ROWS + 1000    # nobody holds a stranger
    first = sr.first_occurrences(ids)
    assert len(first) == sr.N_ROWS + 1000 and (lengths > 0).all()
    half = sr.pseudo_random_half(sr.N_ROWS)
    for a in range(0, sr.N_ROWS, sr.PLAN_ROUND):                      # both kinds in every round, among the planted rows too
        assert 0 < half[a:a + sr.PLAN_ROUND].sum() < len(half[a:a + sr.PLAN_ROUND])
    assert 100 < half[rows.planted].sum() < len(rows.planted) - 100


# ---- the run batch -------------------------------------------------------------------------------------------------------------------------------
def test_the_batch_is_cut_at_64_with_tails_on_both_sides(batch):
    b = batch
    cut = sr.python_cut(b.files)
    assert len(cut) == b.n == sr.PLAN_ROUND + 2048 + 77 == 526413
    assert [c[0] for c in cut] == b.file.tolist() and [c[1] for c in cut] == b.offset.tolist() and [c[2] for c in cut] == b.length.tolist()
    assert b"".join(b.files) == b.data.tobytes() and 33_600_000 < len(b.data) < 33_800_000
    tails = b.tails
    assert len(tails) >= 1000 and all(len(x) % 64 != 0 for x in b.files[:len(tails)])
    assert set((b.length[tails] % 16).tolist()) == set(range(16)) and b.length[tails].min() == 1 and b.length[tails].max() == 63
    assert (tails < sr.PLAN_ROUND).sum() >= 1000 and (tails > sr.PLAN_ROUND).sum() >= 10
    for n in sr.BATCH_SIZES[1:]:
        assert sr.batch_files(n).n == n == len(sr.python_cut(sr.batch_files(n).files))


def test_every_batch_row_has_a_stored_form_proven_or_modelled(batch):
    b = batch
    stored, coded, needed = sr.batch_stored()
    dig = sr.batch_digests()
    assert len(np.unique(dig.view("V32"))) == b.n                    # all chunks distinct
    assert abs(len(b.compressible) - b.n / sr.ONE_IN) < 10 and set(b.compressible.tolist()) <= set(coded)
    assert all(len(coded[k]) < 64 - 4 for k in b.compressible.tolist())                       # the level-1 model codes every planted chunk
    print("random chunks that needed the per-chunk model: %d of %d; coded rows %d (%d of them tails)"
          % (needed, b.n, len(coded), len(set(coded) & set(b.tails.tolist()))))
    assert needed < 100                                               # (a condition on the cost; every such row IS modelled)
    # the proof, held against the per-chunk model on 300 proven rows and on every row the proof has to refuse
    rng = np.random.default_rng(9)
    for k in rng.choice(b.n, 300, replace=False).tolist():
        c = b.data[int(b.at[k]):int(b.at[k]) + int(b.length[k])].tobytes()
        assert len(zc.compress_chunk(c)) == int(stored[k]), k
    rep = bytearray(b.data[:64].tobytes())
    rep[40:44] = rep[10:14]
    assert not sr.no_quad_repeats(np.frombuffer(bytes(rep), dtype=np.uint8), np.array([0]))[0]
    e, blob = sr.model_batch_pack(b)
    assert M.pack_check(blob, e) is None
    ze1, zb1 = sr.model_batch_zpack(b)
    assert M.zpack_check(zb1, ze1) is None and int((ze1["stored"] < ze1["length"]).sum()) == len(coded)
    sel = sr.selections(b.n)
    assert sorted(sel) == ["all", "from the second round on", "half", "the first round"]
    assert int(sel["from the second round on"].sum()) == 2048 + 77 and int(sel["the first round"].sum()) == sr.PLAN_ROUND
    assert 0 < sel["half"][sr.PLAN_ROUND:].sum() < 2048 + 77


def test_the_batch_models_are_pack_cases_and_zbatch_cases_on_a_small_batch():
    b = sr.batch_files(1300)
    assert len(b.files) == 13 and len(b.tails) == 12
    rows = sr.python_cut(b.files)
    half = sr.pseudo_random_half(b.n, 3)
    for select in (None, half):
        want_e, want_b = pc.model_pack(rows, b.files, None if select is None else select.tolist())
        got_e, got_b = sr.model_batch_pack(b, select)
        assert _same(got_e, want_e, PLAIN) and got_b == want_b
        zwant_e, zwant_b = bc.model_zpack(rows, b.files, None if select is None else select.tolist())
        zgot_e, zgot_b = sr.model_batch_zpack(b, select)
        assert _same(zgot_e, zwant_e, CODED) and zgot_b == zwant_b
        z2want_e, z2want_b = z2.model_compress2(want_e, want_b)
        z2got_e, z2got_b = sr.model_batch_zpack(b, select, 2)
        assert _same(z2got_e, z2want_e, CODED) and z2got_b == z2want_b
    assert np.array_equal(rc.recipe_of(rows, b.files, 0)[0], sr.batch_digests(1300)[b.file == 0])
