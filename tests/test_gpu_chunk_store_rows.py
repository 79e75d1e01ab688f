"""GPU tests of the chunk store beyond the sizes every other test stays under: 1 048 876 hand-laid rows
(store_rows_cases.million_rows, whose conditions tests/test_host_chunk_store_rows.py proves from the models alone) through the
plain set, the coders, the decoders, the compressed set, the prune, the recode and the restore.

  * more than 524 288 rows (slots, for the prune and the recode): plan_block_offsets runs a second and a third round and its
    carry decides where every row behind the first round lies; slot_table_probe_kernel's grid of 2 048 * 256 threads and
    zprune_sweep_kernel's 2 048 workgroups go round.  The edge sizes 524 288, 524 289 and 526 413 give no second round, one
    of one block holding one row, and one with a partial last block;
  * more than 2^20 rows: the waves of zpack_encode_kernel (both levels), zh_encode_kernel and zpack_decode_kernel go round, and
    300 of them code or decode a second row over the match table, the counts and the decode table their first row left in LDS.
    The recode's rows are the table's slots in slot order (zrecode_list_kernel), so in a set under the chunks' own digests
    the rows behind 2^20 are whichever digests hash there -- tiny raw rows, almost surely -- and the second trip of
    zrecode_decode_kernel, zrecode_encode_l1 / _l2_kernel and zh_recode_encode_kernel is index arithmetic only.  The recodes
    therefore run a second time over a set under CRAFTED digests (tag k + 1 for row k: every entry at home in slot k + 1,
    slot order = row order), where list rows j and 2^20 + j ARE the planted pairs: those four kernels then decode and code a
    second LZ4 or form H row over what the first left.

NOT reached, and out of reach of this design: the second trip of zrecode_stage_kernel, zrecode_redecode_kernel and the
recheck's unwrap, whose grids are wave_grid(the REPLACED rows) -- 141 and 333 here; tiny rows are never replaced, so it takes
more than 2^20 rows of 13 bytes and more -- and blob offsets beyond 2^32 bytes with this many rows.

Every comparison is bit for bit with the models of store_rows_cases.py: there are no tolerances, and no row is exempt."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import pack_cases as pc  # noqa: E402
import store_rows_cases as sr  # noqa: E402
import zentropy_cases as ze  # noqa: E402
import zpack_cases as zc  # noqa: E402
import zprune_cases as pr  # noqa: E402

pytestmark = pytest.mark.gpu

PLAIN = ("digest", "offset", "chunk_index", "length", "reserved")
CODED = ("digest", "offset", "chunk_index", "length", "stored")
RULE_WORDS = {1: "a match offset of 0", 11: "an entropy form with a stream that ends early"}
FLAGS = {"l1": (1, False), "l2": (2, False), "l1h": (1, True)}     # model -> (level, entropy)
SIZES = sr.EDGE_SIZES + (sr.N_ROWS,)


def _engine(alg=pc.SHA256, **kw):
    return M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0, **kw)


def _same(got, want, fields):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]), np.asarray(want[f])) for f in fields)


def _bad_rows(got, want, fields):
    """the first rows that differ from the model, with the plan round they lie in"""
    if len(got) != len(want):
        return "%d entries, the model has %d" % (len(got), len(want))
    bad = np.zeros(len(got), dtype=bool)
    for f in fields:
        d = np.asarray(got[f]) != np.asarray(want[f])
        bad |= d.any(axis=1) if d.ndim > 1 else d
    return [(int(k), int(k) // sr.PLAN_ROUND, int(got["offset"][k]), int(want["offset"][k])) for k in np.flatnonzero(bad)[:8]]


def _first_difference(got, want):
    if len(got) != len(want):
        return "lengths %d and %d" % (len(got), len(want))
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    return int(np.flatnonzero(a != b)[0]) if (a != b).any() else None


def _raises(code, call, *needles):
    with pytest.raises(M.MiError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)
    return ei.value


def _counts(info):
    return {k: v for k, v in info.as_dict().items() if not k.startswith("ms_")}


def _forms(f):
    return [[int(f.n[i]), int(f.stored[i])] for i in range(4)]


def _pack_of_rows(engine, r):
    """the rows as a Pack on the device: through a plain set, both steps verified"""
    with engine.packset() as s:
        s.add_blob(r.blob, r.entries, verify=True)
        return s.pack(r.digests, r.lens32, verify=True)


def _zpack_of_rows(engine, r, m, verify=False):
    level, entropy = FLAGS[m]
    with _pack_of_rows(engine, r) as p:
        return p.compress(verify=verify, level=level, entropy=entropy)


def _is_the_model(z, model, name=""):
    got_e, got_b = z.entries().copy(), z.read()
    assert _same(got_e, model.zentries, CODED), (name, _bad_rows(got_e, model.zentries, CODED))
    assert got_b == model.zblob, (name, _first_difference(got_b, model.zblob))
    return got_e, got_b


def _sorted_by_digest(d, *more):
    order = np.argsort(np.ascontiguousarray(d).view("V32").reshape(-1), kind="stable")
    return (np.ascontiguousarray(d)[order],) + tuple(np.asarray(x)[order] for x in more)


@pytest.fixture(scope="module")
def rows():
    t = time.time()
    r = sr.million_rows()
    print("the model of %d rows: %.1f s; census with the stage %r" % (sr.N_ROWS, time.time() - t, r.models["l1h"].census))
    yield r
    sr.clear_caches()


# ---- a. the plain set -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_a_plain_set_takes_the_rows_and_packs_them_back(rows, n):
    """mi_packset_add_blob and mi_packset_pack, both verified: the table's insert and probe, the fetch's plan and gather"""
    r = sr.sliced(rows, n)
    with M.Engine() as e, _pack_of_rows(e, r) as p:
        got_e = p.entries().copy()
        assert _same(got_e, r.entries, PLAIN), _bad_rows(got_e, r.entries, PLAIN)
        got = p.bytes()
        assert got == r.blob, _first_difference(got, r.blob)
        assert (p.info.n_entries, p.info.blob_bytes, p.info.chunk_bytes) == (n, len(r.blob), int(r.lengths.astype(np.uint64).sum()))


def test_a_permuted_request_with_repeats_is_packed_in_order_of_first_occurrence(rows):
    r = rows
    ids, digests, lengths = sr.permuted_request(r)
    first = sr.first_occurrences(ids)
    strangers = first[ids[first] >= r.n]
    with M.Engine() as e, e.packset() as s:
        s.add_blob(r.blob, r.entries, verify=True)
        held, want_rows, info = s.missing(digests, lengths)
        assert np.array_equal(held, (ids < r.n).astype(np.uint8)) and np.array_equal(want_rows, strangers.astype(np.uint64))
        assert (info.n_rows, info.n_distinct, info.n_held, info.n_want) == (len(ids), r.n + 1000, r.n, 1000)
        assert (info.held_bytes, info.want_bytes) == (int(r.lengths.astype(np.uint64).sum()), 77 * 1000)
        err = _raises(-1, lambda: s.pack(digests, lengths), "row %d:" % strangers[0], "does not hold")       # the smallest row nobody holds
        assert err.first_bad == strangers[0]
        known = ids < r.n
        ids, digests, lengths = ids[known], np.ascontiguousarray(digests[known]), lengths[known]
        first = sr.first_occurrences(ids)
        assert len(first) == r.n and len(ids) > r.n + 900             # (a repeat of a row is a second occurrence)
        off, blob = sr.gather(r.blob, r.offsets, r.lengths, ids[first])
        want = sr.entries_of(pc.ENTRY_DTYPE, r.digests[ids[first]], off, first, r.lengths[ids[first]])
        with s.pack(digests, lengths, verify=True) as p:
            got_e = p.entries().copy()
            assert _same(got_e, want, PLAIN), _bad_rows(got_e, want, PLAIN)
            got = p.bytes()
            assert got == blob, _first_difference(got, blob)


def _half_is_missing(r, make_set, add):
    """a set that holds a pseudo-random half, asked for every row: the want rows are the other half, ascending"""
    half = sr.pseudo_random_half(r.n)
    rows_held = np.flatnonzero(half)
    with M.Engine() as e, make_set(e) as s:
        add(s, rows_held)
        held, want_rows, info = s.missing(r.digests, r.lens32)
        assert np.array_equal(held, half.astype(np.uint8))
        assert np.array_equal(want_rows, np.flatnonzero(~half).astype(np.uint64))
        assert (info.n_rows, info.n_distinct, info.n_held, info.n_want) == (r.n, r.n, len(rows_held), r.n - len(rows_held))
        assert (info.held_bytes, info.want_bytes) == (int(r.lengths[half].astype(np.uint64).sum()), int(r.lengths[~half].astype(np.uint64).sum()))


@pytest.mark.parametrize("n", [sr.PLAN_ROUND + 1, sr.N_ROWS])
def test_a_plain_set_that_holds_half_wants_the_other_half(rows, n):
    r = sr.sliced(rows, n)

    def add(s, held):
        off, blob = sr.gather(r.blob, r.offsets, r.lengths, held)
        s.add_blob(blob, sr.entries_of(pc.ENTRY_DTYPE, r.digests[held], off, np.arange(len(held)), r.lengths[held]), verify=True)
    _half_is_missing(r, lambda e: e.packset(), add)


# ---- b. the coders --------------------------------------------------------------------------------------------------------------------------
def _coded_to_the_model(r, m, verify, alg=pc.SHA256):
    level, entropy = FLAGS[m]
    z_model = r.models[m]
    with _engine(alg) as e, _pack_of_rows(e, r) as p:
        with p.compress(verify=verify, level=level, entropy=entropy) as z:
            got_e, got_b = _is_the_model(z, z_model, m)
            info = z.info
            assert (info.n_entries, info.blob_bytes, info.stored_bytes, info.n_raw, info.verified) == \
                (r.n, len(z_model.zblob), int(z_model.stored.astype(np.uint64).sum()), z_model.census[0][0], int(verify))
            assert _forms(z.count_forms()) == z_model.census
        assert M.zpack_check(got_b, got_e, alg=alg) is None
        assert p.bytes() == r.blob                                    # the input is unchanged


@pytest.mark.parametrize("m,verify", [("l1", False), ("l1", True), ("l2", False), ("l1h", True)])
def test_the_rows_are_coded_to_the_models_bytes(rows, m, verify):
    """mi_pack_compress: zpack_encode_kernel (level 1), the level-2 encoder and zh_encode_kernel on their second trip; with
    VERIFY zpack_decode_kernel (and the unwrap) on theirs; the layout's plan in three rounds"""
    _coded_to_the_model(rows, m, verify)


# ---- c. the decoders ------------------------------------------------------------------------------------------------------------------------
def _decoded_to_the_rows(r, m, alg=pc.SHA256):
    with _engine(alg) as e, _zpack_of_rows(e, r, m) as z, e.packset() as s:
        s.add_zpack(z, verify=True)
        assert s.info.n_digests == r.n
        with s.pack(r.digests, r.lens32, verify=True) as back:
            got = back.bytes()
            assert got == r.blob, (m, _first_difference(got, r.blob))


@pytest.mark.parametrize("m", ["l1", "l1h"])
def test_the_zpacks_decode_into_a_plain_set_byte_for_byte(rows, m):
    _decoded_to_the_rows(rows, m)


def _second_trip_rows(r, form):
    """the rows WAVE_GRID + j whose row j has the same form with the stage"""
    f = r.models["l1h"].forms
    return [sr.WAVE_GRID + j for j in range(sr.TRIP) if f[j] == form and f[sr.WAVE_GRID + j] == form]


def _damaged(r, how, among):
    """the stage's zblob with ONE row damaged where it lies, sizes unchanged -> (zblob, the row, the rule): "lz4": the first
    match's offset of the first LZ4 row of `among(form)` made 0 (zpack_cases' "offset 0"); "h": a pad bit of stream 0 of the
    first form H row that has one set (zentropy_cases' "a pad bit is set")"""
    z = r.models["l1h"]
    blob = bytearray(z.zblob)

    def form_at(k):
        return z.zblob[int(z.offsets[k]):int(z.offsets[k]) + int(z.stored[k])]
    if how == "lz4":
        k = among(1)[0]
        lit = zc.parse(r.chunk(k))[0][0]
        at = 1 + (len(zc._lengths(lit)) if lit >= 15 else 0) + lit    # behind the token, its extension bytes and the literals
        assert form_at(k)[at:at + 2] != b"\0\0"
        new = form_at(k)[:at] + b"\0\0" + form_at(k)[at + 2:]
        rule = 1
    else:
        k = next(k for k in among(2) if ze._pad_bits(form_at(k)) > 0)
        new = ze._hurt_stream(form_at(k), "pad")
        rule = ze.RULE_BITS
    assert len(new) == int(z.stored[k]) and ze.chunk_rule(new, int(r.lengths[k]))[0] == rule
    blob[int(z.offsets[k]):int(z.offsets[k]) + len(new)] = new
    return bytes(blob), k, rule


def _every_reader_names(r, blob, bad, rule, alg=pc.SHA256):
    z = r.models["l1h"]
    assert M.zpack_check(blob, z.zentries, alg=alg) == bad
    with _engine(alg) as e, e.packset() as ps, e.zset() as zs:
        before = _counts(ps.info)
        err = _raises(-1, lambda: ps.add_zblob(blob, z.zentries, verify=True), "entry %d " % bad, "does not decode: ", RULE_WORDS[rule])
        assert err.first_bad == bad and _counts(ps.info) == before and ps.info.n_digests == 0
        before = _counts(zs.info)
        err = _raises(-1, lambda: zs.add_zblob(blob, z.zentries, verify=True), "entry %d " % bad, RULE_WORDS[rule])
        assert err.first_bad == bad and _counts(zs.info) == before
        ps.add_zblob(z.zblob, z.zentries, verify=True)                # ... and the sound blob is taken by the same set
        assert ps.info.n_digests == r.n


@pytest.mark.parametrize("how", ["lz4", "h"])
def test_a_damaged_row_on_the_second_trip_is_the_row_every_reader_names(rows, how):
    """row 2^20 + j damaged where row j is sound and of the same form: the wave refuses its second row, not its first"""
    blob, bad, rule = _damaged(rows, how, lambda form: _second_trip_rows(rows, form))
    assert bad >= sr.WAVE_GRID
    _every_reader_names(rows, blob, bad, rule)


# ---- d. the compressed set --------------------------------------------------------------------------------------------------------------------
def test_a_compressed_set_holds_cuts_and_counts_the_rows(rows):
    r = rows
    z_model = r.models["l1h"]
    ids, digests, lengths = sr.permuted_request(r)
    known = ids < r.n
    ids, digests, lengths = ids[known], np.ascontiguousarray(digests[known]), lengths[known]
    first = sr.first_occurrences(ids)
    with M.Engine() as e, e.zset() as zs:
        with _zpack_of_rows(e, r, "l1h") as z:
            zs.add_zpack(z, verify=True)
        assert zs.info.n_digests == r.n and zs.usage().table_slots == 4194304
        assert _forms(zs.count_forms()) == z_model.census           # zh_classify_kernel over 4 194 304 slots
        with zs.zpack(r.digests, r.lens32, verify=True) as cut:       # the cut of everything IS the zpack
            _is_the_model(cut, z_model, "the cut of every row")
        off, blob = sr.gather(z_model.zblob, z_model.offsets, z_model.stored, ids[first])
        want = sr.entries_of(zc.ZENTRY_DTYPE, r.digests[ids[first]], off, first, r.lengths[ids[first]], z_model.stored[ids[first]])
        with zs.zpack(digests, lengths, verify=True) as cut:
            got_e, got_b = cut.entries().copy(), cut.read()
            assert _same(got_e, want, CODED), _bad_rows(got_e, want, CODED)
            assert got_b == blob, _first_difference(got_b, blob)
        d, ln, st = zs.entries()
        assert all(np.array_equal(a, b) for a, b in zip(_sorted_by_digest(d, ln, st), _sorted_by_digest(r.digests, r.lengths, z_model.stored)))


@pytest.mark.parametrize("n", [sr.PLAN_ROUND + 1, sr.N_ROWS])
def test_a_compressed_set_that_holds_half_wants_the_other_half(rows, n):
    r = sr.sliced(rows, n)
    z = r.models["l1h"]

    def add(s, held):
        off, blob = sr.gather(z.zblob, z.offsets, z.stored, held)
        s.add_zblob(blob, sr.entries_of(zc.ZENTRY_DTYPE, r.digests[held], off, np.arange(len(held)), r.lengths[held], z.stored[held]), verify=True)
    _half_is_missing(r, lambda e: e.zset(), add)


# ---- e. the prune -----------------------------------------------------------------------------------------------------------------------------
def test_a_prune_to_half_compacts_the_blob_and_keeps_every_kept_byte(rows):
    """mi_zset_prune(KEEP, 600 permille) over 4 194 304 slots: zprune_sweep_kernel's 2 048 workgroups go round 8 times,
    zprune_block_offsets_kernel runs 8 rounds, and a blob with half its bytes live is compacted"""
    r = rows
    z = r.models["l1h"]
    kept = sr.pseudo_random_half(r.n, 1604)
    request = np.ascontiguousarray(r.digests[kept])
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(z.zblob, z.zentries, verify=True)
        cap = zs.usage().table_slots
        with zs.zpack(request, verify=True) as cut:
            before = (cut.entries().copy().tobytes(), cut.read())
        info = zs.prune(request, keep=True, min_live_permille=600)
        want, usage = sr.model_prune(z.stored, r.lengths, kept, len(request), 0, cap, len(z.zblob), 600)
        assert _counts(info) == want, (_counts(info), want)
        assert info.n_blobs_compacted == 1 and info.moved_bytes == int(sr.round16(z.stored[kept].astype(np.int64)).sum())
        assert zs.usage().as_dict() == usage, (zs.usage().as_dict(), usage)
        held, want_rows, _ = zs.missing(r.digests, r.lens32)         # every dropped digest is missing
        assert np.array_equal(held, kept.astype(np.uint8)) and np.array_equal(want_rows, np.flatnonzero(~kept).astype(np.uint64))
        with zs.zpack(request, verify=True) as cut:
            assert (cut.entries().copy().tobytes(), cut.read()) == before
        assert _forms(zs.count_forms()) == sr.census(z.forms[kept], z.stored[kept])
        again = zs.prune(request, keep=True, min_live_permille=600)   # the same prune once more changes nothing
        want2, usage2 = sr.model_prune(z.stored[kept], r.lengths[kept], np.ones(int(kept.sum()), dtype=bool), len(request), 0, usage["table_slots"],
                                       want["moved_bytes"], 600, usage["table_bytes"])
        assert _counts(again) == want2 and again.n_dropped == 0 and zs.usage().as_dict() == usage2 == usage
        with zs.zpack(request, verify=True) as cut:
            assert (cut.entries().copy().tobytes(), cut.read()) == before
        d, ln, st = zs.entries()
        assert all(np.array_equal(a, b) for a, b in zip(_sorted_by_digest(d, ln, st), _sorted_by_digest(request, r.lengths[kept], z.stored[kept])))


# ---- f. the recode ----------------------------------------------------------------------------------------------------------------------------
def _decodes_to_the_rows(e, r, cut, digests, verify):
    with e.packset() as s:
        s.add_zpack(cut, verify=verify)
        with s.pack(digests, r.lens32, verify=verify) as back:
            got = back.bytes()
            assert got == r.blob, _first_difference(got, r.blob)


def _under(zentries, digests):
    out = zentries.copy()
    out["digest"] = digests
    return out


def _recoded_at_level_2(r, digests, verify):
    a, b = r.models["l1"], r.models["l2"]
    smaller = b.stored < a.stored
    stored = np.minimum(a.stored, b.stored)
    want_e, want_b = sr.zpack_of_rows(r, stored, [a, b], smaller.astype(np.int64))
    want_e = _under(want_e, digests)
    print("level 2 replaces %d forms, per plan round %r" % (int(smaller.sum()), np.bincount(np.flatnonzero(smaller) // sr.PLAN_ROUND, minlength=3).tolist()))
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(a.zblob, _under(a.zentries, digests), verify=verify)
        assert zs.usage().table_slots == 4194304
        info = zs.recode(level=2, verify=verify)
        assert (info.n_digests, info.n_recoded, info.n_undecodable, info.n_rounds) == (r.n, int(smaller.sum()), 0, 1)
        assert (info.stored_before, info.stored_after) == (int(a.stored.astype(np.uint64).sum()), int(stored.astype(np.uint64).sum()))
        assert info.n_raw_recoded == int((smaller & (a.stored == r.lengths)).sum()) and info.new_blob_bytes == len(want_b)
        d, ln, st = zs.entries()
        assert all(np.array_equal(x, y) for x, y in zip(_sorted_by_digest(d, ln, st), _sorted_by_digest(digests, r.lengths, stored)))
        usage = zs.usage().as_dict()
        again = zs.recode(level=2, verify=verify)                     # nothing is smaller now: nothing replaced, nothing moved
        assert (again.n_recoded, again.n_undecodable, again.n_blobs_rewritten, again.new_blob_bytes, again.stored_after) == \
            (0, 0, 0, 0, info.stored_after)
        assert zs.usage().as_dict() == usage
        with zs.zpack(digests, r.lens32, verify=verify) as cut:
            got_e, got_b = cut.entries().copy(), cut.read()
            assert _same(got_e, want_e, CODED), _bad_rows(got_e, want_e, CODED)
            assert got_b == want_b, _first_difference(got_b, want_b)
            _decodes_to_the_rows(e, r, cut, digests, verify)


def _recoded_with_the_stage(r, digests, verify):
    a, h = r.models["l1"], r.models["l1h"]
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(a.zblob, _under(a.zentries, digests), verify=verify)
        info = zs.recode(level=1, verify=verify, entropy=True)
        assert (info.n_digests, info.n_recoded, info.n_undecodable, info.n_rounds) == (r.n, int((h.stored < a.stored).sum()), 0, 1)
        assert (info.stored_before, info.stored_after) == (int(a.stored.astype(np.uint64).sum()), int(h.stored.astype(np.uint64).sum()))
        assert _forms(zs.count_forms()) == h.census
        again = zs.recode(level=1, verify=verify, entropy=True)       # the held forms H decoded and coded again: none is smaller
        assert (again.n_recoded, again.n_undecodable, again.stored_after) == (0, 0, info.stored_after)
        with zs.zpack(digests, r.lens32, verify=verify) as cut:
            got_e, got_b = cut.entries().copy(), cut.read()
            want_e = _under(h.zentries, digests)
            assert _same(got_e, want_e, CODED), _bad_rows(got_e, want_e, CODED)
            assert got_b == h.zblob, _first_difference(got_b, h.zblob)
            _decodes_to_the_rows(e, r, cut, digests, verify)


def test_a_level_1_set_recoded_at_level_2_holds_the_smaller_form_of_every_row(rows):
    """mi_zset_recode(LEVEL2 | VERIFY) with the default scratch_bytes (256 MiB): a row needs 32 bytes of it, so ONE round holds all
    1 048 876 rows, listed from 4 194 304 slots by a plan of 8 rounds.  The waves of zrecode_decode_kernel and
    zrecode_encode_l2_kernel go round -- over rows in slot order, so the rows of the second trip are tiny here"""
    _recoded_at_level_2(rows, rows.digests, True)


def test_a_level_1_set_recoded_with_the_stage_holds_the_stages_forms(rows):
    """mi_zset_recode(ENTROPY | VERIFY), default scratch_bytes, one round.  The candidate is the level's form with the stage over
    it and replaces a form only where it is strictly smaller (zrecode_h_cases' rule), so the set ends holding exactly the model
    of level 1 with the stage; a second call decodes those forms H and replaces nothing"""
    _recoded_with_the_stage(rows, rows.digests, True)


@pytest.mark.parametrize("how", ["level 2", "stage"])
def test_recodes_in_row_order_take_the_planted_pairs_on_their_second_trip(rows, how):
    """the same two recodes over a set under store_rows_cases.crafted_digests, without VERIFY (the digests are opaque): slot
    order is row order, so the waves of zrecode_decode_kernel, zrecode_encode_l1 / _l2_kernel and zh_recode_encode_kernel
    that took list rows 0..299 go on to 2^20..2^20 + 299 -- an LZ4 or form H row behind one of the same kind"""
    (_recoded_at_level_2 if how == "level 2" else _recoded_with_the_stage)(rows, sr.crafted_digests(rows.n), False)


# ---- g. the restore ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["plain set", "compressed set"])
def test_files_are_rebuilt_from_the_rows_in_order_alone_and_permuted(rows, source):
    """mi_batch_add_recipes / mi_batch_add_zrecipes with VERIFY: one file of all rows in order, 300 files of one planted row
    each (100 of them rows of the second trip) and one file of the rows in a seeded order"""
    r = rows
    order = np.random.default_rng(1605).permutation(r.n)
    singles = np.concatenate([r.planted[r.planted >= sr.WAVE_GRID][:100], r.planted[r.planted < sr.WAVE_GRID][::2][:200]])
    assert len(singles) == 300
    picks = [np.arange(r.n)] + [np.array([k]) for k in singles] + [order]
    recipes = [(np.ascontiguousarray(r.digests[p]), r.lens32[p]) for p in picks]
    z = r.models["l1h"]
    with M.Engine() as e, (e.packset() if source == "plain set" else e.zset()) as s, e.batch() as b:
        if source == "plain set":
            s.add_blob(r.blob, r.entries, verify=True)
            st = b.add_recipes(s, recipes, verify=True)
        else:
            s.add_zblob(z.zblob, z.zentries, verify=True)
            st = b.add_zrecipes(s, recipes, verify=True)
        total = int(r.lengths.astype(np.uint64).sum())
        assert (st.n_files, st.n_rows, st.bytes) == (302, 2 * r.n + 300, 2 * total + int(r.lengths[singles].sum()))
        b.run()
        bodies = [r.plain_of(p) for p in picks]
        for i, want in enumerate(bodies):
            got = b.read_file(i, 0, len(want))
            assert got == want, (i, _first_difference(got, want))
        # the batch is an ordinary batch: mi_batch_run cuts the rebuilt files with the engine's own CDC parameters.  Rows of
        # 8..12 bytes are nobody's cuts (min_size is 64 at the least), so the roots are not mi_chunk_root over the recipes'
        # digests: they are the roots of the same bytes fed from the host
        with e.batch() as fed:
            for i, want in enumerate(bodies):
                fed.add_bytes(want, i)
            fed.run()
            assert np.array_equal(b.roots(), fed.roots())
            assert np.array_equal(b.chunks()["sha256"], fed.chunks()["sha256"]) and np.array_equal(b.chunks()["length"], fed.chunks()["length"])


# ---- h. BLAKE2s -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blake_rows():
    """526 413 rows under BLAKE2s digests: the plan's second round with a partial last block, no second trip"""
    return sr.sliced(sr.million_rows(pc.BLAKE2S), sr.EDGE_SIZES[2])


def test_blake2s_rows_are_coded_with_the_stage_and_decoded_again(blake_rows):
    """FLAG_CHUNK_BLAKE2S: the coder with the stage and VERIFY, and the decode of the level-1 and of the stage's zpack"""
    _coded_to_the_model(blake_rows, "l1h", True, pc.BLAKE2S)
    for m in ("l1", "l1h"):
        _decoded_to_the_rows(blake_rows, m, pc.BLAKE2S)


@pytest.mark.parametrize("how", ["lz4", "h"])
def test_blake2s_a_damaged_row_of_the_second_round_is_named(blake_rows, how):
    """at this size no wave takes a second row: the damaged row is a planted one behind row 524 288, placed by the carry"""
    r = blake_rows
    f = r.models["l1h"].forms
    blob, bad, rule = _damaged(r, how, lambda form: [int(k) for k in r.planted if k >= sr.PLAN_ROUND and f[k] == form])
    assert sr.PLAN_ROUND <= bad < r.n
    _every_reader_names(r, blob, bad, rule, pc.BLAKE2S)
