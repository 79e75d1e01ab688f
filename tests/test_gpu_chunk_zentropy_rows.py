"""GPU tests of the zpack entropy stage where tests/test_gpu_chunk_zentropy.py does not reach, over the inputs
of zentropy_rows_cases.py (whose conditions tests/test_host_chunk_zentropy_rows.py proves from the model alone):

  1. MANY ROWS.  69 637 rows: zh_classify_kernel, zh_offsets_kernel and zh_place_kernel run as 35 blocks, so a form H row's place
     is its block's offset plus its place in the block; zh_unwrap_kernel's 65 536 workgroups go round, so 4 101 waves unwrap a
     second row over the table and the counts the first one left in LDS, and a refused row on the second trip is the one named;
  2. a sound form H under the digest of other bytes: every verifying reader hashes what form H decodes to;
  3. BLAKE2s digests through the coder and every reader;
  4. forms H the coder never makes and the format allows: empty streams, a code clamped from 21 bits, a complete 256-symbol
     code, a one-symbol code;
  5. the keep rule h < under - (under >> 4) on its line, in the coder and in the recode.

Everything is compared with zentropy_cases.py's model byte for byte: there are no tolerances.  Sections 1 to 3 run at level 1
(300 rows of section 1 also at level 2).  NOT covered here, for their sizes, and covered by tests/test_gpu_chunk_store_rows.py
and tests/test_gpu_chunk_store_rows_batch.py: the second trip of the encode kernels (more than 2^20 rows) and the carry between
the rounds of plan_block_offsets (more than 524 288 rows)."""
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
import zentropy_cases as ze  # noqa: E402
import zentropy_rows_cases as zr  # noqa: E402
import zpack_cases as zc  # noqa: E402
import zrecode_h_cases as zh  # noqa: E402

pytestmark = pytest.mark.gpu

ALGS = [pc.SHA256, pc.BLAKE2S]
RULE_WORDS = {7: "a pad byte behind the stored span", 8: "an entropy form with a bad header", 9: "an entropy form whose code lengths",
              10: "an entropy form whose stream sizes", 11: "an entropy form with a stream that ends early"}


def _engine(alg=pc.SHA256, **kw):
    return M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0, **kw)


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


def _counts(info):
    return {k: v for k, v in info.as_dict().items() if not k.startswith("ms_")}


def _forms(f):
    return [[int(f.n[i]), int(f.stored[i])] for i in range(4)]


def _state(zs, request):
    """everything the public calls say about a compressed set"""
    d, ln, st = zs.entries()
    with zs.zpack(request) as z:
        e, b = z.entries().copy(), z.read()
    return ({bytes(d[i]): (int(ln[i]), int(st[i])) for i in range(len(d))}, e.tobytes(), b, zs.usage().as_dict(), _counts(zs.info))


def _pack_of_chunks(engine, entries, blob):
    with engine.packset() as s:
        s.add_blob(blob, entries, verify=True)
        p = s.pack(np.ascontiguousarray(entries["digest"]), verify=True)
    assert pc.same_entries(p.entries(), entries) and p.bytes() == blob
    return p


def _first_difference(got, want):
    if len(got) != len(want):
        return "lengths %d and %d" % (len(got), len(want))
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    return int(np.flatnonzero(a != b)[0]) if (a != b).any() else None


def _bad_rows(got, want):
    """the first rows whose stored size or offset is not the model's, with the tile they lie in"""
    bad = np.flatnonzero((got["stored"] != want["stored"]) | (got["offset"] != want["offset"]))
    return [(int(k), int(k) // zr.PLAN_TILE, int(got["stored"][k]), int(want["stored"][k])) for k in bad[:8]]


def _recipe(entries, rows=None):
    d, n = np.ascontiguousarray(entries["digest"]), entries["length"].astype(np.uint32)
    return (d, n) if rows is None else (np.ascontiguousarray(d[rows]), n[rows])


@pytest.fixture(scope="module")
def rows():
    t = time.time()
    r = zr.many_rows()
    print("the model of %d rows: %.1f s; census %r, %d form H rows" % (zr.N_ROWS, time.time() - t, r.census, int(r.is_h.sum())))
    return r


# ---- 1. many rows: 35 tiles, 4 101 second trips ------------------------------------------------------------------------------------------
def test_many_rows_are_coded_to_the_models_bytes_with_and_without_verify(rows):
    """mi_pack_compress with the stage; with VERIFY the call unwraps and decodes the forms it has just coded (the unwrap's call
    site in mi_zpack.hip)"""
    r = rows
    with M.Engine() as e:
        with _pack_of_chunks(e, r.entries, r.blob) as p:
            for verify in (False, True):
                with p.compress(verify=verify, level=1, entropy=True) as z:
                    got_e, got_b, info = z.entries().copy(), z.read(), z.info
                    assert _same_zentries(got_e, r.zentries), _bad_rows(got_e, r.zentries)
                    assert got_b == r.zblob, _first_difference(got_b, r.zblob)
                    assert (info.n_entries, info.blob_bytes, info.stored_bytes, info.n_raw, info.verified) == \
                        (zr.N_ROWS, len(r.zblob), int(r.zentries["stored"].sum()), r.census[0][0], int(verify))
                    assert _forms(z.count_forms()) == r.census
            assert M.zpack_check(got_b, got_e) is None
            assert p.bytes() == r.blob                              # the input is unchanged
        # a few hundred rows at level 2, a pack of their own
        chunks, entries, blob, want_e, want_b = zr.level2_rows()
        with _pack_of_chunks(e, entries, blob) as p2, p2.compress(verify=True, level=2, entropy=True) as z:
            assert _same_zentries(z.entries(), want_e) and z.read() == want_b
            assert _forms(z.count_forms()) == ze.count_forms(want_e, want_b)


def test_many_rows_decode_into_a_plain_set_byte_for_byte(rows):
    """mi_packset_add_zpack and _add_zblob with VERIFY: the unwrap in front of the decode, over every row"""
    r = rows
    with M.Engine() as e:
        with _pack_of_chunks(e, r.entries, r.blob) as p, p.compress(level=1, entropy=True) as z:
            for feed in ("zblob", "zpack"):
                with e.packset() as s:
                    if feed == "zblob":
                        s.add_zblob(r.zblob, r.zentries, verify=True)
                    else:
                        s.add_zpack(z, verify=True)
                    assert s.info.n_digests == zr.N_ROWS
                    with s.pack(r.digests, r.lens32, verify=True) as back:
                        got = back.bytes()
                        assert got == r.blob, (feed, _first_difference(got, r.blob))


def test_many_rows_in_a_compressed_set_are_counted_cut_and_restored(rows):
    r = rows
    rng = np.random.default_rng(981)
    order = rng.permutation(zr.N_ROWS)
    tail = np.arange(zr.N_ROWS - 1, zr.UNWRAP_GRID - 1, -1)        # the rows of the second trip, backwards
    front = rng.integers(1, 256, 1001, dtype=np.uint8).tobytes()
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(r.zblob, r.zentries, verify=True)             # MI_ZSET_VERIFY: unwrap, decode, hash
        assert zs.info.n_digests == zr.N_ROWS
        assert _forms(zs.count_forms()) == r.census                 # zh_classify_kernel over the table's slots, tags and all
        with zs.zpack(r.digests, r.lens32, verify=True) as z:       # the cut of everything IS the model's zpack
            got_e, got_b = z.entries().copy(), z.read()
            assert _same_zentries(got_e, r.zentries), _bad_rows(got_e, r.zentries)
            assert got_b == r.zblob, _first_difference(got_b, r.zblob)
        bodies = [b"".join(r.chunks[k] for k in order), b"".join(r.chunks[k] for k in tail)]
        with e.batch() as b:
            b.add_bytes(front, 7)                                   # destinations at odd residues
            st = b.add_zrecipes(zs, [_recipe(r.entries, order)], verify=True)
            assert (st.n_files, st.n_rows, st.bytes) == (1, zr.N_ROWS, len(bodies[0]))
            st = b.add_zrecipes(zs, [_recipe(r.entries, tail)], verify=True)
            assert (st.n_files, st.n_rows, st.bytes) == (1, len(tail), len(bodies[1]))
            b.run()
            for i, x in enumerate([front] + bodies):
                got = b.read_file(i, 0, len(x))
                assert got == x, (i, _first_difference(got, x))


def test_a_level_1_set_of_many_rows_recoded_with_the_stage_holds_the_models_forms(rows):
    """mi_zset_recode(ENTROPY | VERIFY): the recheck unwraps every replaced row (more than a tile of them); the second call is
    the recode's unwrap over more than 65 536 held rows, and a scrub of every one"""
    r = rows
    n_h = int(r.is_h.sum())
    assert n_h > zr.PLAN_TILE
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(r.zb1, r.ze1, verify=True)
        assert _forms(zs.count_forms())[2:] == [[0, 0], [0, 0]]
        info = zs.recode(level=1, verify=True, entropy=True)
        assert (info.n_digests, info.n_recoded, info.n_undecodable) == (zr.N_ROWS, n_h, 0)
        assert (info.stored_before, info.stored_after) == (int(r.ze1["stored"].sum()), int(r.zentries["stored"].sum()))
        assert zs.info.stored_bytes == info.stored_after
        assert _forms(zs.count_forms()) == r.census
        with zs.zpack(r.digests, r.lens32, verify=True) as z:
            got_e, got_b = z.entries().copy(), z.read()
            assert _same_zentries(got_e, r.zentries), _bad_rows(got_e, r.zentries)
            assert got_b == r.zblob, _first_difference(got_b, r.zblob)
        again = zs.recode(level=1, verify=True, entropy=True)
        assert (again.n_recoded, again.n_undecodable, again.stored_after) == (0, 0, info.stored_after)
        assert _forms(zs.count_forms()) == r.census


@pytest.mark.parametrize("how", sorted(zr.DAMAGE))
def test_a_refused_row_on_the_second_trip_is_the_row_every_reader_names(rows, how):
    """two damaged form H rows behind row 65 636, the later one with another rule: the atomicMin over the refused rows is fed
    from second trips only.  "unassigned code" is refused through one table entry that is nobody's, behind a row whose code
    filled the whole table: only a table cleared for every row refuses it (zentropy_rows_cases.unassigned_behind)"""
    r = rows
    zentries, blob, a, b_row, rule = zr.damaged(r, how)
    assert a >= zr.UNWRAP_GRID + 100 and b_row > a
    assert M.zpack_check(blob, zentries) == a
    assert ze.first_refused(zentries[zr.UNWRAP_GRID:], blob) == (a - zr.UNWRAP_GRID, rule)
    word = RULE_WORDS[rule]
    with M.Engine() as e, e.packset() as ps, e.batch() as b:
        b.add_bytes(b"front" * 50, 1)
        ps_info = _counts(ps.info)
        err = _raises(-1, lambda: ps.add_zblob(blob, zentries), "entry %d " % a, "does not decode: ", word)
        assert err.first_bad == a and _counts(ps.info) == ps_info
        with e.zset() as zs:
            before = _counts(zs.info)
            err = _raises(-1, lambda: zs.add_zblob(blob, zentries, verify=True), "entry %d " % a, word)
            assert err.first_bad == a and _counts(zs.info) == before
            zs.add_zblob(blob, zentries)                            # an unverified set takes it: nothing is decoded at add time
            counts = b.counts()
            for verify in (False, True):
                _raises(-1, lambda: b.add_zrecipes(zs, [_recipe(r.entries)], verify=verify), "file 0, row %d " % a, word)
            assert b.counts() == counts
            # ... and the rows in front of the damage still restore from that set
            head = np.arange(a - 300, a)
            b.add_zrecipes(zs, [_recipe(r.entries, head)], verify=True)
            b.run()
            body = b"".join(r.chunks[k] for k in head)
            assert b.read_file(1, 0, len(body)) == body


# ---- 2. a good form H under the wrong digest ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_a_sound_form_h_under_another_digest_is_refused_by_every_verifying_reader_only(alg):
    for name, entries, blob, bad in zr.wrong_digest_zpacks(alg):
        n = len(entries)
        assert M.zpack_check(blob, entries, alg=alg) == bad and ze.first_refused(entries, blob) is None, name
        every = np.ascontiguousarray(entries["digest"])
        recipe = [_recipe(entries)]
        plain = b"".join(ze.expand_chunk(blob[int(en["offset"]):int(en["offset"]) + int(en["stored"])], int(en["length"])) for en in entries)
        with _engine(alg) as e:
            with e.packset() as ps:
                info = _counts(ps.info)
                err = _raises(-1, lambda: ps.add_zblob(blob, entries, verify=True), "entry %d " % bad, "does not hash")
                assert err.first_bad == bad and _counts(ps.info) == info and ps.info.n_digests == 0, name
                with e.zset() as loose, e.batch() as r:
                    loose.add_zblob(blob, entries)
                    with loose.zpack(every) as z:                  # the same entries as a ZPack on the device
                        assert z.read() == blob
                        _raises(-1, lambda: ps.add_zpack(z, verify=True), "entry %d " % bad, "does not hash")
                        assert _counts(ps.info) == info, name
                        ps.add_zpack(z)                             # without the flag it gets past: decoded, not hashed
                    with ps.pack(every) as p:
                        assert b"".join(p.read(int(en["offset"]), int(en["length"])) for en in p.entries()) == plain, name
                    _raises(-5, lambda: r.add_recipes(ps, recipe, verify=True), "row %d " % bad)
                with e.packset() as ps2:
                    ps2.add_zblob(blob, entries)                    # ... and so does the blob
                    assert ps2.info.n_digests == n
            with e.zset() as zs:
                before = _counts(zs.info)
                err = _raises(-1, lambda: zs.add_zblob(blob, entries, verify=True), "entry %d " % bad, "does not hash")
                assert err.first_bad == bad and _counts(zs.info) == before and zs.info.n_digests == 0, name
                zs.add_zblob(blob, entries)                         # an unverified set takes it
                state = _state(zs, every)
                with e.batch() as r:
                    _raises(-5, lambda: r.add_zrecipes(zs, recipe, verify=True), "row %d " % bad)
                    assert r.counts() == (0, 0, 0), name
                    r.add_zrecipes(zs, recipe)                      # the unflagged restore writes what the form decodes to
                    r.run()
                    assert r.read_file(0, 0, len(plain)) == plain, name
                for entropy in (False, True):
                    _raises(-5, lambda: zs.recode(level=1, verify=True, entropy=entropy), "1 of %d entries" % n, bytes(every[bad]).hex(),
                            "hash to another digest", "unchanged")
                    assert _state(zs, every) == state, (name, entropy)
                info = zs.recode(level=1, entropy=True)             # unverified: recoded like any other, nothing undecodable
                assert info.n_undecodable == 0 and info.n_digests == n, name


# ---- 3. BLAKE2s ------------------------------------------------------------------------------------------------------------------------------
def test_blake2s_the_hand_built_zpack_goes_through_every_reader():
    alg = pc.BLAKE2S
    entries, blob = ze.good_zpack(alg)
    want = zc.GOOD_PLAIN + ze.GOOD_PLAIN + bytes(range(40)) + ze.GOOD_PLAIN2
    every = np.ascontiguousarray(entries["digest"])
    assert M.zpack_check(blob, entries, alg=alg) is None and M.zpack_check(blob, entries, alg=pc.SHA256) == 0
    with _engine(alg) as e, e.packset() as ps, e.zset() as zs, e.batch() as b:
        ps.add_zblob(blob, entries, verify=True)
        with ps.pack(every, verify=True) as p:
            assert b"".join(p.read(int(en["offset"]), int(en["length"])) for en in p.entries()) == want
        zs.add_zblob(blob, entries, verify=True)
        assert _forms(zs.count_forms()) == ze.count_forms(entries, blob) and [c for c, _ in _forms(zs.count_forms())] == [1, 1, 1, 1]
        with zs.zpack(every, verify=True) as z, e.packset() as ps2:
            assert z.read() == blob
            ps2.add_zpack(z, verify=True)
            assert ps2.info.n_digests == 4
        b.add_bytes(b"odd", 3)
        b.add_zrecipes(zs, [_recipe(entries)], verify=True)
        b.run()
        assert b.read_file(1, 0, len(want)) == want
        info = zs.recode(level=1, verify=True, entropy=True)        # a scrub with BLAKE2s: every form decodes and hashes
        assert info.n_undecodable == 0 and info.n_digests == 4
    with M.Engine() as sha:                                          # the same zpack in a SHA-256 engine: no digest fits
        with sha.zset() as zs:
            _raises(-1, lambda: zs.add_zblob(blob, entries, verify=True), "entry 0 ", "does not hash")


def test_blake2s_the_malformed_rows_behind_good_entries_are_named_with_their_rules():
    alg = pc.BLAKE2S
    picked = {}
    for name, entries, blob, bad, rule in ze.malformed_zpacks(alg):
        if name.endswith("behind good entries") and rule not in picked and rule >= 7:
            picked[rule] = (name, entries, blob, bad)
    assert sorted(picked) == [7, 8, 9, 10, 11]
    with _engine(alg) as e, e.packset() as ps, e.batch() as b:
        for rule, (name, entries, blob, bad) in sorted(picked.items()):
            assert M.zpack_check(blob, entries, alg=alg) == bad and ze.first_refused(entries, blob) == (bad, rule), name
            word = RULE_WORDS[rule]
            err = _raises(-1, lambda: ps.add_zblob(blob, entries, verify=True), "entry %d " % bad, "does not decode: ", word)
            assert err.first_bad == bad and ps.info.n_digests == 0, name
            with e.zset() as zs:
                before = _counts(zs.info)
                err = _raises(-1, lambda: zs.add_zblob(blob, entries, verify=True), "entry %d " % bad, word)
                assert err.first_bad == bad and _counts(zs.info) == before, name
                zs.add_zblob(blob, entries)
                counts = b.counts()
                _raises(-1, lambda: b.add_zrecipes(zs, [_recipe(entries)], verify=True), "file 0, row %d " % bad, word)
                assert b.counts() == counts, name
                _raises(-5, lambda: zs.recode(level=1, verify=True, entropy=True), word, "unchanged")


def test_blake2s_the_coder_gives_the_models_bytes_on_the_planted_chunks():
    alg = pc.BLAKE2S
    chunks = [c for _, c in ze.planted_chunks_h() if len(c) <= 8192]
    entries, blob, want_e, want_b = zr.model_forms(chunks, 1, alg)
    census = ze.count_forms(want_e, want_b)
    assert all(c > 0 for c, _ in census), census
    with _engine(alg) as e:
        with _pack_of_chunks(e, entries, blob) as p, p.compress(verify=True, level=1, entropy=True) as z:
            got_e, got_b = z.entries().copy(), z.read()
            assert _same_zentries(got_e, want_e) and got_b == want_b and z.info.verified == 1
            assert _forms(z.count_forms()) == census and M.zpack_check(got_b, got_e, alg=alg) is None
            with e.packset() as s:
                s.add_zpack(z, verify=True)
                with s.pack(*_recipe(entries), verify=True) as back:
                    assert back.bytes() == blob
            with e.zset() as zs, e.batch() as b:
                zs.add_zpack(z, verify=True)
                b.add_zrecipes(zs, [_recipe(entries)], verify=True)
                b.run()
                assert b.read_file(0, 0, sum(map(len, chunks))) == b"".join(chunks)


# ---- 4. edge forms for the decoder ------------------------------------------------------------------------------------------------------------
def test_forms_the_coder_never_makes_are_accepted_and_restore_their_chunks():
    """every form alone and all of them in one zpack, into a plain set, into a verified compressed set and out of it through
    mi_batch_add_zrecipes behind fronts of 1, 2 and 3 bytes and behind each other (lengths 1 000, 2 017, ... : odd residues)"""
    zpacks = zr.edge_zpacks()
    assert len(zpacks) == 14
    with M.Engine(max_size=262144) as e:
        for i, (name, entries, blob, chunks) in enumerate(zpacks):
            assert M.zpack_check(blob, entries) is None and ze.first_refused(entries, blob) is None, name
            every = np.ascontiguousarray(entries["digest"])
            body = b"".join(chunks)
            with e.packset() as ps:
                ps.add_zblob(blob, entries, verify=True)
                with ps.pack(every, verify=True) as p:
                    got = b"".join(p.read(int(en["offset"]), int(en["length"])) for en in p.entries())
                    assert got == body, (name, _first_difference(got, body))
            with e.zset() as zs, e.batch() as b:
                zs.add_zblob(blob, entries, verify=True)
                assert sum(c for c, _ in _forms(zs.count_forms())[2:]) == len(chunks), name
                front = b"\x55" * (1 + i % 3)
                b.add_bytes(front, 0)
                order = np.arange(len(chunks))[::-1]
                b.add_zrecipes(zs, [_recipe(entries), _recipe(entries, order)], verify=True)
                b.run()
                assert b.read_file(1, 0, len(body)) == body, name
                back = b"".join(chunks[k] for k in order)
                assert b.read_file(2, 0, len(back)) == back, name
                info = zs.recode(level=1, verify=True)              # a scrub through the unwrap: nothing is undecodable
                assert info.n_undecodable == 0, name


# ---- 5. the keep rule on its line ---------------------------------------------------------------------------------------------------------------
def test_the_keep_rule_is_strictly_less_in_the_coder_and_in_the_recode():
    cases = zr.edge_chunks_h()
    chunks = [c for _, c, _ in cases]
    margins = [[zr.keep_margin(c, level) for c in chunks] for level in (1, 2)]
    assert margins[0] == [0, -1, 0, -1] and 0 in margins[1] and -1 in margins[1]
    with M.Engine() as e:
        for level in (1, 2):
            entries, blob, want_e, want_b = zr.model_forms(chunks, level)
            forms = [ze.form_of(f, len(c)) for f, c in zip(zh.forms_of(want_e, want_b), chunks)]
            assert [f >= 2 for f in forms] == [m < 0 for m in margins[level - 1]]            # kept exactly where h is UNDER the bound
            with _pack_of_chunks(e, entries, blob) as p, p.compress(verify=True, level=level, entropy=True) as z:
                got_e, got_b = z.entries().copy(), z.read()
                assert [int(s) for s in got_e["stored"]] == [int(s) for s in want_e["stored"]], (level, margins[level - 1])
                assert _same_zentries(got_e, want_e) and got_b == want_b
        entries, blob, want_e, want_b = zr.model_forms(chunks, 1)
        ze1, zb1 = zc.model_compress(entries, blob)
        with e.zset() as zs:                                          # the recode's choice: the same line
            zs.add_zblob(zb1, ze1, verify=True)
            info = zs.recode(level=1, verify=True, entropy=True)
            assert (info.n_recoded, info.n_undecodable, info.stored_after) == (2, 0, int(want_e["stored"].sum()))
            with zs.zpack(*_recipe(entries), verify=True) as z:
                got_e = z.entries().copy()
                assert [int(s) for s in got_e["stored"]] == [int(s) for s in want_e["stored"]]
                assert _same_zentries(got_e, want_e) and z.read() == want_b
