"""GPU tests of the consuming side of the chunk packs (mi_packset_*, mi_batch_add_recipes): files assembled on the device from
packs and recipes are compared, every byte, with what the pure-Python models of pack_cases.py and restore_cases.py say --
chunks of every (start mod 16, length mod 16), rows of a few bytes that are joined into units, the edge sizes and the gaps
between files, several packs and a batch that mixes restored and host-fed files, keys that collide in the table, everything
that is refused, damaged blobs with and without the two verification flags, a commit taken apart and put back together on
another engine, destinations past 2^32 and the read bound under the guard allocator.  Bit for bit: there are no tolerances."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (before the engine: the 4 GiB test asks it for the device's free memory)
except ImportError:          # CPU-only collection without torch: the GPU tests are skipped anyway
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import pack_cases as pc  # noqa: E402
import restore_cases as rc  # noqa: E402
from commit_cases import commit_to_bytes, make_tree, write_file  # noqa: E402

pytestmark = pytest.mark.gpu
MTIME = 1_600_000_000
MIB = 1 << 20


def _recipes(rows, files, alg=pc.SHA256):
    return [rc.recipe_of(rows, files, f, alg) for f in range(len(files))]


def _counts(b):
    return b.counts()


# ---- 1. the residue sweep ------------------------------------------------------------------------------------------------
def test_every_start_and_length_residue_is_assembled_byte_for_byte():
    data = np.random.default_rng(31).integers(0, 256, MIB, dtype=np.uint8).tobytes()
    with M.Engine(mask_bits=6, min_size=64, max_size=1024) as e, e.batch() as b:
        b.add_bytes(data, 0)
        b.run()
        chunks, root = b.chunks().copy(), b.files()["chunk_root"][0].tobytes()
        rows = pc.rows_of(chunks)
        # the condition the test rests on: all 256 pairs (chunk start mod 16, length mod 16) occur
        assert len({(off % 16, n % 16) for _, off, n in rows}) == 256 and len(rows) > 8000
        with b.pack() as p:
            entries, blob = p.entries(), p.bytes()
        recipe = (np.ascontiguousarray(chunks["sha256"]), chunks["length"].astype(np.uint32))
        with e.packset() as s, e.batch() as r:
            s.add_blob(blob, entries, verify=True)
            info = s.info
            assert (info.n_packs, info.n_entries, info.blob_bytes, info.alg) == (1, len(entries), len(blob), pc.SHA256)
            assert info.n_digests == len({bytes(d) for d in entries["digest"]}) and info.ms_upload > 0 and info.ms_verify > 0
            st = r.add_recipes(s, [recipe], tags=[77], verify=True)
            assert (st.n_files, st.n_rows, st.bytes) == (1, len(rows), len(data))
            assert st.n_joined_units == rc.joined_units([recipe]) > 0
            assert st.ms_assemble > 0 and st.ms_resolve > 0 and st.ms_verify > 0
            r.run()
            assert r.read_back().tobytes() == data
            got = r.chunks()
            for col in ("file_index", "offset", "length", "dup_of", "sha256"):
                assert np.array_equal(got[col], chunks[col]), col
            fr = r.files()
            assert fr["chunk_root"][0].tobytes() == root and int(fr["user_tag"][0]) == 77 and int(fr["size"][0]) == len(data)


# ---- 2. tiny rows: the joined path, on purpose ------------------------------------------------------------------------------
def _tiny_files():
    rng = np.random.default_rng(41)
    a = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    rows_a = pc.random_cut_rows(rng, [a], 1, 40)
    assert len(rows_a) == 3205
    assert rc.unit_cover_histogram([n for _, _, n in rows_a]) == {1: 1645, 2: 1980, 3: 412, 4: 53, 5: 5, 6: 1}
    assert len({hashlib.sha256(a[o:o + n]).digest() for _, o, n in rows_a}) == 3181          # 1-byte chunks repeat
    lens_b = [1] * 64 + [15, 16, 17, 31, 32, 33, 1]
    b = rng.integers(0, 256, sum(lens_b), dtype=np.uint8).tobytes()
    rows_b, at = [], 0
    for n in lens_b:
        rows_b.append((1, at, n))
        at += n
    assert rc.unit_cover_histogram(lens_b)[16] == 4                                          # four units of sixteen rows each
    # a third file whose tiles hold more rows than the assemble kernel keeps in LDS (1 024): rows of 1..8 bytes, some 3 600 a tile
    c = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    rows_c = [(2, off, n) for _, off, n in pc.random_cut_rows(rng, [c], 1, 8)]
    assert len(rows_c) > 2 * 3000
    return [a, b, c], rows_a + rows_b + rows_c


@pytest.mark.parametrize("alg", [pc.SHA256, pc.BLAKE2S])
def test_rows_of_a_few_bytes_are_joined_into_units(alg):
    files, rows = _tiny_files()
    entries, blob = pc.model_pack(rows, files, None, alg)                                    # one pack carries a digest several times
    recipes = _recipes(rows, files, alg)
    assert rc.model_restore([(entries, blob)], recipes) == files
    want_joined = rc.joined_units(recipes)
    with M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0) as e, e.packset() as s:
        s.add_blob(blob, entries, verify=True)
        assert s.info.n_digests == len({bytes(d) for d in entries["digest"]}) < len(entries) and s.info.alg == alg
        for verify in (False, True):
            with e.batch() as b:
                st = b.add_recipes(s, recipes, verify=verify)
                assert st.n_joined_units == want_joined and st.n_rows == len(rows)
                assert (st.ms_verify > 0) == verify
                b.run()
                for i, x in enumerate(files):
                    assert b.read_file(i, 0, len(x)) == x, (i, verify)


# ---- 3. edge files and the gaps between them ---------------------------------------------------------------------------------
EDGE_SIZES = [0, 0, 1, 15, 16, 17, 255, 256, 257, 4096, 70000, 0]          # two empty files next to each other, one last


def _edge_case(seed=43):
    rng = np.random.default_rng(seed)
    files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in EDGE_SIZES]
    rows = pc.random_cut_rows(rng, files)                                                    # rows of 1..700 bytes
    entries, blob = pc.model_pack(rows, files)
    return files, rows, entries, blob, _recipes(rows, files)


def test_edge_files_come_back_and_the_file_in_front_is_untouched():
    files, rows, entries, blob, recipes = _edge_case()
    front = np.random.default_rng(44).integers(1, 256, 1001, dtype=np.uint8).tobytes()      # ends 23 bytes into a 256-byte slot
    with M.Engine() as e, e.packset() as s, e.batch() as b:
        s.add_blob(blob, entries, verify=True)
        b.add_bytes(front, 5)
        st = b.add_recipes(s, recipes, verify=True)
        assert st.n_files == len(files) and st.bytes == sum(EDGE_SIZES) and st.n_joined_units == rc.joined_units(recipes)
        b.run()
        assert b.read_back().tobytes() == front + b"".join(files)
        fr = b.files()
        assert fr["size"].tolist() == [len(front)] + EDGE_SIZES
        with e.batch() as plain:                                                             # the rows and roots of the same bytes, host-fed
            for i, x in enumerate([front] + files):
                plain.add_bytes(x, i)
            plain.run()
            assert np.array_equal(plain.files()["chunk_root"], fr["chunk_root"])
            assert np.array_equal(plain.chunks()["sha256"], b.chunks()["sha256"])


# ---- 4. several packs, a mixed batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hint", [None, (2, 4096)], ids=["no hints: an arena in pieces", "a small hint: one allocation that moves"])
def test_several_packs_and_a_batch_that_mixes_restored_and_host_fed_files(hint):
    rng = np.random.default_rng(45)
    src = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (200_000, 77_777)]
    with M.Engine(mask_bits=6, min_size=64, max_size=1024) as e, e.batch() as b0, e.packset() as s:
        for i, x in enumerate(src):
            b0.add_bytes(x, i)
        b0.run()
        rows = pc.rows_of(b0.chunks())
        n = len(rows)
        assert n > 2000
        sels = [np.array([i % 3 == k for i in range(n)], dtype=np.uint8) for k in range(3)]  # three disjoint selections
        packs = [b0.pack(select=sel) for sel in sels]
        s.add_pack(packs[0], verify=True)
        s.add_pack(packs[1])
        n_before = s.info.n_digests
        s.add_pack(packs[1], verify=True)                                                    # one of them twice
        assert s.info.n_digests == n_before
        s.add_pack(packs[2], verify=True)
        fourth = pc.model_pack(rows, src, [i % 6 == 0 for i in range(n)])                    # repeats rows of the first
        s.add_blob(fourth[1], fourth[0], verify=True)
        host_packs = [(p.entries(), p.bytes()) for p in packs]
        for p in packs:
            p.close()                                                                        # the set has copies of its own
        info = s.info
        assert info.n_packs == 5 and info.n_entries == n + int(sels[1].sum()) + len(fourth[0])
        assert info.n_digests == len({hashlib.sha256(src[f][o:o + k]).digest() for f, o, k in rows})
        base = _recipes(rows, src)
        r0 = base[0]
        pick = [5, 9, 5, 100, 2001 % len(r0[1]), 5]                                          # one chunk three times within a file
        custom1 = (r0[0][pick], r0[1][pick])
        pick2 = [5, 0, len(r0[1]) - 1]                                                       # ... and again in another file
        custom2 = (r0[0][pick2], r0[1][pick2])
        small = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (10, 3000, 999)]
        big = rng.integers(0, 256, 2 * MIB, dtype=np.uint8).tobytes()                        # the reader threads' way in
        want = [small[0], small[1]] + rc.model_restore(host_packs, [base[0], custom1]) + [big] + \
            rc.model_restore(host_packs, [base[1], custom2]) + [small[2]]
        assert want[2] == src[0] and want[5] == src[1]
        b = e.batch() if hint is None else e.batch(*hint)
        with b:
            b.add_bytes(small[0], 0)
            b.add_bytes(small[1], 1)
            b.add_recipes(s, [base[0], custom1], tags=[2, 3], verify=True)
            b.add_bytes(big, 4)
            b.add_recipes(s, [base[1], custom2], tags=[5, 6])
            b.add_bytes(small[2], 7)
            b.run()
            fr = b.files()
            assert fr["user_tag"].tolist() == list(range(8)) and fr["size"].tolist() == [len(x) for x in want]
            for i, x in enumerate(want):
                assert b.read_file(i, 0, len(x)) == x, i
            with e.batch() as plain:
                for i, x in enumerate(want):
                    plain.add_bytes(x, i)
                plain.run()
                assert np.array_equal(plain.files()["chunk_root"], fr["chunk_root"])


# ---- 5. keys that collide -----------------------------------------------------------------------------------------------------
def test_digests_that_share_their_first_eight_bytes_resolve_to_their_own_chunks():
    rng = np.random.default_rng(46)
    lens = [100, 100, 37, 64, 1, 250, 16, 90]                    # entries 0..2 collide; 0 and 1 have equal lengths
    chunks = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]
    rows, at = [], 0
    for k in lens:
        rows.append((0, at, k))
        at += k
    entries, blob = pc.model_pack(rows, [b"".join(chunks)])
    # verify is off: digests are opaque.  The table of a fresh set has 1 024 slots, slot = first 8 bytes (little endian) & 1023:
    # three digests with one tag walk to slots t, t + 1, t + 2; their neighbours are AT HOME in t + 1, t + 2, t + 3 and t - 1
    tag = 0x1122334455667000 | 0x2FF
    dig = np.zeros((len(lens), 32), dtype=np.uint8)
    for k in range(len(lens)):
        dig[k, 8:] = rng.integers(0, 256, 24, dtype=np.uint8)
    for k, t in enumerate([tag, tag, tag, tag + 1, tag + 2, tag + 3, tag - 1, 0]):             # (tag 0 is stored as 1: the last entry)
        dig[k, :8] = np.frombuffer(int(t).to_bytes(8, "little"), dtype=np.uint8)
    assert len({bytes(d) for d in dig}) == len(lens) and len({bytes(d[:8]) for d in dig[:3]}) == 1
    entries = entries.copy()
    entries["digest"] = dig
    order = [2, 0, 7, 1, 3, 6, 5, 4, 1, 2, 0]
    recipe = (dig[order], np.array([lens[k] for k in order], dtype=np.uint32))
    with M.Engine() as e, e.packset() as s, e.batch() as b:
        s.add_blob(blob, entries)
        assert s.info.n_digests == len(lens)
        b.add_recipes(s, [recipe] + [(dig[k:k + 1], np.array([lens[k]], dtype=np.uint32)) for k in range(len(lens))])
        b.run()
        assert b.read_file(0, 0, sum(lens[k] for k in order)) == b"".join(chunks[k] for k in order)
        for k in range(len(lens)):
            assert b.read_file(1 + k, 0, lens[k]) == chunks[k], k


# ---- 6. what is refused ---------------------------------------------------------------------------------------------------------
def _raises(code, call, *needles):
    with pytest.raises(M.MiError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)
    return ei.value


def test_what_is_refused_leaves_batch_and_set_as_they_were():
    files, rows, entries, blob, recipes = _edge_case(47)
    first = b"abc" * 1000
    with M.Engine() as e, M.Engine() as other, e.packset() as s, other.packset() as s_other:
        s.add_blob(blob, entries, verify=True)
        s_other.add_blob(blob, entries)
        info0 = s.info.as_dict()
        b = e.batch()
        b.add_bytes(first, 9)
        before = _counts(b)

        def unchanged():
            assert _counts(b) == before

        # an unknown digest: the message names file and row; of two bad rows the smaller wins
        f_big = EDGE_SIZES.index(70000)
        dig, lens = recipes[f_big]
        assert len(lens) > 12
        bad = dig.copy()
        bad[7, 3] ^= 1
        bad[3, 31] ^= 0x80
        err = _raises(-1, lambda: b.add_recipes(s, recipes[:f_big] + [(bad, lens)] + recipes[f_big + 1:]),
                      "file %d, row 3 " % f_big, bytes(bad[3]).hex(), "does not hold")
        assert bytes(bad[7]).hex() not in str(err)
        unchanged()
        # a stated length that differs from the entry's; a zero length
        wrong = lens.copy()
        wrong[5] += 1
        _raises(-1, lambda: b.add_recipes(s, [(dig, wrong)], verify=True), "file 0, row 5 ", "with %d bytes" % lens[5], "states %d" % wrong[5])
        unchanged()
        wrong = lens.copy()
        wrong[2] = 0
        _raises(-1, lambda: b.add_recipes(s, [recipes[2], (dig, wrong)]), "file 1, row 2 ", "length 0")
        unchanged()
        # a set of another ctx; NULL arguments
        _raises(-1, lambda: b.add_recipes(s_other, recipes), "another ctx")
        unchanged()
        assert e._lib.mi_batch_add_recipes(b._h, None, 0, None, None, None, None, 0, None) == -1
        one = np.array([1], dtype=np.uint64)
        assert e._lib.mi_batch_add_recipes(b._h, s._h, 1, one.ctypes.data, None, None, None, 0, None) == -1
        assert e._lib.mi_batch_add_recipes(b._h, s._h, 1, None, None, None, None, 0, None) == -1
        assert e._lib.mi_batch_add_recipes(b._h, s._h, 0, None, None, None, None, 0x2, None) == -1          # an unknown flag
        unchanged()

        # entries that leave the blob: MI_ERR_INVALID with first_bad, before any upload; the set's info does not move
        n = len(entries)
        k = next(i for i in range(n // 2, n) if int(entries["length"][i]) > 16)
        shapes = []
        shapes.append((blob[:-1], entries, n - 1))                                          # the last span exceeds the blob by 1
        en = entries.copy()
        en["offset"][k] = 2 ** 64 - 16
        shapes.append((blob, en, k))
        en = entries.copy()
        en["offset"][k] += 8
        shapes.append((blob, en, k))
        en = entries.copy()
        en["offset"][k] = en["offset"][k - 1]
        shapes.append((blob, en, k))
        for verify in (False, True):
            for bl, en, want_bad in shapes:
                err = _raises(-1, lambda: s.add_blob(bl, en, verify=verify))
                assert err.first_bad == want_bad
        assert (s.info.n_packs, s.info.n_entries, s.info.n_digests, s.info.blob_bytes) == tuple(info0[x] for x in ("n_packs", "n_entries", "n_digests", "blob_bytes"))
        bad_n = C.c_uint64()
        assert e._lib.mi_packset_add_blob(s._h, None, 0, entries.ctypes.data, 1 << 32, 0, C.byref(bad_n)) == -1      # n < 2^32, before entry 0 is read
        assert e._lib.mi_packset_add_blob(s._h, None, 0, None, 0, 0x2, None) == -1                                  # an unknown flag

        # mi_ctx_destroy while a set lives
        assert e._lib.mi_ctx_destroy(e._h) == -6 and b"still alive" in e._lib.mi_last_error(e._h)

        # after all of it: a correct add works, and the set may go before the batch runs
        s2 = e.packset()
        s2.add_blob(blob, entries)
        st = b.add_recipes(s2, recipes, verify=True)
        s2.close()
        assert st.n_files == len(files) and _counts(b) == (1 + len(files), 0, len(first) + sum(EDGE_SIZES))
        b.run()
        assert b.read_file(0, 0, len(first)) == first
        for i, x in enumerate(files):
            assert b.read_file(1 + i, 0, len(x)) == x, i
        # a staged batch
        _raises(-6, lambda: b.add_recipes(s, recipes), "batch already ran")
        b.free()

        # one digest with two lengths across packs: MI_ERR_INVALID, and the set answers MI_ERR_STATE from then on
        liar = entries[k:k + 1].copy()
        liar["offset"], liar["length"] = 0, int(entries["length"][k]) // 2 + 1
        assert int(liar["length"][0]) != int(entries["length"][k])
        err = _raises(-1, lambda: s.add_blob(bytes(pc.round16(int(liar["length"][0]))), liar), "another length")
        assert err.first_bad == 0
        _raises(-6, lambda: s.add_blob(blob, entries), "another length")
        with e.batch() as b2:
            _raises(-6, lambda: b2.add_recipes(s, recipes), "another length")
            assert _counts(b2) == (0, 0, 0)
        with pytest.raises(M.MiError):
            s.info


# ---- 6b. the table itself: a conflict inside one add, growth through export and re-insert -----------------------------------------
def test_one_digest_with_two_lengths_in_one_add_is_a_conflict():
    """Two entries of 16 and 17 bytes under one digest, into a fresh set, verify off (digests are opaque).  Both rows probe in
    one launch: one claims the slot, the other meets its own tag there and is the conflict the verify kernel reports -- which of
    the two compare-and-swaps comes first is the hardware's, so the row named is either, with its own length."""
    entries, blob = pc.model_pack([(0, 0, 16), (0, 16, 17)], [bytes(range(33))])
    entries = entries.copy()
    entries["digest"][1] = entries["digest"][0]
    with M.Engine() as e, e.packset() as s:
        err = _raises(-1, lambda: s.add_blob(blob, entries), "another length", "unusable from here on")
        assert err.first_bad in (0, 1) and "entry %d (%d bytes)" % (err.first_bad, 16 + err.first_bad) in str(err), str(err)
        _raises(-6, lambda: s.add_blob(blob, entries), "unusable since", "another length")
        with pytest.raises(M.MiError):
            s.info


def test_a_set_grows_through_export_and_re_insert():
    """A fresh set has 1 024 slots and stays under half full: 513 entries grow it empty, 513 more grow it through the export of
    what it holds and their re-insert.  Every digest is found afterwards, by the want list and by a restore."""
    data = np.random.default_rng(48).integers(0, 256, 1026 * 16, dtype=np.uint8).tobytes()
    halves = [pc.model_pack([(0, 16 * i, 16) for i in range(k, k + 513)], [data]) for k in (0, 513)]
    dig = np.ascontiguousarray(np.concatenate([en["digest"] for en, _ in halves]))
    assert len({bytes(d) for d in dig}) == 1026
    with M.Engine() as e, e.packset() as s, e.batch() as b:
        for en, bl in halves:
            s.add_blob(bl, en)
        assert (s.info.n_digests, s.info.n_entries, s.info.n_packs) == (1026, 1026, 2)
        held, want, info = s.missing(dig)
        assert held.all() and len(want) == 0 and info.n_want == 0
        pick = [0, 512, 1025]                                    # the first, the 513th and the last
        b.add_recipes(s, [(dig[pick], np.full(3, 16, dtype=np.uint32))], verify=True)
        b.run()
        assert b.read_file(0, 0, 48) == b"".join(data[16 * k:16 * k + 16] for k in pick)


# ---- 7. the flags are what catches damage -----------------------------------------------------------------------------------
def test_only_the_flags_catch_a_damaged_blob():
    rng = np.random.default_rng(48)
    files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in EDGE_SIZES]
    with M.Engine() as e0, e0.batch() as b0:                           # the engine's own cuts: the recipes' roots are the files'
        for i, x in enumerate(files):
            b0.add_bytes(x, i)
        b0.run()
        rows, roots0 = pc.rows_of(b0.chunks()), b0.roots().copy()
        with b0.pack() as p:
            entries, blob = p.entries().copy(), p.bytes()
    recipes = _recipes(rows, files)
    assert [M.chunk_root(d) for d, _ in recipes] == [r.tobytes() for r in roots0]
    k = next(i for i in range(len(entries) // 2, len(entries)) if int(entries["length"][i]) % 16 and int(entries["length"][i]) > 16)
    off, length = int(entries["offset"][k]), int(entries["length"][k])
    flipped = bytearray(blob)
    flipped[off + length // 2] ^= 0x10
    flipped = bytes(flipped)
    padded = bytearray(blob)
    padded[off + pc.round16(length) - 1] = 0x80
    padded = bytes(padded)
    assert M.pack_check(flipped, entries) == k and M.pack_check(padded, entries) == k
    f, at = rows[k][0], rows[k][1]                                     # the file and the place the damaged chunk belongs to
    row_in_file = sum(1 for fi, o, _ in rows if fi == f and o < at)
    with M.Engine() as e:
        # with MI_PACKSET_VERIFY the set refuses it and names the entry mi_pack_check names
        with e.packset() as s:
            for damaged in (flipped, padded):
                with pytest.raises(M.MiError) as ei:
                    s.add_blob(damaged, entries, verify=True)
                assert ei.value.code == -1 and ei.value.first_bad == k
                assert (s.info.n_packs, s.info.n_digests) == (0, 0)
        # without it, MI_RECIPE_VERIFY refuses the files: MI_ERR_IO naming file and row; a pad byte is no file's byte
        with e.packset() as s, e.batch() as b:
            s.add_blob(flipped, entries)
            with pytest.raises(M.MiError) as ei:
                b.add_recipes(s, recipes, verify=True)
            assert ei.value.code == -5 and "file %d, row %d " % (f, row_in_file) in str(ei.value) and "arena offset" in str(ei.value)
            assert b.counts() == (0, 0, 0)
            # with neither the call succeeds: exactly that byte is flipped, and the file's root is not the recipe's
            b.add_recipes(s, recipes)
            b.run()
            want = bytearray(files[f])
            want[at + length // 2] ^= 0x10
            for i, x in enumerate(files):
                assert b.read_file(i, 0, len(x)) == (bytes(want) if i == f else x), i
            roots = b.roots()
            for i in range(len(files)):
                assert (roots[i].tobytes() == roots0[i].tobytes()) == (i != f), i
        with e.packset() as s, e.batch() as b:
            s.add_blob(padded, entries)
            b.add_recipes(s, recipes, verify=True)
            b.run()
            for i, x in enumerate(files):
                assert b.read_file(i, 0, len(x)) == x, i


# ---- 8. a commit, taken apart and put back ----------------------------------------------------------------------------------
def test_commits_taken_apart_come_back_as_the_same_layers_on_another_engine(tmp_path):
    root = str(tmp_path / "root")
    files = make_tree(root, seed=23, n_dirs=4, files_per_dir=6, mtime=MTIME)
    kept = []                                                          # per commit: host copies only
    with M.Engine() as eng, M.MemFS(root) as fs, M.ChunkIndex(eng) as ix:
        fs.set_index(ix)
        fs.set_options(chunk_pack=True)

        def commit(name):
            r, raw = commit_to_bytes(fs, tmp_path, name + ".tar", must_scan=True, engine=eng)
            with fs.take_pack() as p:
                kept.append({"entries": p.entries().copy(), "blob": p.bytes(), "layer": r["layer"], "tar_digest": r["tar_digest"],
                             "tar_bytes": r["tar_bytes"]})

        commit("c1")                                                   # all new
        names = sorted(files)
        for rel in names[1::5]:                                        # some files rewritten (same size, same second)
            new = bytes(x ^ 0x33 for x in files[rel][:4000]) + files[rel][4000:]
            write_file(os.path.join(root, rel), new, mtime=MTIME)
            files[rel] = new
        commit("c2")
        rng = np.random.default_rng(24)
        for i, size in enumerate((1, 5000, 123_457)):                  # some added
            write_file(os.path.join(root, "added/n%d.bin" % i), rng.integers(0, 256, size, dtype=np.uint8).tobytes(), mtime=MTIME)
        os.utime(os.path.join(root, "added"), (MTIME, MTIME))
        commit("c3")
        fs.release_device()
    assert [sum(1 for x in c["layer"] if x["kind"] == M.KIND_FILE) > 0 for c in kept] == [True] * 3
    assert len(kept[1]["blob"]) < len(kept[0]["blob"]) and len(kept[2]["entries"]) > 0

    with M.Engine() as eng2, eng2.packset() as s:
        for c in kept:
            s.add_blob(c["blob"], c["entries"], verify=True)
        for c in kept:
            regular = [x for x in c["layer"] if x["kind"] == M.KIND_FILE]
            with eng2.batch() as b:
                st = b.add_recipes(s, [x.get("chunks", []) for x in regular], verify=True)
                assert st.n_files == len(regular) and st.bytes == sum(x["size"] for x in regular)
                b.run()
                roots = b.roots()
                with M.Layer(gzip_level=M.GZIP_OFF) as layer:
                    i = 0
                    for x in c["layer"]:                               # the commit's own entries, in their order
                        if x["kind"] == M.KIND_FILE:
                            assert roots[i].tobytes() == x["root"], x["relpath"]
                            layer.add_batch_file(x, b, i)
                            i += 1
                        else:
                            layer.add(x)
                    res = layer.finish()
                assert res["tar_digest"] == c["tar_digest"] and res["tar_bytes"] == c["tar_bytes"]


# ---- 9. destinations past 2^32 ------------------------------------------------------------------------------------------------
def test_destinations_past_four_gib():
    nf = 4097
    # the guard, before any work and on the device's free memory alone: the arena (4 GiB + 1 MiB + the restored files, hinted: one
    # allocation), the tables of ~520 000 chunk rows (well under 0.5 GiB).  From here on every error of the engine fails the test
    assert torch is not None, "the guard asks torch for the device's free memory"
    free_b = int(torch.cuda.mem_get_info()[0])
    if free_b < (6 << 30):
        pytest.skip("the device has %.1f GiB free, the test needs 6" % (free_b / 2.0 ** 30))
    files, rows, entries, blob, recipes = _edge_case(49)
    # the condition the test rests on: files lie in the arena in add order, a 1 MiB file fills its slot: every restored
    # destination lies past 2^32
    assert nf * MIB > 1 << 32
    with M.Engine() as e, e.packset() as s:
        s.add_blob(blob, entries)
        b = e.batch(nf + len(files), nf * MIB + sum(EDGE_SIZES) + 4096 * len(files))
        with b:
            b.add_synthetic([MIB] * nf)
            st = b.add_recipes(s, recipes, verify=True)
            assert st.n_joined_units == rc.joined_units(recipes)
            b.run()
            for i, x in enumerate(files):
                assert b.read_file(nf + i, 0, len(x)) == x, i
            fr = b.files()
            assert fr["size"][nf:].tolist() == EDGE_SIZES
            with e.batch() as plain:                                                         # the roots of the same bytes, host-fed
                for i, x in enumerate(files):
                    plain.add_bytes(x, i)
                plain.run()
                assert np.array_equal(plain.files()["chunk_root"], fr["chunk_root"][nf:])


# ---- 10. the read bound, checked by the hardware --------------------------------------------------------------------------------
# The bound, from the code (csrc/mi_restore.hip restore_tile): every load of the assemble kernel is 16 bytes long and begins at
# src + a, src the device address of a blob's entry and 0 <= a < len.  So (1) no load begins in front of its entry, hence none in
# front of the blob -- the head of a row that begins inside a unit is loaded from the row's own first byte (a = 0) and shifted
# into place, never from src - (its place in the unit); (2) a load ends at src + a + 15 <= src + len + 14 <= src +
# round16(len) + 15: at most 15 bytes behind offset + round16(length) <= blob_bytes (the structural check), inside the 256
# bytes of slack every blob is allocated with.  The hashing of both verify passes reads up to 67 bytes behind its last item:
# the blob's 256 bytes, the arena's 4 KiB.  Under MI_GUARD_ALLOC=1 every device allocation holds exactly the bytes asked for
# and ends on an unmapped page (tests/test_gpu_overread.py); the batch is reserved exactly.  No positive control: a deliberate
# fault has no place on a shared box.
OVERREAD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import makisu_amd as M
import pack_cases as pc
import restore_cases as rc
rng = np.random.default_rng(50)
lens = [300, 5, 77, 1000, 33, 47, 64]           # the last three: 1, 15 and 0 mod 16; the last ends on the blob's last unit
data = rng.integers(0, 256, sum(lens), dtype=np.uint8).tobytes()
rows, at = [], 0
for n in lens:
    rows.append((0, at, n))
    at += n
entries, blob = pc.model_pack(rows, [data])
assert int(entries["offset"][0]) == 0 and int(entries["offset"][-1]) + 64 == len(blob)
dig = np.ascontiguousarray(entries["digest"])
L = np.array(lens, dtype=np.uint32)
# file 0: entry 0 (at the blob's first byte) begins 5 bytes into a unit -- its head is fetched for a joined unit -- and every
# later row, the last three entries among them, lies at a destination that is not a multiple of 16: loads at every a mod 16
order0 = [1, 0, 4, 5, 6, 2, 6, 5, 4]
# file 1: the last entry alone, aligned; file 2: the three last entries, each begun inside a unit
order1, order2 = [6], [2, 4, 5, 6]
recipes = [(dig[o], L[o]) for o in (order0, order1, order2)]
want = rc.model_restore([(entries, blob)], recipes)
with M.Engine() as e, e.packset() as s:
    s.add_blob(blob, entries, verify=True)
    b = e.batch()
    b.reserve(len(want), sum((len(x) + 255) // 256 * 256 for x in want[:-1]) + len(want[-1]))
    st = b.add_recipes(s, recipes, verify=True)
    assert st.n_joined_units == rc.joined_units(recipes) > 0
    b.run()
    for i, x in enumerate(want):
        assert b.read_file(i, 0, len(x)) == x, i
    b.free()
print("joined", st.n_joined_units, flush=True)
print("OK")
"""


def test_no_assemble_load_leaves_its_blob(tmp_path):
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", OVERREAD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout[-1500:] + p.stderr[-3000:]
