"""GPU tests of the chunk fetch (mi_packset_missing, mi_packset_pack): what a pack set answers about a request's digests and
the pack it cuts for a request are compared, every byte and every counter, with the pure-Python model of fetch_cases.py --
chunks of every length residue from several packs in any order, planted tile edges over a source whose pad bytes are not zero,
requests that repeat every digest, the plan's block boundaries, keys that collide in the table, everything that is refused,
a damaged source with and without the verification flag, the three-step protocol between two engines, and the read bound
under the guard allocator.  Bit for bit: there are no tolerances."""
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
import fetch_cases as fc  # noqa: E402
import pack_cases as pc  # noqa: E402
import restore_cases as rc  # noqa: E402
from commit_cases import commit_to_bytes, make_tree, write_file  # noqa: E402

pytestmark = pytest.mark.gpu
MTIME = 1_600_000_000
MIB = 1 << 20
COUNTERS = ("n_rows", "n_distinct", "n_held", "n_want", "held_bytes", "want_bytes")


def _same_pack(pack, want_entries, want_blob, alg=None):
    """entries, blob and info of a Pack against the model's; -> (entries, blob)"""
    entries, blob, info = pack.entries(), pack.bytes(), pack.info
    assert pc.same_entries(entries, want_entries)
    assert blob == want_blob
    assert (info.n_entries, info.blob_bytes, info.chunk_bytes) == (len(want_entries), len(want_blob), int(want_entries["length"].sum()))
    if alg is not None:
        assert info.alg == alg and M.pack_check(blob, entries, alg=alg) is None
    return entries, blob


def _same_missing(got, want):
    held, rows, info = got
    w_held, w_rows, w_info = want
    assert np.array_equal(held, w_held) and held.dtype == np.uint8
    assert np.array_equal(rows, w_rows) and rows.dtype == np.uint64
    assert {k: getattr(info, k) for k in COUNTERS} == w_info
    assert info.ms_resolve > 0


def _raises(code, call, *needles):
    with pytest.raises(M.MiError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)
    return ei.value


# ---- 1. residues and order --------------------------------------------------------------------------------------------------
def test_every_digest_of_three_packs_in_shuffled_and_in_reverse_order():
    rng = np.random.default_rng(71)
    data = rng.integers(0, 256, MIB, dtype=np.uint8).tobytes()
    with M.Engine(mask_bits=6, min_size=64, max_size=1024) as e, e.batch() as b, e.packset() as s:
        b.add_bytes(data, 0)
        b.run()
        chunks = b.chunks().copy()
        rows = pc.rows_of(chunks)
        n = len(rows)
        assert n > 8000 and {k % 16 for _, _, k in rows} == set(range(16))
        host_packs = []
        for k in range(3):                                                               # three disjoint packs
            with b.pack(select=(np.arange(n) % 3 == k).astype(np.uint8)) as p:
                host_packs.append((p.entries().copy(), p.bytes()))
                s.add_pack(p, verify=True)
        store = rc.chunk_store(host_packs)
        dig, lens = np.ascontiguousarray(chunks["sha256"]), chunks["length"].astype(np.uint32)
        before = s.info.as_dict()
        last = None
        for verify, order in ((True, rng.permutation(n)), (False, np.arange(n)[::-1])):
            want_e, want_b = fc.model_subpack(store, dig[order], pc.SHA256)
            assert len(want_e) == len(store)
            with s.pack(dig[order], lens[order], verify=verify) as sp:
                last = _same_pack(sp, want_e, want_b, pc.SHA256)
                info = sp.info
                assert info.verified == int(verify) and info.ms_gather > 0 and (info.ms_verify > 0) == verify
        after = s.info.as_dict()
        assert {k: after[k] for k in ("n_packs", "n_entries", "n_digests", "blob_bytes")} == \
            {k: before[k] for k in ("n_packs", "n_entries", "n_digests", "blob_bytes")}
        # a set built from the sub-pack alone restores the file
        with e.packset() as s2, e.batch() as r:
            s2.add_blob(last[1], last[0], verify=True)
            r.add_recipes(s2, [(dig, lens)], verify=True)
            r.run()
            assert r.read_back().tobytes() == data


# ---- 2. tile edges over a source whose pads are not zero ------------------------------------------------------------------------
def test_planted_tile_edges_and_pads_that_the_source_does_not_keep_zero():
    dig, chunks, packs = fc.edge_case()
    store = rc.chunk_store(packs)
    lens = np.array(fc.EDGE_LENGTHS, dtype=np.uint32)
    with M.Engine() as e, e.packset() as s, e.packset() as s2:
        for en, bl in packs:
            s.add_blob(bl, en)                                                           # unverified: fake digests, pads of 0xA5
        for order in (np.arange(len(dig)), np.arange(len(dig))[::-1]):
            want_e, want_b = fc.model_subpack(store, dig[order])
            with s.pack(dig[order], lens[order]) as sp:
                entries, blob = _same_pack(sp, want_e, want_b)
                assert sp.info.verified == 0
                # the pads are zero although the source's are not
                raw = np.frombuffer(blob, dtype=np.uint8)
                for o, k in zip(entries["offset"].tolist(), entries["length"].tolist()):
                    assert not raw[o + k:o + pc.round16(k)].any(), (o, k)
                # ... and the pack is a pack where it lies: another set takes it device to device
                p_dev, p_bytes = sp.device()
                assert p_dev and p_bytes == len(want_b)
                if order[0] == 0:
                    s2.add_pack(sp)
        _same_missing(s2.missing(dig, lens), fc.model_missing(store, dig, lens))
        assert s2.info.n_digests == len(dig)
        with s2.pack(dig[::7]) as sp:                                                    # cut again, from the cut
            _same_pack(sp, *fc.model_subpack(store, dig[::7]))


# ---- 3. repeats and first occurrences --------------------------------------------------------------------------------------------
def test_a_request_that_repeats_every_digest_and_a_set_that_holds_every_third():
    rng = np.random.default_rng(72)
    n = 1500
    dig = fc.fake_digests(rng, n)
    chunks = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(1, 300, n)]
    lens_of = np.array([len(c) for c in chunks], dtype=np.uint32)
    whole = fc.raw_pack(dig, chunks)
    third = fc.raw_pack(dig[::3], chunks[::3])
    req, src = fc.tripled_request(rng, dig)
    lens = lens_of[src]
    assert np.bincount(src).tolist() == [3] * n
    with M.Engine() as e, e.packset() as s_all, e.packset() as s_third:
        s_all.add_blob(*whole[::-1])
        s_third.add_blob(*third[::-1])
        want_e, want_b = fc.model_subpack(rc.chunk_store([whole]), req)
        assert len(want_e) == n and want_e["chunk_index"].tolist() == sorted(int(np.flatnonzero(src == i)[0]) for i in range(n))
        with s_all.pack(req, lens) as sp:
            _same_pack(sp, want_e, want_b)
        store3 = rc.chunk_store([third])
        for ln in (lens, None):
            model = fc.model_missing(store3, req, ln)
            assert model[2]["n_held"] == n // 3 and model[2]["n_want"] == n - n // 3 and (model[2]["want_bytes"] > 0) == (ln is not None)
            _same_missing(s_third.missing(req, ln), model)
        _same_missing(s_all.missing(req, lens), fc.model_missing(rc.chunk_store([whole]), req, lens))    # nothing missing
        # cap = 0 sizes; one row too few is MI_ERR_CAPACITY and writes nothing
        L, info = e._lib, M.WantInfo()
        n_want = n - n // 3
        assert L.mi_packset_missing(s_third._h, req.ctypes.data, lens.ctypes.data, len(req), None, None, 0, C.byref(info)) == 0
        assert info.n_want == n_want and info.n_rows == len(req)
        out = np.full(n_want, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        info2 = M.WantInfo()
        assert L.mi_packset_missing(s_third._h, req.ctypes.data, lens.ctypes.data, len(req), None, out.ctypes.data, n_want - 1, C.byref(info2)) == -7
        assert (out == 0xEEEEEEEEEEEEEEEE).all() and info2.n_want == n_want and b"need %d" % n_want in L.mi_last_error(e._h)
        assert L.mi_packset_missing(s_third._h, req.ctypes.data, lens.ctypes.data, len(req), None, out.ctypes.data, n_want, C.byref(info2)) == 0
        assert np.array_equal(out, model[1])
        # n = 0: all-zero info, the empty pack
        held, rows, info = s_third.missing(np.zeros((0, 32), dtype=np.uint8))
        assert len(held) == 0 and len(rows) == 0 and [getattr(info, k) for k in COUNTERS] == [0] * 6
        with s_third.pack(np.zeros((0, 32), dtype=np.uint8), verify=True) as sp:
            assert len(sp) == 0 and sp.info.blob_bytes == 0 and sp.bytes() == b""


# ---- 4. the plan's boundaries ----------------------------------------------------------------------------------------------------
def _uniform_store(dig, chunks16):
    db, cb = dig.tobytes(), chunks16.tobytes()
    return {db[32 * i:32 * i + 32]: cb[16 * i:16 * i + 16] for i in range(len(dig))}


def test_requests_at_the_plan_blocks_edges_and_one_past_the_second_level():
    rng = np.random.default_rng(73)
    n_held, n_unknown = 590_000, 5_000
    dig = fc.fake_digests(rng, n_held + n_unknown)
    chunks16 = rng.integers(0, 256, (n_held, 16), dtype=np.uint8)
    entries = np.zeros(n_held, dtype=pc.ENTRY_DTYPE)
    entries["digest"], entries["offset"], entries["chunk_index"], entries["length"] = dig[:n_held], np.arange(n_held) * 16, np.arange(n_held), 16
    store = _uniform_store(dig[:n_held], chunks16)
    with M.Engine() as e, e.packset(n_held) as s:
        s.add_blob(chunks16.tobytes(), entries)
        for n in (2047, 2048, 2049):                                                     # one block, exactly, and a second block of one row
            pick = rng.integers(0, n_held, n)
            pick[-5:], pick[7], pick[n // 2] = pick[:5], n_held + 3, n_held + 4          # repeats and unknown digests among them
            lens = np.full(n, 16, dtype=np.uint32)
            _same_missing(s.missing(dig[pick], lens), fc.model_missing(store, dig[pick], lens))
            known = pick[pick < n_held]
            known = np.concatenate([known, rng.integers(0, n_held, n - len(known))])    # n rows again, all held
            with s.pack(dig[known]) as sp:
                _same_pack(sp, *fc.model_subpack(store, dig[known]))
        # 600 000 rows: 293 blocks of 2 048, more than the 256 one pass of the second-level scan takes
        big = np.concatenate([rng.permutation(n_held), rng.integers(0, n_held, 10_000)])
        assert len(big) == 600_000 and len(big) // fc.PLAN_BLOCK > 256
        with s.pack(dig[big]) as sp:
            _same_pack(sp, *fc.model_subpack(store, dig[big]))
        mixed = np.concatenate([big, np.arange(n_held, n_held + n_unknown)])[rng.permutation(600_000 + n_unknown)]
        _same_missing(s.missing(dig[mixed]), fc.model_missing(store, dig[mixed]))


# ---- 5. keys that collide ----------------------------------------------------------------------------------------------------------
def test_digests_that_share_their_first_eight_bytes_are_each_their_own():
    rng = np.random.default_rng(74)
    tag = 0x1122334455667000 | 0x2FF
    firsts = [tag, tag, tag, tag, tag, tag + 1, tag + 2, tag - 1, 0, 1]                  # five with one tag; 0 is stored as 1, next to a real 1
    n = len(firsts)
    dig = np.zeros((n, 32), dtype=np.uint8)
    for k, t in enumerate(firsts):
        dig[k, :8] = np.frombuffer(int(t).to_bytes(8, "little"), dtype=np.uint8)
        dig[k, 8:] = rng.integers(0, 256, 24, dtype=np.uint8)
    assert len({bytes(d) for d in dig}) == n and len({bytes(d[:8]) for d in dig[:5]}) == 1
    chunks = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (100, 100, 37, 64, 1, 250, 16, 90, 33, 47)]
    held = [0, 2, 4, 5, 7, 8]                                                            # of the colliding five: three held, two not; 0-tag held, 1 not
    pack = fc.raw_pack(dig[held], [chunks[k] for k in held])
    store = rc.chunk_store([pack])
    order = [3, 9, 2, 0, 8, 1, 4, 7, 6, 5, 1, 3, 8, 0]
    lens = np.array([len(chunks[k]) for k in order], dtype=np.uint32)
    with M.Engine() as e, e.packset() as s:
        s.add_blob(pack[1], pack[0])
        model = fc.model_missing(store, dig[order], lens)
        assert model[0].tolist() == [int(k in held) for k in order] and model[1].tolist() == [0, 1, 5, 8]
        _same_missing(s.missing(dig[order], lens), model)
        mine = [k for k in order if k in held]
        with s.pack(dig[mine]) as sp:
            entries, blob = _same_pack(sp, *fc.model_subpack(store, dig[mine]))
            for en in entries:                                                           # each digest's own chunk
                k = next(i for i in range(n) if bytes(dig[i]) == bytes(en["digest"]))
                assert blob[int(en["offset"]):int(en["offset"]) + int(en["length"])] == chunks[k]
        err = _raises(-1, lambda: s.pack(dig[order]), "row 0", bytes(dig[3]).hex(), "does not hold")
        assert err.first_bad == 0


# ---- 6. everything refused leaves the set as it was ---------------------------------------------------------------------------------
def test_what_is_refused_leaves_the_set_as_it_was():
    rng = np.random.default_rng(75)
    n = 40
    dig = fc.fake_digests(rng, n + 2)
    chunks = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(20, 500, n)]
    lens = np.array([len(c) for c in chunks], dtype=np.uint32)
    pack = fc.raw_pack(dig[:n], chunks)
    store = rc.chunk_store([pack])
    other = M.Engine()
    s_other = other.packset()
    s_other.add_blob(pack[1], pack[0])
    with M.Engine() as e:
        s = e.packset()
        s.add_blob(pack[1], pack[0])
        info0 = s.info.as_dict()

        def unchanged():
            assert s.info.as_dict() == info0

        # an unknown digest: of two the smaller row is named
        req = dig[:n].copy()
        req[31], req[12] = dig[n], dig[n + 1]
        err = _raises(-1, lambda: s.pack(req, lens), "row 12", bytes(dig[n + 1]).hex(), "does not hold")
        assert err.first_bad == 12 and bytes(dig[n]).hex() not in str(err)
        unchanged()
        # ... which missing answers instead of refusing
        got = s.missing(req, lens)
        assert got[1].tolist() == [12, 31] and got[2].want_bytes == int(lens[12]) + int(lens[31])
        # a stated length that differs; a length of 0 -- for both calls, the same words
        wrong = lens.copy()
        wrong[5] += 1
        for call in (lambda: s.pack(dig[:n], wrong), lambda: s.missing(dig[:n], wrong)):
            _raises(-1, call, "row 5", bytes(dig[5]).hex(), "with %d bytes" % lens[5], "states %d" % wrong[5])
            unchanged()
        wrong = lens.copy()
        wrong[9] = wrong[3] = 0
        for call in (lambda: s.pack(dig[:n], wrong), lambda: s.missing(dig[:n], wrong)):
            _raises(-1, call, "row 3 ", "length 0")
            unchanged()
        assert _raises(-1, lambda: s.pack(dig[:n], wrong)).first_bad == 3
        # repeats of a MISSING digest are not compared with each other
        twice = np.stack([dig[n], dig[n], dig[0]])
        got = s.missing(twice, np.array([10, 20, lens[0]], dtype=np.uint32))
        assert got[1].tolist() == [0] and got[2].want_bytes == 10 and got[0].tolist() == [0, 0, 1]
        # unknown flags, 2^32 rows, NULL arguments with a live set
        L, out, bad = e._lib, C.c_void_p(), C.c_uint64()
        assert L.mi_packset_pack(s._h, dig.ctypes.data, None, 1, 0x2, C.byref(out), C.byref(bad)) == -1 and b"unknown flags" in L.mi_last_error(e._h)
        assert L.mi_packset_pack(s._h, dig.ctypes.data, None, 1 << 32, 0, C.byref(out), C.byref(bad)) == -1 and b"2^32" in L.mi_last_error(e._h)
        assert L.mi_packset_missing(s._h, dig.ctypes.data, None, 1 << 32, None, None, 0, None) == -1
        assert L.mi_packset_pack(s._h, None, None, 1, 0, C.byref(out), None) == -1
        assert L.mi_packset_pack(s._h, dig.ctypes.data, None, 1, 0, None, None) == -1
        assert L.mi_packset_missing(s._h, None, None, 1, None, None, 0, None) == -1
        assert L.mi_packset_missing(s._h, dig.ctypes.data, None, 1, None, None, 3, None) == -1        # room without a buffer
        unchanged()
        # the set of an engine whose sibling engine -- with a set of its own over the same pack -- is gone serves on
        s_other.close()
        other.close()
        _same_missing(s.missing(dig[:n], lens), fc.model_missing(store, dig[:n], lens))
        # the pack outlives its set, and mi_ctx_destroy refuses while it lives
        sp = s.pack(dig[:n][::-1], lens[::-1], verify=False)
        want_e, want_b = fc.model_subpack(store, dig[:n][::-1])
        unchanged()
        s.close()
        _same_pack(sp, want_e, want_b)
        assert L.mi_ctx_destroy(e._h) == -6 and b"still alive" in L.mi_last_error(e._h)
        sp.close()

        # a set in its sticky failed state: MI_ERR_STATE with the first message, for both calls
        s = e.packset()
        s.add_blob(pack[1], pack[0])
        liar = pack[0][7:8].copy()
        liar["offset"], liar["length"] = 0, int(lens[7]) + 3
        _raises(-1, lambda: s.add_blob(bytes(pc.round16(int(lens[7]) + 3)), liar), "another length")
        _raises(-6, lambda: s.pack(dig[:n]), "unusable since", "another length")
        _raises(-6, lambda: s.missing(dig[:n]), "unusable since", "another length")
        s.close()


# ---- 7. only the flag catches damage ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", [pc.SHA256, pc.BLAKE2S])
def test_only_the_flag_catches_a_damaged_source(alg):
    rng = np.random.default_rng(76)
    files = [rng.integers(0, 256, 50_000, dtype=np.uint8).tobytes()]
    rows = pc.random_cut_rows(rng, files, 20, 700)
    entries, blob = pc.model_pack(rows, files, None, alg)
    assert len({bytes(d) for d in entries["digest"]}) == len(entries)                     # an entry's index is its request row
    k = next(i for i in range(len(entries) // 2, len(entries)) if int(entries["length"][i]) > 16)
    off, length = int(entries["offset"][k]), int(entries["length"][k])
    flipped = bytearray(blob)
    flipped[off + length // 2] ^= 0x10
    flipped = bytes(flipped)
    assert M.pack_check(flipped, entries, alg=alg) == k and M.pack_check(blob, entries, alg=alg) is None
    order = np.random.default_rng(77).permutation(len(entries))
    req = np.ascontiguousarray(entries["digest"][order])
    row = int(np.flatnonzero(order == k)[0])                                             # where the damaged chunk is asked for
    with M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0) as e, e.packset() as s:
        s.add_blob(flipped, entries)                                                     # without MI_PACKSET_VERIFY
        with s.pack(req) as sp:                                                          # without the flag: a pack, and it is damaged
            got_e, got_b = sp.entries(), sp.bytes()
            assert sp.info.verified == 0 and sp.info.alg == alg
        assert M.pack_check(got_b, got_e, alg=alg) == row
        want_e, want_b = fc.model_subpack(rc.chunk_store([(entries, flipped)]), req)
        assert pc.same_entries(got_e, want_e) and got_b == want_b
        err = _raises(-5, lambda: s.pack(req, verify=True), "row %d " % row, "source address", "blob offset %d" % int(got_e["offset"][row]),
                      bytes(entries["digest"][k]).hex())
        assert err.first_bad == row
        # the same request over the sound blob passes with the flag
        with e.packset() as s2:
            s2.add_blob(blob, entries, verify=True)
            with s2.pack(req, verify=True) as sp:
                _same_pack(sp, *fc.model_subpack(rc.chunk_store([(entries, blob)]), req, alg), alg)
                assert sp.info.verified == 1 and sp.info.ms_verify > 0


# ---- 8. the protocol end to end, on two engines ---------------------------------------------------------------------------------------
def test_a_puller_fetches_only_what_it_lacks_and_rebuilds_the_layer(tmp_path):
    root = str(tmp_path / "root")
    make_tree(root, seed=29, n_dirs=4, files_per_dir=6, mtime=MTIME)
    rng = np.random.default_rng(30)
    first = rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes()
    write_file(os.path.join(root, "added/first.bin"), first, mtime=MTIME)
    os.utime(os.path.join(root, "added"), (MTIME, MTIME))
    kept = []                                                          # per commit: host copies only
    with M.Engine() as eng, M.MemFS(root) as fs, M.ChunkIndex(eng) as ix:
        fs.set_index(ix)
        fs.set_options(chunk_pack=True)

        def commit(name):
            r, raw = commit_to_bytes(fs, tmp_path, name + ".tar", must_scan=True, engine=eng)
            with fs.take_pack() as p:
                kept.append({"entries": p.entries().copy(), "blob": p.bytes(), "layer": r["layer"], "tar_digest": r["tar_digest"],
                             "tar_bytes": r["tar_bytes"], "chunk_bytes": p.info.chunk_bytes})

        commit("c1")                                                   # all new
        fresh = rng.integers(0, 256, 400_000, dtype=np.uint8).tobytes()
        write_file(os.path.join(root, "added/second.bin"), fresh, mtime=MTIME)
        os.utime(os.path.join(root, "added"), (MTIME, MTIME))
        commit("c2")                                                   # one new file: 400 000 bytes the first commit did not hold
        # the planted file of the third commit: bytes of the FIRST commit (the puller holds their chunks), HALF of the second
        # commit's file (chunks only the server holds, in a pack that holds the other half too) and bytes nobody holds
        third = first + fresh[:200_000] + rng.integers(0, 256, 50_000, dtype=np.uint8).tobytes()
        write_file(os.path.join(root, "added/third.bin"), third, mtime=MTIME)
        os.utime(os.path.join(root, "added"), (MTIME, MTIME))
        commit("c3")
        fs.release_device()
    layer3 = kept[2]["layer"]
    regular = [x for x in layer3 if x["kind"] == M.KIND_FILE]
    recipes = [x.get("chunks", []) for x in regular]
    assert [x["relpath"] for x in regular] == ["added/third.bin"] and len(recipes[0]) > 20
    req = np.frombuffer(b"".join(d for d, _ in recipes[0]), dtype=np.uint8).reshape(-1, 32)      # the layer's recipes end to end
    lens = np.array([k for _, k in recipes[0]], dtype=np.uint32)
    # what the planted tree guarantees, from the host copies: the layer needs chunks of all three packs, and the second pack
    # holds chunks the layer does not need -- so the packs that hold a missing chunk are strictly more than the missing chunks
    need = {bytes(d) for d in req}
    in_pack = [{bytes(d) for d in c["entries"]["digest"]} for c in kept]
    assert all(len(need & p) > 3 for p in in_pack) and len(in_pack[1] - need) > 3 and need <= in_pack[0] | in_pack[1] | in_pack[2]
    whole_packs = kept[1]["chunk_bytes"] + kept[2]["chunk_bytes"]
    stores = rc.chunk_store([(c["entries"], c["blob"]) for c in kept])

    with M.Engine() as server, M.Engine() as puller, server.packset() as s_srv, puller.packset() as s_pull:
        for c in kept:
            s_srv.add_blob(c["blob"], c["entries"], verify=True)
        s_pull.add_blob(kept[0]["blob"], kept[0]["entries"], verify=True)
        # puller: recipes -> want list
        held, want_rows, info = s_pull.missing(req, lens)
        _same_missing((held, want_rows, info), fc.model_missing(rc.chunk_store([(kept[0]["entries"], kept[0]["blob"])]), req, lens))
        assert 0 < info.n_want < info.n_distinct
        want = want_rows.astype(np.int64)
        # server: want list -> one pack of exactly those chunks, from two packs
        with s_srv.pack(req[want], lens[want], verify=True) as sp:
            sub_e, sub_b = _same_pack(sp, *fc.model_subpack(stores, req[want], pc.SHA256), pc.SHA256)
            assert sp.info.chunk_bytes == info.want_bytes < whole_packs
            assert {bytes(d) for d in sub_e["digest"]} & in_pack[1] and {bytes(d) for d in sub_e["digest"]} & in_pack[2]
        # puller: the pack in, the layer out
        s_pull.add_blob(sub_b, sub_e, verify=True)
        assert s_pull.missing(req, lens)[2].n_want == 0
        with puller.batch() as b:
            st = b.add_recipes(s_pull, recipes, verify=True)
            assert st.n_files == 1 and st.bytes == len(third)
            b.run()
            assert b.read_file(0, 0, len(third)) == third
            roots = b.roots()
            with M.Layer(gzip_level=M.GZIP_OFF) as layer:
                i = 0
                for x in layer3:                                       # the commit's own entries, in their order
                    if x["kind"] == M.KIND_FILE:
                        assert roots[i].tobytes() == x["root"], x["relpath"]
                        layer.add_batch_file(x, b, i)
                        i += 1
                    else:
                        layer.add(x)
                res = layer.finish()
            assert res["tar_digest"] == kept[2]["tar_digest"] and res["tar_bytes"] == kept[2]["tar_bytes"]


# ---- 9. the read bound, checked by the hardware ----------------------------------------------------------------------------------------
# The bound, from the code (csrc/mi_fetch.hip fetch_gather_kernel): a unit's load begins at src + o, src the device address of an
# entry of a resident blob, o a multiple of 16 with 0 <= o < len, and is 16 bytes long: inside [src, src + round16(len)), which
# the structural check of every add keeps inside the source blob.  So no load begins in front of its entry and none ends behind
# its padded span: a chunk that is the LAST entry of its blob and ends on the blob's last unit is read to the blob's last byte
# and not beyond.  The verify pass reads up to 67 bytes behind the NEW blob's last entry: inside the 256 bytes of slack it is
# allocated with.  Under MI_GUARD_ALLOC=1 every device allocation ends on an unmapped page (tests/test_gpu_overread.py).  No
# positive control: a deliberate fault has no place on a shared box.
OVERREAD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import makisu_amd as M
import fetch_cases as fc
import pack_cases as pc
import restore_cases as rc
rng = np.random.default_rng(78)
packs, last = [], []
for tail in (33, 47, 64):                       # 1, 15 and 0 mod 16: each the last entry of a blob of its own, ending on its last unit
    lens = [300, 5, 77, 1000, tail]
    data = rng.integers(0, 256, sum(lens), dtype=np.uint8).tobytes()
    rows, at = [], 0
    for n in lens:
        rows.append((0, at, n))
        at += n
    entries, blob = pc.model_pack(rows, [data])
    assert int(entries["offset"][-1]) + pc.round16(tail) == len(blob) and int(entries["offset"][0]) == 0
    packs.append((entries, blob))
    last.append(entries["digest"][-1])
store = rc.chunk_store(packs)
firsts = [p[0]["digest"][0] for p in packs]      # ... and each blob's first entry, at the allocation's first byte
req = np.ascontiguousarray(np.stack(last + firsts + last[::-1]))
with M.Engine() as e, e.packset() as s:
    for entries, blob in packs:
        s.add_blob(blob, entries, verify=True)
    for r in (req, req[2:3], req[::-1]):        # the 64-byte tail alone: the new blob's last unit is its last load too
        want_e, want_b = fc.model_subpack(store, r, pc.SHA256)
        with s.pack(r, verify=True) as sp:
            assert pc.same_entries(sp.entries(), want_e) and sp.bytes() == want_b
    held, rows, info = s.missing(req)
    assert held.all() and info.n_want == 0 and info.n_distinct == 6
print("OK")
"""


def test_no_gather_load_leaves_its_entrys_padded_span(tmp_path):
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", OVERREAD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout[-1500:] + p.stderr[-3000:]
