"""GPU tests of the zpacks coded straight from the arena (mi_batch_zpack_chunks, MI_MEMFS_CHUNK_ZPACK, mi_memfs_take_zpack) and of
mi_zset_missing.  A zpack is compared, entries and every byte of the blob, with the model of zbatch_cases.py -- pack_cases' model
handed to zpack_cases', no new coder -- AND with b.pack(sel).compress() in the same process, and it must pass M.zpack_check: raw
and coded sources side by side at every residue, the coder's edges read from the arena, selections at the scan's block edges, the
second trip of the encode launch, arena offsets past 2^32, lifetime, everything that is refused, the commit, the want list over
a compressed set against the plain set's, and the bounds under the guard allocator.  Bit for bit: there are no tolerances."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (before the engine, as in test_gpu_chunk_pack.py: the 5 GiB test asks it for the device's free memory)
except ImportError:          # CPU-only collection without torch: the GPU tests are skipped anyway
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import fetch_cases as fc  # noqa: E402
import pack_cases as pc  # noqa: E402
import restore_cases as rc  # noqa: E402
import zbatch_cases as bc  # noqa: E402
import zpack_cases as zc  # noqa: E402
import zset_cases as qc  # noqa: E402
from commit_cases import commit_to_bytes, make_tree, write_file  # noqa: E402

pytestmark = pytest.mark.gpu
ALGS = [pc.SHA256, pc.BLAKE2S]
MTIME = 1_600_000_000
MIB = 1 << 20
COUNTERS = ["n_rows", "n_distinct", "n_held", "n_want", "held_bytes", "want_bytes"]


def _engine(alg, **kw):
    return M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0, **kw)


def _raises(code, call, *needles):
    with pytest.raises(M.MiError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)
    return ei.value


def _children(e):
    """how many children (batches, packs, zpacks, sets ...) the engine's ctx counts: mi_ctx_destroy refuses and says so"""
    assert e._lib.mi_ctx_destroy(e._h) == -6
    return int(re.search(rb"(\d+) batch", e._lib.mi_last_error(e._h)).group(1))


def _check(b, rows, files, select=None, alg=pc.SHA256, verify=True, existing=True):
    """b.zpack(select) against the model and against b.pack(select).compress(); -> (entries, blob)"""
    want_e, want_b = bc.model_zpack(rows, files, select, alg)
    with b.zpack(select, verify=verify) as z:
        got_e, got_b, info = z.entries().copy(), z.read(), z.info
    assert bc.same_zentries(got_e, want_e), [k for k in range(min(len(got_e), len(want_e))) if got_e[k] != want_e[k]][:10]
    assert got_b == want_b, next(i for i in range(max(len(want_b), len(got_b))) if i >= min(len(got_b), len(want_b)) or got_b[i] != want_b[i])
    assert (info.n_entries, info.blob_bytes, info.chunk_bytes, info.stored_bytes, info.n_raw, info.verified, info.alg) == \
        (len(want_e), len(want_b), int(want_e["length"].sum()), int(want_e["stored"].sum()),
         int((want_e["stored"] == want_e["length"]).sum()), int(verify), alg)
    if len(want_e):
        assert info.ms_encode > 0 and info.ms_compact > 0 and (info.ms_verify > 0) == verify and (info.ms_decode > 0) == verify
    if existing:
        with b.pack(select) as p, p.compress() as old:
            assert old.read() == got_b and bc.same_zentries(old.entries(), got_e)
    assert M.zpack_check(got_b, got_e, alg=alg) is None
    return got_e, got_b


# ---- 1. every source residue, raw and coded side by side --------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_raw_and_coded_sources_at_every_residue_side_by_side(alg):
    data = bc.mixed_file()
    with _engine(alg, mask_bits=6, min_size=64, max_size=1024) as e, e.batch() as b:
        b.add_bytes(data, 0)
        b.run()
        rows = pc.rows_of(b.chunks())
        entries, blob = _check(b, rows, [data], alg=alg, verify=True)
        # the conditions the test rests on (a file begins on a 256-byte boundary of the arena: the offset in the file is the
        # offset in the arena, mod 16)
        coded = bc.kinds(entries)
        start = np.array([rows[int(k)][1] % 16 for k in entries["chunk_index"]])
        assert set(start[~coded].tolist()) == set(range(16)) and set(start[coded].tolist()) == set(range(16))
        assert set((entries["stored"] % 16).tolist()) == set(range(16))
        assert coded.sum() > 100 and (~coded).sum() > 100 and len(bc.tiles_with_both_kinds(entries)) > 0
        again, blob2 = _check(b, rows, [data], alg=alg, verify=False, existing=False)     # without the flag: the same blob, not marked verified
        assert blob2 == blob


# ---- 2. the coder's edges, read from the arena ---------------------------------------------------------------------------------------
def test_the_coders_edges_read_where_the_chunks_lie():
    files = bc.planted_files()
    with M.Engine() as e, e.batch() as b:
        for i, x in enumerate(files):
            b.add_bytes(x, i)
        b.run()
        rows = pc.rows_of(b.chunks())                                  # whatever the cuts are
        short = [i for i, x in enumerate(files) if len(x) < 2048]
        assert all(sum(1 for f, _, _ in rows if f == i) == 1 for i in short)               # under min_size: one row each
        in_last = [(off, n) for f, off, n in rows if f == len(files) - 1]
        assert len(in_last) > 5 and len({off % 16 for off, _ in in_last}) > 3              # the prefix shifts the joined file's chunks
        entries, _ = _check(b, rows, files)
        assert 5 < bc.kinds(entries).sum() < len(entries) - 5


# ---- 3. selections, and entry counts at the scan's block edge -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    data = bc.mixed_file(seed=42, size=640 << 10)
    data += data[:30000]                                              # (the repeat: rows with dup_of >= 0)
    with M.Engine(mask_bits=6, min_size=64, max_size=1024) as e, e.batch() as b:
        b.add_bytes(data, 0)
        b.run()
        chunks = b.chunks().copy()
        yield e, b, [data], chunks, pc.rows_of(chunks)


def _selection(name, chunks):
    n = len(chunks)
    if name.endswith(" entries"):                                     # the layout's scan: its block edge
        return (np.arange(n) >= n - int(name.split()[0])).astype(np.uint8)
    return {"none": np.zeros(n, np.uint8), "every other row": (np.arange(n) % 2 == 0).astype(np.uint8),
            "only row 0": np.eye(1, n, 0, dtype=np.uint8)[0], "only the last row": np.eye(1, n, n - 1, dtype=np.uint8)[0],
            "the two ends": np.eye(1, n, 0, dtype=np.uint8)[0] | np.eye(1, n, n - 1, dtype=np.uint8)[0],
            "dup_of < 0": (chunks["dup_of"] < 0).astype(np.uint8),
            "flags are non-zero bytes, not ones": ((np.arange(n) % 3 == 0) * 0x80).astype(np.uint8)}[name]


@pytest.mark.parametrize("name", ["none", "every other row", "only row 0", "only the last row", "the two ends", "dup_of < 0",
                                  "flags are non-zero bytes, not ones", "%d entries" % (bc.PLAN_BLOCK - 1), "%d entries" % bc.PLAN_BLOCK,
                                  "%d entries" % (bc.PLAN_BLOCK + 1)])
def test_selections(sweep, name):
    e, b, files, chunks, rows = sweep
    assert len(rows) > bc.PLAN_BLOCK + 1 and 0 < (chunks["dup_of"] < 0).sum() < len(rows)
    sel = _selection(name, chunks)
    entries, blob = _check(b, rows, files, select=sel)
    assert len(entries) == int((sel != 0).sum())
    if name == "none":                                                # a valid zpack of nothing
        with b.zpack(select=sel, verify=True) as z:
            assert (z.info.n_entries, z.info.blob_bytes, z.info.verified, z.read(), len(z.entries())) == (0, 0, 1, b"", 0)


# ---- 4. many short rows: the encode launch's second trip -----------------------------------------------------------------------------
def test_more_entries_than_the_encode_launch_has_waves():
    """min_size = max_size = 64: a file of 64 N bytes has exactly N chunks.  The encode launch has 32 768 workgroups (one wave an
    entry): 32 768 + 300 entries send the first 300 workgroups round again, and the scans take 17 blocks"""
    n = bc.ENCODE_GRID + 300
    rng = np.random.default_rng(43)
    pieces = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() if k % 3 else bytes((k + j % (1 + k % 7)) & 255 for j in range(64))
              for k in range(n)]                                       # two of three random (raw), the third a short period (coded)
    data = b"".join(pieces)
    with M.Engine(mask_bits=0, min_size=64, max_size=64) as e, e.batch() as b:
        b.add_bytes(data, 0)
        b.run()
        rows = pc.rows_of(b.chunks())
        assert len(rows) == n and all(r[2] == 64 for r in rows[:100])
        entries, _ = _check(b, rows, [data])
        coded = bc.kinds(entries)
        assert coded[bc.ENCODE_GRID:].any() and (~coded[bc.ENCODE_GRID:]).any()            # both kinds on the second trip


# ---- 5. arena offsets past 4 GiB ----------------------------------------------------------------------------------------------------------
def test_arena_offsets_past_four_gib():
    """a synthetic batch of 5 GiB in 1 MiB files, the last file's rows selected: the chunks the coder reads and the raw entries'
    gather sources lie past 2^32 in the arena (the form of test_gpu_chunk_pack.py's test)"""
    nf = 5 * 1024
    assert torch is not None, "the guard asks torch for the device's free memory"
    free_b = int(torch.cuda.mem_get_info()[0])
    if free_b < (7 << 30):
        pytest.skip("the device has %.1f GiB free, the test needs 7" % (free_b / 2.0 ** 30))
    assert (nf - 1) * MIB > 1 << 32
    with M.Engine() as e:
        b = e.batch(nf, nf * MIB + nf * 4096)
        b.add_synthetic([MIB] * nf)
        b.run()
        files, chunks = b.files(), b.chunks()
        last = nf - 1
        lo, n = int(files[last]["first_chunk"]), int(files[last]["n_chunks"])
        assert lo + n == len(chunks) and n > 10
        sel = np.zeros(len(chunks), np.uint8)
        sel[lo:] = 1
        data = b.read_file(last, 0, MIB)
        entries, blob = _check(b, pc.rows_of(chunks), {last: data}, select=sel)          # the model reads files[file_index]: a dict serves
        assert np.array_equal(entries["chunk_index"], np.arange(lo, lo + n, dtype=np.uint64))
        b.free()


# ---- 6. lifetime ------------------------------------------------------------------------------------------------------------------------
def test_a_zpack_outlives_its_batch_keeps_its_ctx_alive_and_feeds_the_sets():
    data = bc.mixed_file(seed=44, size=300000 // bc.PIECE * bc.PIECE) + b"tail" * 77
    e = M.Engine()
    try:
        b = e.batch()
        b.add_bytes(data, 0)
        b.add_bytes(data[5000:90000], 1)
        b.run()
        rows, chunks, roots = pc.rows_of(b.chunks()), b.chunks().copy(), b.files()["chunk_root"].copy()
        want_e, want_b = bc.model_zpack(rows, [data, data[5000:90000]])
        z1, z2 = b.zpack(), b.zpack(verify=True)                      # neither is read before its batch changes
        b.reset()
        b.add_bytes(bytes(reversed(data)), 0)                         # the arena now holds other bytes
        b.run()
        assert z1.read() == want_b and bc.same_zentries(z1.entries(), want_e)
        b.free()
        assert z2.read() == want_b and bc.same_zentries(z2.entries(), want_e)
        z1.close()
        assert e._lib.mi_ctx_destroy(e._h) == -6 and b"still alive" in e._lib.mi_last_error(e._h)
        assert z2.read(16, 100) == want_b[16:116]                     # ... which is as usable as before
        with e.packset() as ps, e.zset() as zs, e.batch() as t:
            ps.add_zpack(z2, verify=True)
            zs.add_zpack(z2, verify=True)
            distinct = len({bytes(d) for d in want_e["digest"]})
            assert ps.info.n_digests == zs.info.n_digests == distinct
            recipes = []
            for f in (0, 1):
                mine = chunks[chunks["file_index"] == f]
                recipes.append((np.ascontiguousarray(mine["sha256"]), mine["length"].astype(np.uint32)))
            t.add_zrecipes(zs, recipes, verify=True)
            t.run()
            assert np.array_equal(t.files()["chunk_root"], roots)     # the batch rebuilt from it has the original roots
            assert t.read_file(0, 0, len(data)) == data
        z2.close()
    finally:
        e.close()


# ---- 7. the state rules --------------------------------------------------------------------------------------------------------------------
def test_state_rules(tmp_path):
    with M.Engine() as e, e.batch() as b:
        b.add_bytes(zc.text_like(5000, 1), 0)
        kids = _children(e)
        _raises(-6, b.zpack, "must have run")                          # not run
        b.submit()
        _raises(-6, b.zpack, "must have run")                          # in flight
        b.wait()
        chunks = b.chunks().copy()
        n = len(chunks)
        for wrong in (n + 1, n - 1 if n > 1 else 0, 0):
            _raises(-1, lambda: b.zpack(select=np.ones(wrong, np.uint8)), "selection flags")
            assert _children(e) == kids
        out = C.c_void_p(5)
        assert e._lib.mi_batch_zpack_chunks(b._h, None, 0, 0x2, C.byref(out)) == -1 and out.value is None      # an unknown flag
        assert b"unknown flags" in e._lib.mi_last_error(e._h)
        assert e._lib.mi_batch_zpack_chunks(b._h, None, 0, 0, None) == -1
        assert _children(e) == kids and np.array_equal(b.chunks(), chunks)
        with b.zpack(select=np.ones(n, np.uint8)) as z:
            assert z.info.n_entries == n and _children(e) == kids + 1
        assert _children(e) == kids
        b.reset()
        _raises(-6, b.zpack, "must have run")                          # reset: not run again
        assert _children(e) == kids
    # a group head is not reachable through the ABI by itself (test_gpu_chunk_pack.py says why): what a caller can reach is the
    # commit over several ctxs, which refuses the option before anything is walked; and both options at once
    root = str(tmp_path / "root")
    write_file(os.path.join(root, "a"), b"abc" * 1000, mtime=MTIME)
    with M.Engine() as e0, M.Engine() as e1, M.MemFS(root) as fs, M.ChunkIndex(e0) as ix:
        fs.set_index(ix)
        fs.set_options(chunk_zpack=True)
        _raises(-1, lambda: fs.commit_layer(must_scan=True, engine=[e0, e1]), "several GPUs")
        assert fs.commit_stats()["n_walked"] == 0
        _raises(-1, lambda: fs.set_options(chunk_pack=True, chunk_zpack=True), "exclude each other")
        fs.release_device()


# ---- 8. the commit hands over a zpack ----------------------------------------------------------------------------------------------------
def test_the_commit_hands_over_its_zpack_and_its_recipes(tmp_path):
    root = str(tmp_path / "root")
    files = make_tree(root, seed=23, n_dirs=4, files_per_dir=8, mtime=MTIME)
    files["text/notes.txt"] = zc.text_like(60000, 5)                  # (the tree's files are random: this one is coded)
    write_file(os.path.join(root, "text/notes.txt"), files["text/notes.txt"], mtime=MTIME)
    with M.Engine() as eng, M.MemFS(root) as fs, M.MemFS(root) as ref, M.ChunkIndex(eng) as ix, M.ChunkIndex(eng) as ix_ref:
        fs.set_index(ix)
        fs.set_options(chunk_zpack=True)
        ref.set_index(ix_ref)
        ref.set_options(chunk_pack=True)
        _raises(-6, fs.take_zpack, "mi_memfs_take_zpack")              # no commit yet
        seen = set()

        def both(name):
            """the same tree through both handles -> (result, the zpack's entries and blob)"""
            r, raw = commit_to_bytes(fs, tmp_path, name + ".tar", must_scan=True, engine=eng)
            r0, raw0 = commit_to_bytes(ref, tmp_path, name + "_ref.tar", must_scan=True, engine=eng)
            assert raw == raw0 and r["tar_digest"] == r0["tar_digest"]                     # the same layer TarDigest
            assert [(x["relpath"], x.get("root"), x.get("chunks")) for x in r["layer"]] == \
                [(x["relpath"], x.get("root"), x.get("chunks")) for x in r0["layer"]]       # the same recipes
            assert r["stats"]["index_new_bytes"] == r0["stats"]["index_new_bytes"]
            with fs.take_zpack() as z, ref.take_pack() as p:
                assert z.info.verified == 1 or z.info.n_entries == 0
                ze, zb = z.entries().copy(), z.read()
                want_e, want_b = zc.model_compress(p.entries(), p.bytes())
            assert zb == want_b and bc.same_zentries(ze, want_e)
            assert M.zpack_check(zb, ze) is None
            assert int(ze["length"].sum()) == r["stats"]["index_new_bytes"]
            for d in ze["digest"]:
                assert bytes(d) not in seen, "a chunk an earlier zpack held"
                seen.add(bytes(d))
            _raises(-6, fs.take_zpack, "since the last")               # taken: the second take has nothing
            _raises(-6, fs.take_pack)                                  # ... and this handle makes no plain pack
            return r, ze, zb

        r, ze, zb = both("c1")                                         # commit 1, all new
        assert len(ze) > 30 and 0 < bc.kinds(ze).sum() < len(ze)
        r, ze, zb = both("c2")                                         # commit 2, nothing changed: the empty layer, the empty zpack
        assert r["n_entries"] == 0 and len(ze) == 0 and zb == b""
        rel = "text/notes.txt"                                         # commit 3: one file rewritten in its middle, same size, same second
        old = files[rel]
        new = old[:30000] + bytes(x ^ 0x5A for x in old[30000:33000]) + old[33000:]
        write_file(os.path.join(root, rel), new, mtime=MTIME)
        r, ze, zb = both("c3")                                         # (asserts: only chunks that no earlier zpack held)
        assert [x["relpath"] for x in r["layer"] if x["kind"] == 1] == [rel] and 0 < int(ze["length"].sum()) < len(new)
        # a zpack nobody took is freed by the next commit
        write_file(os.path.join(root, rel), old, mtime=MTIME)
        kids = _children(eng)
        assert fs.commit_layer(must_scan=True, engine=eng) is not None and _children(eng) == kids + 1
        write_file(os.path.join(root, rel), new, mtime=MTIME)
        assert fs.commit_layer(must_scan=True, engine=eng) is not None and _children(eng) == kids + 1
        fs.take_zpack().close()
        assert _children(eng) == kids
        fs.release_device()
        ref.release_device()
    with M.Engine() as eng, M.MemFS(root) as fs:                       # the option without an index: MI_ERR_STATE before anything is walked
        fs.set_options(chunk_zpack=True)
        _raises(-6, lambda: fs.commit_layer(must_scan=True, engine=eng), "index")
        assert fs.commit_stats()["n_walked"] == 0
        fs.release_device()


WINDOWED = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import makisu_amd as M
from commit_cases import make_tree
root = os.path.join(sys.argv[1], "root")
make_tree(root, seed=22, n_dirs=3, files_per_dir=8)
with M.Engine() as eng, M.MemFS(root) as fs, M.ChunkIndex(eng) as ix:
    fs.set_index(ix)
    fs.set_options(chunk_zpack=True)
    res = fs.commit_layer(must_scan=True, engine=eng)
    assert res["stats"]["n_windows"] >= 1 and res["n_entries"] > 20, res["stats"]
    try:
        fs.take_zpack()
        raise SystemExit("a windowed commit handed over a zpack")
    except M.MiError as err:
        assert err.code == -6 and "windows" in str(err), str(err)
    assert all("chunks" not in x for x in res["layer"])
    fs.release_device()
print("OK windowed")
"""


def test_a_commit_in_windows_succeeds_and_has_no_zpack(tmp_path):
    assert 'getenv("MI_COMMIT_FORCE_WINDOWS")' in open(os.path.join(ROOT, "makisu_amd", "csrc", "mi_commit.hip")).read()   # the knob exists
    env = dict(os.environ, MI_COMMIT_FORCE_WINDOWS="1", MI_COMMIT_WINDOW_MB="1")
    p = subprocess.run([sys.executable, "-c", WINDOWED % {"root": ROOT}, str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK windowed" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]


# ---- 9. the want list over a compressed set ------------------------------------------------------------------------------------------------
def _same_missing(got, want):
    held, rows, info = got
    w_held, w_rows, w_info = want
    assert np.array_equal(held, w_held) and held.dtype == np.uint8
    assert np.array_equal(rows, w_rows) and rows.dtype == np.uint64
    for k in COUNTERS:
        assert getattr(info, k) == (w_info[k] if isinstance(w_info, dict) else getattr(w_info, k)), k


def test_a_zset_answers_the_want_list_as_the_plain_set_does():
    chunks = [c for _, c, _ in zc.planted_chunks()]
    n = len(chunks)
    dig = qc.digests_of(chunks)
    groups = [list(range(0, n, 3)), list(range(1, n, 3)) + [0]]        # two packs hold two thirds; chunk 0 lies in both
    plain = [zc.pack_of([chunks[k] for k in g]) for g in groups]
    zpacks = [zc.model_compress(*p) for p in plain]
    store = rc.chunk_store(plain)
    request, src = fc.tripled_request(np.random.default_rng(111), dig)
    lens = np.array([len(chunks[k]) for k in src], dtype=np.uint32)
    with M.Engine() as e, e.zset() as zs, e.packset() as ps:
        for (pe, pb), (ze, zb) in zip(plain, zpacks):
            ps.add_blob(pb, pe, verify=True)
            zs.add_zblob(zb, ze, verify=True)
        for ln in (lens, None):
            model = fc.model_missing(store, request, ln)
            assert 0 < model[2]["n_want"] < model[2]["n_distinct"] == n and (model[2]["want_bytes"] > 0) == (ln is not None)
            got = zs.missing(request, ln)
            _same_missing(got, model)
            _same_missing(got, ps.missing(request, ln))                # the plain set fed the same packs in plain form
            assert got[2].held_bytes == sum(len(c) for c in store.values()) and got[2].ms_resolve > 0      # PLAIN lengths
        # cap = 0 sizes; one row too few is MI_ERR_CAPACITY, writes nothing to want_rows and fills held and *info
        L, info, model = e._lib, M.WantInfo(), fc.model_missing(store, request, lens)
        n_want = model[2]["n_want"]
        assert L.mi_zset_missing(zs._h, request.ctypes.data, lens.ctypes.data, len(request), None, None, 0, C.byref(info)) == 0
        assert info.n_want == n_want and info.n_rows == len(request)
        out, held, info2 = np.full(n_want, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64), np.full(len(request), 7, dtype=np.uint8), M.WantInfo()
        assert L.mi_zset_missing(zs._h, request.ctypes.data, lens.ctypes.data, len(request), held.ctypes.data, out.ctypes.data, n_want - 1,
                                 C.byref(info2)) == -7
        assert (out == 0xEEEEEEEEEEEEEEEE).all() and info2.n_want == n_want and b"need %d" % n_want in L.mi_last_error(e._h)
        assert np.array_equal(held, model[0])
        assert L.mi_zset_missing(zs._h, request.ctypes.data, lens.ctypes.data, len(request), None, out.ctypes.data, n_want, C.byref(info2)) == 0
        assert np.array_equal(out, model[1])
        # a stated length that differs from a HELD chunk's; a length of 0: the smallest such row, in the plain set's words
        k_held = [r for r in range(len(request)) if model[0][r]]
        wrong = lens.copy()
        wrong[k_held[5]] += 1
        wrong[k_held[9]] += 2
        for s in (zs, ps):
            _raises(-1, lambda: s.missing(request, wrong), "row %d:" % k_held[5], bytes(request[k_held[5]]).hex(),
                    "with %d bytes" % lens[k_held[5]], "states %d" % wrong[k_held[5]])
        wrong = lens.copy()
        wrong[9] = wrong[3] = 0
        for s in (zs, ps):
            _raises(-1, lambda: s.missing(request, wrong), "row 3 ", "length 0")
        missing_row = int(model[1][0])                                  # a MISSING digest states what it likes
        free = lens.copy()
        free[missing_row] += 5
        assert zs.missing(request, free)[2].want_bytes == model[2]["want_bytes"] + 5
        # n = 0: all-zero info; 2^32 rows; NULL arguments with a live set; the set is as it was
        held0, rows0, info0 = zs.missing(np.zeros((0, 32), dtype=np.uint8))
        assert len(held0) == 0 and len(rows0) == 0 and [getattr(info0, k) for k in COUNTERS] == [0] * 6
        assert L.mi_zset_missing(zs._h, request.ctypes.data, None, 1 << 32, None, None, 0, None) == -1 and b"2^32" in L.mi_last_error(e._h)
        assert L.mi_zset_missing(zs._h, None, None, 1, None, None, 0, None) == -1
        assert L.mi_zset_missing(zs._h, request.ctypes.data, None, 1, None, None, 3, None) == -1          # room without a buffer
        assert zs.info.n_digests == len(store)
        # the puller's round trip without a plain pack: the want list, the server's cut, the add, nothing missing
        with e.zset() as server:
            for ze, zb in zpacks:
                server.add_zblob(zb, ze)
            third = zc.model_compress(*zc.pack_of([chunks[k] for k in range(2, n, 3)]))
            server.add_zblob(third[1], third[0])
            want_rows = zs.missing(request, lens)[1].astype(np.int64)
            with server.zpack(request[want_rows], lens[want_rows], verify=True) as cut:
                zs.add_zpack(cut, verify=True)
            assert zs.missing(request, lens)[2].n_want == 0 and zs.missing(request, lens)[0].all()
        # a set in its sticky failed state: MI_ERR_STATE with the first message
        liar = np.zeros(1, dtype=zc.ZENTRY_DTYPE)
        liar["digest"][0] = dig[0]
        liar["offset"], liar["length"], liar["stored"] = 0, len(chunks[0]) + 3, len(chunks[0]) + 3
        _raises(-1, lambda: zs.add_zblob(bytes(pc.round16(len(chunks[0]) + 3)), liar), "another length")
        _raises(-6, lambda: zs.missing(request), "unusable since", "another length")


def test_digests_that_share_their_first_eight_bytes_are_each_their_own():
    rng = np.random.default_rng(112)
    tag = 0x1122334455667000 | 0x2FF
    firsts = [tag, tag, tag, tag, tag, tag + 1, tag + 2, tag - 1, 0, 1]                  # five with one tag; 0 is stored as 1, next to a real 1
    n = len(firsts)
    dig = np.zeros((n, 32), dtype=np.uint8)
    for k, t in enumerate(firsts):
        dig[k, :8] = np.frombuffer(int(t).to_bytes(8, "little"), dtype=np.uint8)
        dig[k, 8:] = rng.integers(0, 256, 24, dtype=np.uint8)
    assert len({bytes(d) for d in dig}) == n and len({bytes(d[:8]) for d in dig[:5]}) == 1
    chunks = [zc.text_like(k, k) if k in (250, 90) else rng.integers(0, 256, k, dtype=np.uint8).tobytes()
              for k in (100, 100, 37, 64, 1, 250, 16, 90, 33, 47)]
    held = [0, 2, 4, 5, 7, 8]                                                            # of the colliding five: three held, two not; 0-tag held, 1 not
    pe, pb, ze, zb = qc.zpack_of([chunks[k] for k in held], digests=dig[held])
    assert (ze["stored"] < ze["length"]).sum() == 2
    store = rc.chunk_store([(pe, pb)])
    order = [3, 9, 2, 0, 8, 1, 4, 7, 6, 5, 1, 3, 8, 0]
    lens = np.array([len(chunks[k]) for k in order], dtype=np.uint32)
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze)                                           # (verify is off: the digests are opaque)
        model = fc.model_missing(store, dig[order], lens)
        assert model[0].tolist() == [int(k in held) for k in order] and model[1].tolist() == [0, 1, 5, 8]
        _same_missing(zs.missing(dig[order], lens), model)


def test_a_request_of_more_than_256_plan_blocks_against_a_small_zset():
    """600 000 rows are 293 blocks of the plan's 2 048: the one block that scans the block sums (csrc/mi_plan.h) goes round
    twice and carries between the rounds -- from mi_zset_missing, its second caller beside mi_packset_missing
    (test_gpu_chunk_fetch.py).  No lengths are stated.  The compacting kernels that take real chunk bytes (pack, zbatch, the
    zset's cut, zprune) have their 2047 / 2048 / 2049 cases; more than 256 blocks of real chunks is not a test of a few
    seconds: that is left to the shared body and the two want-list tests."""
    rng = np.random.default_rng(113)
    n_set, n_unknown, n = 48, 450_000, 600_000
    dig = fc.fake_digests(rng, n_set + n_unknown)
    chunks = [zc.text_like(k, k) if k % 3 == 0 else rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in range(20, 20 + 7 * n_set, 7)]
    pe, pb, ze, zb = qc.zpack_of(chunks, digests=dig[:n_set])
    # the set's own digests repeated, every unknown digest once and some of them again, permuted
    pick = np.concatenate([rng.integers(0, n_set, 100_000), n_set + np.arange(n_unknown), rng.integers(n_set, n_set + n_unknown, 50_000)])
    pick = pick[rng.permutation(n)]
    assert len(pick) == n and n // fc.PLAN_BLOCK > 256
    # numpy's answer: a digest counts where it occurs first; held iff it is the set's; the want rows ascending
    distinct, first = np.unique(pick, return_index=True)
    w_held = (pick < n_set).astype(np.uint8)
    w_rows = np.sort(first[distinct >= n_set]).astype(np.uint64)
    held_ids = distinct[distinct < n_set]
    w_info = dict(n_rows=n, n_distinct=len(distinct), n_held=len(held_ids), n_want=len(w_rows),
                  held_bytes=sum(len(chunks[k]) for k in held_ids), want_bytes=0)
    assert w_info["n_held"] == n_set and w_info["n_want"] == n_unknown
    with M.Engine() as e, e.zset() as zs:
        zs.add_zblob(zb, ze)                                           # (verify is off: the digests are opaque)
        _same_missing(zs.missing(dig[pick]), (w_held, w_rows, w_info))


# ---- 10. the bounds, checked by the hardware ----------------------------------------------------------------------------------------------
# The bounds, from the code (csrc/mi_zbatch.hip): the coder reads inside the chunk only; a unit's load of the gather begins at
# src + o, o a multiple of 16 below `stored`, and is 16 bytes long -- the last unit of a RAW entry of len bytes ends at most 15 bytes
# behind the chunk (len = 1 mod 16), inside the arena's 4 KiB slack; the last unit of a coded entry lies inside its scratch span;
# the gather writes the new blob to its last byte and not beyond.  Under MI_GUARD_ALLOC=1 every device allocation holds exactly the
# bytes asked for and ends on an unmapped page (tests/test_gpu_overread.py): the arena is reserved exactly and the last selected
# chunk ends on the arena's last byte in use.  No positive control: a deliberate fault has no place on a shared box.
GUARD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import makisu_amd as M
import pack_cases as pc
import zbatch_cases as bc
import zpack_cases as zc
rng = np.random.default_rng(113)
coded = zc.tail_chunk(rng, 6, 1)                                      # stored = 1 mod 16, coded
raw = rng.integers(0, 256, 33, dtype=np.uint8).tobytes()              # stored = length = 1 mod 16, raw
files = [zc.text_like(3000, 3), rng.integers(0, 256, 777, dtype=np.uint8).tobytes(), coded, raw]
with M.Engine() as e:
    b = e.batch()
    b.reserve(len(files), sum((len(x) + 255) // 256 * 256 for x in files[:-1]) + len(files[-1]))
    for i, x in enumerate(files):
        b.add_bytes(x, i)
    b.run()
    rows = pc.rows_of(b.chunks())
    assert rows[-1] == (3, 0, 33) and rows[-2] == (2, 0, len(coded))
    all_but_last = np.ones(len(rows), np.uint8)
    all_but_last[-1] = 0
    for name, sel in (("the last entry raw, on the arena's last byte", None), ("the last entry coded", all_but_last)):
        want_e, want_b = bc.model_zpack(rows, files, sel)
        last = want_e[-1]
        print("case", name, "length", int(last["length"]), "stored", int(last["stored"]), "residue", int(last["stored"]) %% 16, flush=True)
        assert int(last["stored"]) %% 16 == 1 and (int(last["stored"]) < int(last["length"])) == (sel is not None)
        for verify in (True, False):
            z = b.zpack(select=sel, verify=verify)
            assert z.read() == want_b and bc.same_zentries(z.entries(), want_e) and z.info.verified == int(verify)
            z.close()
    b.free()
print("OK")
"""


def test_no_load_leaves_the_chunk_the_scratch_or_the_arenas_slack(tmp_path):
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", GUARD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout[-1500:] + p.stderr[-3000:]
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("case")]) == 2
