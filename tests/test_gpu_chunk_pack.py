"""GPU tests of the chunk packs (mi_batch_pack_chunks, mi_pack_*, MI_MEMFS_CHUNK_PACK): whatever the gather kernel wrote is
compared, every byte of it, with the pure-Python model of pack_cases.py -- hashlib's digests, the layout restated -- on
chunks of every (start mod 16, length mod 16), selections of every shape, the edge sizes, both digest algorithms, arena
offsets past 2^32, packs that outlive their batch, the state rules, the windowed read path, the commit that hands over its
pack and its recipes, and the over-read bound under the guard allocator.  Bit for bit: there are no tolerances."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (before the engine, as in test_gpu_parity.py: the 5 GiB test asks it for the device's free memory)
except ImportError:          # CPU-only collection without torch: the GPU tests are skipped anyway
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import pack_cases as pc  # noqa: E402
from commit_cases import commit_to_bytes, make_tree, write_file  # noqa: E402

pytestmark = pytest.mark.gpu
MTIME = 1_600_000_000
MIB = 1 << 20


def _check(pack, rows, files, select=None, alg=pc.SHA256, verified=None):
    """entries and the whole blob against the model; returns (entries, blob)"""
    want_e, want_b = pc.model_pack(rows, files, select, alg)
    info = pack.info
    got_e, got_b = pack.entries(), pack.bytes()
    assert (info.n_entries, info.blob_bytes, info.alg) == (len(want_e), len(want_b), alg)
    assert info.chunk_bytes == int(want_e["length"].sum(dtype=np.uint64)) if len(want_e) else info.chunk_bytes == 0
    assert pc.same_entries(got_e, want_e)
    assert got_b == want_b
    if verified is not None:
        assert info.verified == verified
    return got_e, got_b


# ---- the alignment sweep and the selections: one batch, one model --------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    data = np.random.default_rng(31).integers(0, 256, MIB, dtype=np.uint8).tobytes()
    with M.Engine(mask_bits=6, min_size=64, max_size=1024) as e, e.batch() as b:
        b.add_bytes(data, 0)
        b.run()
        chunks = b.chunks().copy()
        yield e, b, [data], chunks, pc.rows_of(chunks)


def test_every_start_and_length_residue_comes_out_byte_for_byte(sweep):
    e, b, files, chunks, rows = sweep
    # the condition the test rests on: all 256 pairs (chunk start mod 16, length mod 16) occur (a file begins on a 256-byte
    # boundary of the arena: the offset in the file is the offset in the arena, mod 16)
    pairs = {(off % 16, n % 16) for _, off, n in rows}
    assert len(pairs) == 256 and len(rows) > 8000 and 40 <= min(n for _, _, n in rows) and max(n for _, _, n in rows) <= 1024
    with b.pack(verify=True) as p:
        entries, blob = _check(p, rows, files, verified=1)
        assert M.pack_check(blob, entries) is None
        assert p.info.ms_gather > 0 and p.info.ms_verify > 0
        ptr, n = p.device()
        assert ptr and n == len(blob)
    with b.pack() as p:                                        # without the flag: the same blob, not marked verified
        _check(p, rows, files, verified=0)


def test_selections(sweep):
    e, b, files, chunks, rows = sweep
    n = len(rows)
    first = (chunks["dup_of"] < 0).astype(np.uint8)
    cases = {"none": np.zeros(n, np.uint8), "every other row": (np.arange(n) % 2 == 0).astype(np.uint8),
             "only row 0": np.eye(1, n, 0, dtype=np.uint8)[0], "only the last row": np.eye(1, n, n - 1, dtype=np.uint8)[0],
             "the two ends": np.eye(1, n, 0, dtype=np.uint8)[0] | np.eye(1, n, n - 1, dtype=np.uint8)[0], "dup_of < 0": first,
             "flags are non-zero bytes, not ones": ((np.arange(n) % 3 == 0) * 0x80).astype(np.uint8)}
    for name, sel in cases.items():
        with b.pack(select=sel, verify=True) as p:
            entries, blob = _check(p, rows, files, select=sel, verified=1)
            assert len(entries) == int((sel != 0).sum()), name
    with b.pack(select=cases["none"]) as p:                    # a valid pack of nothing
        assert (p.info.n_entries, p.info.blob_bytes, p.bytes(), p.device()) == (0, 0, b"", (None, 0))


def test_edge_files_under_the_default_config():
    rng = np.random.default_rng(32)
    sizes = [0, 1, 15, 16, 17, 63, 64, 65, 2047, 70000]
    files = [rng.integers(0, 256, s, dtype=np.uint8).tobytes() for s in sizes]
    files.append(bytes(200000))                                # forced cuts at max_size; its chunks duplicate each other
    files.append(files[sizes.index(70000)])                    # a byte-identical copy
    with M.Engine() as e, e.batch() as b:
        for i, x in enumerate(files):
            b.add_bytes(x, i)
        b.run()
        chunks = b.chunks()
        rows = pc.rows_of(chunks)
        assert 0 not in {f for f, _, _ in rows}                # the empty file contributes no row
        assert (chunks["dup_of"] >= 0).sum() >= 3              # the zero file's repeats and the copy: selected together with the firsts
        assert [n for f, _, n in rows if f == 10][:3] == [65536, 65536, 65536]
        with b.pack(verify=True) as p:
            entries, blob = _check(p, rows, files, verified=1)
            one = next(en for en in entries if en["length"] == 1)
            at = int(one["offset"])
            assert blob[at:at + 16] == files[1] + bytes(15)    # the 1-byte file: a 16-byte unit with 15 zero bytes
            assert M.pack_check(blob, entries) is None
        sel = (chunks["dup_of"] >= 0).astype(np.uint8)         # ... and the duplicates alone: the selection belongs to the caller
        with b.pack(select=sel, verify=True) as p:
            _check(p, rows, files, select=sel, verified=1)


def test_a_blake2s_ctx_packs_blake2s_digests():
    rng = np.random.default_rng(33)
    files = [rng.integers(0, 256, s, dtype=np.uint8).tobytes() for s in (1, 5000, 150001)]
    with M.Engine(flags=M.FLAG_CHUNK_BLAKE2S) as e, e.batch() as b:
        for i, x in enumerate(files):
            b.add_bytes(x, i)
        b.run()
        rows = pc.rows_of(b.chunks())
        with b.pack(verify=True) as p:
            entries, blob = _check(p, rows, files, alg=pc.BLAKE2S, verified=1)
            assert bytes(entries[0]["digest"]) == hashlib.blake2s(files[0]).digest()
            assert M.pack_check(blob, entries, M.DIGEST_BLAKE2S) is None
            assert M.pack_check(blob, entries, M.DIGEST_SHA256) == 0


def test_arena_offsets_past_four_gib():
    """a synthetic batch of 5 GiB in 1 MiB files, the last file's rows selected: the sources lie past 2^32 in the arena.  (A blob
    above 4 GiB is not tested: DESIGN.md 4.6.)"""
    nf = 5 * 1024
    # the guard, before any work and on the device's free memory alone: the arena (5 GiB + 20 MiB hinted, one allocation), the
    # tables of ~650 000 chunk rows and 5 120 files (well under 0.5 GiB), the blob of one file.  From here on every error of the
    # engine -- an MI_ERR_NOMEM of the batch, the reserve or the pack included -- fails the test
    assert torch is not None, "the guard asks torch for the device's free memory"
    free_b = int(torch.cuda.mem_get_info()[0])
    if free_b < (7 << 30):
        pytest.skip("the device has %.1f GiB free, the test needs 7" % (free_b / 2.0 ** 30))
    # the condition the test rests on: files lie in the arena in the order they were added, each on a 256-byte boundary, and
    # a 1 MiB file fills its slot: the last file's bytes -- every selected source -- begin past 2^32
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
        stand_in = {last: data}                                # the model reads files[file_index]: a dict serves
        with b.pack(select=sel, verify=True) as p:
            entries, blob = _check(p, pc.rows_of(chunks), stand_in, select=sel, verified=1)
            assert np.array_equal(entries["chunk_index"], np.arange(lo, lo + n, dtype=np.uint64))
            assert blob[:int(entries[0]["length"])] == data[:int(entries[0]["length"])]


def test_a_pack_outlives_its_batch_and_keeps_its_ctx_alive():
    rng = np.random.default_rng(34)
    data = rng.integers(0, 256, 300000, dtype=np.uint8).tobytes()
    e = M.Engine()
    try:
        b = e.batch()
        b.add_bytes(data, 0)
        b.run()
        rows = pc.rows_of(b.chunks())
        want_e, want_b = pc.model_pack(rows, [data])
        p1, p2 = b.pack(), b.pack(verify=True)                 # neither is read before its batch changes
        b.reset()
        b.add_bytes(bytes(reversed(data)), 0)                  # the arena now holds other bytes
        b.run()
        assert p1.bytes() == want_b and pc.same_entries(p1.entries(), want_e)
        b.free()
        assert p2.bytes() == want_b and pc.same_entries(p2.entries(), want_e)
        p1.close()
        assert e._lib.mi_ctx_destroy(e._h) == -6               # MI_ERR_STATE: a pack still points at the ctx
        assert b"still alive" in e._lib.mi_last_error(e._h)
        assert p2.read(16, 100) == want_b[16:116]              # ... which is as usable as before
        p2.close()
    finally:
        e.close()


def test_state_rules(tmp_path):
    with M.Engine() as e, e.batch() as b:
        b.add_bytes(b"x" * 5000, 0)
        with pytest.raises(M.MiError) as ei:                   # not run
            b.pack()
        assert ei.value.code == -6
        b.submit()
        with pytest.raises(M.MiError) as ei:                   # in flight
            b.pack()
        assert ei.value.code == -6
        b.wait()
        n = len(b.chunks())
        for wrong in (n + 1, n - 1 if n > 1 else 0, 0):
            with pytest.raises(M.MiError) as ei:               # a wrong n_select
                b.pack(select=np.ones(wrong, np.uint8))
            assert ei.value.code == -1 and "selection flags" in str(ei.value)
        out = C.c_void_p()
        assert e._lib.mi_batch_pack_chunks(b._h, None, 0, 0x2, C.byref(out)) == -1      # an unknown flag
        with b.pack(select=np.ones(n, np.uint8)) as p:
            assert p.info.n_entries == n
        b.reset()
        with pytest.raises(M.MiError) as ei:                   # reset: not run again
            b.pack()
        assert ei.value.code == -6
    # a group head (the batch behind mi_memfs_commit_layer_n) is not reachable through the ABI by itself -- mi_batch_group_begin
    # is a hidden symbol and no public call hands out the handle's batch -- so the group branch of mi_batch_pack_chunks runs in
    # NO test (DESIGN.md 4.6 says so).  What a caller can reach is tested: the commit over several ctxs refuses the pack option
    # before anything is walked (MI_ERR_INVALID)
    root = str(tmp_path / "root")
    write_file(os.path.join(root, "a"), b"abc" * 1000, mtime=MTIME)
    with M.Engine() as e0, M.Engine() as e1, M.MemFS(root) as fs, M.ChunkIndex(e0) as ix:
        fs.set_index(ix)
        fs.set_options(chunk_pack=True)
        with pytest.raises(M.MiError) as ei:
            fs.commit_layer(must_scan=True, engine=[e0, e1])
        assert ei.value.code == -1 and "several GPUs" in str(ei.value)
        assert fs.commit_stats()["n_walked"] == 0
        fs.release_device()


def test_reads_across_the_window_edge():
    """mi_pack_read through its two 8 MiB windows: pieces that straddle the edge, a stream of odd-sized pieces, the whole blob
    in one call, jumps back and forth, and a read outside the blob"""
    data = np.random.default_rng(35).integers(0, 256, 17 * MIB, dtype=np.uint8).tobytes()
    with M.Engine() as e, e.batch() as b:
        b.add_bytes(data, 0)
        b.run()
        rows = pc.rows_of(b.chunks())
        _, want = pc.model_pack(rows, [data])
        assert len(want) > 16 * MIB + 64
        with b.pack() as p:
            edge = 8 * MIB
            for off in range(edge - 5, edge + 12):
                assert p.read(0, 1) == want[:1]                # the window is [0, 8 MiB) again: the next read leaves it
                assert p.read(off, 37) == want[off:off + 37], off
            for off in (edge - 1, 0, 2 * edge - 3, edge, len(want) - 1, 5):
                assert p.read(off, 1) == want[off:off + 1], off
            got, at, step = [], 0, MIB + 7
            while at < len(want):
                got.append(p.read(at, min(step, len(want) - at)))
                at += step
            assert b"".join(got) == want
            assert p.bytes() == want and p.read(len(want), 0) == b""
            for off, n in ((len(want), 1), (len(want) - 3, 4), (1 << 62, 1)):
                with pytest.raises(M.MiError) as ei:
                    p.read(off, n)
                assert ei.value.code == -1 and "outside the blob" in str(ei.value)


# ---- the commit hands over its pack and its recipes ---------------------------------------------------------------------
def _rebuild(store, recipe):
    return b"".join(store[d][:n] for d, n in recipe)


def _take(fs, eng, store, seen):
    """the commit's pack into the store; returns (entries, blob bytes).  No digest arrives twice."""
    with fs.take_pack() as p:
        assert p.info.verified == 1
        entries, blob = p.entries(), p.bytes()
    assert M.pack_check(blob, entries) is None
    for en in entries:
        d = bytes(en["digest"])
        assert d not in seen, "a chunk an earlier pack held"
        seen.add(d)
        store[d] = blob[int(en["offset"]):int(en["offset"]) + int(en["length"])]
        assert hashlib.sha256(store[d]).digest() == d
    return entries, blob


def test_the_commit_hands_over_its_pack_and_its_recipes(tmp_path):
    root = str(tmp_path / "root")
    files = make_tree(root, seed=21, n_dirs=5, files_per_dir=8, mtime=MTIME)
    assert 35 <= len(files) <= 45 and min(map(len, files.values())) == 0 and max(map(len, files.values())) > 100000
    with M.Engine() as eng, M.MemFS(root) as fs, M.MemFS(root) as plain, M.ChunkIndex(eng) as ix:
        fs.set_index(ix)
        fs.set_options(chunk_pack=True)
        store, seen = {}, set()
        with pytest.raises(M.MiError) as ei:                   # no commit yet
            fs.take_pack()
        assert ei.value.code == -6

        def both(name):
            r, raw = commit_to_bytes(fs, tmp_path, name + ".tar", must_scan=True, engine=eng)
            r0, raw0 = commit_to_bytes(plain, tmp_path, name + "_plain.tar", must_scan=True, engine=eng)
            assert raw == raw0 and r["tar_digest"] == r0["tar_digest"]                     # the option changes nothing else
            assert [(x["relpath"], x.get("root")) for x in r["layer"]] == [(x["relpath"], x.get("root")) for x in r0["layer"]]
            assert all("chunks" not in x for x in r0["layer"])
            return r

        # commit 1, all new
        r = both("c1")
        entries, blob = _take(fs, eng, store, seen)
        assert int(entries["length"].sum()) == r["stats"]["index_new_bytes"] > 0
        by = {x["relpath"]: x for x in r["layer"]}
        with eng.batch() as b:                                 # the rows a batch of the same ctx gives the same bytes
            names = sorted(files)
            for i, rel in enumerate(names):
                b.add_bytes(files[rel], i)
            b.run()
            fr, ch = b.files(), b.chunks()
            for i, rel in enumerate(names):
                lo, n = int(fr[i]["first_chunk"]), int(fr[i]["n_chunks"])
                want = [(bytes(c["sha256"]), int(c["length"])) for c in ch[lo:lo + n]]
                assert by[rel].get("chunks", []) == want, rel
        for rel, data in files.items():
            assert _rebuild(store, by[rel].get("chunks", [])) == data, rel
        assert all("chunks" not in x for x in r["layer"] if x["kind"] != 1)
        with pytest.raises(M.MiError) as ei:                   # taken: the second take has nothing
            fs.take_pack()
        assert ei.value.code == -6 and "since the last" in str(ei.value)

        # commit 2, nothing changed: the empty layer and the empty pack
        r = both("c2")
        assert r["n_entries"] == 0 and r["stats"]["index_new_bytes"] == 0
        with fs.take_pack() as p:
            assert (p.info.n_entries, p.info.blob_bytes) == (0, 0)

        # commit 3: one file rewritten in its middle, same size, same second
        rel = max(files, key=lambda k: len(files[k]))
        old = files[rel]
        new = old[:len(old) // 2] + bytes(x ^ 0x5A for x in old[len(old) // 2:len(old) // 2 + 3000]) + old[len(old) // 2 + 3000:]
        assert len(new) == len(old)
        write_file(os.path.join(root, rel), new, mtime=MTIME)
        r = both("c3")
        assert [x["relpath"] for x in r["layer"] if x["kind"] == 1] == [rel] and r["stats"]["n_content_changed"] == 1
        entries, blob = _take(fs, eng, store, seen)            # (asserts: only chunks that no earlier pack held)
        assert 0 < len(blob) < len(new) and int(entries["length"].sum()) == r["stats"]["index_new_bytes"]
        recipe = next(x for x in r["layer"] if x["relpath"] == rel)["chunks"]
        assert _rebuild(store, recipe) == new
        fs.release_device()
        plain.release_device()

    # the option without an index: MI_ERR_STATE before anything is walked
    with M.Engine() as eng, M.MemFS(root) as fs:
        fs.set_options(chunk_pack=True)
        with pytest.raises(M.MiError) as ei:
            fs.commit_layer(must_scan=True, engine=eng)
        assert ei.value.code == -6 and "index" in str(ei.value) and fs.commit_stats()["n_walked"] == 0
        assert fs.commit_layer(must_scan=True) is not None     # ctx == NULL: the reference's commit, as ever
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
    fs.set_options(chunk_pack=True)
    res = fs.commit_layer(must_scan=True, engine=eng)
    assert res["stats"]["n_windows"] >= 1 and res["n_entries"] > 20, res["stats"]
    try:
        fs.take_pack()
        raise SystemExit("a windowed commit handed over a pack")
    except M.MiError as err:
        assert err.code == -6 and "windows" in str(err), str(err)
    assert all("chunks" not in x for x in res["layer"])
    fs.release_device()
print("OK windowed")
"""


def test_a_commit_in_windows_succeeds_and_has_no_pack(tmp_path):
    assert 'getenv("MI_COMMIT_FORCE_WINDOWS")' in open(os.path.join(ROOT, "makisu_amd", "csrc", "mi_commit.hip")).read()   # the knob exists
    env = dict(os.environ, MI_COMMIT_FORCE_WINDOWS="1", MI_COMMIT_WINDOW_MB="1")
    p = subprocess.run([sys.executable, "-c", WINDOWED % {"root": ROOT}, str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK windowed" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]


# ---- the over-read bound, checked by the hardware ------------------------------------------------------------------------
# The bound, from the code (csrc/mi_pack.hip pack_gather_kernel): a unit's load begins at chunk_off + o, o a multiple of 16
# below the chunk's length -- inside the chunk, never in front of it -- and is 16 bytes long: the last unit of a chunk of
# len bytes ends at chunk_off + round16(len) - 1, at most 15 bytes behind the chunk (len = 1 mod 16), none for len = 0 mod
# 16.  The arena has 4 KiB of slack behind it.  Under MI_GUARD_ALLOC=1 every device allocation holds exactly the bytes asked
# for and ends on an unmapped page (tests/test_gpu_overread.py): the arena is reserved exactly and the last selected chunk
# ends on the arena's last byte.  No positive control: a deliberate fault has no place on a shared box.
OVERREAD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import makisu_amd as M
import pack_cases as pc
rng = np.random.default_rng(36)
with M.Engine() as e:
    for last in (1, 15, 16, 17, 2032, 2047, 70001):
        files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (3000, 777, last)]
        b = e.batch()
        b.reserve(len(files), sum((len(x) + 255) // 256 * 256 for x in files[:-1]) + len(files[-1]))
        for i, x in enumerate(files):
            b.add_bytes(x, i)
        b.run()
        chunks = b.chunks()
        rows = pc.rows_of(chunks)
        print("case", last, "last chunk", rows[-1][2], "residue", rows[-1][2] %% 16, flush=True)
        for sel in (None, np.eye(1, len(rows), len(rows) - 1, dtype=np.uint8)[0]):
            p = b.pack(select=sel, verify=True)
            want_e, want_b = pc.model_pack(rows, files, sel)
            assert p.bytes() == want_b and pc.same_entries(p.entries(), want_e) and p.info.verified == 1
            p.close()
        b.free()
print("OK")
"""


def test_no_gather_load_leaves_the_arenas_slack(tmp_path):
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", OVERREAD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout[-1500:] + p.stderr[-3000:]
    residues = {int(ln.split()[-1]) for ln in p.stdout.splitlines() if ln.startswith("case")}
    assert {1, 15, 0} <= residues, residues
