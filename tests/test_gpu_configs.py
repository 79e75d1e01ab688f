"""GPU parity on BASELINE.json's configs at (or near) full size, every row against the oracle.

VERDICT r1: "full-size configs are property-checked, not oracle-checked".  The oracle generates each
synthetic file inside its worker threads (mi_ref_scan_synthetic), so the whole of C2 (6.25 GiB)
costs it about a second on the GPU box's host cores and never has to exist in host memory:
  C2  all 100 000 x 64 KiB files                                     (configs[1], full size)
  C3  all 1 000 x 128 MiB files as one 134 GB batch                  (configs[2], full size: round 4)
  C4  two ranks' shards of file index mod 8, job-wide marking        (configs[3] shape)
  C4  one rank's FULL shard, 1.25 M x 64 KiB = 76 GiB                (configs[3], full size per rank)
  C5  one GPU's full Zipf shard (3 350 files 1 KiB..1 GiB, 57 GiB), 90 % duplicates  (configs[4], full size)
      + the rounds-1/2 log-uniform shard (6 GiB) + two ranks through bench.py with split files
Cut points: parity UNPINNED w.r.t. the reference (no CDC there); SHA-256 pinned (tests/test_oracle.py).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (must come before the engine: see test_gpu_parity.py)
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _threads():
    sys.path.insert(0, ROOT)
    import bench
    return bench.usable_cores()[0]


def _check_shard(oracle, eng, shard):
    with eng.batch(shard.n_files, shard.n_bytes) as b:
        b.add_synthetic(shard.sizes, shard.cids, seed=shard.seed)
        b.run()
        files, chunks = b.files().copy(), b.chunks().copy()
        st = eng.stats()
    p = oracle.CdcParams(eng.cfg.gear_seed, eng.cfg.mask_bits, eng.cfg.min_size, eng.cfg.max_size)
    rf, rc, nu = oracle.scan_synthetic(shard.seed, shard.cids, shard.sizes, p, True, _threads(), 0)
    assert len(chunks) == len(rc), (len(chunks), len(rc))
    assert np.array_equal(files["n_chunks"], rf["n_chunks"]) and np.array_equal(files["first_chunk"], rf["first_chunk"])
    assert np.array_equal(chunks["file_index"], rc["file_index"])
    assert np.array_equal(chunks["offset"], rc["offset"]), "cut points differ"
    assert np.array_equal(chunks["length"], rc["length"]), "cut points differ"
    assert np.array_equal(chunks["sha256"], rc["sha256"]), "chunk digests differ"
    assert np.array_equal(files["chunk_root"], rf["chunk_root"]), "file roots differ"
    assert np.array_equal(chunks["dup_of"], rc["dup_of"]), "dedup marking differs"
    assert st["n_unique"] == nu
    return files, chunks, nu


@pytest.fixture(scope="module")
def eng():
    import makisu_amd
    e = makisu_amd.Engine()
    yield e
    e.close()


def test_c2_full_size_every_row(oracle, eng):
    from makisu_amd import workloads as W
    files, chunks, nu = _check_shard(oracle, eng, W.c2(0, 1, 100000))
    # distinct contents: nothing repeats, except that two 1-byte tail chunks may coincide (256 values)
    dup = chunks[chunks["dup_of"] >= 0]
    assert len(chunks) > 700000 and nu == len(chunks) - len(dup) and (dup["length"] <= 2).all() and len(dup) <= 3


@pytest.mark.timeout(600)
def test_bench_plain_line_and_its_dumped_outputs(oracle, eng, tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` without --full: the headline line alone (no leg of its own behind
    it), and DIR holds the rows of the last timed step as float .npy files -- the oracle's rows of that step's shard"""
    import json
    from makisu_amd import workloads as W
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--files", "2000", "--steps", "3",
                          "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=500)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    j = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["metric"] == "GiB/s hashed (Gear CDC + SHA-256 per chunk)" and j["unit"] == "GiB/s" and j["higher_is_better"] is True
    assert j["value"] > 0 and j["ms_per_step"] > 0 and j["steps"] == 3 and j["warmup"] == 1 and j["dtype"] == "u32"
    assert not {"roofline", "cpu_baseline", "with_rows_on_host", "commit_e2e", "one_batch_at_a_time", "clocks"} & set(j)
    d = {f[:-4]: np.load(str(tmp_path / "dump" / f)) for f in os.listdir(str(tmp_path / "dump"))}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    n_files, n_chunks = (int(x) for x in d["counts"])
    assert n_files == 2000 and n_chunks == j["config"]["chunks_last_batch"] == len(d["chunk_rows"])     # (small: every row)
    # the last of 3 timed steps ran the first of the 2 batches in flight: generation 0 of the shard
    shard = W.c2(0, 1, 2000, 0)
    p = oracle.CdcParams(eng.cfg.gear_seed, eng.cfg.mask_bits, eng.cfg.min_size, eng.cfg.max_size)
    rf, rc, _ = oracle.scan_synthetic(shard.seed, shard.cids, shard.sizes, p, True, _threads(), 0)
    assert len(rc) == n_chunks
    assert np.array_equal(d["file_n_chunks"], rf["n_chunks"].astype(np.float64))
    assert np.array_equal(d["file_chunk_root"], rf["chunk_root"].astype(np.float32))
    for k in ("file_index", "offset", "length", "dup_of"):
        assert np.array_equal(d["chunk_" + k], rc[k].astype(np.float64)), k
    assert np.array_equal(d["chunk_sha256"], rc["sha256"].astype(np.float32))


@pytest.mark.timeout(900)
def test_c3_full_size_every_row(oracle, eng):
    """BASELINE.json configs[2] as written and as `bench.py --config c3` times it: 1 000 x 128 MiB as ONE
    134 GB batch (13.1 M chunks), every row against the oracle; a third of the files repeat earlier ones, so
    the duplicate marking has 4.4 M rows to find (rounds 1-3 checked 6 and 60 files)."""
    from makisu_amd import workloads as W
    sh = W.c3(0, 1, 1000)
    sh.cids[667:] = sh.cids[:333]
    files, chunks, nu = _check_shard(oracle, eng, sh)
    assert sh.n_bytes == 1000 * (128 << 20) and len(chunks) > 13_000_000
    assert (chunks["dup_of"][chunks["file_index"] >= 667] >= 0).all()
    assert np.array_equal(files["chunk_root"][667:], files["chunk_root"][:333])
    assert 0 <= int(files["n_chunks"][:667].sum()) - nu <= 2      # (two 1-byte tail chunks may coincide)


def _closed_form_in_shard(sh, files):
    """one set of chunks per distinct content present in the shard"""
    first_of_content = np.zeros(sh.n_files, dtype=bool)
    seen = set()
    for i, c in enumerate(sh.cids.tolist()):
        if c not in seen:
            seen.add(c)
            first_of_content[i] = True
    return int(files["n_chunks"][first_of_content].sum())


def test_c5u_loguniform_lpt_shard_closed_form(oracle, eng):
    """Rounds 1-2's stand-in (sizes 2^U(10,28)): one rank's LPT shard of a 2-rank job, every row against
    the oracle, the unique count against the generator's closed form restricted to this shard."""
    from makisu_amd import workloads as W
    sh = W.c5(0, 2, bytes_per_gpu=6 * W.GIB, hi_log2=28, law="loguniform", split_threshold=1 << 40)
    assert sh.n_files > 500 and int(sh.sizes.max()) > 64 * W.MIB and sh.parts is None
    files, chunks, nu = _check_shard(oracle, eng, sh)
    assert nu == _closed_form_in_shard(sh, files)
    other = W.c5(1, 2, bytes_per_gpu=6 * W.GIB, hi_log2=28, law="loguniform", split_threshold=1 << 40)
    assert sh.n_files + other.n_files == sh.n_global_files
    assert len(set(sh.global_index.tolist()) & set(other.global_index.tolist())) == 0
    assert abs(sh.n_bytes - other.n_bytes) <= 0.02 * sh.n_bytes


@pytest.mark.timeout(900)
def test_c5_zipf_full_shard_every_row(oracle, eng):
    """BASELINE.json configs[4] as written -- Zipf(s = 1.1) over the log2 buckets
    2^10..2^30, 64 GiB nominal per GPU (57 GiB drawn), 1 GiB files included -- one GPU's whole shard,
    every row against the oracle; the unique count is the generator's closed form."""
    from makisu_amd import workloads as W
    sh = W.c5(0, 1)
    assert sh.name == "c5" and sh.n_files > 3000 and int(sh.sizes.max()) == 1 << 30 and sh.n_bytes > 50 * W.GIB
    assert (sh.sizes <= 64 * W.KIB).mean() > 0.6
    files, chunks, nu = _check_shard(oracle, eng, sh)
    assert nu == int(files["n_chunks"][sh.originals].sum()) == _closed_form_in_shard(sh, files)
    assert nu < 0.2 * len(chunks)                            # nine copies per original: mostly duplicates


@pytest.mark.timeout(900)
def test_c4_one_rank_full_shard_every_row(oracle):
    """one rank's whole C4 shard -- 1 250 000 x 64 KiB = 76 GiB, the files with global
    index 3 mod 8 -- every one of its ~9 M rows against the oracle."""
    import makisu_amd
    from makisu_amd import workloads as W
    sh = W.c4(3, 8)
    assert sh.n_files == 1250000 and sh.global_index[:2].tolist() == [3, 11]
    with makisu_amd.Engine() as e:
        files, chunks, nu = _check_shard(oracle, e, sh)
    assert len(chunks) > 9_000_000
    dup = chunks[chunks["dup_of"] >= 0]
    assert (dup["length"] <= 2).all() and len(dup) < 100     # only coincidences of 1-2 byte tail chunks


def test_c4_two_of_eight_shards_job_wide_marking(oracle, eng):
    """C4's partition (file index mod 8) for ranks 0 and 1 at 20 000 files per rank, with a few
    files duplicated across the ranks: the job-wide marking over the rank-major digest set
    (mi_dedup_mark_range, what every rank runs after the all-gather) against the oracle's marking
    of the concatenated rows."""
    import makisu_amd
    from makisu_amd import workloads as W
    import torch as T
    shards = [W.c4(r, 8, 20000) for r in (0, 1)]
    assert shards[0].global_index[:3].tolist() == [0, 8, 16] and shards[1].global_index[:3].tolist() == [1, 9, 17]
    shards[1].cids[::50] = shards[0].cids[::50]            # cross-rank duplicates
    p = oracle.CdcParams(eng.cfg.gear_seed, eng.cfg.mask_bits, eng.cfg.min_size, eng.cfg.max_size)
    digs, rows = [], []
    with makisu_amd.Engine(flags=makisu_amd.FLAG_NO_DEDUP) as e2:
        batches = []
        for sh in shards:
            b = e2.batch(sh.n_files, sh.n_bytes)
            b.add_synthetic(sh.sizes, sh.cids, seed=sh.seed)
            b.run()
            batches.append(b)
            _, rc, _ = oracle.scan_synthetic(sh.seed, sh.cids, sh.sizes, p, True, _threads(), oracle.NO_DEDUP)
            assert np.array_equal(b.chunks()["sha256"], rc["sha256"])
            rows.append(rc["sha256"])
        allrows = np.concatenate(rows)
        want, want_unique = oracle.dedup_mt(allrows, _threads())
        glob = T.from_numpy(allrows.copy()).cuda()
        n0 = len(rows[0])
        got_unique = 0
        for r, b in enumerate(batches):
            first = 0 if r == 0 else n0
            got_unique += b.mark_global(glob.data_ptr(), len(allrows), first)
            mine = b.chunks()["dup_of"]
            assert np.array_equal(mine, want[first:first + len(mine)])
        assert got_unique == want_unique < len(allrows)
        for b in batches:
            b.free()


@pytest.mark.timeout(900)
def test_bench_c4_two_ranks_on_one_gpu_gloo():
    """bench.py --gpus 2 --config c4 as the driver launches it (torch.distributed.run), both ranks on
    this one GPU, exchange over gloo: the N > 1 path end to end (sharding, exchange, job-wide unique
    count = the generator's closed form: C4 has no duplicates)."""
    env = dict(os.environ, MI_BENCH_FORCE_DEVICE="0", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29577", os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--config", "c4", "--files", "20000", "--steps", "2", "--warmup", "1",
           "--exchange", "torch", "--backend", "gloo", "--full", "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=800)
    assert out.returncode == 0, out.stderr[-3000:]
    import json
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == 2 and j["config"]["name"] == "c4" and j["value"] > 0
    assert j["config"]["job_bytes_per_step"] == 2 * 20000 * 65536
    assert j["dedup_check"]["ok"], j["dedup_check"]          # job-wide unique count == closed form


@pytest.mark.timeout(900)
def test_bench_c5_two_ranks_split_files_on_one_gpu_gloo():
    """bench.py --gpus 2 --config c5: the Zipf mix LPT-sharded over two ranks (both on this GPU, gloo),
    files >= 32 MiB split into two parts whose owners agree on the boundary cuts (resolve_parts), digest
    exchange, and the job-wide unique count = the closed form of the generator -- which only holds if the
    parts' rows put together are the rows of the whole files."""
    env = dict(os.environ, MI_BENCH_FORCE_DEVICE="0", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29579", os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--config", "c5", "--bytes-per-gpu", "3", "--split-mib", "32", "--steps", "2",
           "--warmup", "1", "--exchange", "torch", "--backend", "gloo", "--full", "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=800)
    assert out.returncode == 0, out.stderr[-3000:]
    import json
    j = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["n_gpus"] == 2 and j["config"]["name"] == "c5" and "Zipf s=1.1" in j["config"]["workload"]
    assert j["config"]["parts_this_rank"] > 0 and j["config"]["files_split_into_parts_job"] > 0
    assert j["config"]["lpt_imbalance_max_over_mean_bytes"] < 1.02
    assert j["dedup_check"]["ok"], j["dedup_check"]
