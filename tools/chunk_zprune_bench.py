"""Pruning a compressed pack set in place, measured (writes profiles/chunk_zprune.txt).

The two corpora of tools/chunk_zset_bench.py (4.10) at its sizes: an incompressible C2-shaped synthetic batch and a compressible
one of regular files under /usr/lib.  The batch's chunk rows are dealt into TEN zpacks (mi_batch_zpack_chunks); a set built of
the ten (mi_zset_add_zpack) is pruned to a random 90 %, 50 % and 10 % of its digests (MI_ZSET_PRUNE_KEEP, 500 permille).  Per
fraction, in the same run, each path in a loop of its own over a FRESH set, median of the runs after a warm-up:
    mi_zset_prune      device time (mi_prune_info: ms_mark, ms_move, ms_rebuild -- HIP events), the call's wall time, what the
                       call allocated at its peak (peak_extra_bytes, from the sizes) and the change of hipMemGetInfo's free
                       bytes across the call (negative: the device got memory BACK);
    the existing path  INTEGRATION's compaction: mi_zset_zpack of the survivors + mi_zset_create + mi_zset_add_zpack -- the wall
                       time of the three calls, the zpack's device time (ms_compact) and the fall of the free bytes at the peak,
                       before the zpack and the old set are freed.
No threshold on any time.  The GPU step is a process of its own under a time limit: `chunk_zprune_bench.py` starts
`chunk_zprune_bench.py --step ...` with timeout(1) and writes nothing if it fails.
chunk_zprune_bench.py [out = profiles/chunk_zprune.txt] [files = 20000] [runs = 10] [bytes = 2e9]   (needs an MI355X)"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEP_LIMIT_S = 420
N_PACKS = 10
PERMILLE = 500


def med(x):
    return statistics.median(x), min(x), max(x)


def free_bytes(hip):
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def leg(eng, hip, b, name, runs, say):
    b.run()
    chunks = b.chunks()
    n_rows = len(chunks)
    zpacks = []
    for k in range(N_PACKS):                                                      # row r goes into zpack r mod 10
        select = np.zeros(n_rows, dtype=np.uint8)
        select[k::N_PACKS] = 1
        zpacks.append(b.zpack(select))
    try:
        def fresh():
            zs = eng.zset()
            for z in zpacks:
                zs.add_zpack(z)
            return zs

        with fresh() as zs:
            held, _, _ = zs.entries()
            held = held.copy()
            u = zs.usage()
            say("%s: %d chunk rows in %d zpacks; the set: %d digests, %d blobs, %d bytes resident, %d live, a table of %d slots" %
                (name, n_rows, N_PACKS, len(held), u.n_blobs, u.resident_bytes, u.live_bytes, u.table_slots))
        rng = np.random.default_rng(11)
        for percent in (90, 50, 10):
            keep = np.ascontiguousarray(held[rng.permutation(len(held))[:len(held) * percent // 100]])
            dev, wall, net, old_wall, old_dev, old_fall = [], [], [], [], [], []
            info = None
            for k in range(runs + 2):                                              # two warm-up rounds
                with fresh() as zs:
                    f0 = free_bytes(hip)
                    t0 = time.perf_counter()
                    info = zs.prune(keep, keep=True, min_live_permille=PERMILLE)
                    t1 = time.perf_counter()
                    f1 = free_bytes(hip)
                    after = zs.usage()
                if k >= 2:
                    dev.append((info.ms_mark, info.ms_move, info.ms_rebuild))
                    wall.append((t1 - t0) * 1e3)
                    net.append(f0 - f1)
            for k in range(runs + 2):
                old = fresh()
                f0 = free_bytes(hip)
                t0 = time.perf_counter()
                z = old.zpack(keep)
                new = eng.zset()
                new.add_zpack(z)
                t1 = time.perf_counter()
                f1 = free_bytes(hip)                                               # the peak: the old set, the zpack and the new set
                ms = z.info.ms_compact
                assert new.info.n_digests == len(keep)
                z.close()
                old.close()
                new.close()
                if k >= 2:
                    old_wall.append((t1 - t0) * 1e3)
                    old_dev.append(ms)
                    old_fall.append(f0 - f1)
            say("    keep %d %% (%d of %d digests) at %d permille: %d dropped, %d blobs freed (%d bytes), %d compacted, %d bytes moved, %d sparse kept; "
                "afterwards %d blobs, %d bytes resident, %d live, a table of %d slots" %
                (percent, len(keep), len(held), PERMILLE, info.n_dropped, info.n_blobs_freed, info.freed_bytes, info.n_blobs_compacted,
                 info.moved_bytes, info.n_blobs_sparse_kept, after.n_blobs, after.resident_bytes, after.live_bytes, after.table_slots))
            mark, move, rebuild = (med([d[i] for d in dev]) for i in range(3))
            total = med([sum(d) for d in dev])
            say("        mi_zset_prune, median of %d runs (min, max): device %.3f ms (%.3f, %.3f) = mark %.3f + move %.3f + rebuild %.3f; the call "
                "%.3f ms (%.3f, %.3f); allocated at its peak %d bytes; free bytes fell by %d across the call" %
                ((len(dev),) + total + (mark[0], move[0], rebuild[0]) + med(wall) + (info.peak_extra_bytes, int(med(net)[0]))))
            say("        mi_zset_zpack + mi_zset_create + mi_zset_add_zpack, median of %d runs (min, max): the calls %.3f ms (%.3f, %.3f), the "
                "cut's device time %.3f ms; free bytes fell by %d at the peak" % ((len(old_wall),) + med(old_wall) + (med(old_dev)[0], int(med(old_fall)[0]))))
            say("        calls, existing / new: %.2f; peak bytes, existing / new: %.2f" %
                (med(old_wall)[0] / med(wall)[0], med(old_fall)[0] / max(1, info.peak_extra_bytes)))
    finally:
        for z in zpacks:
            z.close()


def step(n_files, runs, limit):
    import makisu_amd as M
    from makisu_amd import workloads as W
    from chunk_pack_bench import _hip
    from chunk_zpack_bench import usr_lib_files

    def say(s):
        print(s, flush=True)

    hip = _hip()
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    with M.Engine(device=0) as eng:
        say("pruning compressed pack sets in place (tools/chunk_zprune_bench.py %d %d %d) on %s" % (n_files, runs, limit, eng.device_info()["name"]))
        sh = W.c2(files_per_gpu=n_files)
        with eng.batch(sh.n_files, W.batch_bytes_hint(sh)) as b:
            W.fill_batch(b, sh)
            leg(eng, hip, b, "incompressible leg -- %d synthetic files x 64 KiB, RANDOM bytes: every chunk is stored raw" % sh.n_files, runs, say)
        files, total = usr_lib_files(limit)
        say("compressible leg -- %d regular files under /usr/lib, %d bytes:" % (len(files), total))
        with eng.batch(len(files), total + 4096 * len(files)) as b:
            b.add_paths([p for p, _ in files], [s for _, s in files])
            leg(eng, hip, b, "the files", runs, say)


def main():
    if sys.argv[1:2] == ["--step"]:
        return step(int(sys.argv[2]), int(sys.argv[3]), int(float(sys.argv[4])))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zprune.txt")
    n_files = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    runs = max(10, int(sys.argv[3])) if len(sys.argv) > 3 else 10
    limit = sys.argv[4] if len(sys.argv) > 4 else "2e9"
    # the one GPU step, a fresh process under its own time limit; nothing is started after a failure
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", str(n_files), str(runs), limit]
    p = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(p.stdout)
    sys.stderr.write(p.stderr[-4000:])
    if p.returncode != 0:
        sys.exit("the measuring step ended with status %d: nothing written" % p.returncode)
    with open(out, "w") as f:
        f.write(p.stdout)


if __name__ == "__main__":
    main()
