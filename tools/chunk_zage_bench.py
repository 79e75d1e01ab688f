"""A compressed pack set that ages, measured (writes profiles/chunk_zage.txt).

Three inputs: a set of 10^6 digests (tiny raw chunks of 8..12 bytes under opaque digests, one 16-byte unit each, in the manner of
tests/store_rows_cases.py) and the two corpora of tools/chunk_zprune_bench.py (4.12) at its sizes.  Each input is TEN zpacks; a
fresh set takes zpack k at epoch k + 1, so a tenth of the entries carries each stamp (a digest that several zpacks bring keeps
the last one's).  Per input, in the same run, medians of the runs after two warm-up rounds:
    touch     mi_zset_touch of every held digest at epoch 11: the kernel's device time (ms_touch, HIP events) and the call;
    census    mi_zset_age_census with 16 bounds: the call's wall time (the call reports no device time);
    expire    mi_zset_expire(E, 500 permille) for the E that drops about 10, 50 and 90 %: device time (mi_prune_info: ms_mark,
              ms_move, ms_rebuild -- HIP events) and the call -- next to the only path there was: mi_zset_prune(DROP) of a twin set
              with the same digests uploaded as a list (device time and the call), and the same plus the host-side filter that
              builds the list from a numpy timestamp array kept beside the digests.
No threshold on any time; the tool asserts correctness only: both paths leave equal sets.  The GPU step is a process of its own
under a time limit: `chunk_zage_bench.py` starts `chunk_zage_bench.py --step ...` with timeout(1) and writes nothing if it fails.
chunk_zage_bench.py [out = profiles/chunk_zage.txt] [files = 4000] [runs = 10] [bytes = 4e8] [digests = 1000000]   (needs an MI355X)"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEP_LIMIT_S = 400
N_PACKS = 10
PERMILLE = 500
ODD = 0x9E3779B97F4A7C15


def med(x):
    return statistics.median(x), min(x), max(x)


def tiny_zpacks(M, n):
    """n rows of 8..12 bytes, each one unit of its blob, stored as they are, under opaque digests whose first eight bytes are the
    row's number + 1 -> [(zentries, zblob)] * N_PACKS: row r goes into zpack r mod 10"""
    k = np.arange(1, n + 1, dtype=np.uint64)
    dig = np.random.default_rng(18).integers(0, 256, (n, 32), dtype=np.uint8)
    dig[:, :8] = k.astype("<u8").view(np.uint8).reshape(n, 8)
    lengths = (8 + k % 5).astype(np.uint32)
    blob = np.zeros((n, 16), dtype=np.uint8)
    blob[:, :8] = (k * np.uint64(ODD)).astype("<u8").view(np.uint8).reshape(n, 8)
    for i in range(4):
        blob[(k % 5) > i, 8 + i] = 0x51 + i
    out = []
    for p in range(N_PACKS):
        rows = np.arange(p, n, N_PACKS)
        ze = np.zeros(len(rows), dtype=M.ZPACK_ENTRY_DTYPE)
        ze["digest"], ze["offset"], ze["chunk_index"] = dig[rows], np.arange(len(rows), dtype=np.uint64) * 16, np.arange(len(rows))
        ze["length"] = ze["stored"] = lengths[rows]
        out.append((ze, np.ascontiguousarray(blob[rows]).tobytes()))
    return out


def held_sorted(zs):
    d, _, _ = zs.entries()
    return np.sort(np.ascontiguousarray(d).view([("a", "<u8"), ("b", "<u8"), ("c", "<u8"), ("d", "<u8")]).reshape(-1))


def leg(name, fresh, runs, say):
    """fresh() -> a new set with the ten zpacks added at epochs 1..10"""
    with fresh() as zs:
        held = zs.entries()[0].copy()
        ts = zs.stamps(held).copy()                                                # the host's timestamp array, beside its digests
        u = zs.usage()
        say("%s: the set: %d digests, %d blobs, %d bytes resident, %d live, a table of %d slots, %d bytes of stamps" %
            (name, len(held), u.n_blobs, u.resident_bytes, u.live_bytes, u.table_slots, zs.epoch[2]))
        zs.set_epoch(N_PACKS + 1)
        dev, wall = [], []
        for k in range(runs + 2):
            zs.set_epoch(N_PACKS + 1 + k)                                          # every run refreshes every digest
            t0 = time.perf_counter()
            info = zs.touch(held)
            t1 = time.perf_counter()
            assert (info.n_unknown, info.n_refreshed) == (0, len(held))
            if k >= 2:
                dev.append(info.ms_touch)
                wall.append((t1 - t0) * 1e3)
        say("    mi_zset_touch of all %d digests (%d bytes uploaded), median of %d runs (min, max): device %.3f ms (%.3f, %.3f); the call %.3f ms "
            "(%.3f, %.3f)" % ((len(held), 32 * len(held), len(dev)) + med(dev) + med(wall)))
    with fresh() as zs:
        bounds = np.arange(1, 17, dtype=np.uint32)
        wall = []
        for k in range(runs + 2):
            t0 = time.perf_counter()
            bins = zs.age_census(bounds)
            t1 = time.perf_counter()
            assert sum(b.n_digests for b in bins) == len(held)
            if k >= 2:
                wall.append((t1 - t0) * 1e3)
        say("    mi_zset_age_census with %d bounds, median of %d runs (min, max): the call %.3f ms (%.3f, %.3f)" % ((len(bounds), len(wall)) + med(wall)))
    for min_epoch in (2, 6, 10):
        dev, wall, old_dev, old_wall, filt = [], [], [], [], []
        info = old = None
        for k in range(runs + 2):
            with fresh() as zs:
                t0 = time.perf_counter()
                info = zs.expire(min_epoch, PERMILLE)
                t1 = time.perf_counter()
                after, left = zs.usage(), held_sorted(zs) if k == 0 else None
            with fresh() as zt:
                t2 = time.perf_counter()
                victims = np.ascontiguousarray(held[ts < min_epoch])               # the host-side filter over its timestamps
                t3 = time.perf_counter()
                old = zt.prune(victims, keep=False, min_live_permille=PERMILLE)
                t4 = time.perf_counter()
                if k == 0:                                                         # correctness only: both paths leave equal sets
                    assert np.array_equal(left, held_sorted(zt)) and zt.usage().as_dict() == after.as_dict()
                    assert (info.n_dropped, info.moved_bytes, info.freed_bytes) == (old.n_dropped, old.moved_bytes, old.freed_bytes) and old.n_unknown == 0
            if k >= 2:
                dev.append((info.ms_mark, info.ms_move, info.ms_rebuild))
                wall.append((t1 - t0) * 1e3)
                old_dev.append(old.ms_mark + old.ms_move + old.ms_rebuild)
                old_wall.append((t4 - t3) * 1e3)
                filt.append((t3 - t2) * 1e3)
        say("    expire below epoch %d at %d permille: %d of %d digests dropped (%.1f %%), %d blobs freed (%d bytes), %d compacted, %d bytes moved; "
            "afterwards %d blobs, %d bytes resident, a table of %d slots" %
            (min_epoch, PERMILLE, info.n_dropped, len(held), 100.0 * info.n_dropped / len(held), info.n_blobs_freed, info.freed_bytes,
             info.n_blobs_compacted, info.moved_bytes, after.n_blobs, after.resident_bytes, after.table_slots))
        mark, move, rebuild = (med([d[i] for d in dev]) for i in range(3))
        say("        mi_zset_expire, median of %d runs (min, max): device %.3f ms (%.3f, %.3f) = mark %.3f + move %.3f + rebuild %.3f; the call %.3f ms "
            "(%.3f, %.3f); allocated at its peak %d bytes" %
            ((len(dev),) + med([sum(d) for d in dev]) + (mark[0], move[0], rebuild[0]) + med(wall) + (info.peak_extra_bytes,)))
        say("        mi_zset_prune(DROP) with the %d digests as a list (%d bytes uploaded), median of %d runs (min, max): device %.3f ms (%.3f, %.3f); "
            "the call %.3f ms (%.3f, %.3f); the host-side filter that builds the list %.3f ms (%.3f, %.3f); allocated at its peak %d bytes" %
            ((old.n_rows, 32 * old.n_rows, len(old_dev)) + med(old_dev) + med(old_wall) + med(filt) + (old.peak_extra_bytes,)))
        say("        the calls, list / expire: %.2f; with the filter: %.2f" %
            (med(old_wall)[0] / med(wall)[0], (med(old_wall)[0] + med(filt)[0]) / med(wall)[0]))


def step(n_files, runs, limit, n_digests):
    import makisu_amd as M
    from makisu_amd import workloads as W
    from chunk_zpack_bench import usr_lib_files

    def say(s):
        print(s, flush=True)

    with M.Engine(device=0) as eng:
        say("a compressed pack set that ages (tools/chunk_zage_bench.py %d %d %d %d) on %s" % (n_files, runs, limit, n_digests, eng.device_info()["name"]))

        def aged(add_all):
            def fresh():
                zs = eng.zset()
                zs.set_epoch(1)
                for k in range(N_PACKS):
                    zs.set_epoch(k + 1)
                    add_all(zs, k)
                return zs
            return fresh

        packs = tiny_zpacks(M, n_digests)
        leg("%d tiny raw chunks of 8..12 bytes under opaque digests, ten zpacks from host memory" % n_digests,
            aged(lambda zs, k: zs.add_zblob(packs[k][1], packs[k][0])), runs, say)

        def batch_leg(b, name):
            b.run()
            n_rows = len(b.chunks())
            zpacks = []
            for k in range(N_PACKS):                                               # row r goes into zpack r mod 10
                select = np.zeros(n_rows, dtype=np.uint8)
                select[k::N_PACKS] = 1
                zpacks.append(b.zpack(select))
            try:
                leg("%s: %d chunk rows in %d zpacks" % (name, n_rows, N_PACKS), aged(lambda zs, k: zs.add_zpack(zpacks[k])), runs, say)
            finally:
                for z in zpacks:
                    z.close()

        sh = W.c2(files_per_gpu=n_files)
        with eng.batch(sh.n_files, W.batch_bytes_hint(sh)) as b:
            W.fill_batch(b, sh)
            batch_leg(b, "incompressible leg -- %d synthetic files x 64 KiB, RANDOM bytes: every chunk is stored raw" % sh.n_files)
        files, total = usr_lib_files(limit)
        with eng.batch(len(files), total + 4096 * len(files)) as b:
            b.add_paths([p for p, _ in files], [s for _, s in files])
            batch_leg(b, "compressible leg -- %d regular files under /usr/lib, %d bytes" % (len(files), total))


def main():
    if sys.argv[1:2] == ["--step"]:
        return step(int(sys.argv[2]), int(sys.argv[3]), int(float(sys.argv[4])), int(float(sys.argv[5])))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zage.txt")
    n_files = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    runs = max(10, int(sys.argv[3])) if len(sys.argv) > 3 else 10
    limit = sys.argv[4] if len(sys.argv) > 4 else "4e8"
    n_digests = sys.argv[5] if len(sys.argv) > 5 else "1000000"
    # the one GPU step, a fresh process under its own time limit; nothing is started after a failure
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", str(n_files), str(runs), limit, n_digests]
    p = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(p.stdout)
    sys.stderr.write(p.stderr[-4000:])
    if p.returncode != 0:
        sys.exit("the measuring step ended with status %d: nothing written" % p.returncode)
    with open(out, "w") as f:
        f.write(p.stdout)


if __name__ == "__main__":
    main()
