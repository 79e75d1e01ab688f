"""Pruning the chunk index, measured (writes profiles/chunk_index_prune.txt).

An index of 10^6 and of 10^7 random digests (mi_index_import) is pruned to a random 90 %, 50 % and 10 % of them
(MI_INDEX_PRUNE_KEEP).  Per size and share, in the same run, each path in a loop of its own, medians after two warm-ups:
    mi_index_prune     over a FRESH index every run: device time (mi_index_prune_info: ms_mark + ms_rebuild -- HIP events on the
                       ctx stream), the call's wall time, what the call allocated at its peak (peak_extra_bytes, from the sizes);
    the existing path  the only one there was: mi_index_export, a numpy filter on the host (np.isin over the digests' first eight
                       bytes, which are distinct here), mi_index_create, mi_index_import of the survivors -- the wall time of
                       each step and of all four, and the fall of hipMemGetInfo's free bytes while both indexes exist.  The calls
                       run on the ctx stream and keep their times to themselves: there is no device time to report for them,
                       and the export's and the import's transient buffers (32 and 40 bytes a digest) are freed before the
                       free bytes can be read, so the fall understates that path's peak.
No threshold on any time.  The GPU step is a process of its own under a time limit: `chunk_index_prune_bench.py` starts
`chunk_index_prune_bench.py --step ...` with timeout(1), passes its lines on as they come and writes nothing if it fails.
chunk_index_prune_bench.py [out = profiles/chunk_index_prune.txt] [runs = 10] [sizes = 1000000,10000000]   (needs an MI355X)"""
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
STEP_LIMIT_S = 540


def med(x):
    return statistics.median(x), min(x), max(x)


def free_bytes(hip):
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def size_leg(eng, hip, n, runs, say):
    rng = np.random.default_rng(13)
    dig = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    first8 = np.ascontiguousarray(dig[:, :8]).view(np.uint64).reshape(-1)
    assert len(np.unique(first8)) == n
    blob = dig.tobytes()
    with eng.index() as src:
        t0 = time.perf_counter()
        assert src.load(blob) == n
        say("%d random digests: imported in %.1f ms" % (n, (time.perf_counter() - t0) * 1e3))
        for percent in (90, 50, 10):
            keep = np.ascontiguousarray(dig[rng.permutation(n)[:n * percent // 100]])
            keep8 = np.ascontiguousarray(keep[:, :8]).view(np.uint64).reshape(-1)
            dev, wall, info = [], [], None
            for k in range(runs + 2):                                              # two warm-up rounds
                with eng.index() as idx:
                    idx.load(blob)
                    t0 = time.perf_counter()
                    info = idx.prune(keep, keep=True)
                    t1 = time.perf_counter()
                    assert (info.n_after, info.rebuilt) == (len(keep), 1) and len(idx) == len(keep)
                if k >= 2:
                    dev.append((info.ms_mark, info.ms_rebuild))
                    wall.append((t1 - t0) * 1e3)
            steps, old_fall = [], []
            for k in range(runs + 2):
                f0 = free_bytes(hip)
                t0 = time.perf_counter()
                out = np.frombuffer(src.export(), dtype=np.uint8).reshape(-1, 32)
                t1 = time.perf_counter()
                stay = np.ascontiguousarray(out[np.isin(np.ascontiguousarray(out[:, :8]).view(np.uint64).reshape(-1), keep8)])
                t2 = time.perf_counter()
                new = eng.index(len(stay))
                t3 = time.perf_counter()
                assert new.load(stay.tobytes()) == len(keep)
                t4 = time.perf_counter()
                f1 = free_bytes(hip)                                               # both indexes exist
                new.close()
                if k >= 2:
                    steps.append(tuple((b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t3, t4), (t0, t4))))
                    old_fall.append(f0 - f1)
            say("    keep %d %% (%d of %d digests): %d dropped, the table %d -> %d slots" %
                (percent, len(keep), n, info.n_dropped, info.slots_before, info.slots_after))
            mark, rebuild = (med([d[i] for d in dev]) for i in range(2))
            say("        mi_index_prune, median of %d runs (min, max): device %.3f ms (%.3f, %.3f) = mark %.3f + rebuild %.3f; the call %.3f ms "
                "(%.3f, %.3f); allocated at its peak %d bytes" %
                ((len(dev),) + med([sum(d) for d in dev]) + (mark[0], rebuild[0]) + med(wall) + (info.peak_extra_bytes,)))
            e, f, c, i, t = (med([s[j] for s in steps]) for j in range(5))
            say("        export + numpy filter + create + import, median of %d runs (min, max): the four %.3f ms (%.3f, %.3f) = export %.3f + "
                "filter %.3f + create %.3f + import %.3f; free bytes fell by %d while both indexes exist" %
                ((len(steps),) + t + (e[0], f[0], c[0], i[0], int(med(old_fall)[0]))))
            say("        calls, existing / new: %.2f; without the host's filter: %.2f" % (t[0] / med(wall)[0], (t[0] - f[0]) / med(wall)[0]))


def step(runs, sizes):
    import makisu_amd as M
    from chunk_pack_bench import _hip

    def say(s):
        print(s, flush=True)

    hip = _hip()
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    with M.Engine(device=0) as eng:
        say("pruning the chunk index (tools/chunk_index_prune_bench.py %d %s) on %s" % (runs, ",".join(map(str, sizes)), eng.device_info()["name"]))
        for n in sizes:
            size_leg(eng, hip, n, runs, say)


def main():
    if sys.argv[1:2] == ["--step"]:
        return step(int(sys.argv[2]), [int(float(x)) for x in sys.argv[3].split(",")])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_index_prune.txt")
    runs = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
    sizes = sys.argv[3] if len(sys.argv) > 3 else "1000000,10000000"
    # the one GPU step, a fresh process under its own time limit; nothing is started after a failure
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", str(runs), sizes]
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    lines = []
    for line in p.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
        lines.append(line)
    if p.wait() != 0:
        sys.exit("the measuring step ended with status %d: nothing written" % p.returncode)
    with open(out, "w") as f:
        f.writelines(lines)


if __name__ == "__main__":
    main()
