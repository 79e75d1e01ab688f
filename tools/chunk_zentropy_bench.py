"""The zpack entropy stage, measured (writes profiles/chunk_zentropy.txt).

The two inputs of tools/chunk_zrecode_bench.py at its sizes: an incompressible C2-shaped synthetic batch and a compressible one of
regular files under /usr/lib.  The batch's chunk rows are gathered into one pack (mi_batch_pack_chunks).  In the same run, each
path in a loop of its own, median of the runs after a warm-up:
    encode    mi_pack_compress at level 1 without and with MI_ZPACK_ENTROPY: the coder's device time (ms_encode: with the flag
              the LZ4 kernel and the entropy kernel behind it) and the layout's (ms_compact), the call's wall time, the stored
              bytes and the census of the forms (mi_zpack_count_forms);
    restore   mi_batch_add_zrecipes of every held chunk as one file from a set of the level-1 zpack and from a set of the zpack
              with form H: ms_assemble (HIP events around the classify launch, the unwrap where there is one, and the fused
              kernel) and the call's wall time;
    classify  what the stage costs a reader where NO form H is: the level-1 row above carries one classify launch and its
              synchronisation; mi_zset_count_forms on that set is the same launch over the set's table, timed alone (wall).
    recode    mi_zset_recode of a fresh set of the level-1 zpack at level 1 with MI_ZPACK_ENTROPY and at level 2 without it: the
              device times mi_recode_info reports, the call's wall time and the bytes won back.
No threshold on any time.  The GPU step is a process of its own under a time limit: `chunk_zentropy_bench.py` starts
`chunk_zentropy_bench.py --step ...` with timeout(1) and writes nothing if it fails.
chunk_zentropy_bench.py [out = profiles/chunk_zentropy.txt] [files = 4000] [runs = 10] [bytes = 4e8]   (needs an MI355X)"""
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


def med(x):
    return statistics.median(x), min(x), max(x)


def leg(eng, b, name, runs, say):
    b.run()
    with b.pack() as p:
        say("%s: %d chunk rows, %d chunk bytes in one pack" % (name, len(p), p.info.chunk_bytes))
        kept = {}
        for entropy in (False, True):
            dev, lay, wall = [], [], []
            for k in range(runs + 2):                                              # two warm-up rounds
                t0 = time.perf_counter()
                z = p.compress(level=1, entropy=entropy)
                t1 = time.perf_counter()
                if k >= 2:
                    dev.append(z.info.ms_encode)
                    lay.append(z.info.ms_compact)
                    wall.append((t1 - t0) * 1e3)
                if k == runs + 1:
                    kept[entropy] = z
                else:
                    z.close()
            z = kept[entropy]
            say("    mi_pack_compress(level 1%s): %d stored bytes of %d (%.4f), forms %r" %
                (", ENTROPY" if entropy else "", z.info.stored_bytes, z.info.chunk_bytes, z.info.stored_bytes / max(1, z.info.chunk_bytes),
                 z.count_forms().as_dict()))
            say("        median of %d runs (min, max): ms_encode %.3f (%.3f, %.3f), ms_compact %.3f (%.3f, %.3f), the call %.3f ms (%.3f, %.3f)" %
                ((len(dev),) + med(dev) + med(lay) + med(wall)))
        try:
            say("    stored with the stage / without: %.4f" % (kept[True].info.stored_bytes / max(1, kept[False].info.stored_bytes)))
            for entropy in (False, True):
                with eng.zset() as zs:
                    zs.add_zpack(kept[entropy])
                    dig, lens, _ = zs.entries()
                    dig, lens = np.ascontiguousarray(dig.copy()), lens.astype(np.uint32).copy()
                    dev, wall, count = [], [], []
                    for k in range(runs + 2):
                        with eng.batch(1, int(lens.sum()) + 65536) as r:
                            t0 = time.perf_counter()
                            st = r.add_zrecipes(zs, [(dig, lens)])
                            t1 = time.perf_counter()
                        t2 = time.perf_counter()
                        zs.count_forms()
                        t3 = time.perf_counter()
                        if k >= 2:
                            dev.append(st.ms_assemble)
                            wall.append((t1 - t0) * 1e3)
                            count.append((t3 - t2) * 1e3)
                    say("    mi_batch_add_zrecipes of %d rows, %d bytes, from the set %s form H: median of %d runs (min, max): ms_assemble %.3f (%.3f, %.3f), "
                        "the call %.3f ms (%.3f, %.3f); mi_zset_count_forms alone %.3f ms (%.3f, %.3f)" %
                        ((len(dig), int(lens.sum()), "WITH" if entropy else "without", len(dev)) + med(dev) + med(wall) + med(count)))
            for what, kw in (("level 1, ENTROPY", dict(level=1, entropy=True)), ("level 2", dict(level=2)), ("level 2, ENTROPY", dict(level=2, entropy=True))):
                dev, wall, info = [], [], None
                for k in range(min(runs, 5) + 1):                                  # (each run recodes a fresh set; one warm-up round)
                    with eng.zset() as zs:
                        zs.add_zpack(kept[False])
                        t0 = time.perf_counter()
                        info = zs.recode(**kw)
                        t1 = time.perf_counter()
                    if k >= 1:
                        dev.append((info.ms_decode, info.ms_encode, info.ms_move + info.ms_rebuild))
                        wall.append((t1 - t0) * 1e3)
                say("    mi_zset_recode(%s) of the level-1 set: %d of %d forms replaced, stored %d -> %d (%.4f); median of %d runs: decode %.3f + encode %.3f + "
                    "move and rebuild %.3f ms, the call %.3f ms (%.3f, %.3f); allocated at its peak %d bytes" %
                    ((what, info.n_recoded, info.n_digests, info.stored_before, info.stored_after, info.stored_after / max(1, info.stored_before), len(dev)) +
                     tuple(med([d[i] for d in dev])[0] for i in range(3)) + med(wall) + (info.peak_extra_bytes,)))
        finally:
            for z in kept.values():
                z.close()


def step(n_files, runs, limit):
    import makisu_amd as M
    from makisu_amd import workloads as W
    from chunk_zpack_bench import usr_lib_files

    def say(s):
        print(s, flush=True)

    with M.Engine(device=0) as eng:
        say("the zpack entropy stage (tools/chunk_zentropy_bench.py %d %d %d) on %s" % (n_files, runs, limit, eng.device_info()["name"]))
        sh = W.c2(files_per_gpu=n_files)
        with eng.batch(sh.n_files, W.batch_bytes_hint(sh)) as b:
            W.fill_batch(b, sh)
            leg(eng, b, "incompressible leg -- %d synthetic files x 64 KiB, RANDOM bytes: every chunk is stored raw" % sh.n_files, runs, say)
        files, total = usr_lib_files(limit)
        say("compressible leg -- %d regular files under /usr/lib, %d bytes:" % (len(files), total))
        with eng.batch(len(files), total + 4096 * len(files)) as b:
            b.add_paths([p for p, _ in files], [s for _, s in files])
            leg(eng, b, "the files", runs, say)


def main():
    if sys.argv[1:2] == ["--step"]:
        return step(int(sys.argv[2]), int(sys.argv[3]), int(float(sys.argv[4])))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zentropy.txt")
    n_files = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    runs = max(3, int(sys.argv[3])) if len(sys.argv) > 3 else 10
    limit = sys.argv[4] if len(sys.argv) > 4 else "4e8"
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
