"""The two cuts for plainer readers, measured (writes profiles/chunk_zserve.txt).

The two inputs of tools/chunk_zentropy_bench.py at its sizes: an incompressible C2-shaped synthetic batch and a compressible one
of regular files under /usr/lib.  The batch's chunk rows are gathered into one pack, coded at level 1 with MI_ZPACK_ENTROPY (a
densified set: what INTEGRATION's "ingest at level 1, densify at rest" ends up holding) and added to a compressed set; HALF of the
set's digests are requested in random order.  In the same run, each path in a loop of its own, median of the runs after two
warm-up rounds:
    the plain cut       mi_zset_pack next to the composition of existing calls that gives the same bytes: mi_zset_zpack +
                        mi_packset_add_zpack (into a throwaway set) + mi_packset_pack;
    the unwrapped cut   mi_zset_zpack_unwrapped next to the plain-cut composition + mi_pack_compress at level 1.
Per path: the calls' wall time (every call blocks on the ctx stream), the device times the results report (HIP events: the new
calls' ms_compact / ms_gather; of the compositions the cuts' and the coder's -- the decode into the throwaway set reports none)
and the fall of hipMemGetInfo's free bytes while everything the path made is alive.  The bytes of both paths are compared once.
No threshold on any time.  The GPU step is a process of its own under a time limit: `chunk_zserve_bench.py` starts
`chunk_zserve_bench.py --step ...` with timeout(1) and writes nothing if it fails.
chunk_zserve_bench.py [out = profiles/chunk_zserve.txt] [files = 4000] [runs = 10] [bytes = 4e8]   (needs an MI355X)"""
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


def med(x):
    return statistics.median(x), min(x), max(x)


def free_bytes(hip):
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def measure(hip, runs, path):
    """path() -> (device ms, [handles to close], how to read the result's bytes); -> wall, device, fall of the free bytes, and the
    last run's bytes (read outside the timed part)"""
    wall, dev, fall, last = [], [], [], None
    for k in range(runs + 2):                                                      # two warm-up rounds
        f0 = free_bytes(hip)
        t0 = time.perf_counter()
        ms, handles, read = path()
        t1 = time.perf_counter()
        f1 = free_bytes(hip)                                                       # everything the path made is alive
        if k == runs + 1:
            last = read()
        for h in handles:
            h.close()
        if k >= 2:
            wall.append((t1 - t0) * 1e3)
            dev.append(ms)
            fall.append(f0 - f1)
    return wall, dev, fall, last


def leg(eng, hip, b, name, runs, say):
    b.run()
    with b.pack() as p, p.compress(level=1, entropy=True) as dense, eng.zset() as zs:
        zs.add_zpack(dense)
        held, lens, _ = zs.entries()
        rng = np.random.default_rng(417)
        pick = rng.permutation(len(held))[: len(held) // 2]
        req, req_len = np.ascontiguousarray(held[pick].copy()), lens[pick].astype(np.uint32).copy()
        say("%s: %d chunk rows, %d chunk bytes; the densified set: %d digests, %d stored bytes, forms %r; requested: %d digests, %d chunk bytes, in random order" %
            (name, len(p), p.info.chunk_bytes, len(held), zs.info.stored_bytes, zs.count_forms().as_dict(), len(req), int(req_len.sum())))

        def new_plain():
            r = zs.pack(req, req_len)
            return r.info.ms_gather, [r], r.bytes

        def old_plain():
            z = zs.zpack(req, req_len)
            ps = eng.packset()
            ps.add_zpack(z)
            r = ps.pack(req, req_len)
            return z.info.ms_compact + r.info.ms_gather, [r, ps, z], r.bytes

        def new_unwrapped():
            r = zs.zpack_unwrapped(req, req_len)
            return r.info.ms_compact, [r], r.read

        def old_unwrapped():
            z = zs.zpack(req, req_len)
            ps = eng.packset()
            ps.add_zpack(z)
            q = ps.pack(req, req_len)
            r = q.compress(level=1)
            return z.info.ms_compact + q.info.ms_gather + r.info.ms_encode + r.info.ms_compact, [r, q, ps, z], r.read

        for what, new, old, new_name, old_name, old_note in (
                ("the plain cut", new_plain, old_plain, "mi_zset_pack", "mi_zset_zpack + mi_packset_add_zpack + mi_packset_pack",
                 "the two cuts' device time (the decode into the throwaway set reports none)"),
                ("the unwrapped cut", new_unwrapped, old_unwrapped, "mi_zset_zpack_unwrapped",
                 "mi_zset_zpack + mi_packset_add_zpack + mi_packset_pack + mi_pack_compress(level 1)",
                 "the cuts' and the coder's device time (the decode into the throwaway set reports none)")):
            nw, nd, nf, nb = measure(hip, runs, new)
            ow, od, of, ob = measure(hip, runs, old)
            say("    %s, %d bytes; both paths give the same bytes: %s" % (what, len(nb), "yes" if nb == ob else "NO"))
            say("        %s, median of %d runs (min, max): the call %.3f ms (%.3f, %.3f); device time it reports %.3f ms (%.3f, %.3f); free bytes fell by %d "
                "while the result lives" % ((new_name, len(nw)) + med(nw) + med(nd) + (int(med(nf)[0]),)))
            say("        %s, median of %d runs (min, max): the calls %.3f ms (%.3f, %.3f); %s %.3f ms (%.3f, %.3f); free bytes fell by %d at the peak" %
                ((old_name, len(ow)) + med(ow) + (old_note,) + med(od) + (int(med(of)[0]),)))
            ratio = med(nw)[0] / med(ow)[0]
            say("        the new call takes %.3f of the composition's wall time%s" % (ratio, "" if ratio < 1 else ": THE NEW CALL IS NOT FASTER"))


def step(n_files, runs, limit):
    import makisu_amd as M
    from makisu_amd import workloads as W
    from chunk_pack_bench import _hip
    from chunk_zpack_bench import usr_lib_files

    def say(s):
        print(s, flush=True)

    hip = _hip()
    with M.Engine(device=0) as eng:
        say("the cuts for plainer readers (tools/chunk_zserve_bench.py %d %d %d) on %s" % (n_files, runs, limit, eng.device_info()["name"]))
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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zserve.txt")
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
