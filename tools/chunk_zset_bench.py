"""Compressed pack sets, measured (writes profiles/chunk_zset.txt).

The two legs of tools/chunk_zpack_bench.py (4.9): an incompressible C2-shaped synthetic batch (every chunk stored raw) and a
compressible one of regular files under /usr/lib.  Each batch is packed whole and compressed once; the zpack feeds a compressed
set (mi_zset_add_zpack) and, for the comparison, a plain set (mi_packset_add_zpack).  Everything compared is measured in the
same run, median of the runs after a warm-up, device times from HIP events where the library takes them:
    (a) the cut      mi_zset_zpack of half the distinct chunks in random order (mi_zpack_info.ms_compact: lookup, scan and
                     gather) next to mi_packset_pack + mi_pack_compress for the same request (ms_gather + ms_encode +
                     ms_compact: the plain cut's own lookup is not in its events, so the existing path is UNDERSTATED), and
                     both calls' wall time;
    (b) the restore  mi_batch_add_zrecipes of every file (ms_resolve + ms_assemble) next to mi_packset_add_zpack (wall: it
                     decodes the whole zpack into a plain blob) + mi_batch_add_recipes (ms_resolve + ms_assemble), and next to
                     a hipMemcpyAsync device-to-device of the plain byte count.
No threshold on any time.  Each GPU step is a process of its own under a time limit: `chunk_zset_bench.py` starts
`chunk_zset_bench.py --step ...` with timeout(1) and stops at the first step that fails.
chunk_zset_bench.py [out = profiles/chunk_zset.txt] [files = 20000] [runs = 10] [bytes = 2e9]   (needs an MI355X)"""
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


def leg(eng, hip, b, name, runs, say):
    from chunk_pack_bench import d2d_copy_ms
    b.run()
    chunks = b.chunks()
    fr = b.files()
    dig_col = "sha256"
    counts = np.bincount(chunks["file_index"].astype(np.int64), minlength=len(fr))
    bounds = np.concatenate([[0], np.cumsum(counts)])
    assert (np.diff(chunks["file_index"].astype(np.int64)) >= 0).all()
    recipes = [(np.ascontiguousarray(chunks[dig_col][a:z]), chunks["length"][a:z].astype(np.uint32)) for a, z in zip(bounds, bounds[1:])]
    n_bytes = int(fr["size"].sum())
    rng = np.random.default_rng(7)
    with b.pack() as p, p.compress() as z, eng.zset() as zs, eng.packset() as ps:
        zi = z.info.as_dict()
        zs.add_zpack(z)
        ps.add_zpack(z)
        cb = zi["chunk_bytes"]
        say("%s: %d files, %d chunk rows, %d file bytes; the zpack: %d entries (%d raw), stored / chunk bytes %.4f, blob %d bytes" %
            (name, len(fr), len(chunks), n_bytes, zi["n_entries"], zi["n_raw"], zi["stored_bytes"] / cb, zi["blob_bytes"]))
        # (a) the cut
        distinct = np.unique(chunks[dig_col], axis=0)
        request = np.ascontiguousarray(distinct[rng.permutation(len(distinct))[:len(distinct) // 2]])
        cut, cut_wall, old, old_wall, cut_bytes = [], [], [], [], 0
        for k in range(runs + 2):                                                 # two warm-up rounds
            t0 = time.perf_counter()
            with zs.zpack(request) as c:
                t1 = time.perf_counter()
                ci = c.info.as_dict()
            t2 = time.perf_counter()
            with ps.pack(request) as sub:
                with sub.compress() as again:
                    t3 = time.perf_counter()
                    oi, gi = again.info.as_dict(), sub.info.as_dict()
            assert (oi["blob_bytes"], oi["stored_bytes"]) == (ci["blob_bytes"], ci["stored_bytes"])
            if k >= 2:
                cut.append(ci["ms_compact"])
                cut_wall.append((t1 - t0) * 1e3)
                old.append(gi["ms_gather"] + oi["ms_encode"] + oi["ms_compact"])
                old_wall.append((t3 - t2) * 1e3)
            cut_bytes = ci["chunk_bytes"]
        say("    (a) a compressed sub-pack of %d of the %d distinct chunks in random order, %d chunk bytes; median of %d runs (min, max):" %
            (len(request), len(distinct), cut_bytes, len(cut)))
        say("        mi_zset_zpack, device (lookup + scan + gather): %.3f ms (%.3f, %.3f); the call: %.3f ms (%.3f, %.3f)" % (med(cut) + med(cut_wall)))
        say("        mi_packset_pack + mi_pack_compress, device (gather + encode + compact, without the plain cut's lookup): %.3f ms (%.3f, %.3f); "
            "the calls: %.3f ms (%.3f, %.3f)" % (med(old) + med(old_wall)))
        say("        device times, existing / new: %.1f; calls: %.1f" % (med(old)[0] / med(cut)[0], med(old_wall)[0] / med(cut_wall)[0]))
        # (b) the restore
        new, new_resolve, exist, exist_add, exist_resolve = [], [], [], [], []
        for k in range(runs + 2):
            with eng.batch(len(fr), n_bytes + 4096 * len(fr)) as r:
                st = r.add_zrecipes(zs, recipes)
            with eng.packset() as fresh:
                t0 = time.perf_counter()
                fresh.add_zpack(z)
                t1 = time.perf_counter()
                with eng.batch(len(fr), n_bytes + 4096 * len(fr)) as r:
                    so = r.add_recipes(fresh, recipes)
            if k >= 2:
                new.append(st.ms_assemble)
                new_resolve.append(st.ms_resolve)
                exist.append(so.ms_assemble)
                exist_resolve.append(so.ms_resolve)
                exist_add.append((t1 - t0) * 1e3)
        gbs = lambda ms: n_bytes / (ms * 1e-3) / 1e9                              # noqa: E731
        say("    (b) every file rebuilt from its recipe, %d rows, %d bytes; median of %d runs (min, max), GB/s of file bytes:" %
            (len(chunks), n_bytes, len(new)))
        say("        mi_batch_add_zrecipes: the fused kernel %.3f ms (%.3f, %.3f) = %.2f GB/s; its resolve %.3f ms" %
            (med(new) + (gbs(med(new)[0]), med(new_resolve)[0])))
        say("        mi_packset_add_zpack (the call: decode into a plain blob, table) %.3f ms (%.3f, %.3f) + mi_batch_add_recipes: the assemble "
            "kernel %.3f ms (%.3f, %.3f) = %.2f GB/s; its resolve %.3f ms" % (med(exist_add) + med(exist) + (gbs(med(exist)[0]), med(exist_resolve)[0])))
        say("        fused / (add_zpack + assemble): %.2f; fused / assemble alone: %.2f" %
            (med(new)[0] / (med(exist_add)[0] + med(exist)[0]), med(new)[0] / med(exist)[0]))
        ptr, nb = p.device()
        copy = d2d_copy_ms(hip, C.c_void_p(ptr), nb, runs)
        say("        hipMemcpyAsync device-to-device of the plain %d bytes, the same run: %.3f ms (%.3f, %.3f) = %.2f GB/s; fused / copy: %.1f" %
            ((nb,) + med(copy) + (nb / (med(copy)[0] * 1e-3) / 1e9, med(new)[0] / med(copy)[0])))


def step(n_files, runs, limit):
    import makisu_amd as M
    from makisu_amd import workloads as W
    from chunk_pack_bench import _hip
    from chunk_zpack_bench import usr_lib_files

    def say(s):
        print(s, flush=True)

    hip = _hip()
    with M.Engine(device=0) as eng:
        say("compressed pack sets (tools/chunk_zset_bench.py %d %d %d) on %s" % (n_files, runs, limit, eng.device_info()["name"]))
        sh = W.c2(files_per_gpu=n_files)
        with eng.batch(sh.n_files, W.batch_bytes_hint(sh)) as b:
            W.fill_batch(b, sh)
            leg(eng, hip, b, "incompressible leg -- %d synthetic files x 64 KiB, RANDOM bytes: every chunk is stored raw, the fused kernel's "
                "raw copy only" % sh.n_files, runs, say)
        files, total = usr_lib_files(limit)
        say("compressible leg -- %d regular files under /usr/lib, %d bytes, largest first:" % (len(files), total))
        for p, size in files[:12]:
            say("        %12d  %s" % (size, p))
        if len(files) > 12:
            say("        ... and %d smaller ones" % (len(files) - 12))
        with eng.batch(len(files), total + 4096 * len(files)) as b:
            b.add_paths([p for p, _ in files], [s for _, s in files])
            leg(eng, hip, b, "the files", runs, say)


def main():
    if sys.argv[1:2] == ["--step"]:
        return step(int(sys.argv[2]), int(sys.argv[3]), int(float(sys.argv[4])))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zset.txt")
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
