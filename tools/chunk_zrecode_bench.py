"""Recoding a compressed pack set in place, measured (writes profiles/chunk_zrecode.txt).

The two corpora of tools/chunk_zprune_bench.py (4.12) at its sizes: an incompressible C2-shaped synthetic batch and a compressible
one of regular files under /usr/lib.  The batch's chunk rows are dealt into TEN level-1 zpacks (mi_batch_zpack_chunks); a set
built of the ten (mi_zset_add_zpack) is recoded at level 2.  In the same run, each path in a loop of its own over a FRESH set,
median of the runs after a warm-up:
    mi_zset_recode     with and without MI_ZSET_RECODE_VERIFY: device time (mi_recode_info: ms_decode, ms_encode, ms_move,
                       ms_rebuild, ms_verify -- HIP events), the call's wall time and what the call allocated at its peak
                       (peak_extra_bytes, from the sizes);
    the existing path  the only alternative there is without the call: mi_zset_zpack of everything, mi_packset_add_zpack (the
                       decode into a plain set), mi_packset_pack, mi_pack_compress(MI_ZPACK_LEVEL2) and a new set's
                       mi_zset_add_zpack -- the wall time of the calls, the device times they report (the cut's ms_compact, the
                       coder's ms_encode + ms_compact) and the fall of hipMemGetInfo's free bytes at the peak, before anything is
                       freed.  It holds level 2's form of EVERY chunk, the larger ones among them.
No threshold on any time.  The GPU step is a process of its own under a time limit: `chunk_zrecode_bench.py` starts
`chunk_zrecode_bench.py --step ...` with timeout(1) and writes nothing if it fails.
chunk_zrecode_bench.py [out = profiles/chunk_zrecode.txt] [files = 4000] [runs = 10] [bytes = 4e8]   (needs an MI355X)"""
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
PARTS = ("ms_decode", "ms_encode", "ms_move", "ms_rebuild", "ms_verify")


def med(x):
    return statistics.median(x), min(x), max(x)


def free_bytes(hip):
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def leg(eng, hip, b, name, runs, say):
    b.run()
    n_rows = len(b.chunks())
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
            held = np.ascontiguousarray(held.copy())
            u = zs.usage()
            say("%s: %d chunk rows in %d level-1 zpacks; the set: %d digests, %d blobs, %d bytes resident, %d live, %d stored" %
                (name, n_rows, N_PACKS, len(held), u.n_blobs, u.resident_bytes, u.live_bytes, zs.info.stored_bytes))
        for verify in (False, True):
            dev, wall = [], []
            info = None
            for k in range(runs + 2):                                              # two warm-up rounds
                with fresh() as zs:
                    t0 = time.perf_counter()
                    info = zs.recode(level=2, verify=verify)
                    t1 = time.perf_counter()
                    after = zs.usage()
                if k >= 2:
                    dev.append(tuple(getattr(info, p) for p in PARTS))
                    wall.append((t1 - t0) * 1e3)
            say("    mi_zset_recode(level 2%s): %d of %d forms replaced (%d were raw), %d undecodable; stored %d -> %d (%.4f), live %d -> %d; %d blobs "
                "rewritten into one of %d bytes, %d bytes freed; %d round(s); afterwards %d blobs, %d bytes resident" %
                (", VERIFY" if verify else "", info.n_recoded, info.n_digests, info.n_raw_recoded, info.n_undecodable, info.stored_before,
                 info.stored_after, info.stored_after / max(1, info.stored_before), info.live_before, info.live_after, info.n_blobs_rewritten,
                 info.new_blob_bytes, info.freed_bytes, info.n_rounds, after.n_blobs, after.resident_bytes))
            parts = [med([d[i] for d in dev])[0] for i in range(len(PARTS))]
            say("        median of %d runs (min, max): device %.3f ms (%.3f, %.3f) = decode %.3f + encode %.3f + move %.3f + rebuild %.3f + verify %.3f; "
                "the call %.3f ms (%.3f, %.3f); allocated at its peak %d bytes" %
                ((len(dev),) + med([sum(d) for d in dev]) + tuple(parts) + med(wall) + (info.peak_extra_bytes,)))
        old_wall, old_dev, old_fall, stored = [], [], [], 0
        for k in range(runs + 2):
            old = fresh()
            f0 = free_bytes(hip)
            t0 = time.perf_counter()
            z = old.zpack(held)
            ps = eng.packset()
            ps.add_zpack(z)
            p = ps.pack(held)
            z2 = p.compress(level=2)
            new = eng.zset()
            new.add_zpack(z2)
            t1 = time.perf_counter()
            f1 = free_bytes(hip)                                                   # the peak: everything the path made is alive
            ms = z.info.ms_compact + z2.info.ms_encode + z2.info.ms_compact
            stored = new.info.stored_bytes
            assert new.info.n_digests == len(held)
            for h in (new, z2, p, ps, z, old):
                h.close()
            if k >= 2:
                old_wall.append((t1 - t0) * 1e3)
                old_dev.append(ms)
                old_fall.append(f0 - f1)
        say("    mi_zset_zpack + mi_packset_add_zpack + mi_packset_pack + mi_pack_compress(level 2) + mi_zset_add_zpack, median of %d runs (min, max): "
            "the calls %.3f ms (%.3f, %.3f); the cut's and the coder's device time %.3f ms (the decode and the plain cut report none); free bytes "
            "fell by %d at the peak; the new set stores %d bytes" % ((len(old_wall),) + med(old_wall) + (med(old_dev)[0], int(med(old_fall)[0]), stored)))
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
        say("recoding compressed pack sets in place (tools/chunk_zrecode_bench.py %d %d %d) on %s" % (n_files, runs, limit, eng.device_info()["name"]))
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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zrecode.txt")
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
