"""Zpacks coded straight from the arena, measured (writes profiles/chunk_zbatch.txt).

The two legs of tools/chunk_zset_bench.py (4.10): an incompressible C2-shaped synthetic batch (random 64 KiB files: every chunk is
stored raw) and a compressible one of regular files found under /usr/lib, named in the output.  The selection is what a commit
selects: the first occurrences (dup_of < 0).  Everything compared is measured in the same run, median of the runs after a warm-up,
device times from HIP events where the library takes them, and the wall time of the calls (each path in a loop of its own):
    Batch.zpack(sel, verify=True)                              mi_zpack_info: ms_encode + ms_compact + ms_verify
    Batch.pack(sel, verify=True) then .compress(verify=True)   mi_pack_info: ms_gather + ms_verify; mi_zpack_info: the three --
                                                               what the commit path costs without MI_MEMFS_CHUNK_ZPACK
    the same pair without verification
    peak device bytes of the pair, from the sizes the calls allocate (the blobs and the coder's scratch; the per-entry arrays,
    some hundred bytes a chunk in both, are left out): zpack: scratch + zblob; pack + compress: plain blob + scratch + zblob.
No threshold on any time.  Each GPU step is a process of its own under a time limit: `chunk_zbatch_bench.py` starts
`chunk_zbatch_bench.py --step ...` with timeout(1) and stops at the first step that fails.
chunk_zbatch_bench.py [out = profiles/chunk_zbatch.txt] [files = 20000] [runs = 10] [bytes = 2e9]   (needs an MI355X)"""
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


def worst_span(n):
    return (n + n // 255 + 16 + 15) // 16 * 16


def leg(b, name, runs, say):
    b.run()
    chunks = b.chunks()
    sel = (chunks["dup_of"] < 0).astype(np.uint8)
    lens = chunks["length"][sel != 0].astype(np.int64)
    scratch = int(sum(worst_span(int(n)) for n in lens))
    plain = int(((lens + 15) // 16 * 16).sum())
    for verify in (True, False):
        new_dev, new_wall, old_dev, old_wall, parts = [], [], [], [], {}
        # each path in a loop of its own, back to back.  Interleaved call by call, Batch.zpack's wall time read 24-27 ms against
        # 2.7 ms alone with the same device time (one run; the cause was not looked for -- device memory of three large buffers
        # had just been freed by the other path in front of every such call)
        for k in range(runs + 2):                                                 # two warm-up rounds
            t0 = time.perf_counter()
            with b.zpack(sel, verify=verify) as z:
                t1 = time.perf_counter()
                zi = z.info.as_dict()
            if k >= 2:
                new_dev.append(zi["ms_encode"] + zi["ms_compact"] + zi["ms_verify"])
                new_wall.append((t1 - t0) * 1e3)
                for key in ("encode", "compact", "verify", "decode"):
                    parts.setdefault("new " + key, []).append(zi["ms_" + key])
        for k in range(runs + 2):
            t2 = time.perf_counter()
            with b.pack(sel, verify=verify) as p:
                with p.compress(verify=verify) as old:
                    t3 = time.perf_counter()
                    pi, oi = p.info.as_dict(), old.info.as_dict()
            assert (oi["blob_bytes"], oi["stored_bytes"], oi["n_raw"]) == (zi["blob_bytes"], zi["stored_bytes"], zi["n_raw"])
            if k >= 2:
                old_dev.append(pi["ms_gather"] + pi["ms_verify"] + oi["ms_encode"] + oi["ms_compact"] + oi["ms_verify"])
                old_wall.append((t3 - t2) * 1e3)
                for key, v in (("old gather", pi["ms_gather"]), ("old pack verify", pi["ms_verify"]), ("old encode", oi["ms_encode"]),
                               ("old compact", oi["ms_compact"]), ("old zpack verify", oi["ms_verify"])):
                    parts.setdefault(key, []).append(v)
        if verify:
            say("%s: %d chunk rows, %d selected (dup_of < 0) with %d chunk bytes; the zpack: %d raw entries, stored / chunk bytes %.4f, blob %d "
                "bytes" % (name, len(chunks), zi["n_entries"], zi["chunk_bytes"], zi["n_raw"], zi["stored_bytes"] / max(zi["chunk_bytes"], 1),
                           zi["blob_bytes"]))
            say("    peak device bytes of the pair, from the sizes allocated: zpack: scratch %d + zblob %d = %d; pack + compress: plain blob %d + "
                "scratch %d + zblob %d = %d (%.2f x)" % (scratch, zi["blob_bytes"], scratch + zi["blob_bytes"], plain, scratch, zi["blob_bytes"],
                                                         plain + scratch + zi["blob_bytes"],
                                                         (plain + scratch + zi["blob_bytes"]) / max(scratch + zi["blob_bytes"], 1)))
        say("    %s verification; median of %d runs (min, max):" % ("WITH" if verify else "WITHOUT", len(new_dev)))
        say("        Batch.zpack, device (encode + compact%s): %.3f ms (%.3f, %.3f); the call: %.3f ms (%.3f, %.3f)" %
            ((" + verify" if verify else "",) + med(new_dev) + med(new_wall)))
        say("        Batch.pack + Pack.compress, device (gather + encode + compact%s): %.3f ms (%.3f, %.3f); the calls: %.3f ms (%.3f, %.3f)" %
            ((" + both verifications" if verify else "",) + med(old_dev) + med(old_wall)))
        say("        device times, existing / new: %.2f; calls: %.2f" % (med(old_dev)[0] / med(new_dev)[0], med(old_wall)[0] / med(new_wall)[0]))
        say("        the parts, medians in ms: " + ", ".join("%s %.3f" % (key, statistics.median(v)) for key, v in parts.items()))


def step(n_files, runs, limit):
    import makisu_amd as M
    from makisu_amd import workloads as W
    from chunk_zpack_bench import usr_lib_files

    def say(s):
        print(s, flush=True)

    with M.Engine(device=0) as eng:
        say("zpacks straight from the arena (tools/chunk_zbatch_bench.py %d %d %d) on %s" % (n_files, runs, limit, eng.device_info()["name"]))
        sh = W.c2(files_per_gpu=n_files)
        with eng.batch(sh.n_files, W.batch_bytes_hint(sh)) as b:
            W.fill_batch(b, sh)
            leg(b, "incompressible leg -- %d synthetic files x 64 KiB, RANDOM bytes: every chunk is stored raw" % sh.n_files, runs, say)
        files, total = usr_lib_files(limit)
        say("compressible leg -- %d regular files under /usr/lib, %d bytes, largest first:" % (len(files), total))
        for p, size in files[:12]:
            say("        %12d  %s" % (size, p))
        if len(files) > 12:
            say("        ... and %d smaller ones" % (len(files) - 12))
        with eng.batch(len(files), total + 4096 * len(files)) as b:
            b.add_paths([p for p, _ in files], [s for _, s in files])
            leg(b, "the files", runs, say)


def main():
    if sys.argv[1:2] == ["--step"]:
        return step(int(sys.argv[2]), int(sys.argv[3]), int(float(sys.argv[4])))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zbatch.txt")
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
