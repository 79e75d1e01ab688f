"""Compressed chunk packs, measured (writes profiles/chunk_zpack.txt).

Two resident batches, each packed whole (mi_batch_pack_chunks) and compressed with mi_pack_compress(MI_ZPACK_VERIFY):
    incompressible  a C2-shaped synthetic batch (files x 64 KiB).  Its bytes are random: every chunk is stored raw, so this leg
                    measures the parse that finds nothing, the raw path of the gather and the raw path of the decoder;
    compressible    regular files found under /usr/lib of the box (largest first, up to --bytes), named in the output: what
                    a layer of binaries and scripts looks like.
For each: encode, compact and decode from HIP events (mi_zpack_info: ms_encode, ms_compact, ms_decode), median of the runs
after a warm-up, in GB/s of CHUNK bytes; stored / chunk bytes; the decode next to a hipMemcpyAsync device-to-device of the plain
byte count in the same run; the encode next to zlib level 1 over the same chunks on 16 host threads in the same run (the gzip
leg's compressor: the only yardstick there is for "compressing these bytes on this box"); MI_ZPACK_VERIFY next to the batch's
own chunk pass.  No threshold on any time.
Each GPU step is a process of its own under a time limit: `chunk_zpack_bench.py` starts `chunk_zpack_bench.py --step ...` with
timeout(1) and stops at the first step that fails.
--level 2: every leg ALSO compresses the same pack with MI_ZPACK_LEVEL2 in the same run and states ms_encode and the
stored bytes of both levels side by side; the output then goes to profiles/chunk_zpack_l2.txt.
chunk_zpack_bench.py [--level 1|2] [out = profiles/chunk_zpack.txt] [files = 20000] [runs = 10] [bytes = 2e9]   (needs an MI355X)"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEP_LIMIT_S = 300
HOST_THREADS = 16


def usr_lib_files(limit):
    """regular files under /usr/lib, largest first, until `limit` bytes; every file at most once (hard links by inode)"""
    found, seen = [], set()
    for dp, _, fns in os.walk("/usr/lib"):
        for fn in fns:
            p = os.path.join(dp, fn)
            try:
                st = os.lstat(p)
            except OSError:
                continue
            if not os.path.isfile(p) or os.path.islink(p) or st.st_size < 4096 or (st.st_dev, st.st_ino) in seen or not os.access(p, os.R_OK):
                continue
            seen.add((st.st_dev, st.st_ino))
            found.append((st.st_size, p))
    found.sort(reverse=True)
    out, total = [], 0
    for size, p in found:
        if size > 1 << 30 or total + size > limit:
            continue
        out.append((p, size))
        total += size
    return out, total


def zlib_level1_seconds(blob, offsets, lengths):
    """zlib.compress(chunk, 1) of every chunk on HOST_THREADS threads (zlib releases the GIL) -> (seconds, bytes out)"""
    view = memoryview(blob)
    bounds = np.linspace(0, len(offsets), HOST_THREADS * 8 + 1).astype(np.int64)

    def work(i):
        total = 0
        for k in range(bounds[i], bounds[i + 1]):
            total += len(zlib.compress(view[offsets[k]:offsets[k] + lengths[k]], 1))
        return total

    t0 = time.perf_counter()
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        out = sum(ex.map(work, range(len(bounds) - 1)))
    return time.perf_counter() - t0, out


def leg(eng, hip, b, name, runs, say, host_yardstick, level=1):
    from chunk_pack_bench import d2d_copy_ms
    b.run()
    b.rerun()
    ms_chunk_pass = eng.stats()["ms_sha_chunks"]
    n_chunks = b.counts()[1]
    with b.pack() as p:
        pi = p.info.as_dict()
        enc, comp, dec, ver = [], [], [], []
        zi = None
        for k in range(runs + 2):                                                 # two warm-up rounds
            with p.compress(verify=True) as z:
                zi = z.info.as_dict()
            if k >= 2:
                enc.append(zi["ms_encode"])
                comp.append(zi["ms_compact"])
                dec.append(zi["ms_decode"])
                ver.append(zi["ms_verify"])
        cb = zi["chunk_bytes"]
        gbs = lambda ms: cb / (ms * 1e-3) / 1e9                                  # noqa: E731
        e, c, d, v = (statistics.median(x) for x in (enc, comp, dec, ver))
        say("%s: %d chunk rows, %d chunk bytes, a plain blob of %d bytes" % (name, n_chunks, cb, pi["blob_bytes"]))
        say("    stored / chunk bytes: %.4f (%d entries of %d raw); compressed blob %d bytes" %
            (zi["stored_bytes"] / cb, zi["n_raw"], zi["n_entries"], zi["blob_bytes"]))
        say("    median of %d runs after a warm-up, GB/s of chunk bytes:" % len(enc))
        say("    encode  %.3f ms (min %.3f, max %.3f): %.2f GB/s" % (e, min(enc), max(enc), gbs(e)))
        say("    compact %.3f ms (min %.3f, max %.3f): %.2f GB/s" % (c, min(comp), max(comp), gbs(c)))
        say("    decode  %.3f ms (min %.3f, max %.3f): %.2f GB/s" % (d, min(dec), max(dec), gbs(d)))
        say("    MI_ZPACK_VERIFY (decode + hash + compare): %.3f ms; the batch's own chunk pass over every row: %.3f ms" % (v, ms_chunk_pass))
        if level == 2:                                                            # the same pack, the same run, the denser parse
            enc2, zi2 = [], None
            for k in range(runs + 2):
                with p.compress(verify=True, level=2) as z:
                    zi2 = z.info.as_dict()
                if k >= 2:
                    enc2.append(zi2["ms_encode"])
            e2 = statistics.median(enc2)
            say("    level 2 (MI_ZPACK_LEVEL2), the same pack: encode %.3f ms (min %.3f, max %.3f): %.2f GB/s against level 1's %.3f ms = "
                "%.2f x the time" % (e2, min(enc2), max(enc2), gbs(e2), e, e2 / e))
            say("    level 2 stored / chunk bytes: %.4f (%d bytes, %d entries raw) against level 1's %.4f (%d bytes, %d raw): %.4f of level 1's "
                "stored bytes; verified %d" % (zi2["stored_bytes"] / cb, zi2["stored_bytes"], zi2["n_raw"], zi["stored_bytes"] / cb,
                                               zi["stored_bytes"], zi["n_raw"], zi2["stored_bytes"] / zi["stored_bytes"], zi2["verified"]))
        ptr, nb = p.device()
        copy = d2d_copy_ms(hip, C.c_void_p(ptr), nb, runs)
        cm = statistics.median(copy)
        say("    hipMemcpyAsync device-to-device of the plain %d bytes, the same run: median %.3f ms of %d (min %.3f, max %.3f): %.2f GB/s; "
            "decode / copy: %.1f" % (nb, cm, len(copy), min(copy), max(copy), nb / (cm * 1e-3) / 1e9, d / cm))
        if host_yardstick:
            entries, blob = p.entries(), p.bytes()
            secs, out = zlib_level1_seconds(blob, entries["offset"].astype(np.int64), entries["length"].astype(np.int64))
            say("    zlib level 1 over the same chunks on %d host threads, the same run: %.3f s = %.2f GB/s, %.4f of the chunk bytes; "
                "encode + compact are %.1f x as fast and store %.2f x as much" %
                (HOST_THREADS, secs, cb / secs / 1e9, out / cb, secs * 1e3 / (e + c), zi["stored_bytes"] / out))


def step(n_files, runs, limit, level=1):
    import makisu_amd as M
    from makisu_amd import workloads as W
    from chunk_pack_bench import _hip

    def say(s):
        print(s, flush=True)

    hip = _hip()
    with M.Engine(device=0) as eng:
        say("compressed chunk packs (tools/chunk_zpack_bench.py %d %d %d) on %s" % (n_files, runs, limit, eng.device_info()["name"]))
        sh = W.c2(files_per_gpu=n_files)
        with eng.batch(sh.n_files, W.batch_bytes_hint(sh)) as b:
            W.fill_batch(b, sh)
            leg(eng, hip, b, "incompressible leg -- %d synthetic files x 64 KiB, RANDOM bytes: every chunk is stored raw, this measures the "
                "raw path only" % sh.n_files, runs, say, False, level)
        files, total = usr_lib_files(limit)
        say("compressible leg -- %d regular files under /usr/lib, %d bytes, largest first:" % (len(files), total))
        for p, size in files[:12]:
            say("        %12d  %s" % (size, p))
        if len(files) > 12:
            say("        ... and %d smaller ones" % (len(files) - 12))
        with eng.batch(len(files), total + 4096 * len(files)) as b:
            b.add_paths([p for p, _ in files], [s for _, s in files])
            leg(eng, hip, b, "the files", runs, say, True, level)


def main():
    level = 1
    if "--level" in sys.argv:
        at = sys.argv.index("--level")
        level = int(sys.argv[at + 1])
        del sys.argv[at:at + 2]
        if level not in (1, 2):
            sys.exit("--level 1 or 2")
    if sys.argv[1:2] == ["--step"]:
        return step(int(sys.argv[2]), int(sys.argv[3]), int(float(sys.argv[4])), level)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zpack_l2.txt" if level == 2 else "chunk_zpack.txt")
    n_files = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    runs = max(10, int(sys.argv[3])) if len(sys.argv) > 3 else 10
    limit = sys.argv[4] if len(sys.argv) > 4 else "2e9"
    # the one GPU step, a fresh process under its own time limit; nothing is started after a failure
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", str(n_files), str(runs), limit,
           "--level", str(level)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(p.stdout)
    sys.stderr.write(p.stderr[-4000:])
    if p.returncode != 0:
        sys.exit("the measuring step ended with status %d: nothing written" % p.returncode)
    with open(out, "w") as f:
        f.write(p.stdout)


if __name__ == "__main__":
    main()
