"""The layer writer's device gzip leg, measured (writes profiles/gzip_device.txt).  One run on the GPU.

    coder     mi_deflate_buffer on the project's two standard inputs -- 400 MB of regular files under /usr/lib (largest first) and
              262 MB of random bytes: the device time the call reports (HIP events around each window's launches, summed), GB/s
              of input by it and by the call's wall time, the bytes and the pieces by form; the blob is inflated once by zlib;
    layer     the /usr/lib bytes as a tree of 4 MiB files, written through the layer writer (digests only, out_fd = -1) with the
              host leg at level 1 and at the default level on 16 threads (MI_GZIP_THREADS=16) and with the device leg, in the
              same run: wall time, GB/s of tar, the blob's size;
    commit    a content-aware scan commit of that tree at the default level without and with MI_MEMFS_GZIP_DEVICE: wall time and
              the commit's own stage times.  With the option the coder and the chunk pass share the GPU: s_scan and s_write of the
              two commits, side by side, are the figure for what each costs the other.
No threshold on any time.  The GPU step is a process of its own under a time limit: `gzip_device_bench.py` starts
`gzip_device_bench.py --step ...` with timeout(1) and writes nothing if it fails.
gzip_device_bench.py [out = profiles/gzip_device.txt] [bytes = 4e8] [random = 2.62e8] [runs = 3]   (needs an MI355X)"""
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 540


def usr_lib(limit):
    files = []
    for d, _, names in os.walk("/usr/lib"):
        for n in names:
            p = os.path.join(d, n)
            try:
                if os.path.isfile(p) and not os.path.islink(p):
                    files.append((os.path.getsize(p), p))
            except OSError:
                pass
    files.sort(key=lambda t: (-t[0], t[1]))
    out, total = [], 0
    for size, p in files:
        if total >= limit:
            break
        try:
            b = open(p, "rb").read(limit - total)
        except OSError:
            continue
        out.append(b)
        total += len(b)
    return b"".join(out), len(out)


def step(out, limit, n_random, runs):
    import makisu_amd as M
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device gzip leg (tools/gzip_device_bench.py %d %d %d), window %s MiB" % (limit, n_random, runs, os.environ.get("MI_GZIP_DEVICE_WINDOW_MB", "32 (default)")))
    lib_bytes, n_files = usr_lib(limit)
    rnd = np.random.default_rng(7).integers(0, 256, n_random, dtype=np.uint8).tobytes()
    with M.Engine(device=0) as eng:
        say("%s" % eng.device_info()["name"])
        for name, data in (("/usr/lib, %d files" % n_files, lib_bytes), ("random bytes", rnd)):
            best = None
            for k in range(runs + 1):                                              # one warm-up round
                t0 = time.perf_counter()
                blob, crc, info = eng.deflate_buffer(data)
                wall = time.perf_counter() - t0
                if k and (best is None or info["ms_device"] < best[0]["ms_device"]):
                    best = (info, wall)
            info, wall = best
            ok = zlib.decompressobj(-15).decompress(blob + b"\x03\x00") == data and crc == zlib.crc32(data)
            say("mi_deflate_buffer, %s: %d bytes -> %d (%.4f), %d pieces (%d dynamic, %d stored); device %.1f ms = %.2f GB/s of input, the call %.1f ms = %.2f GB/s "
                "(best of %d by device time); inflates to the input and the CRC is zlib's: %s"
                % (name, len(data), len(blob), len(blob) / len(data), info["n_pieces"], info["n_dynamic"], info["n_stored"], info["ms_device"],
                   len(data) / info["ms_device"] / 1e6, wall * 1e3, len(data) / wall / 1e9, runs, ok))
            for level, lname in ((1, "1"), (-1, "default")):
                t0 = time.perf_counter()
                z = sum(len(zlib.compress(data[at:at + (1 << 20)], level)) for at in range(0, min(len(data), 64 << 20), 1 << 20))
                say("    (zlib level %s on the first 64 MiB, one thread: %.4f of the input, %.0f MB/s)" % (lname, z / min(len(data), 64 << 20),
                                                                                                      min(len(data), 64 << 20) / (time.perf_counter() - t0) / 1e6))
        tmp = tempfile.mkdtemp(prefix="gzdev_")
        try:
            root = os.path.join(tmp, "root")
            os.makedirs(os.path.join(root, "lib"))
            for k, at in enumerate(range(0, len(lib_bytes), 4 << 20)):
                with open(os.path.join(root, "lib", "f%04d" % k), "wb") as f:
                    f.write(lib_bytes[at:at + (4 << 20)])
            ents = M.tree_walk(root, root, (), M.TREE_SCAN, full=True)
            os.environ["MI_GZIP_THREADS"] = "16"
            for what, level, dev in (("host leg, level 1", 1, False), ("host leg, default level", M.GZIP_DEFAULT, False), ("device leg", M.GZIP_DEFAULT, True)):
                ts = []
                for _ in range(runs):
                    l = M.Layer(out_fd=-1, gzip_level=level)
                    t0 = time.perf_counter()
                    if dev:
                        l.set_gzip_engine(eng)
                    for e in ents:
                        l.add(e, os.path.join(root, e["relpath"]) if e["kind"] == 1 else None)
                    res = l.finish()
                    ts.append(time.perf_counter() - t0)
                    l.close()
                say("layer, %s, 16 threads: %d tar bytes -> %d (%.4f) in %.3f s = %.2f GB/s of tar (best of %d; all: %s)"
                    % (what, res["tar_bytes"], res["gzip_bytes"], res["gzip_bytes"] / res["tar_bytes"], min(ts), res["tar_bytes"] / min(ts) / 1e9, runs,
                       " ".join("%.3f" % t for t in ts)))
            for dev in (False, True):
                for k in range(2):                                                 # the second commit of a fresh handle is reported
                    with M.MemFS(root) as fs:
                        fs.set_options(gzip_device=dev)
                        t0 = time.perf_counter()
                        res = fs.commit_layer(must_scan=True, gzip_level=M.GZIP_DEFAULT, engine=eng, want_layer=False)
                        wall = time.perf_counter() - t0
                st = res["stats"]
                say("commit (content-aware, default level)%s: %.3f s; %d tar bytes -> %d; stages: %s"
                    % (" with MI_MEMFS_GZIP_DEVICE" if dev else "", wall, res["tar_bytes"], res["gzip_bytes"],
                       ", ".join("%s %.3f" % (k, v) for k, v in sorted(st.items()) if k.startswith("s_"))))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(float(sys.argv[3])), int(float(sys.argv[4])), int(sys.argv[5]))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gzip_device.txt")
    args = [sys.argv[k] if len(sys.argv) > k else d for k, d in ((2, "4e8"), (3, "2.62e8"), (4, "3"))]
    rc = subprocess.call(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", out] + args)
    if rc:
        sys.exit("the GPU step failed (%d): nothing written" % rc)


if __name__ == "__main__":
    main()
