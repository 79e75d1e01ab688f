"""The device inflate, measured (writes profiles/gunzip_device.txt).  One run on the GPU.

    input     400 MB of regular files under /usr/lib (largest first) as a tree of 4 MiB files, written as a layer (a) by the device
              deflate leg and (b) by the host leg at the default level; and 262 MB of random bytes in one file, by the host leg;
    buffer    mi_inflate_buffer on each blob: ms_size (marking + size pass), ms_write (the rounds' decodes), candidates, live
              segments and rounds, the call's wall time;
    tar       mi_tar_inflate_ctx against mi_tar_inflate on the same blob in the same run, with and without an output file: wall time,
              GB/s of tar, the same digests;
    floor     the serial SHA-256 alone over the tar (hashlib), which both calls contain.
No threshold on any time.  The GPU step is a process of its own under a time limit: `gunzip_device_bench.py` starts
`gunzip_device_bench.py --step ...` with timeout(1) and writes nothing if it fails.
gunzip_device_bench.py [out = profiles/gunzip_device.txt] [bytes = 4e8] [random = 2.62e8] [runs = 2]   (needs an MI355X)"""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEP_LIMIT_S = 840


def _layer(M, root, path, engine):
    ents = M.tree_walk(root, root, (), M.TREE_SCAN, full=True)
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    l = M.Layer(out_fd=fd, gzip_level=M.GZIP_DEFAULT)
    try:
        if engine is not None:
            l.set_gzip_engine(engine)
        for e in ents:
            l.add(e, os.path.join(root, e["relpath"].lstrip("/")) if e["kind"] == 1 else None)
        return l.finish()
    finally:
        l.close()
        os.close(fd)


def step(out, limit, n_random, runs):
    import makisu_amd as M
    from gzip_device_bench import usr_lib
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device inflate (tools/gunzip_device_bench.py %d %d %d), window %s MiB" % (limit, n_random, runs, os.environ.get("MI_INFLATE_WINDOW_MB", "64 (default)")))
    lib_bytes, n_files = usr_lib(limit)
    tmp = tempfile.mkdtemp(prefix="gunzdev_")
    os.environ["MI_GZIP_THREADS"] = "16"
    try:
        lib_root, rnd_root = os.path.join(tmp, "lib_root"), os.path.join(tmp, "rnd_root")
        os.makedirs(os.path.join(lib_root, "lib"))
        os.makedirs(rnd_root)
        for k, at in enumerate(range(0, len(lib_bytes), 4 << 20)):
            with open(os.path.join(lib_root, "lib", "f%04d" % k), "wb") as f:
                f.write(lib_bytes[at:at + (4 << 20)])
        with open(os.path.join(rnd_root, "random.bin"), "wb") as f:
            f.write(np.random.default_rng(7).integers(0, 256, n_random, dtype=np.uint8).tobytes())
        with M.Engine(device=0) as eng:
            say("%s" % eng.device_info()["name"])
            blobs = []
            for name, root, leg in (("/usr/lib (%d files), device leg" % n_files, lib_root, eng), ("/usr/lib (%d files), host leg, default level" % n_files, lib_root, None),
                                    ("random bytes, host leg, default level", rnd_root, None)):
                path = os.path.join(tmp, "blob%d.gz" % len(blobs))
                res = _layer(M, root, path, leg)
                blobs.append((name, path, res))
            for name, path, res in blobs:
                blob = open(path, "rb").read()
                best = None
                for k in range(runs + 1):                                          # one warm-up round
                    t0 = time.perf_counter()
                    data, info = eng.inflate_buffer(blob)
                    wall = time.perf_counter() - t0
                    if k and (best is None or wall < best[1]):
                        best = (info, wall)
                info, wall = best
                ok = info["verdict"] != 0 or hashlib.sha256(data).digest() == res["tar_sha256"]
                say("mi_inflate_buffer, %s: %d bytes -> %d, verdict %d (rule %d); %d candidates, %d live segments, %d rounds; ms_size %.1f, ms_write %.1f, "
                    "the call %.1f ms = %.2f GB/s of output (best of %d by wall time; the Python binding's own copy of the output is inside it); "
                    "the tar's digest: %s" % (name, len(blob), info["out_bytes"], info["verdict"], info["rule"], info["n_candidates"], info["n_segments"],
                                              info["n_rounds"], info["ms_size"], info["ms_write"], wall * 1e3, max(info["out_bytes"], 1) / wall / 1e9, runs, ok))
                del data
                tar_path = os.path.join(tmp, "out.tar")
                for what, call in (("mi_tar_inflate (host, zlib)", M.tar_inflate), ("mi_tar_inflate_ctx (device)", eng.tar_inflate)):
                    for to_file in (False, True):
                        ts = []
                        for _ in range(runs):
                            t0 = time.perf_counter()
                            r = call(path, tar_path if to_file else None)
                            ts.append(time.perf_counter() - t0)
                        fb = r.get("info", {}).get("fell_back", "-")
                        say("    %s, %s: %d tar bytes in %.3f s = %.2f GB/s of tar (best of %d; all: %s); fell_back %s; TarDigest agrees: %s"
                            % (what, "to a file" if to_file else "digests only", r["tar_bytes"], min(ts), r["tar_bytes"] / min(ts) / 1e9, runs,
                               " ".join("%.3f" % t for t in ts), fb, r["tar_digest"] == "sha256:" + res["tar_sha256"].hex()))
                tar = open(tar_path, "rb").read()
                t0 = time.perf_counter()
                hashlib.sha256(tar).digest()
                dt = time.perf_counter() - t0
                say("    the serial SHA-256 alone over the tar (hashlib): %.3f s = %.2f GB/s" % (dt, len(tar) / dt / 1e9))
                del tar
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(float(sys.argv[3])), int(float(sys.argv[4])), int(sys.argv[5]))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gunzip_device.txt")
    args = [sys.argv[k] if len(sys.argv) > k else d for k, d in ((2, "4e8"), (3, "2.62e8"), (4, "2"))]
    rc = subprocess.call(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", out] + args)
    if rc:
        sys.exit("the GPU step failed (%d): nothing written" % rc)


if __name__ == "__main__":
    main()
