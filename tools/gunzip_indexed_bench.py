"""The indexed device inflate, measured (writes profiles/gunzip_indexed.txt).  One run on the GPU, everything in it.

    input     400 MB of regular files under /usr/lib (largest first) as a tree of 4 MiB files -- the corpus of 4.19 to 4.21 -- as a
              layer in three forms: a foreign one-stream gzip at level 6 (gzip.compress of the tar), ONE zlib stream with
              Z_SYNC_FLUSH every 128 KiB (matches reach across the flushes: what pgzip's blocks look like to a decoder), and the
              host leg's blob at the default level;
    index     mi_inflate_index_build at spacings 64 KiB, 256 KiB and 1 MiB: the index's bytes, its points, the build's time (with
              the TarDigest out of the same pass);
    tar       mi_tar_inflate_ctx_indexed (to a file) per spacing, against mi_tar_inflate and mi_tar_inflate_ctx on the same blob;
    add       Batch.add_layer_blob_indexed + run per spacing, against Batch.add_layer_blob + run; the same roots everywhere.
Medians of `runs` rounds behind one warm-up, with the spread (min .. max).  No threshold on any time.  The GPU step is a process of
its own under a time limit: `gunzip_indexed_bench.py` starts `gunzip_indexed_bench.py --step ...` with timeout(1) and writes nothing
if it fails.
gunzip_indexed_bench.py [out = profiles/gunzip_indexed.txt] [bytes = 4e8] [runs = 3]   (needs an MI355X)"""
import gzip
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEP_LIMIT_S = 1080
SPACINGS = (65536, 262144, 1 << 20)


def _stat(ts, digits=1):
    return "%.*f ms (%.*f .. %.*f)" % (digits, statistics.median(ts), digits, min(ts), digits, max(ts))


def _no_reset(data, block=128 << 10, level=6):
    c, parts = zlib.compressobj(level, zlib.DEFLATED, -15), []
    for at in range(0, len(data), block):
        parts.append(c.compress(data[at:at + block]) + c.flush(zlib.Z_SYNC_FLUSH))
    parts.append(c.flush(zlib.Z_FINISH))
    return (bytes((0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255)) + b"".join(parts) + (zlib.crc32(data) & 0xFFFFFFFF).to_bytes(4, "little")
            + (len(data) & 0xFFFFFFFF).to_bytes(4, "little"))


def step(out, limit, runs):
    import makisu_amd as M
    from gunzip_device_bench import _layer
    from gzip_device_bench import usr_lib
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        ts, last = [], None
        for k in range(runs + 1):
            t0 = time.perf_counter()
            last = fn()
            if k:
                ts.append((time.perf_counter() - t0) * 1e3)
        return ts, last

    say("indexed device inflate (tools/gunzip_indexed_bench.py %d %d), inflate window %s MiB; medians of %d rounds behind one warm-up (min .. max)"
        % (limit, runs, os.environ.get("MI_INFLATE_WINDOW_MB", "64 (default)"), runs))
    lib_bytes, n_files = usr_lib(limit)
    tmp = tempfile.mkdtemp(prefix="gunzidx_")
    os.environ["MI_GZIP_THREADS"] = "16"
    try:
        lib_root = os.path.join(tmp, "lib_root")
        os.makedirs(os.path.join(lib_root, "lib"))
        for k, at in enumerate(range(0, len(lib_bytes), 4 << 20)):
            with open(os.path.join(lib_root, "lib", "f%04d" % k), "wb") as f:
                f.write(lib_bytes[at:at + (4 << 20)])
        del lib_bytes
        with M.Engine(device=0) as eng:
            say("%s" % eng.device_info()["name"])
            paths = {"host-leg blob": os.path.join(tmp, "host.gz")}
            _layer(M, lib_root, paths["host-leg blob"], None)
            tar_path = os.path.join(tmp, "layer.tar")
            ref = M.tar_inflate(paths["host-leg blob"], tar_path)
            tar = open(tar_path, "rb").read()
            for name, make in (("foreign gzip", lambda: gzip.compress(tar, 6)), ("no-reset stream", lambda: _no_reset(tar))):
                paths[name] = os.path.join(tmp, "blob%d.gz" % len(paths))
                with open(paths[name], "wb") as f:
                    f.write(make())
            say("the tar: %d bytes, %d files of /usr/lib in 4 MiB members" % (len(tar), n_files))
            out_tar = os.path.join(tmp, "out.tar")
            ref_roots = None
            for name in ("foreign gzip", "no-reset stream", "host-leg blob"):
                blob = open(paths[name], "rb").read()
                say("%s, %d bytes" % (name, len(blob)))
                ts, r = timed(lambda: M.tar_inflate(paths[name], out_tar))
                say("    mi_tar_inflate (host, zlib), to a file: %s; TarDigest agrees: %s" % (_stat(ts), r["tar_digest"] == ref["tar_digest"]))
                ts, r = timed(lambda: eng.tar_inflate(paths[name], out_tar))
                say("    mi_tar_inflate_ctx (device, no index), to a file: %s; fell_back %d; TarDigest agrees: %s"
                    % (_stat(ts), r["info"]["fell_back"], r["tar_digest"] == ref["tar_digest"]))

                def add_plain():
                    with eng.batch() as b:
                        _, _, info, _ = b.add_layer_blob(blob)
                        b.run()
                        return info, b.roots().copy()
                ts, (info, roots) = timed(add_plain)
                ref_roots = roots if ref_roots is None else ref_roots
                say("    add_layer_blob + run (no index): %s; source %d; the same roots: %s" % (_stat(ts), info["source"], np.array_equal(roots, ref_roots)))
                for spacing in SPACINGS:
                    ts, (ix, built) = timed(lambda: M.inflate_index_build(blob, spacing, want_digest=True))
                    say("    spacing %d: index %d bytes = %.3f of the tar, %d points over %d blocks; mi_inflate_index_build with the TarDigest %s; "
                        "TarDigest agrees: %s" % (spacing, len(ix), len(ix) / len(tar), built["n_points"], built["n_blocks"], _stat(ts),
                                                  built["tar_digest"] == ref["tar_digest"]))
                    ts, r = timed(lambda: eng.tar_inflate_indexed(paths[name], ix, out_tar))
                    i = r["info"]
                    say("        mi_tar_inflate_ctx_indexed, to a file: %s = %.2f GB/s of tar; verdict %d, fell_back %d, %d spans, %d rounds, ms_write %.1f; "
                        "TarDigest agrees: %s" % (_stat(ts), len(tar) / statistics.median(ts) / 1e6, i["verdict"], i["fell_back"], i["n_segments"], i["n_rounds"],
                                                  i["ms_write"], r["tar_digest"] == ref["tar_digest"]))

                    def add_indexed():
                        with eng.batch() as b:
                            _, _, info, _ = b.add_layer_blob_indexed(blob, ix)
                            b.run()
                            return info, b.roots().copy()
                    ts, (info, roots) = timed(add_indexed)
                    say("        add_layer_blob_indexed + run: %s = %.2f GB/s of tar; source %d, fell_back %d, ms_upload %.1f, ms_write %.1f, ms_headers %.1f; "
                        "the same roots: %s" % (_stat(ts), len(tar) / statistics.median(ts) / 1e6, info["source"], info["inflate"]["fell_back"], info["ms_upload"],
                                                info["inflate"]["ms_write"], info["ms_headers"], np.array_equal(roots, ref_roots)))
                del blob
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(float(sys.argv[3])), int(sys.argv[4]))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gunzip_indexed.txt")
    args = [sys.argv[k] if len(sys.argv) > k else d for k, d in ((2, "4e8"), (3, "3"))]
    rc = subprocess.call(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", out] + args)
    if rc:
        sys.exit("the GPU step failed (%d): nothing written" % rc)


if __name__ == "__main__":
    main()
