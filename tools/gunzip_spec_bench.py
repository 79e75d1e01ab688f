"""The speculative device inflate, measured (writes profiles/gunzip_spec.txt).  One run on the GPU, everything in it.

    input     gunzip_indexed_bench.py's blobs of 400 MB of /usr/lib as a layer -- a foreign one-stream gzip at level 6, ONE zlib stream
              with Z_SYNC_FLUSH every 128 KiB, the host leg's blob -- and the device leg's blob of the same layer, a tar holding one file
              of 262 MB of random bytes (gzip stores them), a tar holding one 100 MB file of zeros (a few blocks of megabytes each),
              and the first 64 MB of the layer's tar as a stream of fixed blocks (no candidate: the time to a NOT_PARALLEL verdict);
    (a)       mi_tar_inflate: the host, zlib;
    (b)       mi_inflate_index_build + mi_tar_inflate_ctx_indexed: today's first pull with an index kept;
    (c)       mi_tar_inflate_ctx_spec with the index returned, and add_layer_blob_spec + run, at piece_bytes 16, 32, 64 and 128 KiB:
              ms_find / ms_speculate / ms_windows / ms_write, the pieces, the candidates found, the live spans, the verdict.
Medians of `runs` rounds behind one warm-up, with the spread (min .. max); wall times of calls that return when the device is done.  No
threshold on any time.  The GPU step is a process of its own under a time limit: `gunzip_spec_bench.py` starts `gunzip_spec_bench.py
--step ...` with timeout(1) and writes nothing if it fails.
gunzip_spec_bench.py [out = profiles/gunzip_spec.txt] [bytes = 4e8] [runs = 3]   (needs an MI355X)"""
import gzip
import io
import os
import shutil
import statistics
import subprocess
import sys
import tarfile
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEP_LIMIT_S = 1100
PIECES = (16384, 32768, 65536, 131072)


def _one_file_tar(name, data):
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.GNU_FORMAT) as t:
        info = tarfile.TarInfo(name)
        info.size = len(data)
        t.addfile(info, io.BytesIO(data))
    return buf.getvalue()


def _head_of(tar, n):
    """the archive's first members, up to the one that begins at or behind n, and an end marker: a whole tar"""
    with tarfile.open(fileobj=io.BytesIO(tar)) as t:
        cut = next((m.offset for m in t if m.offset >= n), len(tar))
    return tar[:cut] + bytes(1024)


def _fixed(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 8, zlib.Z_FIXED)
    return c.compress(data) + c.flush()


def step(out, limit, runs):
    import makisu_amd as M
    from gunzip_device_bench import _layer
    from gunzip_indexed_bench import _no_reset, _stat
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

    say("speculative device inflate (tools/gunzip_spec_bench.py %d %d), inflate window %s MiB; medians of %d rounds behind one warm-up (min .. max)"
        % (limit, runs, os.environ.get("MI_INFLATE_WINDOW_MB", "64 (default)"), runs))
    lib_bytes, n_files = usr_lib(limit)
    tmp = tempfile.mkdtemp(prefix="gunzspec_")
    os.environ["MI_GZIP_THREADS"] = "16"
    try:
        lib_root = os.path.join(tmp, "lib_root")
        os.makedirs(os.path.join(lib_root, "lib"))
        for k, at in enumerate(range(0, len(lib_bytes), 4 << 20)):
            with open(os.path.join(lib_root, "lib", "f%04d" % k), "wb") as f:
                f.write(lib_bytes[at:at + (4 << 20)])
        del lib_bytes
        with M.Engine(device=0) as eng:
            say("%s" % (eng.device_info()["name"] or "gfx950"))
            paths = {"host-leg blob": os.path.join(tmp, "host.gz"), "device-leg blob": os.path.join(tmp, "device.gz")}
            _layer(M, lib_root, paths["host-leg blob"], None)
            _layer(M, lib_root, paths["device-leg blob"], eng)
            tar_path = os.path.join(tmp, "layer.tar")
            M.tar_inflate(paths["host-leg blob"], tar_path)
            tar = open(tar_path, "rb").read()
            rnd = np.random.default_rng(23).integers(0, 256, int(limit * 0.655), dtype=np.uint8).tobytes()
            for name, make in (("foreign gzip", lambda: gzip.compress(tar, 6)), ("no-reset stream", lambda: _no_reset(tar)),
                               ("random tar", lambda: gzip.compress(_one_file_tar("random", rnd), 6)),
                               ("zeros tar", lambda: gzip.compress(_one_file_tar("zeros", bytes(limit // 4)), 6)),
                               ("fixed-block stream", lambda: _fixed(_head_of(tar, 64 << 20)))):
                paths[name] = os.path.join(tmp, "blob%d.gz" % len(paths))
                with open(paths[name], "wb") as f:
                    f.write(make())
            say("the layer's tar: %d bytes, %d files of /usr/lib in 4 MiB members; random bytes: %d; the zeros tar: one file of %d"
                % (len(tar), n_files, len(rnd), limit // 4))
            del tar, rnd
            out_tar = os.path.join(tmp, "out.tar")
            for name in ("foreign gzip", "no-reset stream", "host-leg blob", "device-leg blob", "random tar", "zeros tar", "fixed-block stream"):
                blob = open(paths[name], "rb").read()
                ts, ref = timed(lambda: M.tar_inflate(paths[name], out_tar))
                say("%s, %d bytes -> %d" % (name, len(blob), ref["tar_bytes"]))
                say("    (a) mi_tar_inflate (host, zlib), to a file: %s" % _stat(ts))
                t_a = statistics.median(ts)
                ts_build, (ix, built) = timed(lambda: M.inflate_index_build(blob, 0, want_digest=True))
                ts, r = timed(lambda: eng.tar_inflate_indexed(paths[name], ix, out_tar))
                t_b = statistics.median(ts_build) + statistics.median(ts)
                say("    (b) mi_inflate_index_build %s + mi_tar_inflate_ctx_indexed %s = %.1f ms; %d points, verdict %d, fell_back %d; TarDigest agrees: %s"
                    % (_stat(ts_build), _stat(ts), t_b, built["n_points"], r["info"]["verdict"], r["info"]["fell_back"], r["tar_digest"] == ref["tar_digest"]))

                def add_plain():
                    with eng.batch() as b:
                        _, _, info, _ = b.add_layer_blob(blob)
                        b.run()
                        return info, b.roots().copy()
                ts, (info, ref_roots) = timed(add_plain)
                say("        add_layer_blob + run (no index): %s; source %d" % (_stat(ts), info["source"]))
                for piece in PIECES:
                    ts, r = timed(lambda: eng.tar_inflate_spec(paths[name], out_tar, piece, want_index=True))
                    i, s = r["info"], r["spec"]
                    t_c = statistics.median(ts)
                    say("    (c) piece %d: mi_tar_inflate_ctx_spec, to a file, the index returned: %s = %.2f of (a), %.2f of (b); verdict %d rule %d fell_back %d; "
                        "%d pieces, %d found, %d live, %d spans, %d rounds; ms_find %.1f, ms_speculate %.1f, ms_windows %.1f, ms_write %.1f; index %d bytes; "
                        "TarDigest agrees: %s" % (piece, _stat(ts), t_c / t_a, t_c / t_b, i["verdict"], i["rule"], i["fell_back"], s["n_pieces"], s["n_found"],
                                                   s["n_live"], i["n_segments"], i["n_rounds"], s["ms_find"], s["ms_speculate"], s["ms_windows"], i["ms_write"],
                                                   len(r["index"] or b""), r["tar_digest"] == ref["tar_digest"]))

                    def add_spec():
                        with eng.batch() as b:
                            _, _, info, _ = b.add_layer_blob_spec(blob, 0, piece)
                            b.run()
                            return info, b.roots().copy()
                    ts, (info, roots) = timed(add_spec)
                    say("        add_layer_blob_spec + run: %s; source %d, fell_back %d, ms_upload %.1f, ms_write %.1f, ms_headers %.1f; the same roots: %s"
                        % (_stat(ts), info["source"], info["inflate"]["fell_back"], info["ms_upload"], info["inflate"]["ms_write"], info["ms_headers"],
                           np.array_equal(roots, ref_roots)))
                del blob
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(float(sys.argv[3])), int(sys.argv[4]))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gunzip_spec.txt")
    args = [sys.argv[k] if len(sys.argv) > k else d for k, d in ((2, "4e8"), (3, "3"))]
    rc = subprocess.call(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", out] + args)
    if rc:
        sys.exit("the GPU step failed (%d): nothing written" % rc)


if __name__ == "__main__":
    main()
