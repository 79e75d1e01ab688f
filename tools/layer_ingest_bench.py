"""A pulled layer becomes a batch, measured (writes profiles/layer_ingest.txt).  One run on the GPU.

    input     400 MB of regular files under /usr/lib (largest first) as a tree of 4 MiB files -- the corpus of 4.19 and 4.20 -- as a
              layer in four forms: the device leg's blob, the host leg's at the default level, a foreign gzip (gzip.compress of the
              tar) and the plain tar;
    (a)       Batch.add_layer_blob + run on each form: the call's wall time, ms_upload, the inflate's ms_size and ms_write, ms_headers,
              the run, marked / live blocks, fetches;
    (b)       the path it replaces, in the same run: Engine.tar_inflate to a file + tar_entries + add_path_range per member + run
              (these calls are what they were before this change);
    (c)       the header pass alone (mark + compaction + gather, device time from the launcher's events, through the kernel probe)
              against a device-to-device copy of the same tar bytes.
Medians of `runs` rounds behind one warm-up, with the spread (min .. max).  No threshold on any time.  The GPU step is a process of
its own under a time limit: `layer_ingest_bench.py` starts `layer_ingest_bench.py --step ...` with timeout(1) and writes nothing if it
fails.
layer_ingest_bench.py [out = profiles/layer_ingest.txt] [bytes = 4e8] [runs = 3]   (needs an MI355X)"""
import ctypes as C
import gzip
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEP_LIMIT_S = 840


def _stat(ts, digits=1):
    return "%.*f ms (%.*f .. %.*f)" % (digits, statistics.median(ts), digits, min(ts), digits, max(ts))


def step(out, limit, runs):
    import torch
    import makisu_amd as M
    from gunzip_device_bench import _layer
    from gzip_device_bench import usr_lib
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("layer ingest (tools/layer_ingest_bench.py %d %d), inflate window %s MiB; medians of %d rounds behind one warm-up (min .. max)"
        % (limit, runs, os.environ.get("MI_INFLATE_WINDOW_MB", "64 (default)"), runs))
    lib_bytes, n_files = usr_lib(limit)
    tmp = tempfile.mkdtemp(prefix="layering_")
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
            paths = {}
            for name, leg in (("device-leg blob", eng), ("host-leg blob", None)):
                paths[name] = os.path.join(tmp, "blob%d.gz" % len(paths))
                _layer(M, lib_root, paths[name], leg)
            tar_path = os.path.join(tmp, "layer.tar")
            eng.tar_inflate(paths["host-leg blob"], tar_path)
            tar = open(tar_path, "rb").read()
            paths["plain tar"] = tar_path
            paths["foreign gzip"] = os.path.join(tmp, "foreign.gz")
            with open(paths["foreign gzip"], "wb") as f:
                f.write(gzip.compress(tar, 6))
            say("the tar: %d bytes, %d files of /usr/lib in 4 MiB members" % (len(tar), n_files))
            ref_roots = None
            for name in ("device-leg blob", "host-leg blob", "foreign gzip", "plain tar"):
                blob = open(paths[name], "rb").read()
                # (a) the new call + run
                rec = {"add": [], "run": [], "up": [], "size": [], "write": [], "hdr": []}
                for k in range(runs + 1):
                    with eng.batch() as b:
                        t0 = time.perf_counter()
                        ents, _, info, _ = b.add_layer_blob(blob)
                        t1 = time.perf_counter()
                        b.run()
                        t2 = time.perf_counter()
                        roots = b.roots().copy()
                    if k:
                        for key, v in (("add", (t1 - t0) * 1e3), ("run", (t2 - t1) * 1e3), ("up", info["ms_upload"]), ("size", info["inflate"]["ms_size"]),
                                       ("write", info["inflate"]["ms_write"]), ("hdr", info["ms_headers"])):
                            rec[key].append(v)
                both = [a + r for a, r in zip(rec["add"], rec["run"])]
                say("(a) %s, %d bytes, source %d: add_layer_blob %s [ms_upload %s, ms_size %s, ms_write %s, ms_headers %s] + run %s = %s = %.2f GB/s of tar; "
                    "%d entries, %d files, %d blocks marked, %d live, %d fetches (%d bytes); %d segments, %d rounds"
                    % (name, len(blob), info["source"], _stat(rec["add"]), _stat(rec["up"]), _stat(rec["size"]), _stat(rec["write"]), _stat(rec["hdr"]),
                       _stat(rec["run"]), _stat(both), len(tar) / statistics.median(both) / 1e6, info["n_entries"], info["n_files"], info["n_marked"],
                       info["n_live"], info["n_fetched"], info["fetched_bytes"], info["inflate"]["n_segments"], info["inflate"]["n_rounds"]))
                # (b) the path it replaces
                rec = {"inflate": [], "list": [], "add": [], "run": []}
                out_tar = os.path.join(tmp, "replaced.tar")
                for k in range(runs + 1):
                    t0 = time.perf_counter()
                    r = eng.tar_inflate(paths[name], out_tar)
                    t1 = time.perf_counter()
                    listing = M.tar_entries(out_tar)
                    t2 = time.perf_counter()
                    with eng.batch() as b:
                        for e in listing:
                            if e["kind"] == M.KIND_FILE:
                                b.add_path_range(out_tar, e["data_offset"], e["size"], tag=e["file_index"])
                        t3 = time.perf_counter()
                        b.run()
                        t4 = time.perf_counter()
                        roots_b = b.roots().copy()
                    if k:
                        for key, v in (("inflate", t1 - t0), ("list", t2 - t1), ("add", t3 - t2), ("run", t4 - t3)):
                            rec[key].append(v * 1e3)
                whole = [sum(x) for x in zip(rec["inflate"], rec["list"], rec["add"], rec["run"])]
                same = np.array_equal(roots, roots_b) and (ref_roots is None or np.array_equal(roots, ref_roots))
                ref_roots = roots
                say("(b) %s: mi_tar_inflate_ctx to a file %s (fell_back %s) + mi_tar_open %s + add_path_range per member %s + run %s = %s = %.2f GB/s of tar; "
                    "the same roots as (a) and as every other form: %s"
                    % (name, _stat(rec["inflate"]), r["info"]["fell_back"], _stat(rec["list"]), _stat(rec["add"]), _stat(rec["run"]), _stat(whole),
                       len(tar) / statistics.median(whole) / 1e6, same))
                del blob
            # (c) the header pass alone against a device-to-device copy
            probe = C.CDLL(os.path.join(ROOT, "tests", "kernel_probe", "libmi_tar_probe.so"))
            probe.probe_tar_scan_ms.restype = C.c_int
            probe.probe_tar_scan_ms.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
            d_tar = torch.from_numpy(np.frombuffer(tar, dtype=np.uint8).copy()).cuda()
            d_dst = torch.empty_like(d_tar)
            scan, copy = [], []
            for k in range(runs + 3):
                n, ms = C.c_uint64(), C.c_float()
                assert probe.probe_tar_scan_ms(d_tar.data_ptr(), d_tar.numel(), C.byref(n), C.byref(ms)) == 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                d_dst.copy_(d_tar)
                e1.record()
                torch.cuda.synchronize()
                if k:
                    scan.append(ms.value)
                    copy.append(e0.elapsed_time(e1))
            say("(c) the header pass alone over the %d bytes (mark + count + scan | scatter + gather, device time): %s = %.0f GB/s read, %d blocks marked; "
                "a device-to-device copy of the same bytes: %s = %.0f GB/s read (and as much written); the pass / the copy = %.2f"
                % (len(tar), _stat(scan, 3), len(tar) / statistics.median(scan) / 1e6, n.value, _stat(copy, 3), len(tar) / statistics.median(copy) / 1e6,
                   statistics.median(scan) / statistics.median(copy)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(float(sys.argv[3])), int(sys.argv[4]))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "layer_ingest.txt")
    args = [sys.argv[k] if len(sys.argv) > k else d for k, d in ((2, "4e8"), (3, "3"))]
    rc = subprocess.call(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", out] + args)
    if rc:
        sys.exit("the GPU step failed (%d): nothing written" % rc)


if __name__ == "__main__":
    main()
