"""A pack set cut by digest, measured (writes profiles/chunk_fetch.txt).

On a C2-shaped resident batch (100 000 x 64 KiB synthetic files) every first occurrence is packed into a pack set; then a
sub-pack of a RANDOM HALF of the set's digests, in random order, is cut with mi_packset_pack:
    gather      the gather kernel's time from HIP events (mi_pack_info.ms_gather), median of the runs after a warm-up, and the
                bytes it reads plus writes per second -- against a hipMemcpyAsync device-to-device copy of the same byte count
                in the same run (the runtime's figure for "read N + write N"), and their ratio;
    resolve     mi_packset_missing over the same request against a set that holds the OTHER half: the request's way up, the
                lookup, the marking of first occurrences, the plan and the compaction (mi_want_info.ms_resolve), per million rows;
    verify      MI_SUBPACK_VERIFY's pass next to the batch's own chunk pass.
Each GPU step is a process of its own under a time limit: `chunk_fetch_bench.py` starts `chunk_fetch_bench.py --step ...` with
timeout(1) and stops at the first step that fails.
chunk_fetch_bench.py [out = profiles/chunk_fetch.txt] [files = 100000] [runs = 12]   (needs an MI355X)"""
import ctypes as C
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEP_LIMIT_S = 300


def step(n_files, runs):
    import makisu_amd as M
    from makisu_amd import workloads as W
    from chunk_pack_bench import _hip, d2d_copy_ms

    def say(s):
        print(s, flush=True)

    hip = _hip()
    rng = np.random.default_rng(81)
    with M.Engine(device=0) as eng:
        say("chunk fetch (tools/chunk_fetch_bench.py %d %d) on %s" % (n_files, runs, eng.device_info()["name"]))
        sh = W.c2(files_per_gpu=n_files)
        with eng.batch(sh.n_files, W.batch_bytes_hint(sh)) as b, eng.packset() as s, eng.packset() as s_other:
            W.fill_batch(b, sh)
            b.run()
            b.rerun()
            ms_chunk_pass = eng.stats()["ms_sha_chunks"]
            chunks = b.chunks().copy()
            first = np.flatnonzero(chunks["dup_of"] < 0)
            sel = np.zeros(len(chunks), dtype=np.uint8)
            sel[first] = 1
            with b.pack(select=sel) as p:
                pi = p.info.as_dict()
                s.add_pack(p, verify=True)
            say("batch: %d files x 64 KiB = %.2f GB, %d chunk rows; the set: %d first occurrences, a blob of %d bytes" %
                (sh.n_files, sh.n_bytes / 1e9, len(chunks), pi["n_entries"], pi["blob_bytes"]))
            half = rng.permutation(first)[:len(first) // 2]                       # a random half, in random order
            dig = np.ascontiguousarray(chunks["sha256"][half])
            lens = chunks["length"][half].astype(np.uint32)
            rest = np.zeros(len(chunks), dtype=np.uint8)
            rest[np.setdiff1d(first, half)] = 1
            with b.pack(select=rest) as p:
                s_other.add_pack(p)
            b.free()
            gather, verify, resolve = [], [], []
            info = None
            for k in range(runs + 2):                                             # two warm-up rounds
                with s.pack(dig, lens, verify=True) as sp:
                    info = sp.info.as_dict()
                w = s_other.missing(dig, lens)[2]
                assert w.n_want == len(half) and w.n_held == 0
                if k >= 2:
                    gather.append(info["ms_gather"])
                    verify.append(info["ms_verify"])
                    resolve.append(w.ms_resolve)                                  # (of the binding's second call: the sizing call ran the same work before it)
            nb = info["blob_bytes"]
            g = statistics.median(gather)
            say("sub-pack of a random half (%d digests, %d bytes of chunks, a blob of %d bytes), median of %d runs after a warm-up:" %
                (info["n_entries"], info["chunk_bytes"], nb, len(gather)))
            say("    gather kernel: %.3f ms (min %.3f, max %.3f): %.2f TB/s read + written" % (g, min(gather), max(gather), 2 * nb / (g * 1e-3) / 1e12))
            say("    MI_SUBPACK_VERIFY (the new blob hashed + compared): %.3f ms; the batch's own chunk pass over every row: %.3f ms" %
                (statistics.median(verify), ms_chunk_pass))
            r = statistics.median(resolve)
            say("    mi_packset_missing over the same %d rows (36 bytes a row up, lookup, first occurrences, plan, want list): %.3f ms = "
                "%.3f ms per million rows" % (len(half), r, r / (len(half) / 1e6)))
        mem = C.c_void_p()
        assert hip.hipMalloc(C.byref(mem), nb) == 0
        try:
            copy = d2d_copy_ms(hip, mem, nb, runs)
        finally:
            hip.hipFree(mem)
        c = statistics.median(copy)
        say("hipMemcpyAsync device-to-device, the same %d bytes, the same run: median %.3f ms of %d (min %.3f, max %.3f): %.2f TB/s read + written" %
            (nb, c, len(copy), min(copy), max(copy), 2 * nb / (c * 1e-3) / 1e12))
        say("ratio gather / copy: %.2f" % (g / c))


def main():
    if sys.argv[1:2] == ["--step"]:
        return step(int(sys.argv[2]), int(sys.argv[3]))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_fetch.txt")
    n_files = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    runs = max(10, int(sys.argv[3])) if len(sys.argv) > 3 else 12
    # the one GPU step, a fresh process under its own time limit; nothing is started after a failure
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", str(n_files), str(runs)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(p.stdout)
    sys.stderr.write(p.stderr[-4000:])
    if p.returncode != 0:
        sys.exit("the measuring step ended with status %d: nothing written" % p.returncode)
    with open(out, "w") as f:
        f.write(p.stdout)


if __name__ == "__main__":
    main()
