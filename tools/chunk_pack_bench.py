"""Chunk packs, measured (writes profiles/chunk_pack.txt).

On a C2-shaped resident batch (100 000 x 64 KiB synthetic files, a chunk index) the first occurrences are packed:
    gather      the gather kernel's time from HIP events (mi_pack_info.ms_gather), median of the runs after a warm-up, and the
                bytes it reads plus writes per second -- against a hipMemcpyAsync device-to-device copy of the same byte count
                in the same run (the runtime's figure for "read N + write N", not this code's), and their ratio;
    verify      the MI_PACK_VERIFY pass (mi_pack_info.ms_verify) next to the batch's own chunk pass (mi_stats.ms_sha_chunks);
    delivery    mi_pack_read of the whole blob in GB/s -- against mi_batch_read_file once per chunk in row order (what a
                caller had before packs; a 1/64 sample of the rows) and against mi_batch_read_back of the whole arena;
    commit      a small tree committed all new with MI_MEMFS_CHUNK_PACK, with an index only, and with neither.
chunk_pack_bench.py [out = profiles/chunk_pack.txt] [files = 100000] [runs = 12] [commit files = 20000]   (needs an MI355X)"""
import ctypes as C
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import makisu_amd as M  # noqa: E402
from makisu_amd import workloads as W  # noqa: E402


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    return hip


def d2d_copy_ms(hip, src, nbytes, runs):
    """hipMemcpyAsync device-to-device of nbytes from src into memory of its own, on the null stream: ms per run"""
    dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dst), nbytes) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    out = []
    try:
        for _ in range(runs + 2):
            hip.hipEventRecord(e0, None)
            assert hip.hipMemcpyAsync(dst, src, nbytes, 3, None) == 0            # hipMemcpyDeviceToDevice
            hip.hipEventRecord(e1, None)
            hip.hipEventSynchronize(e1)
            ms = C.c_float()
            hip.hipEventElapsedTime(C.byref(ms), e0, e1)
            out.append(ms.value)
    finally:
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        hip.hipFree(dst)
    return out[2:]                                                                # two warm-up copies


def resident(eng, n_files, runs, say):
    sh = W.c2(files_per_gpu=n_files)
    hip = _hip()
    with eng.batch(sh.n_files, W.batch_bytes_hint(sh)) as b, eng.index() as ix:
        W.fill_batch(b, sh)
        b.run()
        b.rerun()
        ms_chunk_pass = eng.stats()["ms_sha_chunks"]
        chunks = b.chunks()
        known, n_new, n_known = ix.add_batch(b)
        sel = ((known == 0) & (chunks["dup_of"] < 0)).astype(np.uint8)
        st = os.environ.get("MI_ARENA") or "default"
        say("batch: %d files x 64 KiB = %.2f GB, %d chunk rows, %d selected (first occurrences the index did not know); arena: %s" %
            (sh.n_files, sh.n_bytes / 1e9, len(chunks), int(sel.sum()),
             "one allocation (a batch told its size: mi_batch_begin's hints)" if st == "default" else "MI_ARENA=" + st))
        gather, verify = [], []
        info = None
        for r in range(runs + 2):                                                 # two warm-up packs
            with b.pack(select=sel, verify=True) as p:
                info = p.info.as_dict()
                assert info["verified"] == 1
                if r >= 2:
                    gather.append(info["ms_gather"])
                    verify.append(info["ms_verify"])
                if r == runs + 1:
                    ptr, nb = p.device()
                    copy = d2d_copy_ms(hip, ptr, nb, runs)
                    # host delivery: the whole blob through the pack's windows into pageable memory of the caller's
                    buf = np.zeros(nb, dtype=np.uint8)
                    reads = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        eng._check(eng._lib.mi_pack_read(p._h, 0, buf.ctypes.data, nb))
                        reads.append(time.perf_counter() - t0)
        nb = info["blob_bytes"]
        g, c, v = statistics.median(gather), statistics.median(copy), statistics.median(verify)
        say("gather kernel: median %.3f ms of %d runs (min %.3f, max %.3f) for a blob of %d bytes (%d chunk bytes, %d entries): %.2f TB/s read + written" %
            (g, len(gather), min(gather), max(gather), nb, info["chunk_bytes"], info["n_entries"], 2 * nb / (g * 1e-3) / 1e12))
        say("hipMemcpyAsync device-to-device, the same %d bytes, the same run: median %.3f ms of %d (min %.3f, max %.3f): %.2f TB/s read + written" %
            (nb, c, len(copy), min(copy), max(copy), 2 * nb / (c * 1e-3) / 1e12))
        say("ratio gather / copy: %.2f" % (g / c))
        say("verification (MI_PACK_VERIFY: the blob's entries hashed again + compared): median %.3f ms; the batch's own chunk pass: %.3f ms" % (v, ms_chunk_pass))
        say("host delivery, mi_pack_read of the whole blob: best %.3f s of 3 = %.2f GB/s (first %.3f s, with the windows' pinned allocation)" %
            (min(reads), nb / min(reads) / 1e9, reads[0]))
        # what a caller had before: mi_batch_read_file per chunk, in row order, on every 64th selected row
        rows = np.flatnonzero(sel)[::64]
        scratch = np.zeros(1 << 20, dtype=np.uint8)
        fi, off, ln = chunks["file_index"], chunks["offset"], chunks["length"]
        t0 = time.perf_counter()
        got = 0
        for i in rows.tolist():
            eng._check(eng._lib.mi_batch_read_file(b._h, int(fi[i]), int(off[i]), scratch.ctypes.data, int(ln[i])))
            got += int(ln[i])
        dt = time.perf_counter() - t0
        say("mi_batch_read_file once per chunk, every 64th selected row in row order (%d calls, %d bytes): %.3f s = %.3f GB/s, %.1f us per call "
            "(through ctypes: a few us of each are the binding's)" % (len(rows), got, dt, got / dt / 1e9, dt / max(len(rows), 1) * 1e6))
        t0 = time.perf_counter()
        back = b.read_back()
        dt = time.perf_counter() - t0
        say("mi_batch_read_back of the whole arena (%d bytes, one plain copy per file into pageable memory): %.3f s = %.2f GB/s" % (len(back), dt, len(back) / dt / 1e9))


def commit_cost(eng, n_files, file_bytes, say):
    from commit_layer_bench import _make_tree
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    root = tempfile.mkdtemp(prefix="mi_pack_commit_", dir=base)
    try:
        _make_tree(root, n_files, file_bytes, 200)
        time.sleep(0.05)
        res = {"pack + index": [], "index only": [], "neither": []}
        extra = ""
        for rnd in range(4):                                                      # the first round warms the ctx: not counted
            for side in res:
                with M.MemFS(root) as fs, M.ChunkIndex(eng) as ix:
                    if side != "neither":
                        fs.set_index(ix)
                    fs.set_options(chunk_pack=side == "pack + index")
                    t0 = time.perf_counter()
                    r = fs.commit_layer(must_scan=True, gzip_level=M.GZIP_OFF, engine=eng, want_layer=False)
                    dt = time.perf_counter() - t0
                    if side == "pack + index":
                        with fs.take_pack() as p:
                            i = p.info.as_dict()
                        extra = "pack of %d entries, %d bytes: gather %.3f ms, verify %.3f ms; index_new_bytes %d" % (
                            i["n_entries"], i["blob_bytes"], i["ms_gather"], i["ms_verify"], r["stats"]["index_new_bytes"])
                    if rnd:
                        res[side].append(dt)
                    fs.release_device()
        say("commit, %d files x %d bytes all new (fresh handle and index each time; median of 3 after a warm-up round):" % (n_files, file_bytes))
        for side, v in res.items():
            say("    %-13s %.4f s  (%s)" % (side, statistics.median(v), ", ".join("%.4f" % x for x in v)))
        say("    " + extra)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_pack.txt")
    n_files = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    runs = max(10, int(sys.argv[3])) if len(sys.argv) > 3 else 12
    n_commit = int(sys.argv[4]) if len(sys.argv) > 4 else 20000
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with M.Engine(device=0) as eng:
        info = eng.device_info()
        say("chunk packs (tools/chunk_pack_bench.py %d %d %d) on %s" % (n_files, runs, n_commit, info.get("name", info) if isinstance(info, dict) else info))
        resident(eng, n_files, runs, say)
        commit_cost(eng, n_commit, 4096, say)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
