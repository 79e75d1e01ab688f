"""Files rebuilt from chunk packs and recipes, measured (writes profiles/chunk_restore.txt).

On a C2-shaped resident batch (100 000 x 64 KiB synthetic files) every first occurrence is packed, a pack set is built from
the device pack, and ALL files are restored from their recipes into a second batch:
    set         mi_packset_add_pack: the device-to-device copy, MI_PACKSET_VERIFY's pass, the table insert (mi_packset_info);
    assemble    the assemble kernel's time from HIP events (mi_recipe_stats.ms_assemble), median of the runs after a warm-up,
                and the bytes it reads plus writes per second -- against a hipMemcpyAsync device-to-device copy of the same
                byte count in the same run (the runtime's figure for "read N + write N"), and their ratio; the resolve step
                (36 bytes a row up + the lookup) and MI_RECIPE_VERIFY's pass next to the batch's own chunk pass;
    identity    the restored batch, run, has the first batch's roots.
chunk_restore_bench.py [out = profiles/chunk_restore.txt] [files = 100000] [runs = 12]   (needs an MI355X)"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import makisu_amd as M  # noqa: E402
from makisu_amd import workloads as W  # noqa: E402
from chunk_pack_bench import _hip, d2d_copy_ms  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_restore.txt")
    n_files = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    runs = max(10, int(sys.argv[3])) if len(sys.argv) > 3 else 12
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    hip = _hip()
    with M.Engine(device=0) as eng:
        info = eng.device_info()
        say("chunk restore (tools/chunk_restore_bench.py %d %d) on %s" % (n_files, runs, info["name"]))
        sh = W.c2(files_per_gpu=n_files)
        with eng.batch(sh.n_files, W.batch_bytes_hint(sh)) as b, eng.packset() as s:
            W.fill_batch(b, sh)
            b.run()
            b.rerun()
            ms_chunk_pass = eng.stats()["ms_sha_chunks"]
            files, chunks = b.files().copy(), b.chunks().copy()
            roots = b.roots().copy()
            sel = (chunks["dup_of"] < 0).astype(np.uint8)
            with b.pack(select=sel) as p:
                pi = p.info.as_dict()
                s.add_pack(p, verify=True)
            si = s.info.as_dict()
            say("batch: %d files x 64 KiB = %.2f GB, %d chunk rows, %d first occurrences packed: a blob of %d bytes" %
                (sh.n_files, sh.n_bytes / 1e9, len(chunks), pi["n_entries"], pi["blob_bytes"]))
            say("set from the device pack: copy %.3f ms, MI_PACKSET_VERIFY %.3f ms, table insert %.3f ms (host clocks around the "
                "synchronised steps); %d distinct digests" % (si["ms_upload"], si["ms_verify"], si["ms_insert"], si["n_digests"]))
            dig, lens = np.ascontiguousarray(chunks["sha256"]), chunks["length"].astype(np.uint32)
            first, cnt = files["first_chunk"].astype(np.int64), files["n_chunks"].astype(np.int64)
            recipes = [(dig[f:f + n], lens[f:f + n]) for f, n in zip(first.tolist(), cnt.tolist())]
            b.free()                                                              # the second batch takes its place
            resolve, assemble, verify = [], [], []
            st = None
            with eng.batch(sh.n_files, W.batch_bytes_hint(sh)) as r:
                for k in range(runs + 2):                                         # two warm-up rounds
                    r.reset()
                    st = r.add_recipes(s, recipes, verify=True).as_dict()
                    if k >= 2:
                        resolve.append(st["ms_resolve"])
                        assemble.append(st["ms_assemble"])
                        verify.append(st["ms_verify"])
                nb = st["bytes"]
                a = statistics.median(assemble)
                say("restore of all %d files (%d rows, %d bytes, %d joined units), median of %d runs after a warm-up:" %
                    (st["n_files"], st["n_rows"], nb, st["n_joined_units"], len(assemble)))
                say("    resolve (36 bytes a row up, the lookup, the first bad row back): %.3f ms (min %.3f, max %.3f)" %
                    (statistics.median(resolve), min(resolve), max(resolve)))
                say("    assemble kernel: %.3f ms (min %.3f, max %.3f): %.2f TB/s read + written" %
                    (a, min(assemble), max(assemble), 2 * nb / (a * 1e-3) / 1e12))
                say("    MI_RECIPE_VERIFY (the rows hashed in the arena + compared): %.3f ms; the first batch's own chunk pass: %.3f ms" %
                    (statistics.median(verify), ms_chunk_pass))
                r.run()
                same = bool(np.array_equal(r.roots(), roots))
                say("the restored batch, run: its %d roots are the first batch's: %s" % (len(roots), same))
                assert same
        # the runtime's copy of the same byte count, in the same run, out of memory of its own
        mem = C.c_void_p()
        assert hip.hipMalloc(C.byref(mem), nb) == 0
        try:
            copy = d2d_copy_ms(hip, mem, nb, runs)
        finally:
            hip.hipFree(mem)
        c = statistics.median(copy)
        say("hipMemcpyAsync device-to-device, the same %d bytes, the same run: median %.3f ms of %d (min %.3f, max %.3f): %.2f TB/s read + written" %
            (nb, c, len(copy), min(copy), max(copy), 2 * nb / (c * 1e-3) / 1e12))
        say("ratio assemble / copy: %.2f" % (a / c))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
