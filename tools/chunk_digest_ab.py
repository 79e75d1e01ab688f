#!/usr/bin/env python3
"""SHA-256 against BLAKE2s-256 as the chunk digest (MI_FLAG_CHUNK_BLAKE2S), same process, same box, alternating.

C2 resident in HBM (--files x 64 KiB synthetic, one allocation per ctx), one batch at a time: an SHA-256 ctx and a BLAKE2s
ctx take turns, --alternations turns of --steps warmed steps each.  Per algorithm: minimum and median of ms_sha_chunks (the
chunk pass), ms_sha_files (the root passes) and ms_total from mi_get_stats; both VALU roofs of the same run (the compression
alone, at 8 and 4 waves per SIMD); each chunk pass as a fraction of its OWN roof; the spread between turns.  Then the geometry
and load-scheme trials of DESIGN.md 4.2b: the BLAKE2s ctx as it ships against one with 3 and 4 workgroups per CU and one
with the cooperative loads, alternating the same way (--trial-alternations turns).

    python tools/chunk_digest_ab.py [--files 100000] [--out profiles/chunk_digest_ab.txt]

Needs the GPU: there is no CPU path to time."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401,E402  (before the engine: one HIP runtime per process)
except ImportError:
    pass
import makisu_amd as M  # noqa: E402
from makisu_amd import workloads  # noqa: E402

KEYS = ("ms_sha_chunks", "ms_sha_files", "ms_total")


class Side:
    """one ctx with its C2 batch, run once"""

    def __init__(self, name, sh, **cfg):
        self.name, self.cfg = name, cfg
        self.eng = M.Engine(**cfg)
        self.b = self.eng.batch(sh.n_files, sh.n_bytes)
        self.b.add_synthetic(sh.sizes, sh.cids, seed=sh.seed)
        self.b.run()
        self.turns = []                       # per turn: {key: [ms per step]}

    def turn(self, steps, warm):
        rec = {k: [] for k in KEYS}
        for i in range(warm + steps):
            self.b.rerun()
            if i >= warm:
                st = self.eng.stats()
                for k in KEYS:
                    rec[k].append(st[k])
        self.turns.append(rec)

    def all(self, k):
        return np.concatenate([t[k] for t in self.turns])

    def turn_medians(self, k):
        return [float(np.median(t[k])) for t in self.turns]

    def close(self):
        self.b.free()
        self.eng.close()


def alternate(sides, turns, steps, warm):
    for _ in range(turns):
        for s in sides:
            s.turn(steps, warm)


def report(out, s, n_bytes, roof):
    for k in KEYS:
        a, tm = s.all(k), s.turn_medians(k)
        out("%-22s %-14s min %.4f  median %.4f ms   per turn %s   spread of turn medians %.4f ms (%.2f %%)"
            % (s.name, k, a.min(), np.median(a), " ".join("%.4f" % x for x in tm), max(tm) - min(tm),
               100.0 * (max(tm) - min(tm)) / np.median(tm)))
    med = float(np.median(s.all("ms_sha_chunks")))
    rate = n_bytes / (med * 1e-3)
    out("%-22s chunk pass %.1f GB/s = %.3f of its own VALU roof (%.1f GB/s, the better of 8 and 4 waves per SIMD)"
        % (s.name, rate / 1e9, rate / roof, roof / 1e9))
    return med, rate / roof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=100000)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--trial-alternations", type=int, default=3)
    ap.add_argument("--trial-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    sh = workloads.c2(files_per_gpu=args.files)
    out("chunk_digest_ab: C2 %d x 64 KiB = %.2f GB resident, one batch at a time; %d turns x %d steps (+ %d warm-up steps per turn)"
        % (sh.n_files, sh.n_bytes / 1e9, args.alternations, args.steps, args.warm))
    sha, b2s = Side("sha256", sh), Side("blake2s", sh, flags=M.FLAG_CHUNK_BLAKE2S)
    info = sha.eng.device_info()
    out("device: %s, %d CUs" % (info["name"], info["n_cu"]))
    n_chunks = len(sha.b.chunks())
    assert np.array_equal(sha.b.chunks()["length"], b2s.b.chunks()["length"]) and len(b2s.b.chunks()) == n_chunks
    assert not np.array_equal(sha.b.chunks()["sha256"][:64], b2s.b.chunks()["sha256"][:64])
    out("%d chunks either way (the cuts do not depend on the digest)" % n_chunks)
    alternate([sha, b2s], args.alternations, args.steps, args.warm)
    roofs = {"sha256": {w: sha.eng.sha_valu_roof(w, 0) for w in (8, 4)}, "blake2s": {w: sha.eng.blake2s_valu_roof(w, 0) for w in (8, 4)}}
    for name, r in roofs.items():
        out("%-22s VALU roof (the compression alone, this run): 8 waves per SIMD %.1f GB/s, 4 waves %.1f GB/s" % (name, r[8] / 1e9, r[4] / 1e9))
    m_sha, f_sha = report(out, sha, sh.n_bytes, max(roofs["sha256"].values()))
    m_b2s, f_b2s = report(out, b2s, sh.n_bytes, max(roofs["blake2s"].values()))
    out("blake2s / sha256: chunk pass %.3f, roof %.3f (sha256 roof / blake2s roof), ms_total %.3f"
        % (m_b2s / m_sha, max(roofs["sha256"].values()) / max(roofs["blake2s"].values()),
           float(np.median(b2s.all("ms_total"))) / float(np.median(sha.all("ms_total")))))
    sha.close()

    out("")
    out("trials on the BLAKE2s ctx (%d turns x %d steps each, alternating with the ctx as it ships):" % (args.trial_alternations, args.trial_steps))
    b2s.turns = []
    b2s.name = "blake2s as shipped"
    for name, cfg in (("3 workgroups per CU", {"sha_blocks_per_cu": 3}), ("4 workgroups per CU", {"sha_blocks_per_cu": 4}),
                      ("cooperative loads", {"sha_load_scheme": M.SHA_LOADS_COOP}),
                      ("cooperative, 3 per CU", {"sha_load_scheme": M.SHA_LOADS_COOP, "sha_coop_blocks_per_cu": 3})):
        t = Side("blake2s " + name, sh, flags=M.FLAG_CHUNK_BLAKE2S, **cfg)
        n0 = len(b2s.turns)
        alternate([b2s, t], args.trial_alternations, args.trial_steps, args.warm)
        base = [float(np.median(x["ms_sha_chunks"])) for x in b2s.turns[n0:]]
        mine = t.turn_medians("ms_sha_chunks")
        out("%-32s chunk pass per turn %s   as shipped beside it %s   difference of medians %+.4f ms (spread as shipped %.4f)"
            % (name, " ".join("%.4f" % x for x in mine), " ".join("%.4f" % x for x in base),
               float(np.median(mine)) - float(np.median(base)), max(base) - min(base)))
        t.close()
    b2s.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
