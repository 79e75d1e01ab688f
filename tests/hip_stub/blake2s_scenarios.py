"""Scenarios for tests/test_host_blake2s_double.py: the HOST rules of MI_FLAG_CHUNK_BLAKE2S on the HIP test double.  Kernels
do not run there, so no digest is checked here (tests/test_gpu_blake2s.py does) -- what is checked is who may meet whom: a
MemFS handle keeps the algorithm of the roots it holds, a chunk index its ctx's, the ctxs of one commit agree, and every
refusal comes before anything is walked or changed.  Run with LD_PRELOAD=<the double>; prints one "OK <name>" line each."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import makisu_amd as M  # noqa: E402
from commit_cases import make_tree  # noqa: E402

INVALID, STATE = -1, -6


def refused(code, what, f, *a, **kw):
    try:
        f(*a, **kw)
    except M.MiError as ex:
        assert ex.code == code and what in str(ex), (ex.code, str(ex))
        return
    raise SystemExit("not refused: " + what)


def scenario_handle(tmp, sha, sha_too, b2s, b2s_too):
    root = os.path.join(tmp, "handle_root")
    files = make_tree(root, seed=5)
    assert (sha.chunk_digest, b2s.chunk_digest) == (M.DIGEST_SHA256, M.DIGEST_BLAKE2S)
    with M.MemFS(root) as fs:
        r = fs.commit_layer(must_scan=True, engine=b2s, gzip_level=M.GZIP_OFF)
        assert r["stats"]["n_scanned_files"] == len(files)
        before = fs.entries()
        # the other kind: MI_ERR_STATE, the tree as it was, no layer, nothing walked
        refused(STATE, "other chunk digest algorithm", fs.commit_layer, must_scan=True, engine=sha, gzip_level=M.GZIP_OFF)
        assert fs.entries() == before and fs.commit_stats()["n_scanned_files"] == 0
        refused(STATE, "other chunk digest algorithm", fs.commit_layer, must_scan=True, engine=[sha, sha_too], gzip_level=M.GZIP_OFF)
        # ctxs that disagree among themselves: MI_ERR_INVALID, whatever the handle holds
        refused(INVALID, "different algorithms", fs.commit_layer, must_scan=True, engine=[b2s, sha], gzip_level=M.GZIP_OFF)
        assert fs.entries() == before
        # its own kind goes on: another ctx of the same algorithm, one or two of them; the reference's commit always may
        assert fs.commit_layer(must_scan=True, engine=b2s_too, gzip_level=M.GZIP_OFF)["n_entries"] == 0
        assert fs.commit_layer(must_scan=True, engine=[b2s, b2s_too], gzip_level=M.GZIP_OFF)["n_entries"] == 0
        assert fs.commit_layer(must_scan=True, gzip_level=M.GZIP_OFF)["n_entries"] == 0
        refused(STATE, "mi_memfs_reset first", fs.commit_layer, must_scan=True, engine=sha, gzip_level=M.GZIP_OFF)
        # mi_memfs_reset forgets the tree, its roots and their algorithm
        fs.reset()
        r = fs.commit_layer(must_scan=True, engine=sha, gzip_level=M.GZIP_OFF)
        assert r["stats"]["n_scanned_files"] == len(files) and r["n_entries"] > len(files)
        refused(STATE, "other chunk digest algorithm", fs.commit_layer, must_scan=True, engine=b2s, gzip_level=M.GZIP_OFF)
    with M.MemFS(root) as fs:                       # a handle without roots takes either: header-only commits leave none
        fs.commit_layer(must_scan=True, gzip_level=M.GZIP_OFF)
        assert fs.commit_layer(must_scan=True, engine=sha, gzip_level=M.GZIP_OFF)["n_entries"] == 0
    with M.MemFS(root) as fs:
        fs.commit_layer(must_scan=True, gzip_level=M.GZIP_OFF)
        assert fs.commit_layer(must_scan=True, engine=b2s, gzip_level=M.GZIP_OFF)["n_entries"] == 0
    print("OK handle")


def scenario_index(tmp, sha, b2s, b2s_too):
    root = os.path.join(tmp, "index_root")
    make_tree(root, seed=6, n_dirs=2)
    blob = np.random.default_rng(3).integers(0, 256, 100_000, dtype=np.uint8).tobytes()
    with M.ChunkIndex(sha) as xs, M.ChunkIndex(b2s) as xb:
        with b2s.batch() as b:
            b.add_bytes(blob)
            b.run()
            xb.add_batch(b)                  # (an index takes batches of its own ctx only -- the rule it always had -- and so
                                             # of its own algorithm; what is new is the commit's check below)
        # the commit feeds its handle's index: one of the other algorithm fails the commit before it starts, on either way in
        # (the index's own ctx: mi_index_add_batch; another ctx: the digests through the host)
        for idx, eng, ok in ((xs, b2s, False), (xb, sha, False), (xb, b2s, True), (xb, b2s_too, True), (xs, sha, True)):
            with M.MemFS(root) as fs:
                fs.set_index(idx)
                if ok:
                    assert fs.commit_layer(must_scan=True, engine=eng, gzip_level=M.GZIP_OFF)["n_entries"] > 0
                else:
                    refused(INVALID, "chunk index: the index holds digests of the other", fs.commit_layer, must_scan=True, engine=eng,
                            gzip_level=M.GZIP_OFF)
                    assert fs.entries() == [] and fs.commit_stats()["n_scanned_files"] == 0
    print("OK index")


def scenario_api(tmp, sha, b2s, b2s_too):
    refused(INVALID, "mi_debug_sha_wave_stats", b2s.debug_sha_wave_stats, os.path.join(tmp, "waves.bin"))
    sha.debug_sha_wave_stats(os.path.join(tmp, "waves.bin"))
    sha.debug_sha_wave_stats(None)
    os.environ["MI_SHA_WAVE_STATS"] = os.path.join(tmp, "waves_env.bin")      # ignored by a flagged ctx: no error left behind
    try:
        with M.Engine(flags=M.FLAG_FILE_SHA256 | M.FLAG_CHUNK_BLAKE2S, n_streams=1) as both:
            assert both.chunk_digest == M.DIGEST_BLAKE2S
            assert both._lib.mi_last_error(both._h) in (None, b"")
    finally:
        del os.environ["MI_SHA_WAVE_STATS"]
    print("OK api")


if __name__ == "__main__":
    tmp = sys.argv[1]
    with M.Engine(n_streams=2, staging_bytes=1 << 20) as sha, M.Engine(n_streams=1) as sha_too, \
            M.Engine(flags=M.FLAG_CHUNK_BLAKE2S, n_streams=2, staging_bytes=1 << 20) as b2s, \
            M.Engine(flags=M.FLAG_CHUNK_BLAKE2S, n_streams=2, staging_bytes=1 << 20) as b2s_too:
        scenario_handle(tmp, sha, sha_too, b2s, b2s_too)
        scenario_index(tmp, sha, b2s, b2s_too)
        scenario_api(tmp, sha, b2s, b2s_too)
