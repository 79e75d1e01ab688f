"""What tests/test_gpu_blake2s.py holds a batch of an MI_FLAG_CHUNK_BLAKE2S ctx against, and its child-process cases (settings
that a process reads once: the arena's piece size, the commit's split threshold, the RCCL double).

The reference for the digests is hashlib.blake2s -- RFC 7693 as OpenSSL / the Python core implement it, written by nobody here.
The oracle supplies what does not depend on the digest: cut points (cdc_two_phase) and, given the digests, the duplicate marks."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tree_model(digests, hash_fn=hashlib.blake2s):
    """mi_chunk_root_alg: one hash over at most 64 digests put end to end, levels of fan-out 64 above that"""
    nodes = [bytes(d) for d in digests]
    while len(nodes) > 64:
        nodes = [hash_fn(b"".join(nodes[i:i + 64])).digest() for i in range(0, len(nodes), 64)]
    return hash_fn(b"".join(nodes)).digest()


def model_rows(oracle, cfg, blobs, hash_fn=hashlib.blake2s):
    """(file index, offset, length, digest) per chunk and the root per file, from the oracle's cuts and hashlib"""
    p = oracle.CdcParams(cfg.gear_seed, cfg.mask_bits, cfg.min_size, cfg.max_size)
    fi, off, ln, dg, roots = [], [], [], [], []
    for f, blob in enumerate(blobs):
        blob = bytes(blob)
        ends = [int(e) for e in oracle.cdc_two_phase(np.frombuffer(blob, dtype=np.uint8), p)] if blob else []
        mine, at = [], 0
        for e in ends:
            fi.append(f); off.append(at); ln.append(e - at)
            mine.append(hash_fn(blob[at:e]).digest())
            at = e
        assert at == len(blob)
        dg += mine
        roots.append(tree_model(mine, hash_fn))
    d = np.frombuffer(b"".join(dg), dtype=np.uint8).reshape(-1, 32) if dg else np.zeros((0, 32), np.uint8)
    return (np.array(fi, np.uint64), np.array(off, np.uint64), np.array(ln, np.uint64), d,
            np.frombuffer(b"".join(roots), dtype=np.uint8).reshape(-1, 32) if roots else np.zeros((0, 32), np.uint8))


def check_batch(oracle, eng, blobs, hash_fn=hashlib.blake2s, hinted=True):
    """blobs through the engine's C ABI; every column bit for bit against the model.  Returns (files, chunks)."""
    with (eng.batch(len(blobs), sum(len(b) for b in blobs)) if hinted else eng.batch()) as b:
        for i, blob in enumerate(blobs):
            b.add_bytes(bytes(blob), tag=i)
        b.run()
        files, chunks = b.files().copy(), b.chunks().copy()
        n_unique = eng.stats()["n_unique"]
    fi, off, ln, dg, roots = model_rows(oracle, eng.cfg, blobs, hash_fn)
    assert len(chunks) == len(fi), (len(chunks), len(fi))
    assert np.array_equal(chunks["file_index"], fi)
    assert np.array_equal(chunks["offset"], off) and np.array_equal(chunks["length"], ln), "cut points differ from the oracle's"
    bad = np.nonzero((chunks["sha256"] != dg).any(axis=1))[0]
    assert bad.size == 0, "chunk digests differ from hashlib's: rows %s (lengths %s)" % (bad[:8], ln[bad[:8]])
    bad = np.nonzero((files["chunk_root"] != roots).any(axis=1))[0]
    assert bad.size == 0, "roots differ from the tree model's: files %s (chunks %s)" % (bad[:8], files["n_chunks"][bad[:8]])
    dup, uniq = oracle.dedup(dg) if len(dg) else (np.zeros(0, np.int64), 0)
    assert np.array_equal(chunks["dup_of"], dup) and n_unique == uniq, "dedup marking differs from the oracle's on these digests"
    return files, chunks


def scheme_blobs(oracle):
    """a batch mixing tiny, small and multi-group files at odd sizes: chunk starts at every byte alignment"""
    sizes = [1, 63, 64, 65, 0, 1000, 70001, 262145, 3 * 262144 + 17, 5, 2048, 2049, 1 << 20, 7 * 65536 + 3, 127, 128, 129] * 3
    return [oracle.synth_fill(0x4D414B49, 900 + i, 0, n).tobytes() for i, n in enumerate(sizes)]


# ---- child-process cases -------------------------------------------------------------------------------------------
def case_pieces(tmp):
    """MI_ARENA_PIECE_MB=2 (the caller's environment): a batch that learns its size as it goes lies on an arena of 2 MiB pieces,
    and from 0 bytes on such an arena takes the cooperative loads (MI_SHA_COOP_MIN_GIB_PIECES=0)"""
    import makisu_amd as M
    from oracle import mi_oracle as O
    rng = np.random.default_rng(41)
    blobs = scheme_blobs(O) + [rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes() for _ in range(12)]
    rows = []
    for scheme in (M.SHA_LOADS_AUTO, M.SHA_LOADS_LANE):
        with M.Engine(flags=M.FLAG_CHUNK_BLAKE2S, sha_load_scheme=scheme) as e:
            rows.append(check_batch(O, e, blobs, hinted=False)[1]["sha256"])
    assert np.array_equal(rows[0], rows[1])
    print("OK pieces", len(rows[0]))


def case_split_commit(tmp):
    """mi_memfs_commit_layer_n with two flagged ctxs on one device, MI_COMMIT_SPLIT_MIB=2 (the caller's environment): the larger
    files are split over the ctxs as parts, and a split file's root -- mi_chunk_root_alg over its parts' digests -- is the root
    of the whole file"""
    import makisu_amd as M
    from oracle import mi_oracle as O
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from commit_cases import write_file
    root = os.path.join(tmp, "split_root")
    rng = np.random.default_rng(43)
    files = {"big/a.bin": rng.integers(0, 256, 7 * (1 << 20) + 12345, dtype=np.uint8).tobytes(),
             "big/b.bin": rng.integers(0, 256, 3 * (1 << 20) + 1, dtype=np.uint8).tobytes(),
             "big/zeros.bin": bytes(5 << 20),
             "small/c.bin": rng.integers(0, 256, 70001, dtype=np.uint8).tobytes(), "small/empty": b"", "small/one": b"x"}
    for rel, data in files.items():
        write_file(os.path.join(root, rel), data, 0o644, 1_600_000_000)
    with M.Engine(flags=M.FLAG_CHUNK_BLAKE2S) as e0, M.Engine(flags=M.FLAG_CHUNK_BLAKE2S) as e1, M.Engine() as sha:
        with M.MemFS(root) as fs:
            r = fs.commit_layer(must_scan=True, engine=[e0, e1], gzip_level=M.GZIP_OFF)
            st = r["stats"]
            assert st["n_ctxs"] == 2 and st["n_split_files"] >= 2, st
            for rel, data in files.items():
                want = model_rows(O, e0.cfg, [data])[4][0].tobytes()
                assert fs.root_of("/" + rel) == want, rel
            try:
                fs.commit_layer(must_scan=True, engine=[sha, e1], gzip_level=M.GZIP_OFF)
                raise SystemExit("ctxs of two algorithms were accepted")
            except M.MiError as ex:
                assert ex.code == -1, ex
    print("OK split_commit", st["n_split_files"])


def case_exchange(tmp):
    """MI_RCCL_LIB = the RCCL double (the caller's environment): the _all forms of the exchange refuse batches of two algorithms
    and mark two BLAKE2s batches job-wide"""
    import makisu_amd as M
    from oracle import mi_oracle as O
    blobs = [O.synth_fill(0x4D414B49, 7000 + i, 0, 300000).tobytes() for i in range(4)]
    for flags, ok in (((M.FLAG_CHUNK_BLAKE2S, 0), False), ((0, M.FLAG_CHUNK_BLAKE2S), False),
                      ((M.FLAG_CHUNK_BLAKE2S, M.FLAG_CHUNK_BLAKE2S), True)):
        engs = [M.Engine(flags=f) for f in flags]
        M.comm_init_all(engs)
        bs = [e.batch() for e in engs]
        for k, b in enumerate(bs):
            for blob in blobs[k: k + 3]:                       # rank 1 repeats two of rank 0's files
                b.add_bytes(blob)
            b.run()
        for form in ("allgather", "alltoall"):
            if ok:
                n_total, n_unique = M.dedup_allgather_all(bs, form=form)
                allrows = np.concatenate([b.chunks()["sha256"] for b in bs])
                assert (n_total, n_unique) == (len(allrows), O.dedup(allrows)[1]) and n_unique < n_total
            else:
                try:
                    M.dedup_allgather_all(bs, form=form)
                    raise SystemExit("an exchange of two algorithms was accepted")
                except M.MiError as ex:
                    assert ex.code == -1 and "another algorithm" in str(ex), ex
        for b in bs:
            b.free()
        for e in engs:
            e.comm_destroy()
            e.close()
    print("OK exchange")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    try:
        import torch  # noqa: F401  (before the engine: one HIP runtime per process)
    except ImportError:
        pass
    {"pieces": case_pieces, "split_commit": case_split_commit, "exchange": case_exchange}[sys.argv[1]](sys.argv[2])
