"""MI_FLAG_CHUNK_BLAKE2S on the GPU, through the C ABI: every chunk digest = hashlib.blake2s of the chunk's bytes, every root the
fan-out-64 tree with BLAKE2s-256 at every node, bit for bit; cuts and duplicate marks the oracle's (they do not depend on the
digest); and who may meet whom -- handle, index, parts, both flags, the default path untouched (tests/blake2s_cases.py has the
model)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (before the engine: one HIP runtime per process)
except ImportError:
    torch = None

from blake2s_cases import ROOT, check_batch, model_rows, scheme_blobs, tree_model

pytestmark = pytest.mark.gpu
SEED = 0x4D414B49
CASES = os.path.join(ROOT, "tests", "blake2s_cases.py")


@pytest.fixture(scope="module")
def b2s():
    import makisu_amd
    e = makisu_amd.Engine(flags=makisu_amd.FLAG_CHUNK_BLAKE2S)
    assert e.chunk_digest == makisu_amd.DIGEST_BLAKE2S
    yield e
    e.close()


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _edge_blobs():
    rng = np.random.default_rng(17)
    sizes = list(range(0, 201)) + [64 * k + d for k in range(2, 9) for d in (-1, 0, 1)] + [2048, 65535, 65536]
    return [_rand(rng, n) for n in sizes]


def test_every_small_size_and_every_block_boundary(oracle, b2s):
    """one file of every size 0..200; 64k-1, 64k, 64k+1 for k = 2..8 (the last block is full, or one byte, or one byte short); 2 048,
    65 535, 65 536.  A file below min_size is one chunk: these ARE the string lengths the kernel sees, at whatever alignment the
    arena gives them; the empty file has no chunk and its root is the hash of the empty string"""
    files, chunks = check_batch(oracle, b2s, _edge_blobs())
    assert files["n_chunks"][0] == 0 and bytes(files["chunk_root"][0]) == hashlib.blake2s(b"").digest()
    assert bytes(chunks["sha256"][0]) == hashlib.blake2s(_edge_blobs()[1]).digest()


def test_random_zero_and_periodic_files(oracle, b2s):
    rng = np.random.default_rng(18)
    period = _rand(rng, 1000)
    check_batch(oracle, b2s, [_rand(rng, 5 << 20), bytes(5 << 20), (period * 5300)[: 5 << 20]])


def test_a_three_level_root(oracle):
    """2 MiB under min 64 / max 256: more than 4 096 chunks, so the root is hashed over three levels (two reduction passes)"""
    import makisu_amd
    with makisu_amd.Engine(flags=makisu_amd.FLAG_CHUNK_BLAKE2S, mask_bits=6, min_size=64, max_size=256) as e:
        files, _ = check_batch(oracle, e, [oracle.synth_fill(SEED, 4100, 0, 2 << 20).tobytes(), oracle.synth_fill(SEED, 4101, 0, 300000).tobytes(),
                                           b"", bytes(70000)])
        assert files["n_chunks"][0] > 4096


def test_root_tree_exact_chunk_counts(oracle):
    """test_gpu_parity.py's test_chunk_root_tree_exact_chunk_counts with BLAKE2s at every node: files of exactly N chunks
    (mask_bits 0, min_size = max_size = 64) at the tree's edges up to 262 145 chunks (three reduction passes), then a batch
    whose one planned reduction pass has no file to reduce"""
    import makisu_amd
    from table_models import ROOT_EDGE_CHUNKS
    with makisu_amd.Engine(flags=makisu_amd.FLAG_CHUNK_BLAKE2S, mask_bits=0, min_size=64, max_size=64) as e:
        counts = ROOT_EDGE_CHUNKS[:5] + [0] + ROOT_EDGE_CHUNKS[5:]
        files, _ = check_batch(oracle, e, [oracle.synth_fill(SEED, 7000 + i, 0, 64 * n).tobytes() for i, n in enumerate(counts)])
        assert files["n_chunks"].tolist() == counts and max(counts) == 262145
        counts = [63, 1, 0, 62, 63]
        files, _ = check_batch(oracle, e, [oracle.synth_fill(SEED, 7100 + i, 0, 64 * n).tobytes() for i, n in enumerate(counts)])
        assert files["n_chunks"].tolist() == counts


@pytest.mark.parametrize("mask_bits,min_size,max_size", [(0, 64, 64), (4, 128, 3000), (9, 512, 10000), (16, 4096, 262144),
                                                         (13, 2048, 1 << 20)])
def test_param_sets_of_the_large_file_suite(oracle, mask_bits, min_size, max_size):
    """test_gpu_large_files.py's sweep (five of its sets, the ends and the middle): dense tiles, chunks longer than a group -- on
    files of several groups; strings of up to 1 MiB on one lane"""
    import makisu_amd
    G = 256 * 1024
    with makisu_amd.Engine(flags=makisu_amd.FLAG_CHUNK_BLAKE2S, mask_bits=mask_bits, min_size=min_size, max_size=max_size) as e:
        blobs = [oracle.synth_fill(SEED, 3200, 0, 5 * G + 4321).tobytes(), oracle.synth_fill(SEED, 3201, 0, G + 70000).tobytes(),
                 bytes(3 * G + 17), oracle.synth_fill(SEED, 3202, 0, 300).tobytes(), oracle.synth_fill(SEED, 3203, 0, 2 * G).tobytes()]
        check_batch(oracle, e, blobs)


def test_duplicated_files(oracle, b2s):
    rng = np.random.default_rng(19)
    a, b, c = _rand(rng, 300000), _rand(rng, 70001), _rand(rng, 5)
    files, chunks = check_batch(oracle, b2s, [a, b, a, c, b + a, a, c, bytes(100000), bytes(100000)])
    assert (chunks["dup_of"] >= 0).sum() > len(chunks) // 3
    assert np.array_equal(files["chunk_root"][0], files["chunk_root"][2]) and not np.array_equal(files["chunk_root"][0], files["chunk_root"][1])


@pytest.mark.parametrize("kw", [{"sha_load_scheme": 2}, {"sha_load_scheme": 2, "sha_coop_blocks_per_cu": 3}, {"sha_load_scheme": 1},
                                {"sha_load_scheme": 1, "sha_blocks_per_cu": 3}, {"sha_sched": 1}],
                         ids=["coop", "coop3", "lane", "lane3", "flat"])
def test_each_load_scheme_forced(oracle, kw):
    """the knobs test_gpu_sha_schemes.py uses (mi_config.sha_load_scheme: 1 = lane-owned, 2 = quad-cooperative; workgroups per CU;
    the flat string sharing): the same batch, the same rows"""
    import makisu_amd
    with makisu_amd.Engine(flags=makisu_amd.FLAG_CHUNK_BLAKE2S, **kw) as e:
        check_batch(oracle, e, scheme_blobs(oracle) + _edge_blobs()[:130])


def _child(case, tmp, **env):
    p = subprocess.run([sys.executable, CASES, case, str(tmp)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and ("OK " + case) in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]


def test_on_an_arena_of_2_mib_pieces(tmp_path):
    _child("pieces", tmp_path, MI_ARENA_PIECE_MB="2", MI_SHA_COOP_MIN_GIB_PIECES="0")


@pytest.mark.parametrize("seed", range(20))
def test_seeded_random_batches(oracle, b2s, seed):
    """several hundred files, sizes log-uniform from 1 B to 8 MiB, a tenth of them copies of earlier ones"""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(300, 500))
    sizes = np.exp(rng.uniform(0, np.log(8 << 20), n)).astype(np.int64)
    blobs = []
    for s in sizes:
        blobs.append(blobs[int(rng.integers(0, len(blobs)))] if blobs and rng.random() < 0.1 else _rand(rng, int(s)))
    check_batch(oracle, b2s, blobs)


def test_flag_off_is_sha256_as_before(oracle):
    """a default ctx on the same inputs: SHA-256 digests and roots equal to the oracle's (and to hashlib's through the same model):
    the new path is not reached by default"""
    import makisu_amd
    blobs = _edge_blobs() + scheme_blobs(oracle)[:20]
    with makisu_amd.Engine() as e:
        assert e.chunk_digest == makisu_amd.DIGEST_SHA256
        files, chunks = check_batch(oracle, e, blobs, hash_fn=hashlib.sha256)
        data = np.frombuffer(b"".join(blobs), dtype=np.uint8)
        sizes = np.array([len(x) for x in blobs], dtype=np.uint64)
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
        p = oracle.CdcParams(e.cfg.gear_seed, e.cfg.mask_bits, e.cfg.min_size, e.cfg.max_size)
        rf, rc = oracle.scan_batch(data, offs, sizes, p, True, 8, 0)
        assert np.array_equal(chunks["sha256"], rc["sha256"]) and np.array_equal(files["chunk_root"], rf["chunk_root"])
        assert np.array_equal(chunks["dup_of"], rc["dup_of"])


def test_both_flags(oracle):
    """FLAG_FILE_SHA256 | FLAG_CHUNK_BLAKE2S: the whole-file digest Docker sees stays SHA-256, the chunk digests are BLAKE2s; so does
    sha256_many on such a ctx"""
    import makisu_amd
    blobs = _edge_blobs()[::7] + scheme_blobs(oracle)[:17]
    with makisu_amd.Engine(flags=makisu_amd.FLAG_FILE_SHA256 | makisu_amd.FLAG_CHUNK_BLAKE2S) as e:
        files, _ = check_batch(oracle, e, blobs)
        for i, blob in enumerate(blobs):
            assert bytes(files["file_sha256"][i]) == hashlib.sha256(blob).digest(), i
        assert [bytes(g) for g in e.sha256_many(blobs[:40])] == [hashlib.sha256(x).digest() for x in blobs[:40]]


def test_a_file_in_three_parts_has_the_root_of_the_whole_file(oracle, b2s, tmp_path):
    """mi_batch_add_path_part, a batch per part: the parts' chunk digests put end to end are the whole file's, and mi_chunk_root_alg
    over them is the root the engine gives the file scanned whole"""
    import makisu_amd
    from makisu_amd.distributed import resolve_parts_local
    n = 3 * (1 << 20) + 4567
    data = oracle.synth_fill(SEED, 5100, 0, n).tobytes()
    path = tmp_path / "whole.bin"
    path.write_bytes(data)
    files, chunks = check_batch(oracle, b2s, [data])
    from makisu_amd.workloads import PART_ALIGN as G                        # part bounds are multiples of it; the last end is the file's
    bounds = [(0, 4 * G), (4 * G, 9 * G), (9 * G, n)]
    batches = [b2s.batch() for _ in bounds]
    try:
        for b, (lo, hi) in zip(batches, bounds):
            b.add_path_part(str(path), lo, hi, file_size=n)
        resolve_parts_local([(b, [(0, k)]) for k, b in enumerate(batches)])
        rows = []
        for b in batches:
            b.run()
            rows.append(b.chunks()["sha256"].copy())
        got = np.concatenate(rows)
    finally:
        for b in batches:
            b.free()
    assert np.array_equal(got, chunks["sha256"])
    assert makisu_amd.chunk_root(got, alg=makisu_amd.DIGEST_BLAKE2S) == bytes(files["chunk_root"][0]) == tree_model(got)
    assert makisu_amd.chunk_root(got) != bytes(files["chunk_root"][0])


def test_a_commit_over_two_ctxs_splits_files_and_keeps_their_roots(tmp_path):
    _child("split_commit", tmp_path, MI_COMMIT_SPLIT_MIB="2")


def test_the_exchange_refuses_batches_of_two_algorithms(tmp_path):
    from test_gpu_native_exchange import STUB, STUB_DIR
    src = os.path.join(STUB_DIR, "mi_rccl_stub.cpp")
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", STUB,
                               "-lrt", "-lpthread"])
    _child("exchange", tmp_path, MI_RCCL_LIB=STUB)


def test_content_aware_commit_and_the_handles_algorithm(oracle, b2s, tmp_path):
    """one content-aware commit on a flagged ctx: every stored root is the model's; a same-size same-second rewrite is caught; a
    commit on the same handle with an SHA-256 ctx is MI_ERR_STATE and changes nothing; after mi_memfs_reset it succeeds"""
    import makisu_amd as M
    from commit_cases import make_tree
    root = str(tmp_path / "root")
    mtime = 1_600_000_000
    tree = make_tree(root, seed=23, mtime=mtime)
    with M.MemFS(root) as fs, M.Engine() as sha:
        r = fs.commit_layer(must_scan=True, engine=b2s, gzip_level=M.GZIP_OFF)
        assert r["stats"]["n_scanned_files"] == len(tree)
        for rel, data in tree.items():
            assert fs.root_of("/" + rel) == model_rows(oracle, b2s.cfg, [data])[4][0].tobytes(), rel
        assert fs.commit_layer(must_scan=True, engine=b2s, gzip_level=M.GZIP_OFF)["n_entries"] == 0
        rel = next(k for k, v in sorted(tree.items()) if len(v) > 20000)
        new = bytearray(tree[rel])
        new[len(new) // 2] ^= 0x55
        st = os.stat(os.path.join(root, rel))
        with open(os.path.join(root, rel), "r+b") as f:                       # in place: same size, and the same second put back
            f.write(bytes(new))
        os.utime(os.path.join(root, rel), ns=(st.st_atime_ns, st.st_mtime_ns))
        r = fs.commit_layer(must_scan=True, engine=b2s, gzip_level=M.GZIP_OFF)
        parts = rel.split("/")
        assert [e["relpath"] for e in r["layer"]] == ["/".join(parts[:k]) for k in range(1, len(parts) + 1)]   # the file + its ancestors
        assert r["stats"]["n_content_changed"] == 1, r["stats"]
        assert fs.root_of("/" + rel) == model_rows(oracle, b2s.cfg, [bytes(new)])[4][0].tobytes()
        before = fs.entries()
        with pytest.raises(M.MiError) as ei:
            fs.commit_layer(must_scan=True, engine=sha, gzip_level=M.GZIP_OFF)
        assert ei.value.code == -6 and "other chunk digest algorithm" in str(ei.value)
        assert fs.entries() == before and fs.commit_stats()["n_scanned_files"] == 0
        assert fs.commit_layer(must_scan=True, engine=b2s, gzip_level=M.GZIP_OFF)["n_entries"] == 0     # no layer was added in between
        fs.reset()
        r = fs.commit_layer(must_scan=True, engine=sha, gzip_level=M.GZIP_OFF)
        assert r["stats"]["n_scanned_files"] == len(tree)
        tree[rel] = bytes(new)
        for k, data in list(tree.items())[:12]:
            assert fs.root_of("/" + k) == model_rows(oracle, sha.cfg, [data], hashlib.sha256)[4][0].tobytes(), k


def test_the_index_keeps_to_its_algorithm(oracle, b2s):
    """add_batch from a ctx of the other kind is MI_ERR_INVALID; two flagged batches with shared content: the second finds the shared
    chunks known, and only those"""
    import makisu_amd as M
    rng = np.random.default_rng(29)
    shared, own1, own2 = _rand(rng, 400000), _rand(rng, 300000), _rand(rng, 200000)
    with M.Engine() as sha, M.ChunkIndex(b2s) as xb, M.ChunkIndex(sha) as xs:
        with b2s.batch() as b1, b2s.batch() as b2, sha.batch() as bs:
            for b, blobs in ((b1, [shared, own1]), (b2, [own2, shared]), (bs, [shared])):
                for x in blobs:
                    b.add_bytes(x)
                b.run()
            for idx, b in ((xs, b1), (xb, bs)):
                with pytest.raises(M.MiError) as ei:
                    idx.add_batch(b)
                assert ei.value.code == -1
            known, n_new, n_known = xb.add_batch(b1)
            assert n_known == 0 and n_new == len(known) == len(xb)
            known, n_new, n_known = xb.add_batch(b2)
            ch = b2.chunks()
            assert np.array_equal(known.astype(bool), ch["file_index"] == 1) and n_known == int((ch["file_index"] == 1).sum()) > 0
            digests = {hashlib.blake2s(shared[int(o): int(o) + int(n)]).digest() for o, n in zip(ch["offset"][ch["file_index"] == 1],
                                                                                                 ch["length"][ch["file_index"] == 1])}
            blob = xb.export()
            assert digests <= {blob[i: i + 32] for i in range(0, len(blob), 32)}
            known, _, n_known = xs.add_batch(bs)                         # the same content under SHA-256: another index, nothing known
            assert n_known == 0


def test_the_wave_record_is_sha_only_and_the_roof_is_positive(b2s):
    import makisu_amd as M
    with pytest.raises(M.MiError) as ei:
        b2s.debug_sha_wave_stats("/tmp/never_written.bin")
    assert ei.value.code == -1
    r8, r4 = b2s.blake2s_valu_roof(), b2s.blake2s_valu_roof(4, 256)
    assert r8 > 0 and r4 > 0
    with M.Engine() as sha:
        assert sha.blake2s_valu_roof(2, 64) > 0                            # any ctx may ask
