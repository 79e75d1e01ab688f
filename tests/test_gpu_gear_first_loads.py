"""The bitmap-free Gear marking kernels (csrc/gear_cdc.hip: gear_cdc_small_fast_kernel, gear_tile_mark_kernel) read
a wave's descriptor and issue its first loads BEFORE the workgroup fills the Gear table and meets at its barrier, and
fill the table with one global load per entry.  What can go wrong with that sits at the edges of a launch: waves past
the list's end that only help with the table (a last workgroup that is not full), empty files and files shorter than
a piece, whose lanes issue no first loads, tile slots past a large file's end, and a dense file, which leaves through the
dense list after the barrier.  Every batch is checked row by row against the oracle's scan_batch, like
tests/test_gpu_parity.py."""
import numpy as np
import pytest

try:
    import torch  # noqa: F401  (before the engine: its HIP runtime serves the library too; see test_gpu_parity.py)
except ImportError:          # CPU-only collection without torch: the GPU tests are skipped anyway
    torch = None

import planted_gear as PG

pytestmark = pytest.mark.gpu

SEED = 0x4D414B49
T = 64 * 1024
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 65535, 65536]


@pytest.fixture(scope="module")
def eng():
    import makisu_amd
    e = makisu_amd.Engine()
    yield e
    e.close()


def _check(oracle, eng, blobs):
    """Every row of the batch against the oracle's."""
    with eng.batch(len(blobs), sum(len(b) for b in blobs)) as b:
        for i, blob in enumerate(blobs):
            b.add_bytes(blob, tag=i)
        b.run()
        files, chunks = b.files().copy(), b.chunks().copy()
    if not len(blobs):
        assert len(files) == 0 and len(chunks) == 0
        return files, chunks
    sizes = np.array([len(x) for x in blobs], dtype=np.uint64)
    data = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    c = eng.cfg
    rf, rc = oracle.scan_batch(data if data.size else np.zeros(1, np.uint8), offs, sizes,
                               oracle.CdcParams(c.gear_seed, c.mask_bits, c.min_size, c.max_size))
    assert np.array_equal(files["size"], sizes)
    assert np.array_equal(files["n_chunks"], rf["n_chunks"])
    assert np.array_equal(files["first_chunk"], rf["first_chunk"])
    assert len(chunks) == len(rc)
    assert np.array_equal(chunks["file_index"], rc["file_index"])
    assert np.array_equal(chunks["offset"], rc["offset"]), "cut points differ"
    assert np.array_equal(chunks["length"], rc["length"]), "cut points differ"
    assert np.array_equal(chunks["sha256"], rc["sha256"]), "chunk digests differ"
    assert np.array_equal(files["chunk_root"], rf["chunk_root"]), "file roots differ"
    assert np.array_equal(chunks["dup_of"], rc["dup_of"]), "dedup marking differs"
    return files, chunks


def _sizes(n):
    """n sizes out of SIZES: neighbours in a workgroup differ, an empty file sits between two full ones, and the list's
    last file is shorter than a piece."""
    s = [SIZES[(7 * i + 9) % len(SIZES)] for i in range(n)]
    for k, v in enumerate([65536, 0, 65536]):
        if k < n:
            s[k] = v
    if n:
        s[-1] = 65
    return s


@pytest.fixture(scope="module")
def content(oracle):
    """One tile of random bytes per residue; a file is a prefix of one of them (files that share one are duplicates of
    each other in their first chunks, which the dedup columns then have to show)."""
    return [oracle.synth_fill(SEED, k, 0, T).tobytes() for k in range(7)]


def _blobs(content, sizes):
    return [content[i % len(content)][:n] for i, n in enumerate(sizes)]


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 17])
def test_small_batches_around_a_workgroup_of_eight(oracle, eng, content, n):
    """Eight files per workgroup: lists that leave waves of the last workgroup without a file."""
    _check(oracle, eng, _blobs(content, _sizes(n)))


def test_every_size_class_in_every_wave(oracle, eng, content):
    """Each of the ten sizes in each of the eight wave positions of a workgroup."""
    sizes = [SIZES[(i // 8 + i % 8) % len(SIZES)] for i in range(8 * len(SIZES))]
    _check(oracle, eng, _blobs(content, sizes))


def test_a_dense_file_between_ordinary_files(oracle, eng, content):
    """A file with more than 64 candidates is handed to the bitmap kernel through the dense list; its neighbours in the
    workgroup are marked as ever."""
    ends = [1000 + 128 * j for j in range(70)]
    dense = PG.plant(T, ends)
    cls = PG.classify(ends, T)
    assert not cls["large"] and cls["tiles"][0]["count"] > 64 and cls["tiles"][0]["dense"]
    blobs = _blobs(content, _sizes(24))
    blobs[10] = dense
    assert len(blobs[9]) and len(blobs[11])
    _check(oracle, eng, blobs)


def test_large_files_with_ragged_last_tiles(oracle, eng):
    """Three large files of 2, 5 and 9 tiles, the first and last with a ragged last tile: six groups, 24 tile slots of
    which 8 lie past their file's end."""
    blobs = [oracle.synth_fill(SEED, 100 + i, 0, n).tobytes() for i, n in enumerate([T + 1, 5 * T, 9 * T - 1])]
    _check(oracle, eng, blobs)
