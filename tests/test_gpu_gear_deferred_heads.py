"""The bitmap-free Gear marking kernels (csrc/gear_cdc.hip: gear_cdc_small_fast_kernel, gear_tile_mark_kernel) read no
warm-up line: a lane rolls the first 64 bytes of its 1 KiB run untested, and tests them at the END of its run from the
hash its left neighbour hands up (DEFERRED HEADS, mark_tile_loaded).  What can go wrong with that sits where the scheme
adds a boundary: a file or a last run shorter than a head, a candidate whose 64-byte window straddles two lanes, a
candidate at the last offset of a head or the first behind it, lane 0 of a later tile (which still loads across the
tile's edge), the order of head and body candidates in the 64-entry list, and a run that overflows its packs.  Every
batch is checked row by row against the oracle's scan_batch, like tests/test_gpu_gear_first_loads.py."""
import numpy as np
import pytest

try:
    import torch  # noqa: F401  (before the engine: its HIP runtime serves the library too; see test_gpu_parity.py)
except ImportError:          # CPU-only collection without torch: the GPU tests are skipped anyway
    torch = None

import planted_gear as PG

pytestmark = pytest.mark.gpu

SEED = PG.SEED
T, RUN, W = PG.T, PG.RUN, PG.W
SMALL = [0, 1, 63, 64, 65, 127, 128, 1023, 1024, 1025, 1087, 1088, 1089, 2047, 2048, 2049,
         64512 + 1, 64512 + 63, 64512 + 64, 64512 + 65, 65535, 65536]
LARGE = [65537, 65536 + 1024 + 10, 3 * 65536 + 70]
OFFSETS = [0, 1, 62, 63, 64, 65]                                  # run offset of a stone's last byte
PLANT = PG.Params(SEED, 13, 64, 1 << 20)                          # min_size 64: a stone that ends at byte 1 025 is still cut;
                                                                  # max_size 1 MiB: no forced cut gets in front of a stone


@pytest.fixture(scope="module")
def engines():
    import makisu_amd
    made = {}

    def get(**over):
        key = tuple(sorted(over.items()))
        if key not in made:
            made[key] = makisu_amd.Engine(**over)
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _check(oracle, eng, blobs):
    """Every row of the batch against the oracle's."""
    with eng.batch(len(blobs), sum(len(b) for b in blobs)) as b:
        for i, blob in enumerate(blobs):
            b.add_bytes(blob, tag=i)
        b.run()
        files, chunks = b.files().copy(), b.chunks().copy()
    sizes = np.array([len(x) for x in blobs], dtype=np.uint64)
    data = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    c = eng.cfg
    rf, rc = oracle.scan_batch(data if data.size else np.zeros(1, np.uint8), offs, sizes,
                               oracle.CdcParams(c.gear_seed, c.mask_bits, c.min_size, c.max_size), True, 8)
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


# ---- sizes around every boundary the scheme adds ----------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [dict(), dict(mask_bits=10, min_size=64)], ids=["default", "mask10-min64"])
def test_sizes_around_heads_runs_and_tiles(oracle, engines, cfg):
    """Every size once, each file of content of its own; at mask 10 (the smallest mask the bitmap-free small-file kernel
    takes) and min_size 64 a file of a few hundred bytes already has cuts, and most heads hold a candidate somewhere."""
    sizes = SMALL + LARGE
    _check(oracle, engines(**cfg), [oracle.synth_fill(SEED, 300 + i, 0, n).tobytes() for i, n in enumerate(sizes)])


def test_sizes_in_every_wave_of_a_workgroup(oracle, engines):
    """The small sizes again, each in each of the eight wave positions of a workgroup, prefixes of shared content."""
    content = [oracle.synth_fill(SEED, 400 + k, 0, T).tobytes() for k in range(5)]
    sizes = [SMALL[(i // 8 + i % 8) % len(SMALL)] for i in range(8 * len(SMALL))]
    _check(oracle, engines(mask_bits=10, min_size=64), [content[i % 5][:n] for i, n in enumerate(sizes)])


# ---- planted candidates: the positions whose hash now comes from the neighbour's state ----------------------------------

def _planted(tile, lanes, n_tiles):
    """One file per (lane, offset): its only candidate is a stone whose last byte is run offset `o` of lane `l` of tile
    `tile` -- offsets 0..62 have their window in two lanes, 63 is the head's last position, 64 the body's first."""
    blobs, ends = [], []
    for l in lanes:
        for o in OFFSETS:
            e = tile * T + l * RUN + o + 1                        # cut END offset
            size = n_tiles * T - (7 * len(blobs)) % 50            # the files differ in their last run
            blobs.append(PG.plant(size, [e], params=PLANT, seed=len(blobs)))
            ends.append(e)
    return blobs, ends


@pytest.mark.parametrize("tile,lanes,n_tiles", [(0, (1, 31, 32, 63), 1), (1, (0, 1, 31, 32, 63), 2), (4, (0, 1, 63), 5)],
                         ids=["small-file", "second-tile", "second-group"])
def test_planted_stone_at_a_run_start(oracle, engines, tile, lanes, n_tiles):
    blobs, ends = _planted(tile, lanes, n_tiles)
    eng = engines(mask_bits=PLANT.mask_bits, min_size=PLANT.min_size, max_size=PLANT.max_size)
    files, chunks = _check(oracle, eng, blobs)
    for f, (blob, e) in enumerate(zip(blobs, ends)):
        mine = chunks[chunks["file_index"] == f]
        got = (mine["offset"] + mine["length"]).tolist()
        assert got == PG.select([e], len(blob), PLANT.min_size, PLANT.max_size) and e in got, (f, e, got)


# ---- random data at small masks: several head candidates per run, full lists, overflowing lanes ------------------------

def _quiet_fill(oracle, mask_bits):
    """A byte that makes no candidate by itself at this mask: a tile of it is a tile with an empty list."""
    table = oracle.gear_table(SEED)
    return next(b for b in range(0x5A, 0x5A + 256) if PG._fill_ok(table, mask_bits, b & 255)) & 255


def _tail_tiles(oracle, mask_bits, want, n=1, need_heads=0):
    """n files `one quiet tile + a random tail`: tile 1 has exactly `want` candidates, none of its runs more than six when
    want <= 64 (so its group is listed, not dense), at least need_heads of them in the heads of lanes > 0.  The tail is a
    multiple of a piece, so no lane hashes slack and the count is the kernel's.  -> [(bytes, candidates of tile 1)]"""
    fill = _quiet_fill(oracle, mask_bits)
    out = []
    for k in range(400):
        buf = np.concatenate([np.full(T, fill, np.uint8), oracle.synth_fill(SEED, 900 + 16 * mask_bits + k, 0, T // 2)])
        idx = oracle.gear_candidates(buf, SEED, mask_bits).astype(np.int64) - 1     # byte index of each candidate
        assert not (idx < T - 1).any()
        idx = idx[idx >= T] - T                                   # tile-relative
        for tail in range(128, T // 2 + 1, 128):
            c = idx[idx < tail]
            if c.size > want:
                break
            if c.size != want or (want <= 64 and np.bincount(c // RUN).max() > PG.PACK):
                continue
            if np.count_nonzero((c % RUN < W) & (c >= RUN)) < need_heads:
                continue
            out.append((buf[:T + tail].tobytes(), c))
            break
        if len(out) == n:
            return out
    raise AssertionError("no such tail among 400 draws")


@pytest.mark.parametrize("mask_bits,want", [(8, 64), (8, 65), (7, 65), (6, 65)])
def test_tile_list_exactly_full_and_one_over(oracle, engines, mask_bits, want):
    """64 entries (mask 8, where 64 candidates can still come six to a run at the most): the list path with its last slot
    taken; 65: the tile is dense and its group goes to the per-file pass."""
    (blob, c), = _tail_tiles(oracle, mask_bits, want)
    assert c.size == want and (want > 64 or np.bincount(c // RUN).max() <= PG.PACK)
    _check(oracle, engines(mask_bits=mask_bits, min_size=64), [blob])


def test_listed_tiles_with_head_candidates(oracle, engines):
    """Listed tiles (no run over six) whose heads hold at least three candidates: head entries go in front of the body's."""
    got = [b for want in (24, 33, 40, 47) for b, _ in _tail_tiles(oracle, 8, want, n=2, need_heads=3)]
    _check(oracle, engines(mask_bits=8, min_size=64), got)


@pytest.mark.parametrize("mask_bits", [6, 7, 8])
def test_overflowing_lanes_leave_through_the_dense_path(oracle, engines, mask_bits):
    """Random tiles at 4 to 16 expected candidates per run: lanes overflow their packs (mask 8: some by head and body
    together), every tile is dense, and the bitmap kernels' rows are the oracle's."""
    blobs = [oracle.synth_fill(SEED, 500 + 8 * mask_bits + i, 0, n).tobytes() for i, n in enumerate([T + 1, 3 * T + 70])]
    _check(oracle, engines(mask_bits=mask_bits, min_size=64), blobs)
