"""GPU tests of mi_batch_pack_chunks (mi_pack.hip) and mi_batch_zpack_chunks (mi_zbatch.hip) beyond the plan's first round: a run
batch of 526 413 chunks -- 33.7 MB in 1 252 files cut at 64 bytes, 1 251 of them ending in a shorter tail
(store_rows_cases.batch_files, whose conditions tests/test_host_chunk_store_rows.py proves without a GPU) -- so that
plan_block_offsets carries the first round's rows and bytes into a second round with a partial last block, and batches of exactly
524 288 and 524 289 chunks: no second round, and one of one block holding one row.

Every row is compared with the plain models, bit for bit: a random chunk's stored form is PROVEN raw (no 4-byte value occurs
twice in it) or comes from zpack_cases.compress_chunk (level 2: zpack2_cases.compress_chunk2); there are no tolerances."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import store_rows_cases as sr  # noqa: E402

pytestmark = pytest.mark.gpu

PLAIN = ("digest", "offset", "chunk_index", "length", "reserved")
CODED = ("digest", "offset", "chunk_index", "length", "stored")


def _same(got, want, fields):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]), np.asarray(want[f])) for f in fields)


def _bad_rows(got, want, fields):
    if len(got) != len(want):
        return "%d entries, the model has %d" % (len(got), len(want))
    bad = np.zeros(len(got), dtype=bool)
    for f in fields:
        d = np.asarray(got[f]) != np.asarray(want[f])
        bad |= d.any(axis=1) if d.ndim > 1 else d
    return [(int(k), int(got["chunk_index"][k]), int(got["offset"][k]), int(want["offset"][k])) for k in np.flatnonzero(bad)[:8]]


def _first_difference(got, want):
    if len(got) != len(want):
        return "lengths %d and %d" % (len(got), len(want))
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    return int(np.flatnonzero(a != b)[0]) if (a != b).any() else None


class _Run:
    """one engine and one batch of the files, run, for the tests of a module"""

    def __init__(self, files):
        self.files = files
        self.engine = M.Engine(mask_bits=0, min_size=64, max_size=64)
        self.batch = self.engine.batch()
        t = time.time()
        for i, x in enumerate(files.files):
            self.batch.add_bytes(x, i)
        self.batch.run()
        print("a batch of %d chunks in %d files: %.1f s" % (files.n, len(files.files), time.time() - t))

    def close(self):
        self.batch.free()
        self.engine.close()


@pytest.fixture(scope="module")
def run():
    r = _Run(sr.batch_files())
    yield r
    r.close()
    sr.clear_caches()


def _pack_is_the_model(b, files, select):
    want_e, want_b = sr.model_batch_pack(files, select)
    with b.pack(select, verify=True) as p:
        got_e, got_b, info = p.entries().copy(), p.bytes(), p.info
    assert _same(got_e, want_e, PLAIN), _bad_rows(got_e, want_e, PLAIN)
    assert got_b == want_b, _first_difference(got_b, want_b)
    assert (info.n_entries, info.blob_bytes, info.chunk_bytes, info.verified) == (len(want_e), len(want_b), int(want_e["length"].sum()), 1)


def _zpack_is_the_model(b, files, select):
    want_e, want_b = sr.model_batch_zpack(files, select)
    with b.zpack(select, verify=True) as z:
        got_e, got_b, info = z.entries().copy(), z.read(), z.info
    assert _same(got_e, want_e, CODED), _bad_rows(got_e, want_e, CODED)
    assert got_b == want_b, _first_difference(got_b, want_b)
    assert (info.n_entries, info.blob_bytes, info.stored_bytes, info.n_raw, info.verified) == \
        (len(want_e), len(want_b), int(want_e["stored"].sum()), int((want_e["stored"] == want_e["length"]).sum()), 1)
    return got_e, got_b


def test_the_batch_has_the_rows_a_cut_at_64_gives(run):
    f = run.files
    chunks = run.batch.chunks()
    assert len(chunks) == f.n == sr.BATCH_CHUNKS
    assert np.array_equal(chunks["file_index"], f.file) and np.array_equal(chunks["offset"], f.offset) and np.array_equal(chunks["length"], f.length)
    assert np.array_equal(np.asarray(chunks["sha256"]), sr.batch_digests())


@pytest.mark.parametrize("name", sorted(sr.selections(1)))
def test_a_selection_is_packed_to_the_plain_model(run, name):
    """mi_batch_pack_chunks with VERIFY: rows and bytes carried into the second round; a selection that begins there, one that
    ends in front of it, and half of everything"""
    _pack_is_the_model(run.batch, run.files, sr.selections(run.files.n)[name])


def test_the_batch_is_coded_to_the_level_1_model_every_row_compared(run):
    """mi_batch_zpack_chunks with VERIFY against the model, and against pack().compress() in the same process"""
    b = run.batch
    got_e, got_b = _zpack_is_the_model(b, run.files, None)
    assert M.zpack_check(got_b, got_e) is None
    with b.pack() as p, p.compress(level=1) as z:
        assert _same(z.entries(), got_e, CODED) and z.read() == got_b


def test_half_of_the_batch_is_coded_to_the_level_1_model(run):
    _zpack_is_the_model(run.batch, run.files, sr.selections(run.files.n)["half"])


def test_the_batch_coded_at_level_2_is_the_packs_level_2_zpack(run):
    b = run.batch
    with b.zpack_at(2, verify=True) as z:
        got_e, got_b = z.entries().copy(), z.read()
    assert M.zpack_check(got_b, got_e) is None
    with b.pack() as p, p.compress(level=2) as old:
        want_e, want_b = old.entries().copy(), old.read()
    assert _same(got_e, want_e, CODED), _bad_rows(got_e, want_e, CODED)
    assert got_b == want_b, _first_difference(got_b, want_b)
    model_e, model_b = sr.model_batch_zpack(run.files, None, 2)      # ... and the level-2 model, every row compared
    assert _same(got_e, model_e, CODED), _bad_rows(got_e, model_e, CODED)
    assert got_b == model_b, _first_difference(got_b, model_b)


@pytest.mark.parametrize("n", sr.BATCH_SIZES[1:])
def test_batches_on_and_one_beyond_the_first_round(n):
    """524 288 chunks: the plan's one round is full; 524 289: a second round of one block that holds one row"""
    r = _Run(sr.batch_files(n))
    try:
        assert len(r.batch.chunks()) == n
        _pack_is_the_model(r.batch, r.files, None)
        _zpack_is_the_model(r.batch, r.files, None)
    finally:
        r.close()
        sr.clear_caches()
