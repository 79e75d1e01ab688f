"""GPU parity for the Gear kernels on PLANTED candidates (tests/planted_gear.py): every row of the scenario table puts
its candidates exactly where one rare branch of gear_cdc.hip needs them -- a lane's pack overflowing, a tile list
exactly full, a validation that meets the speculation at entry 63, 64 or 65 or never, a repair that cascades over a
chosen number of groups, a candidate exactly at min_size or max_size from the previous cut.  That a row forces its
branch is asserted on the CPU (tests/test_planted_gear_model.py); here the engine's rows for it have to be the oracle's,
column for column, and its chunk ends the plain-Python selection's.  The planted file sits between two ordinary random
files, so that an overrun of its slots or regions shows in a neighbour's rows.
Cut points: parity UNPINNED w.r.t. the reference (it has no CDC); the oracle is this repo's spec.
"""
import numpy as np
import pytest

try:
    import torch  # noqa: F401  (must come before the engine: see test_gpu_parity.py)
except ImportError:
    torch = None

import planted_gear as P

pytestmark = pytest.mark.gpu

BATCH = [n for n, s in P.SCENARIOS.items() if s.parts is None]
PARTS = [n for n, s in P.SCENARIOS.items() if s.parts is not None]


def _params(oracle, p):
    return oracle.CdcParams(p.seed, p.mask_bits, p.min_size, p.max_size)


@pytest.fixture(scope="module")
def engines():
    """One engine per parameter set of the table: the default one, and max_size 1 MiB."""
    import makisu_amd
    made = {}

    def get(p):
        if p not in made:
            over = {} if p == P.DEFAULT else dict(mask_bits=p.mask_bits, min_size=p.min_size, max_size=p.max_size)
            made[p] = makisu_amd.Engine(**over)
            c = made[p].cfg
            assert (c.gear_seed, c.mask_bits, c.min_size, c.max_size) == tuple(p)
        return made[p]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def neighbours(oracle):
    """The ordinary files around the planted one: a small one in front, a large one behind."""
    return (oracle.synth_fill(P.SEED, 7001, 0, 50001).tobytes(), oracle.synth_fill(P.SEED, 7002, 0, P.G + 70003).tobytes())


def _check_batch(oracle, eng, blobs, p):
    """Every column test_gpu_parity._check_batch asserts, against oracle.scan_batch."""
    with eng.batch(len(blobs), sum(len(b) for b in blobs)) as b:
        for i, blob in enumerate(blobs):
            b.add_bytes(blob, tag=1000 + i)
        b.run()
        files, chunks = b.files().copy(), b.chunks().copy()
        back = b.read_back().copy()
    data = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    assert np.array_equal(back, data), "staged bytes differ from what was added"
    sizes = np.array([len(x) for x in blobs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    rf, rc = oracle.scan_batch(data, offs, sizes, _params(oracle, p), True, 8)
    assert len(chunks) == len(rc), (len(chunks), len(rc))
    assert np.array_equal(files["n_chunks"], rf["n_chunks"])
    assert np.array_equal(files["first_chunk"], rf["first_chunk"])
    assert np.array_equal(files["size"], sizes)
    assert np.array_equal(files["user_tag"], 1000 + np.arange(len(blobs)))
    assert np.array_equal(chunks["file_index"], rc["file_index"])
    assert np.array_equal(chunks["offset"], rc["offset"]), "cut points differ"
    assert np.array_equal(chunks["length"], rc["length"]), "cut points differ"
    assert np.array_equal(chunks["sha256"], rc["sha256"]), "chunk digests differ"
    assert np.array_equal(files["chunk_root"], rf["chunk_root"]), "file roots differ"
    assert np.array_equal(chunks["dup_of"], rc["dup_of"]), "dedup marking differs"
    return files, chunks


@pytest.mark.parametrize("name", BATCH)
def test_planted_scenario(oracle, engines, neighbours, name):
    b = P.built(name)
    p = b["sc"].params
    files, chunks = _check_batch(oracle, engines(p), [neighbours[0], b["data"], neighbours[1]], p)
    mine = chunks[chunks["file_index"] == 1]
    ends = (mine["offset"] + mine["length"]).tolist()
    assert ends == b["cuts"], "%s: chunk ends differ from the spec's selection" % b["sc"].says


@pytest.mark.parametrize("name", PARTS)
def test_planted_parts(oracle, engines, neighbours, tmp_path, name):
    """The file as parts, a batch each (tests/test_gpu_parts.py _check_parts), every part between two ordinary files: the
    parts' rows put end to end are the whole file's rows, every part enters at the last cut select() puts at or before
    its first byte, and the halos -- which speculate on the wrong phase or are dense -- needed more than one round."""
    from makisu_amd.distributed import resolve_parts_local
    b = P.built(name)
    p, n, bounds = b["sc"].params, b["size"], b["sc"].parts
    eng = engines(p)
    path = tmp_path / "planted.bin"
    path.write_bytes(b["data"])
    _, ref = oracle.scan_batch(np.frombuffer(b["data"], dtype=np.uint8), np.array([0], dtype=np.uint64),
                               np.array([n], dtype=np.uint64), _params(oracle, p), True, 8, 0)
    assert (ref["offset"] + ref["length"]).tolist() == b["cuts"]
    batches = []
    try:
        for lo, hi in bounds:
            bt = eng.batch()
            batches.append(bt)
            bt.add_bytes(neighbours[0])
            bt.add_path_part(str(path), lo, hi, file_size=n)
            bt.add_bytes(neighbours[1])
        rounds = resolve_parts_local([(bt, [(0, k)]) for k, bt in enumerate(batches)])
        rows = []
        for (lo, hi), bt in zip(bounds, batches):
            bt.run()
            ch, fl = bt.chunks().copy(), bt.files().copy()
            (st,) = bt.parts()
            assert st["file_index"] == 1 and (st["begin"], st["end"]) == (lo, hi)
            mine = ch[ch["file_index"] == 1]
            assert fl["n_chunks"][1] == len(mine) > 0
            ends = mine["offset"] + mine["length"]
            assert ends[0] > lo and ends[-1] <= hi
            assert st["entry"] == max([0] + [c for c in b["cuts"] if c <= lo]) == mine["offset"][0]
            assert st["exit"] == max(c for c in b["cuts"] if c <= hi) == ends[-1]
            rows.append(mine)
            for f, blob in ((0, neighbours[0]), (2, neighbours[1])):     # the neighbours' rows are their own
                _, want = oracle.scan_batch(np.frombuffer(blob, dtype=np.uint8), np.array([0], dtype=np.uint64),
                                            np.array([len(blob)], dtype=np.uint64), _params(oracle, p), True, 8, 0)
                got = ch[ch["file_index"] == f]
                assert np.array_equal(got["offset"], want["offset"]) and np.array_equal(got["sha256"], want["sha256"])
        got = np.concatenate(rows)
        assert len(got) == len(ref), (len(got), len(ref))
        assert np.array_equal(got["offset"], ref["offset"]), "cut points differ"
        assert np.array_equal(got["length"], ref["length"]), "cut points differ"
        assert np.array_equal(got["sha256"], ref["sha256"]), "chunk digests differ"
        assert rounds == P.part_rounds(b["ends"], n, bounds, p)[0] > 1
    finally:
        for bt in batches:
            bt.free()
