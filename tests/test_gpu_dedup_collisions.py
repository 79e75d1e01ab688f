"""The GPU digest tables on digests that collide in their keys.

Every table here keys its slots on a digest's first 8 bytes: the in-batch and job-wide marking (csrc/tables.hip:
dedup_insert_kernel, dedup_probe_kernel, dedup_finish_range_kernel) and the chunk index (csrc/mi_index.hip: the probe
and verify kernels, whose tag stores a zero key as 1).  SHA-256 outputs and uniform random rows never make two
different digests share those 8 bytes, so the code that runs only then -- the 32-byte compare after a key match, the
tag-then-digest compare of the probe, the index's verify and re-probe rounds -- is driven here by crafted rows:

  same key, different tail   one group per byte position p = 8..31, the rows differ only at byte p (single bits too)
  same slot, different key   equal low 32 bits of the key (so equal under any table mask), different high bits
  special values             all zero, all 0xFF, key 0 next to key 01 00 .. 00 (both index tag 1)
  a long cluster             hundreds of rows with one key whose slot is the table's last, so probing wraps to slot 0

shuffled together with random rows and exact repeats.  The reference is a plain dict from the 32 digest bytes to the
first row holding them; it shares nothing with the kernels' (or the oracle's) bucketing.
"""
import numpy as np
import pytest

try:
    import torch  # noqa: F401  (before the engine: its HIP runtime serves the library too; see test_gpu_parity.py)
except ImportError:          # CPU-only collection without torch: the GPU tests are skipped anyway
    torch = None

pytestmark = pytest.mark.gpu

SEED = 0x4D414B49


@pytest.fixture(scope="module")
def eng():
    import makisu_amd
    e = makisu_amd.Engine()
    yield e
    e.close()


def reference(rows):
    """(dup_of, n_unique): dup_of[i] = the first row holding row i's 32 bytes, -1 for that row itself."""
    first, dup = {}, np.empty(len(rows), dtype=np.int64)
    for i, r in enumerate(rows):
        j = first.setdefault(r.tobytes(), i)
        dup[i] = -1 if j == i else j
    return dup, len(first)


def keys(rows):
    """The tables' key: the first 8 digest bytes as a little-endian u64."""
    return np.ascontiguousarray(rows[:, :8]).view("<u8").ravel()


def as_set(rows):
    return {r.tobytes() for r in np.asarray(rows).reshape(-1, 32)}


def distinct(rows):
    """The distinct rows in first-occurrence order."""
    dup, _ = reference(rows)
    return rows[dup < 0]


def families(rng, cluster):
    """Crafted digests by family; every same-key group has at most `cluster` (<= 2 000) rows."""
    fam = {}
    groups = []
    for p in range(8, 32):                                   # same key, different tail
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        g = np.repeat(base[None], 12, axis=0)
        for b in range(8):
            g[1 + b, p] ^= np.uint8(1 << b)
        g[9:, p] = (int(base[p]) + np.array([17, 85, 128])) % 256
        groups.append(g)
    fam["same_key"] = np.concatenate(groups)
    base = rng.integers(0, 256, 32, dtype=np.uint8)          # same slot, different key: bytes 4..7 differ
    g = np.repeat(base[None], 48, axis=0)
    g[1:, 4:8] = rng.integers(0, 256, (47, 4), dtype=np.uint8)
    g[24:, 8:] = rng.integers(0, 256, (24, 24), dtype=np.uint8)
    fam["same_slot"] = g
    tail = rng.integers(0, 256, 24, dtype=np.uint8)
    sp = np.zeros((8, 32), dtype=np.uint8)
    sp[1] = 0xFF
    sp[2, 8:] = tail                                         # key 0 (index tag 1) ...
    sp[3, 0], sp[3, 8:] = 1, tail                            # ... next to key 1, same tail
    sp[4, 0] = 1                                             # differs from the all-zero digest in byte 0 only
    sp[5, :8] = 0xFF                                         # key all ones, tail zero
    sp[6, 8:] = 0xFF                                         # key zero, tail all ones
    sp[7, 0], sp[7, 8:] = 1, 0xFF
    fam["special"] = sp
    hi = rng.integers(0, 256, 4, dtype=np.uint8)             # a long cluster: key & mask = mask for every table size
    g = rng.integers(0, 256, (cluster, 32), dtype=np.uint8)
    g[:, :4], g[:, 4:8] = 0xFF, hi
    s = rng.integers(0, 256, (16, 32), dtype=np.uint8)       # ... and rows in the same slot with other keys
    s[:, :4] = 0xFF
    fam["cluster"] = np.concatenate([g, s])
    return fam


def mixed(rng, cluster, n_random, n_repeat):
    """All families, random rows and exact repeats of any of them, shuffled."""
    crafted = np.concatenate(list(families(rng, cluster).values()))
    base = np.concatenate([crafted, rng.integers(0, 256, (n_random, 32), dtype=np.uint8)])
    rows = np.concatenate([base, base[rng.integers(0, len(base), n_repeat)]])
    return np.ascontiguousarray(rows[rng.permutation(len(rows))])


def check_collides(rows):
    """The rows really exercise the paths under test: many distinct digests share a key with another one."""
    u = distinct(rows)
    k = keys(u)
    _, inv, cnt = np.unique(k, return_inverse=True, return_counts=True)
    assert (cnt[inv] > 1).sum() > 24 * 10, "too few distinct digests share a key"
    assert cnt.max() >= 200, "no long same-key cluster"
    assert as_set(np.zeros((1, 32), np.uint8)) <= as_set(u)


def diffs(got, want, rows, first=0):
    bad = np.nonzero(got != want)[0][:6]
    return "; ".join("row %d (%s): got %d, want %d" % (first + i, rows[first + i].tobytes().hex(), got[i], want[i])
                     for i in bad)


def flip(rows, p, bit):
    out = np.array(rows, dtype=np.uint8, copy=True)
    out[:, p] ^= np.uint8(bit)
    return out


def test_dedup_mark_on_colliding_keys(oracle, eng):
    """mi_dedup_mark: dup_of and n_unique equal the dict's, and the oracle's."""
    import torch
    rng = np.random.default_rng(101)
    rows = mixed(rng, cluster=1500, n_random=3000, n_repeat=2500)
    check_collides(rows)
    want, n_unique = reference(rows)
    o_dup, o_unique = oracle.dedup(rows)
    assert np.array_equal(o_dup, want) and o_unique == n_unique
    assert (want[-300:] < 0).any() and (want[:300] < 0).any() and (want[-300:] >= 0).any()   # firsts early and late
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(rows).to(dev)
    dup = torch.full((len(rows),), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    nu = eng.dedup_mark(d.data_ptr(), len(rows), dup.data_ptr())
    got = dup.cpu().numpy()
    assert np.array_equal(got, want), diffs(got, want, rows)
    assert nu == n_unique


def test_dedup_mark_range_on_colliding_keys(oracle, eng):
    """mi_dedup_mark_range for several rank splits of a job-wide set whose earlier ranks hold rows that match a later
    rank's in key (tail flipped at byte 8, 16 or 31; key 0 against key 1) but differ -- those rows stay first
    occurrences or point inside their own rank -- and exact copies, which win as the global minimum."""
    import torch
    rng = np.random.default_rng(202)
    own = mixed(rng, cluster=800, n_random=1500, n_repeat=1000)
    u = distinct(own)
    pick = u[rng.permutation(len(u))[:900]]
    near = [flip(pick[:300], 31, 0x01), flip(pick[300:600], 16, 0x80), flip(pick[600:], 8, 0x10)]
    k = keys(u)
    z, o = u[k == 0], u[k == 1]                               # index tag 1 both: swap the two keys, keep the tails
    alias = np.concatenate([flip(z, 0, 0x01), flip(o, 0, 0x01)])
    exact = u[rng.permutation(len(u))[:300]]
    foreign = np.concatenate(near + [alias, exact])
    foreign = foreign[rng.permutation(len(foreign))]
    later = np.concatenate([own[rng.integers(0, len(own), 400)], rng.integers(0, 256, (200, 32), dtype=np.uint8)])
    rows = np.ascontiguousarray(np.concatenate([foreign, own, later]))
    nf_, no = len(foreign), len(own)
    want, n_unique = reference(rows)
    assert np.array_equal(oracle.dedup(rows)[0], want)
    mine = want[nf_:nf_ + no]
    near_keys = set(keys(np.concatenate(near + [alias])).tolist())
    shared = np.array([kk in near_keys for kk in keys(own).tolist()])
    assert (shared & (mine < 0)).sum() > 500                  # own firsts that share a key with an earlier rank's row
    assert (mine >= 0).any() and (mine[mine >= 0] < nf_).sum() >= 300   # exact copies won
    dev = torch.device("cuda", 0)
    glob = torch.from_numpy(rows).to(dev)
    n = len(rows)
    for bounds in ([0, nf_, nf_ + no, n],
                   [0, nf_ // 2, nf_, nf_ + no // 3, nf_ + no, n],
                   [0, 0, nf_ + no // 2, nf_ + no // 2, n - 1, n]):
        firsts = 0
        for a, b in zip(bounds[:-1], bounds[1:]):
            dup = torch.full((max(b - a, 1),), -7, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            nf = eng.dedup_mark_range(glob.data_ptr(), n, a, b - a, dup.data_ptr())
            got = dup.cpu().numpy()[: b - a]
            assert np.array_equal(got, want[a:b]), (bounds, a, b, diffs(got, want[a:b], rows, a))
            assert nf == int((want[a:b] < 0).sum()), (bounds, a, b)
            firsts += nf
        assert firsts == n_unique


def _run_batch(e, rng, n_files=60):
    """A real batch with in-batch repeats; -> the batch (the caller frees it) and its digests."""
    sizes = [65536] * n_files + [300000, 5, 1 << 20, 4097]
    cids = list(range(500, 500 + n_files)) + [900, 901, 902, 903]
    for i in rng.permutation(n_files)[:10]:
        cids[i] = cids[(i + 7) % n_files]
    b = e.batch()
    b.add_synthetic(sizes, cids, seed=SEED)
    b.run()
    return b, b.chunks()["sha256"].copy()


def test_batch_mark_global_on_colliding_keys(eng):
    """mi_batch_mark_global on a real batch whose job-wide set is [crafted earlier-rank rows] + its own digests (copied
    from the device): the crafted rows are the batch's digests with byte 31 flipped, plus a few exact copies."""
    import torch
    from makisu_amd.distributed import digests_tensor
    rng = np.random.default_rng(303)
    dev = torch.device("cuda", 0)
    b, host = _run_batch(eng, rng)
    try:
        own = digests_tensor(b, dev).clone()
        torch.cuda.synchronize()
        assert np.array_equal(own.cpu().numpy(), host)
        crafted = np.concatenate([flip(host, 31, 0x01), host[rng.permutation(len(host))[:8]]])
        crafted = np.ascontiguousarray(crafted[rng.permutation(len(crafted))])
        glob = torch.cat([torch.from_numpy(crafted).to(dev), own])
        rows = np.concatenate([crafted, host])
        want, _ = reference(rows)
        mine = want[len(crafted):]
        assert (mine >= len(crafted)).any() and ((mine >= 0) & (mine < len(crafted))).sum() >= 8
        torch.cuda.synchronize()
        nf = b.mark_global(glob.data_ptr(), len(rows), len(crafted))
        got = b.chunks()["dup_of"].copy()
        assert np.array_equal(got, mine), diffs(got, mine, rows, len(crafted))
        assert nf == int((mine < 0).sum())
    finally:
        b.free()


def test_index_add_batch_against_tail_flipped_digests(eng):
    """An index holding the batch's digests with a flipped tail byte (31, 16 or 8) and exact copies of every other
    one: add_batch flags as known only the exact ones and the rows that repeat them, and counts the rest as new."""
    rng = np.random.default_rng(404)
    b, host = _run_batch(eng, rng)
    try:
        u = distinct(host)
        variants = np.concatenate([flip(u, 31, 0x01), flip(u[::3], 16, 0x80), flip(u[1::3], 8, 0x04)])
        exact = u[::2]
        blob = np.concatenate([variants, exact])
        blob = np.ascontiguousarray(blob[rng.permutation(len(blob))])
        held, exact_set = as_set(blob), as_set(exact)
        with eng.index() as idx:
            assert idx.load(blob.tobytes()) == len(held) == len(idx)
            known, n_new, n_known = idx.add_batch(b)
            want = np.array([r.tobytes() in exact_set for r in host], dtype=np.uint8)
            assert want.sum() < len(host) and (reference(host)[0][want == 1] >= 0).any()   # repeats of exact rows too
            assert np.array_equal(known, want), diffs(known, want, host)
            assert n_known == int(want.sum())
            assert n_new == len(as_set(u) - exact_set)
            assert len(idx) == len(held | as_set(u))
            out = idx.export()
            assert len(out) == 32 * len(idx) and as_set(np.frombuffer(out, np.uint8)) == held | as_set(u)
    finally:
        b.free()


def test_index_grows_while_holding_collisions(eng):
    """Colliding groups imported piecewise into the minimal index (1 024 slots): the table is rebuilt at twice the size
    while it holds same-key groups, both index-tag-1 keys and a cluster that wraps; the export is everything imported."""
    rng = np.random.default_rng(505)
    fam = families(rng, cluster=400)
    rows = distinct(np.concatenate(list(fam.values()) + [rng.integers(0, 256, (600, 32), dtype=np.uint8)]))
    rows = rows[rng.permutation(len(rows))]
    assert len(rows) > 1024                                   # the 1 024-slot table grows more than once
    held = set()
    with eng.index() as idx:
        for part in np.array_split(rows, 5):
            blob = np.concatenate([part, part[:7]])            # repeats inside a blob are fine
            assert idx.load(blob.tobytes()) == len(as_set(part) - held)
            held |= as_set(part)
            assert len(idx) == len(held)
        assert idx.load(rows[::5].tobytes()) == 0
        out = idx.export()
        assert len(out) == 32 * len(held) and as_set(np.frombuffer(out, np.uint8)) == held
    with eng.index() as idx2:
        assert idx2.load(out) == len(held)
        assert as_set(np.frombuffer(idx2.export(), np.uint8)) == held


def test_index_same_key_group_of_200(eng):
    """200 new digests sharing their first 8 bytes take 200 probe rounds; the import must converge, count them all and
    export them all -- also when the group then grows to 1 200 through the rebuilt table."""
    rng = np.random.default_rng(606)
    g = rng.integers(0, 256, (1200, 32), dtype=np.uint8)
    g[:, :8] = rng.integers(0, 256, 8, dtype=np.uint8)
    assert len(as_set(g)) == len(g)
    with eng.index() as idx:
        assert idx.load(g[:200].tobytes()) == 200
        assert len(idx) == 200
        assert as_set(np.frombuffer(idx.export(), np.uint8)) == as_set(g[:200])
        assert idx.load(g.tobytes()) == 1000
        assert len(idx) == 1200
        out = idx.export()
        assert len(out) == 32 * 1200 and as_set(np.frombuffer(out, np.uint8)) == as_set(g)
