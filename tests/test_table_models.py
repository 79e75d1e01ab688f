"""tests/table_models.py pinned on hand-written cases: three to ten elements, one per branch, the expected values worked
out by hand and written down as literals.  tests/test_gpu_table_kernels.py compares the kernels of csrc/tables.hip with
this model and nothing else, so the model being right is what gives those tests their teeth; its roots are held against
the oracle's mi_ref_chunk_root and hashlib here."""
import hashlib

import numpy as np
import pytest

import table_models as M


def test_exclusive_scan():
    first, total = M.exclusive_scan([3, 0, 0, 2, 1])
    assert first.dtype == np.uint64 and first.tolist() == [0, 3, 3, 3, 5] and total == 6
    first, total = M.exclusive_scan([])
    assert first.tolist() == [] and total == 0
    first, total = M.exclusive_scan([0, 0, 0])
    assert first.tolist() == [0, 0, 0] and total == 0
    # totals beyond 32 bits: u32 counts, u64 sums
    first, total = M.exclusive_scan(np.array([0xFFFFFFFF, 1, 0xFFFFFFFF, 2], dtype=np.uint32))
    assert first.tolist() == [0, 0xFFFFFFFF, 0x100000000, 0x1FFFFFFFF] and total == 0x200000001


def test_chunk_rows_small_segments_with_empty_runs():
    # five small files = five segments; files 0, 2 and 4 are empty (front, middle, end)
    file_off = [1000, 1256, 2048, 2304, 9000]
    file_seg0 = [0, 1, 2, 3, 4, 5]
    seg_file = [0, 1, 2, 3, 4]
    seg_slot = [0, 4, 8, 12, 16]                              # slots need not be dense
    ends32 = np.full(20, 777, dtype=np.uint32)                # 777: never part of a list
    ends32[4:6] = [10, 25]
    ends32[12:15] = [7, 8, 100]
    t = M.chunk_rows(file_off, file_seg0, seg_file, seg_slot, ends32, seg_n=[0, 2, 0, 3, 0])
    assert t["chunk_file"].tolist() == [1, 1, 3, 3, 3]
    assert t["chunk_start"].tolist() == [0, 10, 0, 7, 8]
    assert t["chunk_len"].tolist() == [10, 15, 7, 1, 92]
    assert t["chunk_off"].tolist() == [1256, 1266, 2304, 2311, 2312]
    assert t["first"].tolist() == [0, 0, 2, 2, 5] and t["n_chunks"].tolist() == [0, 2, 0, 3, 0]
    off, ln = M.flat_root_items(t["first"], t["n_chunks"])
    assert off.tolist() == [0, 0, 64, 64, 160] and ln.tolist() == [0, 64, 0, 96, 0]


def _recs(rows):
    r = np.zeros(len(rows), dtype=M.GROUP_REC)
    for i, (entry, spec_n, pcnt, sidx) in enumerate(rows):
        r[i]["entry"], r[i]["spec_n"], r[i]["pcnt"], r[i]["sidx"] = entry, spec_n, pcnt, sidx
        r[i]["spec_exit"], r[i]["final_exit"], r[i]["flags"] = 0xDEAD, 0xBEEF, 2      # never read by the compaction
    return r


def test_chunk_rows_group_segments():
    # file 0 small (one chunk), file 1 large with four groups, file 2 small.  region = 4: a group owns 8 entries, the
    # speculative list in the first four, the prefix in the last four.
    G = M.GROUP_BYTES
    assert M.GROUP_REC.itemsize == 40
    file_off = [0, 256, 1 << 33]
    file_seg0 = [0, 1, 5, 6]
    seg_file = [0, 1, 1, 1, 1, 2]
    seg_group = [M.NO_GROUP, 0, 1, 2, 3, M.NO_GROUP]
    seg_slot = [0, 2, 10, 18, 26, 34]
    ends32 = np.full(40, 777, dtype=np.uint32)
    ends32[0] = 50                                                        # file 0: one chunk of 50 bytes
    # group 0: pcnt == 0, all speculation from sidx 0: cuts at 100 and 200000
    ends32[2:4] = [100, 200000]
    # group 1: a non-zero entry (the file's cut at 200000), both parts: prefix = [5000], spec[1:3] = [6000, G]; spec[0] is
    # a speculative cut the final list dropped
    ends32[10:13] = [4000, 6000, G]
    ends32[14] = 5000
    # group 2: no rows (one chunk runs through it): pcnt == 0 and sidx == spec_n
    ends32[18] = 123
    # group 3: sidx == spec_n, all prefix: entry is group 1's last cut, two groups back
    ends32[26:28] = [11, 22]
    ends32[30:32] = [64, 1000]
    ends32[34:36] = [1, 2]                                                # file 2: two one-byte chunks
    recs = _recs([(0, 2, 0, 0), (200000, 3, 1, 1), (2 * G, 1, 0, 1), (2 * G, 2, 2, 2)])
    seg_n = [1, 2, 3, 0, 2, 2]
    t = M.chunk_rows(file_off, file_seg0, seg_file, seg_slot, ends32, seg_n, seg_group, recs, region=4)
    assert t["chunk_file"].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 2, 2]
    assert t["chunk_start"].tolist() == [0, 0, 100, 200000, G + 5000, G + 6000, 2 * G, 3 * G + 64, 0, 1]
    assert t["chunk_len"].tolist() == [50, 100, 199900, G + 5000 - 200000, 1000, G - 6000, G + 64, 936, 1, 1]
    assert t["chunk_off"].tolist() == [0] + [256 + s for s in t["chunk_start"].tolist()[1:8]] + [1 << 33, (1 << 33) + 1]
    assert t["first"].tolist() == [0, 1, 8] and t["n_chunks"].tolist() == [1, 7, 2]
    with pytest.raises(AssertionError):                                   # a count that is not the final list's length
        M.chunk_rows(file_off, file_seg0, seg_file, seg_slot, ends32, [1, 2, 2, 0, 2, 2], seg_group, recs, region=4)


def test_sha_blocks_and_bins():
    # data + 0x80 + 8 bytes of length: 55 bytes still fit one block, 56 need two
    assert [M.sha_blocks(n) for n in (0, 1, 55, 56, 63, 64, 119, 120, 128)] == [1, 1, 1, 2, 2, 2, 2, 3, 3]
    # bin = blocks >> shift, the last bin takes everything above
    assert [M.length_bin(n, 4, 2) for n in (0, 183, 184, 695, 696, 1 << 20)] == [0, 0, 1, 2, 3, 3]
    assert M.length_bin(65463, 257, 2) == 255 and M.length_bin(65464, 257, 2) == 256 and M.length_bin(1 << 30, 257, 2) == 256
    assert M.length_bin(523703, 1024, 3) == 1022 and M.length_bin(523704, 1024, 3) == 1023
    assert M.length_bin(524288, 1024, 3) == 1023                          # 8193 blocks >> 3 = 1024: clamped
    lens = [0, 56, 184, 695, 696, 5000, 183]
    assert M.length_histogram(lens, 4, 2).tolist() == [3, 1, 1, 2]
    assert M.length_bins(lens, 4, 2).tolist() == [0, 0, 1, 2, 3, 3, 0]


def test_longest_first_property():
    lens = [0, 56, 184, 695, 696, 5000, 183]
    order = M.longest_first(lens, 4, 2)
    assert order.tolist() == [4, 5, 3, 2, 0, 1, 6]
    queue = [lens[i] for i in order]
    assert M.bins_never_increase(queue, 4, 2)
    assert not M.bins_never_increase(queue[::-1], 4, 2)                   # a sort that came out ascending is caught
    assert not M.bins_never_increase([696, 184, 695, 0], 4, 2)            # ... and one bin out of place
    assert M.bins_never_increase([5000, 696], 4, 2) and M.bins_never_increase([], 4, 2)


def test_root_level_by_hand():
    # five files with 0, 64 (carried: exactly the fan-out), 65 (two nodes, the last with one child), 3 and 130 chunks
    n_chunks = [0, 64, 65, 3, 130]
    first, total = M.exclusive_scan(n_chunks)
    cur = M.root_init(first, n_chunks)
    assert cur == [("digests", 0, 0), ("digests", 0, 64), ("digests", 64 * 32, 65), ("digests", 129 * 32, 3),
                   ("digests", 132 * 32, 130)]
    seg_cnt, seg_first, total, items, nxt = M.root_level(cur, "L0")
    assert seg_cnt == [0, 0, 2, 0, 3] and seg_first.tolist() == [0, 0, 0, 2, 2] and total == 5
    assert items == [("digests", 64 * 32, 2048), ("digests", 128 * 32, 32),
                     ("digests", 132 * 32, 2048), ("digests", 196 * 32, 2048), ("digests", 260 * 32, 64)]
    assert nxt == [("digests", 0, 0), ("digests", 0, 64), ("L0", 0, 2), ("digests", 129 * 32, 3), ("L0", 64, 3)]
    # a pass to which no file contributes: nothing moves
    seg_cnt, seg_first, total, items, nxt2 = M.root_level(nxt, "L1")
    assert seg_cnt == [0] * 5 and total == 0 and items == [] and nxt2 == nxt
    assert M.root_final_items(nxt) == [("digests", 0, 0), ("digests", 0, 2048), ("L0", 0, 64), ("digests", 129 * 32, 96),
                                       ("L0", 64, 96)]


def test_root_level_twice_for_4097():
    cur = [("digests", 0, 4097), ("digests", 4097 * 32, 4096)]
    _, _, total, items, nxt = M.root_level(cur, "L0")
    assert total == 65 + 64 and nxt == [("L0", 0, 65), ("L0", 65 * 32, 64)]
    assert items[64] == ("digests", 4096 * 32, 32) and items[65] == ("digests", 4097 * 32, 2048)
    seg_cnt, _, total, items, nxt = M.root_level(nxt, "L1")
    assert seg_cnt == [2, 0] and total == 2 and items == [("L0", 0, 2048), ("L0", 2048, 32)]
    assert nxt == [("L1", 0, 2), ("L0", 65 * 32, 64)]


@pytest.mark.parametrize("hash_fn", [hashlib.sha256, hashlib.blake2s])
def test_tree_roots_against_the_oracle_and_hashlib(oracle, hash_fn):
    counts = [0, 1, 63, 64, 65, 4096, 4097]
    rng = np.random.default_rng(11)
    digests = rng.integers(0, 256, (sum(counts), 32), dtype=np.uint8)
    roots, levels = M.tree_roots(digests, counts, hash_fn)
    assert levels == 2                                                    # 4097 -> 65 -> 2
    at = 0
    for n, root in zip(counts, roots):
        d = digests[at: at + n]
        at += n
        nodes = [d[i].tobytes() for i in range(n)]
        while len(nodes) > 64:
            nodes = [hash_fn(b"".join(nodes[i:i + 64])).digest() for i in range(0, len(nodes), 64)]
        assert root == hash_fn(b"".join(nodes)).digest(), n
        if hash_fn is hashlib.sha256:
            assert root == oracle.chunk_root(d), n
    assert roots[0] == hash_fn(b"").digest()
