"""Plain restatements of the chunk-table operations of csrc/tables.hip, for tests/test_gpu_table_kernels.py to hold the
kernels against and for tests/test_table_models.py to pin on hand-written cases.

Written from the contracts in csrc/mi_common.h and the comments above the kernels, not from the kernels' arithmetic: no tiles,
no binary searches, no LDS histograms, no atomics -- loops over segments and files, Python integers, numpy where a case has
millions of elements.

  exclusive_scan      first[i] = sum(counts[:i]), and the total
  chunk_rows          the chunk table from the segments' end lists (small files and 256 KiB groups), first row / row count per file
  flat_root_items     the root pass's strings when no file needs a reduction pass
  sha_blocks, length_bin, length_histogram
  bins_never_increase the one property the longest-first queue promises
  root_level          one reduction pass of the fan-out-64 root tree over (node list per file)
  root_final_items, tree_roots
"""
import hashlib

import numpy as np

FANOUT = 64                      # kChunkRootFanout
GROUP_BYTES = 4 * 65536          # kGroupBytes: one group segment of a large file
NO_GROUP = 0xFFFFFFFF            # seg_group of a small-file segment
# chunk counts at the root tree's edges, for the end-to-end runs with exactly N chunks per file (test_gpu_parity.py,
# test_gpu_blake2s.py): around the fan-out, around two of them, around 64^2 (and 65 nodes), around 64^3
ROOT_EDGE_CHUNKS = [62, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4160, 262144, 262145]
# GroupRec (csrc/mi_common.h): final list = prefix[0, pcnt) ++ spec[sidx, spec_n), the first start at `entry`
GROUP_REC = np.dtype([("spec_exit", "<u8"), ("final_exit", "<u8"), ("entry", "<u8"),
                      ("spec_n", "<u4"), ("pcnt", "<u4"), ("sidx", "<u4"), ("flags", "<u4")])


# ---- scan ------------------------------------------------------------------------------------------------------------
def exclusive_scan(counts):
    """(first, total): first[i] = counts[0] + .. + counts[i-1] as uint64, total = the sum as a Python integer."""
    c = np.asarray(counts, dtype=np.uint64)
    inc = np.cumsum(c, dtype=np.uint64)
    first = np.zeros(len(c), dtype=np.uint64)
    first[1:] = inc[:-1]
    return first, (int(inc[-1]) if len(c) else 0)


# ---- chunk rows ------------------------------------------------------------------------------------------------------
def segment_ends(s, seg_slot, ends32, seg_n, seg_group=None, recs=None, region=0):
    """(ends relative to the segment start, entry): the final end list of segment s.  A small-file segment holds one list
    of seg_n[s] ends at ends32[seg_slot[s] ..] and starts at 0.  A group segment owns 2 x region entries -- the speculative
    list, then the prefix -- and its final list is prefix[0, pcnt) ++ spec[sidx, spec_n), starting from rec.entry."""
    slot = int(seg_slot[s])
    if seg_group is None or int(seg_group[s]) == NO_GROUP:
        return [int(e) for e in ends32[slot: slot + int(seg_n[s])]], None
    r = recs[int(seg_group[s])]
    spec = ends32[slot: slot + region]
    prefix = ends32[slot + region: slot + 2 * region]
    final = [int(e) for e in prefix[: int(r["pcnt"])]] + [int(e) for e in spec[int(r["sidx"]): int(r["spec_n"])]]
    assert len(final) == int(seg_n[s]), "a group segment's count is the length of its final list"
    return final, int(r["entry"])


def chunk_rows(file_off, file_seg0, seg_file, seg_slot, ends32, seg_n, seg_group=None, recs=None, region=0):
    """The chunk table: rows in segment order, a segment's rows in list order.  A row is (chunk_off = absolute arena
    offset, chunk_len, chunk_file, chunk_start = offset inside the file); a group segment's ends are relative to
    (s - file_seg0[f]) * GROUP_BYTES and its first row starts at the group's `entry` (file-relative), every other row at
    the end before it.  Also first[f] / n_chunks[f]: file f's rows are those of segments file_seg0[f] .. file_seg0[f+1]."""
    off, ln, fi, st = [], [], [], []
    rows_of_seg = []
    for s in range(len(seg_file)):
        f = int(seg_file[s])
        ends, entry = segment_ends(s, seg_slot, ends32, seg_n, seg_group, recs, region)
        if entry is None:
            base, start = 0, 0
        else:
            base, start = (s - int(file_seg0[f])) * GROUP_BYTES, entry
        for e in ends:
            end = base + e
            off.append(int(file_off[f]) + start)
            ln.append(end - start)
            fi.append(f)
            st.append(start)
            start = end
        rows_of_seg.append(len(ends))
    n_files = len(file_seg0) - 1
    first, n_chunks, at = [], [], 0
    seg = 0
    for f in range(n_files):
        assert int(file_seg0[f]) == seg
        n = sum(rows_of_seg[int(file_seg0[f]): int(file_seg0[f + 1])])
        first.append(at)
        n_chunks.append(n)
        at += n
        seg = int(file_seg0[f + 1])
    return {"chunk_off": np.array(off, dtype=np.uint64), "chunk_len": np.array(ln, dtype=np.uint64),
            "chunk_file": np.array(fi, dtype=np.uint32), "chunk_start": np.array(st, dtype=np.uint64),
            "first": np.array(first, dtype=np.uint64), "n_chunks": np.array(n_chunks, dtype=np.uint32)}


def flat_root_items(first, n_chunks):
    """(offset into the digest table, length) in bytes per file: file f's root string is its digest run."""
    return (np.asarray(first, dtype=np.uint64) * np.uint64(32), np.asarray(n_chunks, dtype=np.uint64) * np.uint64(32))


# ---- length bins -----------------------------------------------------------------------------------------------------
def sha_blocks(length):
    """64-byte compressions SHA-256 needs for `length` bytes: the data, one 0x80 byte and the 8-byte bit count."""
    length = int(length)
    return length // 64 + 1 + (1 if length % 64 > 55 else 0)


def length_bin(length, n_bins, bin_shift):
    return min(sha_blocks(length) >> bin_shift, n_bins - 1)


def length_bins(lens, n_bins, bin_shift):
    return np.array([length_bin(x, n_bins, bin_shift) for x in lens], dtype=np.int64)


def length_histogram(lens, n_bins, bin_shift):
    h = np.zeros(n_bins, dtype=np.uint32)
    for x in lens:
        h[length_bin(x, n_bins, bin_shift)] += 1
    return h


def bins_never_increase(queue_lens, n_bins, bin_shift):
    """The hashing queue is consumed in order and wants the longest strings first: the bin never increases along it.
    (The order inside a bin is not specified.)"""
    b = length_bins(queue_lens, n_bins, bin_shift)
    return bool((b[1:] <= b[:-1]).all())


def longest_first(lens, n_bins, bin_shift):
    """One valid queue: row indices by descending bin (stable, so row order inside a bin)."""
    b = length_bins(lens, n_bins, bin_shift)
    return np.argsort(-b, kind="stable")


# ---- root tree -------------------------------------------------------------------------------------------------------
# A file's node list is (buffer, byte offset inside it, digest count): `buffer` names where the 32-byte nodes lie -- the
# chunk digest table at first, the output of a reduction pass afterwards.
def root_init(first, n_chunks, buffer="digests"):
    return [(buffer, int(a) * 32, int(n)) for a, n in zip(first, n_chunks)]


def root_level(cur, out_buffer):
    """One reduction pass.  A file with more than FANOUT nodes contributes ceil(cnt / FANOUT) new nodes, each the hash of
    a run of FANOUT children (the last run: what is left, at least one); its new nodes are consecutive in `out_buffer`,
    files in file order.  A file with FANOUT nodes or fewer contributes nothing and keeps its list.
    Returns (seg_cnt, seg_first, total, items, nxt): items[g] = (buffer, byte offset, byte length) of new node g's string,
    whose digest goes to out_buffer[32 * g]."""
    seg_cnt = [(-(-c // FANOUT) if c > FANOUT else 0) for _, _, c in cur]
    seg_first, total = exclusive_scan(seg_cnt)
    items, nxt = [], []
    for (buf, off, cnt), n_nodes, f0 in zip(cur, seg_cnt, seg_first):
        if n_nodes == 0:
            nxt.append((buf, off, cnt))
            continue
        for j in range(n_nodes):
            children = min(FANOUT, cnt - j * FANOUT)
            items.append((buf, off + j * FANOUT * 32, children * 32))
        nxt.append((out_buffer, int(f0) * 32, n_nodes))
    assert len(items) == total
    return seg_cnt, seg_first, total, items, nxt


def root_final_items(cur):
    """The final pass's strings: every file's whole node list (at most FANOUT nodes once the passes are done)."""
    return [(buf, off, cnt * 32) for buf, off, cnt in cur]


def tree_roots(digests, n_chunks, hash_fn=hashlib.sha256):
    """Every file's chunk root, by running the passes above over real bytes: reduction passes until none contributes,
    then the final one."""
    digests = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    first, total = exclusive_scan(n_chunks)
    assert total == len(digests)
    buffers = {"digests": digests.tobytes()}
    cur = root_init(first, n_chunks)
    level = 0
    while True:
        name = "level%d" % level
        _, _, total, items, nxt = root_level(cur, name)
        if total == 0:
            assert nxt == cur
            break
        buffers[name] = b"".join(hash_fn(buffers[b][o: o + n]).digest() for b, o, n in items)
        cur, level = nxt, level + 1
    assert all(c <= FANOUT for _, _, c in cur)
    return [hash_fn(buffers[b][o: o + n]).digest() for b, o, n in root_final_items(cur)], level
