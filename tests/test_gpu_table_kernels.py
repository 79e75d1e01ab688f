"""The small kernels of csrc/tables.hip driven ALONE, on arrays made for the purpose, against tests/table_models.py.

End to end (mi_batch_run) these kernels only ever see what the Gear pass makes of a real batch, and one of them -- the
longest-first order -- leaves no trace in any result.  Here each launcher is called through tests/kernel_probe (host-only
wrappers over the library's own exported launchers, nothing added to the product) on inputs that walk its edges on purpose:

  scan         every tile residue, the two-launch form up to 4096 tiles and the three-launch form beyond it (scan_block_offsets_kernel
               + scan_final_kernel, which no batch of the suite is large enough to reach), whole tiles of zeros, sums beyond 32 bits
  compaction   runs of empty segments at the front, behind the last row and across a scan tile; 255 / 256 / 257 files; a grid-stride
               second trip; group segments that are all prefix, all speculation, both, empty, entered from a cut groups back; lengths
               on both sides of a SHA-256 block count and of the clamp bin
  order        s_id a permutation, descriptors those of their rows, the bin never increasing along the queue (four 256-bin
               rounds at 1024 bins), the cursor the histogram
  root levels  files of exactly the fan-out (carried), one more (a last node with one child), a pass nobody contributes to,
               a second pass over the first one's output, the final strings

Every comparison is exact.  Every output buffer is pre-filled with a sentinel and has 64 sentinel elements behind it; rows at
and beyond the real count must come back untouched.  The model is pinned by hand-written cases in tests/test_table_models.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (before the engine: its HIP runtime serves the library and the probe too; see test_gpu_parity.py)
except ImportError:          # CPU-only collection without torch: the GPU tests are skipped anyway
    torch = None

import table_models as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIR = os.path.join(ROOT, "tests", "kernel_probe")
PROBE = os.path.join(PROBE_DIR, "libmi_tables_probe.so")
GUARD = 64                       # sentinel elements behind every output buffer
FILL = 0xA5                      # the sentinel, byte by byte
TILE = 2048                      # counts per scan tile
G = M.GROUP_BYTES
JUNK = 0xDDDDDDDD                # in end-list entries no final list holds: a row made from one would be far off


def build_probe():
    src = os.path.join(PROBE_DIR, "tables_probe.cpp")
    lib = os.path.join(ROOT, "makisu_amd", "libmakisu_mi.so")
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall",
                               src, "-o", PROBE, "-L", os.path.dirname(lib), "-lmakisu_mi",
                               "-Wl,-rpath,$ORIGIN/../../makisu_amd", "-Wl,--no-undefined"])
    return PROBE


def sentinel(dtype):
    return np.frombuffer(bytes([FILL]) * np.dtype(dtype).itemsize, dtype=dtype)[0]


class In:
    """A host array on the device (with a guard behind it, so that an empty array still has an address)."""
    def __init__(self, a):
        a = np.ascontiguousarray(a)
        raw = np.concatenate([a.view(np.uint8).reshape(-1), np.full(GUARD, FILL, np.uint8)])
        self.t = torch.from_numpy(raw).cuda()
        self.ptr = self.t.data_ptr()


class Out:
    """n elements + GUARD more, every byte the sentinel."""
    def __init__(self, n, dtype):
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.t = torch.full(((self.n + GUARD) * self.dtype.itemsize,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy().view(self.dtype)


class Tables:
    """The probe: numpy in, numpy out (outputs WITH their guards: the caller checks them)."""
    def __init__(self, path):
        lib = C.CDLL(path)
        P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
        lib.probe_scan_scratch_elems.restype, lib.probe_scan_scratch_elems.argtypes = U64, [U64]
        lib.probe_group_rec_bytes.restype, lib.probe_group_rec_bytes.argtypes = U64, []
        for name, args in (("probe_scan_counts", [P, P, P, U64, P]),
                           ("probe_compact_chunks", [P] * 8 + [U32, U64, U64, U64] + [P] * 8 + [U32, U32] + [P] * 3),
                           ("probe_bin_order", [P, P, U32, P, P, P, U32, U32, P, P, P]),
                           ("probe_root_init", [P, P, P, U64, P, P]),
                           ("probe_root_level", [U64, U64] + [P] * 11),
                           ("probe_root_final_items", [P, P, U64, P, P])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = C.c_int, args
        self.lib = lib
        assert lib.probe_group_rec_bytes() == M.GROUP_REC.itemsize

    def _call(self, name, *args):
        torch.cuda.synchronize()
        rc = getattr(self.lib, name)(*args)
        assert rc == 0, "%s: HIP status %d" % (name, rc)

    def scratch_elems(self, n):
        return int(self.lib.probe_scan_scratch_elems(n))

    def scan(self, counts):
        n = len(counts)
        d_counts = In(np.asarray(counts, dtype=np.uint32))
        first, total, scratch = Out(n, np.uint64), Out(1, np.uint64), Out(self.scratch_elems(n), np.uint64)
        self._call("probe_scan_counts", d_counts.ptr, first.ptr, total.ptr, n, scratch.ptr)
        return {"first": first.get(), "total": total.get(), "scratch_guard": scratch.get()[scratch.n:]}

    def compact(self, t, seg_first, total, n_max, n_bins, bin_shift, want_items):
        nf, ns = len(t["file_off"]), len(t["seg_file"])
        has_groups = t["recs"] is not None
        ins = [In(t["file_off"]), In(t["file_seg0"]), In(t["seg_file"]), In(t["seg_slot"]), In(t["ends32"]),
               In(np.asarray(seg_first, dtype=np.uint64))]
        d_group = In(t["seg_group"]) if has_groups else None
        d_recs = In(t["recs"]) if has_groups else None
        d_n = In(np.array([total], dtype=np.uint64))
        out = {"chunk_off": Out(n_max, np.uint64), "chunk_len": Out(n_max, np.uint64), "chunk_file": Out(n_max, np.uint32),
               "chunk_start": Out(n_max, np.uint64), "first": Out(nf, np.uint64), "n_chunks": Out(nf, np.uint32),
               "item_off": Out(nf, np.uint64), "item_len": Out(nf, np.uint64)}
        hist = Out(n_bins, np.uint32)
        hist.t[: n_bins * 4] = 0                                   # zeroed by the caller, the guard stays
        digests = Out(0, np.uint8)                                 # an address; the compaction never reads digests
        self._call("probe_compact_chunks", *[i.ptr for i in ins], d_group.ptr if has_groups else None,
                   d_recs.ptr if has_groups else None, t["region"], nf, ns, n_max, d_n.ptr,
                   out["chunk_off"].ptr, out["chunk_len"].ptr, out["chunk_file"].ptr, out["chunk_start"].ptr,
                   out["first"].ptr, out["n_chunks"].ptr, hist.ptr, n_bins, bin_shift, digests.ptr,
                   out["item_off"].ptr if want_items else None, out["item_len"].ptr if want_items else None)
        got = {k: v.get() for k, v in out.items()}
        got["hist"] = hist.get()
        got["digests_base"] = digests.ptr
        return got

    def order(self, off, lens, n_real, hist, n_bins, bin_shift):
        """n_real None: no device count, all n rows are real"""
        n = len(lens)
        d_off, d_len = In(np.asarray(off, dtype=np.uint64)), In(np.asarray(lens, dtype=np.uint64))
        d_n = In(np.array([n_real], dtype=np.uint64)) if n_real is not None else None
        d_hist = In(np.asarray(hist, dtype=np.uint32))
        cursor = Out(n_bins, np.uint32)
        cursor.t[: n_bins * 4] = 0
        s_off, s_len, s_id = Out(n, np.uint64), Out(n, np.uint64), Out(n, np.uint32)
        self._call("probe_bin_order", d_off.ptr, d_len.ptr, n, d_n.ptr if d_n else None, d_hist.ptr, cursor.ptr, n_bins,
                   bin_shift, s_off.ptr, s_len.ptr, s_id.ptr)
        return {"s_off": s_off.get(), "s_len": s_len.get(), "s_id": s_id.get(), "cursor": cursor.get(),
                "hist": d_hist.t.cpu().numpy()[: n_bins * 4].view(np.uint32)}

    def root_passes(self, first, n_chunks, n_passes, ubs):
        """root_init, n_passes x root_level (ping-pong, as mi_batch_run does), root_final_items.  Addresses come back as they
        are, with the bases of the digest table and of every pass's output buffer."""
        nf = len(n_chunks)
        digests = Out(0, np.uint8)                                 # addresses only: nothing here reads a digest
        d_first, d_cnt = In(np.asarray(first, dtype=np.uint64)), In(np.asarray(n_chunks, dtype=np.uint32))
        addr = [Out(nf, np.uint64), Out(nf, np.uint64)]
        cnt = [Out(nf, np.uint32), Out(nf, np.uint32)]
        self._call("probe_root_init", digests.ptr, d_first.ptr, d_cnt.ptr, nf, addr[0].ptr, cnt[0].ptr)
        res = {"bases": {"digests": digests.ptr}, "init": (addr[0].get(), cnt[0].get()), "passes": []}
        keep = [digests]
        for r in range(n_passes):
            ub = ubs[r]
            level = Out(0, np.uint8)                               # a pass's output: written by the hashing launch, not here
            keep.append(level)
            res["bases"]["level%d" % r] = level.ptr
            seg_cnt, seg_first, seg_total = Out(nf, np.uint32), Out(nf, np.uint64), Out(1, np.uint64)
            scratch = Out(self.scratch_elems(nf), np.uint64)
            item_off, item_len = Out(ub, np.uint64), Out(ub, np.uint64)
            nxt_addr, nxt_cnt = Out(nf, np.uint64), Out(nf, np.uint32)       # fresh: what a pass leaves untouched shows
            self._call("probe_root_level", nf, ub, addr[0].ptr, cnt[0].ptr, nxt_addr.ptr, nxt_cnt.ptr, seg_cnt.ptr,
                       seg_first.ptr, seg_total.ptr, scratch.ptr, level.ptr, item_off.ptr, item_len.ptr)
            res["passes"].append({"seg_cnt": seg_cnt.get(), "seg_first": seg_first.get(), "seg_total": seg_total.get(),
                                  "item_off": item_off.get(), "item_len": item_len.get(), "next_addr": nxt_addr.get(),
                                  "next_cnt": nxt_cnt.get(), "scratch_guard": scratch.get()[scratch.n:],
                                  "cur_addr": addr[0].get(), "cur_cnt": cnt[0].get()})
            addr, cnt = [nxt_addr, addr[0]], [nxt_cnt, cnt[0]]
        f_off, f_len = Out(nf, np.uint64), Out(nf, np.uint64)
        self._call("probe_root_final_items", addr[0].ptr, cnt[0].ptr, nf, f_off.ptr, f_len.ptr)
        res["final"] = (f_off.get(), f_len.get())
        return res


@pytest.fixture(scope="module")
def tables():
    import makisu_amd
    makisu_amd.load_library()                                      # torch, then the engine, then the probe
    return Tables(build_probe())


def same(got, want, n, what):
    """got[:n] == want exactly, and everything from n on is still the sentinel"""
    got, want = np.asarray(got), np.asarray(want, dtype=got.dtype)
    assert len(want) == n and len(got) >= n + GUARD, what
    bad = np.nonzero(got[:n] != want)[0]
    assert bad.size == 0, "%s: %d differ, first at %d: got %s, want %s" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])
    touched = np.nonzero(got[n:] != sentinel(got.dtype))[0]
    assert touched.size == 0, "%s: written beyond its %d rows, first at +%d" % (what, n, touched[0])


# ---- scan --------------------------------------------------------------------------------------------------------------
SCAN_NS = [0, 1, 2047, 2048, 2049, 4096 * TILE - 1, 4096 * TILE, 4096 * TILE + 1, 4096 * TILE + 2049]


def scan_counts(n, variant):
    """random 0..3 with whole tiles of zeros ("tiles"); all zero ("zeros"); the first with 0xFFFFFFFF at three places, in three
    tiles wherever there are three ("wide": the sums pass 2^32 and 2^33)"""
    if variant == "zeros":
        return np.zeros(n, dtype=np.uint32)
    c = np.random.default_rng(n).integers(0, 4, n, dtype=np.uint32)
    n_tiles = (n + TILE - 1) // TILE
    for t in {1, 2, n_tiles // 2, n_tiles - 2}:
        if t >= 1 and (t + 1) * TILE <= n:
            c[t * TILE: (t + 1) * TILE] = 0
    if variant == "wide" and n:
        c[sorted({min(5, n - 1), n // 2, n - 3 if n >= 3 else n - 1})] = 0xFFFFFFFF
    return c


def check_scan(got, counts):
    n = len(counts)
    first, total = M.exclusive_scan(counts)
    same(got["first"], first, n, "first")
    same(got["total"], [total], 1, "total")
    assert (got["scratch_guard"] == sentinel(np.uint64)).all(), "written beyond scan_scratch_elems(n)"
    return total


@pytest.mark.parametrize("n", SCAN_NS)
def test_scan(tables, n):
    """n > 4096 tiles of 2048 takes the three-launch form -- 8 388 609 counts are the fewest that do.  The totals of "wide"
    are above 2^33: the u64 of the prototype is meant."""
    for variant in ("tiles", "zeros", "wide"):
        counts = scan_counts(n, variant)
        total = check_scan(tables.scan(counts), counts)
        if variant == "wide" and n >= 3:
            assert total > 3 * 0xFFFFFFFF - 1 and total >= 1 << 33
        if variant == "zeros":
            assert total == 0


# ---- compaction --------------------------------------------------------------------------------------------------------
BINS = [(4, 2), (257, 2), (1024, 3)]
# on both sides of a block count (len % 64 == 55 | 56) and of each setting's clamp bin: 695 | 696 = 11 | 12 blocks (bin 2 | 3 of
# 4 at shift 2), 65 463 | 65 464 = 1023 | 1024 blocks (bin 255 | 256 of 257 at shift 2), 523 703 | 523 704 = 8183 | 8184 blocks
# (bin 1022 | 1023 of 1024 at shift 3); 524 288 and more are above the last bin of every setting
EDGE_LENS = [1, 55, 56, 63, 64, 119, 120, 183, 184, 695, 696, 2048, 5000]


def align(x, a=256):
    return (x + a - 1) // a * a


def build_tables(files, region=0):
    """The segment tables of a batch.  files: ("small", [chunk lengths]) -- one segment, its ends one list -- or
    ("large", [absolute cuts, the last = the size], [style per group, cycled]): one segment per 256 KiB group holding the cuts
    in (g G, (g+1) G], stored the way the style says -- "spec0": all speculation from entry 0 of the list; "spec": all
    speculation behind two dropped entries; "prefix": all prefix, sidx == spec_n; "both": half and half.  A group's entry is
    the last cut before its first row."""
    file_off, seg0, seg_file, seg_slot, seg_n, seg_group, recs, ends = [], [0], [], [], [], [], [], []
    at, slot, any_large = 0, 0, any(f[0] == "large" for f in files)
    for f, spec in enumerate(files):
        if f == len(files) // 2:
            at += 1 << 32                                          # arena offsets beyond 32 bits
        file_off.append(at)
        if spec[0] == "small":
            e = np.cumsum(np.asarray(spec[1], dtype=np.uint64)).astype(np.uint32)
            size = int(e[-1]) if len(e) else 0
            assert size <= 65536
            seg_file.append(f); seg_slot.append(slot); seg_n.append(len(e)); seg_group.append(M.NO_GROUP)
            ends += [e, np.full(2, JUNK, np.uint32)]
            slot += len(e) + 2
        else:
            cuts, styles = spec[1], spec[2]
            size, prev = cuts[-1], 0
            for g in range((size + G - 1) // G):
                rel = [c - g * G for c in cuts if g * G < c <= (g + 1) * G]
                style = styles[g % len(styles)]
                if style == "spec0":
                    prefix, sp, sidx = [], rel, 0
                elif style == "spec":
                    prefix, sp, sidx = [], [JUNK - 1, JUNK - 2] + rel, 2
                elif style == "prefix":
                    prefix, sp, sidx = rel, [JUNK - 3, JUNK - 4], 2
                else:
                    k = (len(rel) + 1) // 2
                    prefix, sp, sidx = rel[:k], [JUNK - 5] + rel[k:], 1
                assert len(prefix) <= region and len(sp) <= region
                seg = np.full(2 * region, JUNK, np.uint32)
                seg[: len(sp)] = sp
                seg[region: region + len(prefix)] = prefix
                ends.append(seg)
                seg_file.append(f); seg_slot.append(slot); seg_n.append(len(rel)); seg_group.append(len(recs))
                recs.append((0x1111, 0x2222, prev, len(sp), len(prefix), sidx, 2))
                slot += 2 * region
                if rel:
                    prev = g * G + rel[-1]
        seg0.append(len(seg_file))
        at += align(size) if size else 0
    return {"file_off": np.array(file_off, dtype=np.uint64), "file_seg0": np.array(seg0, dtype=np.uint64),
            "seg_file": np.array(seg_file, dtype=np.uint32), "seg_slot": np.array(seg_slot, dtype=np.uint64),
            "seg_n": np.array(seg_n, dtype=np.uint32), "ends32": np.concatenate(ends + [np.full(2, JUNK, np.uint32)]),
            "seg_group": np.array(seg_group, dtype=np.uint32) if any_large else None,
            "recs": np.array(recs, dtype=M.GROUP_REC) if any_large else None, "region": region}


def small_files(rng, n):
    """n small files of 1..6 chunks with the edge lengths among them, one-chunk files at the 257-bin clamp, a few empty"""
    out = []
    for i in range(n):
        if i % 11 == 3:
            out.append(("small", []))
        elif i % 13 == 5:
            out.append(("small", [[65463, 65464, 65536][i % 3]]))
        else:
            out.append(("small", [int(x) for x in rng.choice(EDGE_LENS, rng.integers(1, 7))]))
    return out


def large_file(lens, styles):
    return ("large", [int(c) for c in np.cumsum(lens)], styles)


@functools.lru_cache(maxsize=None)
def compaction_case(name):
    """(tables, model rows, scanned segment counts, total)"""
    rng = np.random.default_rng(len(name))
    empty = ("small", [])
    if name.startswith("files"):                                   # 255 / 256 / 257 files: file_rows_kernel's block edge
        n = int(name[5:])
        files = [empty] * 3 + small_files(rng, n - 5) + [empty] * 2
        assert len(files) == n
        t = build_tables(files)
    elif name == "runs":                                           # empty segments: in front, across a scan tile, at the end
        files = [empty] * 7 + small_files(rng, 30) + [empty] * (TILE + 5) + small_files(rng, 20) + [empty] * 9
        t = build_tables(files)
    elif name == "second_trip":                                    # more rows than 2048 workgroups x 256 threads take at once
        ones = ("small", [1] * 65536)
        files = [empty] * 2 + [ones] * 5 + [empty] * 3 + [ones] * 4 + [("small", [55, 56])] + [empty]
        t = build_tables(files)
    else:                                                          # "groups": files of several group segments between small ones
        assert name == "groups"
        # cuts on purpose: the edge lengths, one chunk through a whole group (a group without rows), chunks at and above the
        # last bin of 1024 (entered from a cut two and three groups back)
        a = large_file(EDGE_LENS + [65463, 65464, 100000, 523703, 7, 523704, 56, 524288, 55, 3 * G + 5, 1000, 696, 695, 120, 119,
                                    G, 64], ["spec0", "prefix", "both", "spec", "both", "prefix", "spec"])
        b = large_file([70000, 70000, 70000, 55, 56, 60000], ["both", "spec"])
        c = large_file([G + 1], ["prefix"])                         # two groups, the first without rows
        files = small_files(rng, 6) + [empty, a, empty, empty] + small_files(rng, 3) + [b, c] + small_files(rng, 2) + [empty]
        t = build_tables(files, region=32)
        assert (t["seg_n"][t["seg_group"] != M.NO_GROUP] == 0).sum() >= 3
    rows = M.chunk_rows(t["file_off"], t["file_seg0"], t["seg_file"], t["seg_slot"], t["ends32"], t["seg_n"],
                        t["seg_group"], t["recs"], t["region"])
    seg_first, total = M.exclusive_scan(t["seg_n"])
    assert total == len(rows["chunk_len"]) == int(rows["n_chunks"].sum())
    return t, rows, seg_first, total


def check_compaction(got, rows, total, n_files, n_bins, bin_shift, want_items):
    for k in ("chunk_off", "chunk_len", "chunk_file", "chunk_start"):
        same(got[k], rows[k], total, k)
    same(got["first"], rows["first"], n_files, "first")
    same(got["n_chunks"], rows["n_chunks"], n_files, "n_chunks")
    same(got["hist"], M.length_histogram(rows["chunk_len"], n_bins, bin_shift), n_bins, "hist")
    if want_items:
        off, ln = M.flat_root_items(rows["first"], rows["n_chunks"])
        same(got["item_off"], off + np.uint64(got["digests_base"]), n_files, "item_off")
        same(got["item_len"], ln, n_files, "item_len")
    else:
        same(got["item_off"], [], 0, "item_off (not requested)")
        same(got["item_len"], [], 0, "item_len (not requested)")


@pytest.mark.parametrize("name", ["files255", "files256", "files257", "runs", "second_trip", "groups"])
def test_compaction(tables, name):
    t, rows, seg_first, total = compaction_case(name)
    n_max = total + 300                                            # the real count is below the upper bound
    if name == "second_trip":
        assert n_max > 2048 * 256
    if name == "groups":
        lens = rows["chunk_len"].tolist()
        assert {55, 56, 695, 696, 65463, 65464, 523703, 523704, 524288, 3 * G + 5} <= set(lens)
    for i, (n_bins, bin_shift) in enumerate(BINS):
        want_items = i != 1
        got = tables.compact(t, seg_first, total, n_max, n_bins, bin_shift, want_items)
        check_compaction(got, rows, total, len(t["file_off"]), n_bins, bin_shift, want_items)


# ---- order -------------------------------------------------------------------------------------------------------------
def len_of_bin(b, bin_shift, rng):
    """a length whose bin is b (b below the clamp bin, or the clamp bin itself)"""
    if b == 0:
        return int(rng.integers(0, 56))
    blocks = (b << bin_shift) + int(rng.integers(0, 1 << bin_shift))
    return (blocks - 1) * 64 + int(rng.integers(0, 56))


def order_lens(n, n_bins, bin_shift):
    """n lengths: the first and the last bin of every 256-bin round of the start scan (from the top: n_bins-1 .. n_bins-256,
    ...), bins drawn from all of them, and lengths far above the last bin"""
    rng = np.random.default_rng(n * 1031 + n_bins)
    edges = sorted({b for i in range(0, n_bins, 256) for b in (n_bins - 1 - i, max(n_bins - 256 - i, 0))})
    lens = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            lens.append(len_of_bin(edges[(i // 4) % len(edges)], bin_shift, rng))
        elif kind == 3 and i % 16 == 3:
            lens.append(((n_bins << bin_shift) + int(rng.integers(0, 5000))) * 64)
        else:
            lens.append(len_of_bin(int(rng.integers(0, n_bins)), bin_shift, rng))
    lens = np.array(lens, dtype=np.uint64)
    return lens[rng.permutation(n)], edges


def check_order(got, off, lens, n_real, n_bins, bin_shift):
    hist = M.length_histogram(lens[:n_real], n_bins, bin_shift)
    s_id = got["s_id"][:n_real].astype(np.int64)
    assert np.array_equal(np.sort(s_id), np.arange(n_real)), "s_id is not a permutation of the real rows"
    same(got["s_off"], off[s_id], n_real, "s_off")
    same(got["s_len"], lens[s_id], n_real, "s_len")
    same(got["s_id"], s_id, n_real, "s_id")
    assert M.bins_never_increase(got["s_len"][:n_real], n_bins, bin_shift), "the queue is not longest-first"
    same(got["cursor"], hist, n_bins, "cursor")
    assert np.array_equal(got["hist"], hist), "the histogram was changed"


@pytest.mark.parametrize("n_bins,bin_shift", BINS)
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 20000])
def test_order(tables, n, n_bins, bin_shift):
    lens, edges = order_lens(n, n_bins, bin_shift)
    off = np.random.default_rng(n).integers(0, 1 << 40, n).astype(np.uint64)
    for n_real in (None, n - max(1, n // 7)):                      # no device count; a real count below n
        real = n if n_real is None else n_real
        if real >= 64:
            assert set(edges) <= set(M.length_bins(lens[:real], n_bins, bin_shift).tolist())
        hist = M.length_histogram(lens[:real], n_bins, bin_shift)
        check_order(tables.order(off, lens, n_real, hist, n_bins, bin_shift), off, lens, real, n_bins, bin_shift)


# ---- root levels -------------------------------------------------------------------------------------------------------
ROOT_COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097]


def root_counts(n_files, flat):
    rng = np.random.default_rng(n_files)
    pool = [c for c in ROOT_COUNTS if c <= 64] if flat else ROOT_COUNTS
    if n_files == 1:
        return np.array([pool[-1]], dtype=np.uint32)
    c = np.array([pool[i % len(pool)] for i in range(n_files)], dtype=np.uint32)
    return c[rng.permutation(n_files)]


def to_addr(lst, bases):
    return np.array([bases[b] + o for b, o, _ in lst], dtype=np.uint64)


def check_root_passes(got, first, counts, n_passes, ubs):
    nf, bases = len(counts), got["bases"]
    cur = M.root_init(first, counts)
    same(got["init"][0], to_addr(cur, bases), nf, "root_init addr")
    same(got["init"][1], [c for _, _, c in cur], nf, "root_init cnt")
    totals = []
    for r in range(n_passes):
        p = got["passes"][r]
        seg_cnt, seg_first, total, items, nxt = M.root_level(cur, "level%d" % r)
        assert total <= ubs[r]
        same(p["cur_addr"], to_addr(cur, bases), nf, "pass %d: cur_addr (read only)" % r)
        same(p["cur_cnt"], [c for _, _, c in cur], nf, "pass %d: cur_cnt (read only)" % r)
        same(p["seg_cnt"], seg_cnt, nf, "pass %d: seg_cnt" % r)
        same(p["seg_first"], seg_first, nf, "pass %d: seg_first" % r)
        same(p["seg_total"], [total], 1, "pass %d: seg_total" % r)
        same(p["item_off"], to_addr(items, bases), total, "pass %d: item_off" % r)
        same(p["item_len"], [n for _, _, n in items], total, "pass %d: item_len" % r)
        same(p["next_addr"], to_addr(nxt, bases), nf, "pass %d: next_addr" % r)
        same(p["next_cnt"], [c for _, _, c in nxt], nf, "pass %d: next_cnt" % r)
        assert (p["scratch_guard"] == sentinel(np.uint64)).all()
        for (b0, _, c0), (b1, _, _) in zip(cur, nxt):                # carried files keep their list, reduced ones move on
            assert (b1 == b0) == (c0 <= M.FANOUT) and (b1 == b0 or b1 == "level%d" % r)
        cur = nxt
        totals.append(total)
    fin = M.root_final_items(cur)
    same(got["final"][0], to_addr(fin, bases), nf, "final item_off")
    same(got["final"][1], [n for _, _, n in fin], nf, "final item_len")
    return totals


@pytest.mark.parametrize("n_files", [1, 2048, 2049])
@pytest.mark.parametrize("flat", [False, True], ids=["tree", "flat"])
def test_root_levels(tables, n_files, flat):
    """Three passes over every set: with counts up to 4097 the first reduces (4097 -> 65, 65 -> 2, 64 carried), the second
    reduces only what still exceeds the fan-out (65 -> 2) and the third is empty; with no count above 64 every pass is empty
    -- *seg_total == 0 under an upper bound that is not, the state root_passes' own upper bound leaves the hashing launch in."""
    counts = root_counts(n_files, flat)
    first, total = M.exclusive_scan(counts)
    ubs, ub = [], total
    for _ in range(3):
        ub = ub // M.FANOUT + n_files                              # mi_batch_run's bound of the nodes a pass can make
        ubs.append(ub)
    totals = check_root_passes(tables.root_passes(first, counts, 3, ubs), first, counts, 3, ubs)
    if flat:
        assert totals == [0, 0, 0]
    else:
        assert totals[0] > 0 and totals[1] > 0 and totals[2] == 0
        assert totals[1] == 2 * int((counts == 4097).sum())
