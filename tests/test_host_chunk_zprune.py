"""Pruning a compressed pack set without a GPU: the header declares and tags the calls and the binding covers them, mi_prune_info
and mi_zset_usage have the header's layout, NULL and bad arguments are refused without a device, and the prune's model
(zprune_cases.py) is pinned by hand on a three-blob, six-chunk store."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import zpack_cases as zc
import zprune_cases as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")
NEW_CALLS = ["mi_zset_prune", "mi_zset_get_usage", "mi_zset_entries"]
PRUNE_FIELDS = ["n_rows", "n_unknown", "n_dropped", "dropped_stored_bytes", "dropped_chunk_bytes", "n_blobs_freed", "freed_bytes",
                "n_blobs_compacted", "moved_bytes", "n_blobs_sparse_kept", "peak_extra_bytes", "ms_mark", "ms_move", "ms_rebuild"]
USAGE_FIELDS = ["n_blobs", "resident_bytes", "live_bytes", "table_slots", "table_bytes"]


def test_the_header_declares_and_tags_the_calls_and_the_binding_covers_them(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tags = dict((m.group(2), m.group(1)) for m in
                re.finditer(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b(mi_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name in NEW_CALLS:
        assert tags.get(name) == "MI_BLOCK", (name, tags.get(name))
        assert name in engine_lib._mi_symbols and hasattr(engine_lib, name), name
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M)        # additive: the version stays
    assert re.search(r"^#define\s+MI_ZSET_PRUNE_KEEP\s+0x1u", src, re.M) and re.search(r"^#define\s+MI_ZSET_PRUNE_DROP\s+0x2u", src, re.M)
    import makisu_amd as M
    assert (M.ZSET_PRUNE_KEEP, M.ZSET_PRUNE_DROP) == (1, 2)
    for attr in ("prune", "usage", "entries"):
        assert hasattr(M.ZSet, attr), attr
    for name in ("PruneInfo", "ZSetUsage", "ZSET_PRUNE_KEEP", "ZSET_PRUNE_DROP"):
        assert name in M.__all__, name


def test_the_struct_layouts_match_the_header(tmp_path):
    import makisu_amd as M
    lines = ['printf("%zu %zu\\n", sizeof(mi_prune_info), sizeof(mi_zset_usage));']
    lines += ['printf("%%zu\\n", offsetof(mi_prune_info, %s));' % f for f in PRUNE_FIELDS]
    lines += ['printf("%%zu\\n", offsetof(mi_zset_usage, %s));' % f for f in USAGE_FIELDS]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "makisu_mi.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    P, U = M.PruneInfo, M.ZSetUsage
    assert got == [C.sizeof(P), C.sizeof(U)] + [getattr(P, f).offset for f in PRUNE_FIELDS] + [getattr(U, f).offset for f in USAGE_FIELDS]
    assert got[:2] == [112, 40] and [n for n, _ in P._fields_] == PRUNE_FIELDS and [n for n, _ in U._fields_] == USAGE_FIELDS


def test_null_and_bad_arguments_are_refused_without_a_device(engine_lib):
    import makisu_amd as M
    L = engine_lib
    info, usage, n = M.PruneInfo(), M.ZSetUsage(), C.c_uint64(7)
    info.n_rows = 9
    dig = np.zeros((2, 32), dtype=np.uint8)
    assert L.mi_zset_prune(None, dig.ctypes.data, 2, M.ZSET_PRUNE_KEEP, 0, C.byref(info)) == -1 and info.n_rows == 0
    assert L.mi_zset_prune(None, None, 0, M.ZSET_PRUNE_DROP, 0, None) == -1
    assert L.mi_zset_prune(None, None, 0, 3, 1001, None) == -1
    assert L.mi_zset_get_usage(None, C.byref(usage)) == -1 and L.mi_zset_get_usage(None, None) == -1
    assert L.mi_zset_entries(None, None, None, None, 0, C.byref(n)) == -1 and L.mi_zset_entries(None, None, None, None, 0, None) == -1


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def test_the_prune_model_pinned_by_hand_on_a_three_blob_six_chunk_store():
    """A = {x1: 5 bytes raw, x2: 40 bytes raw}, 64 bytes.  B = {x3: 31 stored for 34, x2 CODED: it lost to A's form and was never
    live}, 32 + 16 bytes.  C = {x4: 16 raw, x5: 17 raw, x6: 100 raw}, 16 + 32 + 112 = 160 bytes.  KEEP [x2, x4, x5, a stranger,
    x4] at 500 permille: x1, x3 and x6 go; A keeps 48 of 64 bytes (750 permille: it stays), B keeps nothing (freed), C keeps 48
    of 160 (300 permille: compacted into a new blob of 48 bytes)."""
    x1, x2, x4, x5, x6 = b"hello", bytes([9]) * 40, bytes(range(16)), bytes(range(50, 67)), bytes(range(100, 200))
    coded2 = zc.compress_chunk(x2)
    assert len(coded2) <= 16
    a = zc.build_zpack([zc._entry(x1, 5, x1, pad=0xA5), zc._entry(x2, 40, x2, pad=0x11)])
    b = zc.build_zpack([zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN, pad=0x22), zc._entry(coded2, 40, x2)])
    c = zc.build_zpack([zc._entry(x4, 16, x4), zc._entry(x5, 17, x5, pad=0x33), zc._entry(x6, 100, x6)])
    assert [len(z[1]) for z in (a, b, c)] == [64, 48, 160]
    d1, d2, d3, d4, d5, d6 = (zc.sha(x) for x in (x1, x2, zc.GOOD_PLAIN, x4, x5, x6))
    s = pr.Store()
    for z in (a, b, c):
        s.add(*z)
    assert s.info() == {"n_packs": 3, "n_entries": 7, "n_digests": 6, "blob_bytes": 272, "stored_bytes": 5 + 40 + 31 + 16 + 17 + 100,
                        "chunk_bytes": 5 + 40 + 34 + 16 + 17 + 100}
    assert s.live() == {0: 64, 1: 32, 2: 160} and s.held[d2][2] == 40                                   # the raw form is the one held
    assert s.usage() == {"n_blobs": 3, "resident_bytes": 3 * 512, "live_bytes": 256, "table_slots": 1024,
                         "table_bytes": (8192 + 1024 + 256) + (49152 + 6144 + 256)}
    request = np.frombuffer(d2 + d4 + d5 + zc.sha(b"a stranger") + d4, dtype=np.uint8).reshape(-1, 32)
    before = dict(s.held)
    info = s.prune(request, keep=True, permille=500)
    # scratch: the request (160 -> 512), marks (1 024 -> 1 280), per-slot blob (4 096 -> 4 352), bases and sums (24 -> 512 each),
    # totals (512); fates (512), the scan (80 -> 512), the new blob (48 -> 512), the move list (64 -> 512), per-slot addresses
    # (8 192 -> 8 448); the new table (8 448 + 49 408), records (144 -> 512), the insert's three (512 each)
    assert info == {"n_rows": 5, "n_unknown": 1, "n_dropped": 3, "dropped_stored_bytes": 136, "dropped_chunk_bytes": 139, "n_blobs_freed": 2,
                    "freed_bytes": 1024, "n_blobs_compacted": 1, "moved_bytes": 48, "n_blobs_sparse_kept": 0,
                    "peak_extra_bytes": 7680 + 10496 + 59904}
    assert sorted(s.held) == sorted([d2, d4, d5]) and all(s.held[k][:3] == before[k][:3] for k in s.held)
    assert s.held[d5][1] == x5 + bytes([0x33]) * 15                                                      # the pad moves as it was
    assert s.live() == {0: 48, 3: 48} and s.blobs == {0: 64, 3: 48}
    assert s.usage() == {"n_blobs": 2, "resident_bytes": 1024, "live_bytes": 96, "table_slots": 1024, "table_bytes": 8448 + 49408}
    assert s.info() == {"n_packs": 3, "n_entries": 7, "n_digests": 3, "blob_bytes": 272, "stored_bytes": 73, "chunk_bytes": 73}
    assert s.missing(np.frombuffer(d1 + d2 + d6, dtype=np.uint8).reshape(-1, 32)) == [0, 1, 0]
    # nothing to drop: only the first scratch is counted, the store is as it was
    usage = s.usage()
    info = s.prune(request, keep=True, permille=1000)
    assert info["n_dropped"] == 0 and info["n_unknown"] == 1 and info["peak_extra_bytes"] == 512 + 1280 + 4352 + 2 * 512 + 512
    assert s.usage() == usage
    # DROP with the same list empties it; a later add brings the coded form of x2
    info = s.prune(request, keep=False)
    assert (info["n_dropped"], info["n_blobs_freed"], info["freed_bytes"], info["moved_bytes"]) == (3, 2, 1024, 0)
    assert s.usage()["n_blobs"] == 0 and s.usage()["resident_bytes"] == 0 and not s.held
    s.add(*b)
    assert s.held[d2][2] == len(coded2) and s.held[d3][2] == 31


def test_the_edge_store_puts_spans_on_and_across_tile_edges_and_the_last_span_on_both_last_units():
    chunks, dig, ze, zb, cand = pr.edge_store()
    assert all(13 <= len(c) <= 40 for c in chunks) and 0 < int((ze["stored"] < ze["length"]).sum()) < 100
    last = len(chunks) - 1
    assert int(ze["offset"][last]) + zc.round16(int(ze["stored"][last])) == len(zb)
    for n in (2047, 2048, 2049):
        layout, total = pr.edge_layout(ze, cand[:n])
        assert len(layout) == n and layout[-1][0] == last and layout[-1][1] + layout[-1][2] == total
        assert any(at + span == 49152 for _, at, span in layout)                         # ends on a 16 KiB tile edge
        assert any(at < edge < at + span for _, at, span in layout for edge in (16384, 32768))   # straddles one
        s = pr.Store()
        s.add(ze, zb)
        assert s.slots == 8192                                                            # no tag reaches the table's size: nothing collides
        info = s.prune(dig[cand[:n]], keep=True, permille=1000)
        assert (info["n_blobs_compacted"], info["moved_bytes"], info["n_dropped"]) == (1, total, len(chunks) - n)
        assert s.slots == (4096 if n <= 2048 else 8192)


def test_the_three_fates_store_is_what_its_name_says():
    a, b, c, stay = pr.three_fates()
    chunks = a + b + c
    assert len(set(chunks)) == len(chunks)
    zb = [zc.model_compress(*zc.pack_of(x)) for x in (a, b, c)]
    eb = zb[1][0]
    kept = eb[stay]
    assert {int(x) % 16 for x in kept["stored"]} >= {0, 1, 15}
    assert any(kept["stored"] == kept["length"]) and any(kept["stored"] < kept["length"])
    for ze, _ in zb:
        assert any(ze["stored"] == ze["length"]) and any(ze["stored"] < ze["length"])
    s = pr.Store()
    for z in zb:
        s.add(*z)
    keep = np.concatenate([eb["digest"][stay], zb[2][0]["digest"]])
    live_after = sum(zc.round16(int(x)) for x in kept["stored"])
    assert 0 < live_after * 1000 < 600 * len(zb[1][1])                  # B is under 600 permille: 600 and 1000 compact it, 0 does not
    info = s.prune(keep, keep=True, permille=1000)
    assert (info["n_blobs_freed"], info["n_blobs_compacted"], info["moved_bytes"]) == (2, 1, live_after)
    # the memory claim: what the call allocates is below the live bytes the cut-and-re-add path allocates twice
    assert info["peak_extra_bytes"] < 2 * s.usage()["live_bytes"]
