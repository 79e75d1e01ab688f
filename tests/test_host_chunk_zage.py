"""Ageing a compressed pack set without a GPU: the header declares and tags the calls and the binding covers them, mi_touch_info
and mi_zage_bin have the header's layout, NULL is refused without a device, and the model (zage_cases.py) is pinned by hand on a
dozen digests over four epochs; its expiry agrees with the list prune of zprune_cases.py fed the victims."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pack_cases as pc
import zage_cases as ag
import zprune_cases as pr
import zset_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")
NEW_CALLS = ["mi_zset_set_epoch", "mi_zset_get_epoch", "mi_zset_touch", "mi_zset_stamps", "mi_zset_age_census", "mi_zset_expire"]
TOUCH_FIELDS = ["n_rows", "n_unknown", "n_refreshed", "ms_touch"]
BIN_FIELDS = ["n_digests", "stored_bytes", "live_bytes", "chunk_bytes"]


def test_the_header_declares_and_tags_the_calls_and_the_binding_covers_them(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tags = dict((m.group(2), m.group(1)) for m in
                re.finditer(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b(mi_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name in NEW_CALLS:
        assert tags.get(name) == "MI_BLOCK", (name, tags.get(name))
        assert name in engine_lib._mi_symbols and hasattr(engine_lib, name), name
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M)        # additive: the version stays
    import makisu_amd as M
    for attr in ("set_epoch", "epoch", "touch", "stamps", "age_census", "expire"):
        assert hasattr(M.ZSet, attr), attr
    assert isinstance(M.ZSet.epoch, property)
    for name in ("TouchInfo", "AgeBin", "STAMP_NONE"):
        assert name in M.__all__, name
    assert M.STAMP_NONE == ag.NONE == 0xFFFFFFFF
    assert "mi_zage.hip" in __import__("makisu_amd.build", fromlist=["SOURCES"]).SOURCES


def test_the_struct_layouts_match_the_header(tmp_path):
    import makisu_amd as M
    lines = ['printf("%zu %zu\\n", sizeof(mi_touch_info), sizeof(mi_zage_bin));']
    lines += ['printf("%%zu\\n", offsetof(mi_touch_info, %s));' % f for f in TOUCH_FIELDS]
    lines += ['printf("%%zu\\n", offsetof(mi_zage_bin, %s));' % f for f in BIN_FIELDS]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "makisu_mi.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    T, B = M.TouchInfo, M.AgeBin
    assert got == [C.sizeof(T), C.sizeof(B)] + [getattr(T, f).offset for f in TOUCH_FIELDS] + [getattr(B, f).offset for f in BIN_FIELDS]
    assert got[:2] == [32, 32] and [n for n, _ in T._fields_] == TOUCH_FIELDS and [n for n, _ in B._fields_] == BIN_FIELDS


def test_null_is_refused_without_a_device(engine_lib):
    import makisu_amd as M
    L = engine_lib
    ti, pi = M.TouchInfo(), M.PruneInfo()
    ti.n_rows = pi.n_rows = 9
    dig, out, bounds, bins = np.zeros((2, 32), dtype=np.uint8), np.zeros(2, dtype=np.uint32), np.array([1], dtype=np.uint32), (M.AgeBin * 2)()
    assert L.mi_zset_set_epoch(None, 1) == -1
    assert L.mi_zset_get_epoch(None, None, None, None) == -1
    assert L.mi_zset_touch(None, dig.ctypes.data, 2, C.byref(ti)) == -1 and ti.n_rows == 0
    assert L.mi_zset_stamps(None, dig.ctypes.data, 2, out.ctypes.data) == -1
    assert L.mi_zset_age_census(None, bounds.ctypes.data, 1, C.addressof(bins)) == -1
    assert L.mi_zset_expire(None, 0, 0, C.byref(pi)) == -1 and pi.n_rows == 0


# ---- the model, by hand ---------------------------------------------------------------------------------------------------------
def _dozen():
    """twelve distinct chunks of 20 + i random bytes (raw: stored = length, a span of 32 bytes each) in three zpacks of four"""
    rng = np.random.default_rng(1801)
    chunks = [rng.integers(0, 256, 20 + i, dtype=np.uint8).tobytes() for i in range(12)]
    dig = qc.digests_of(chunks, pc.SHA256)
    packs = [qc.zpack_of(chunks[a:a + 4], pc.SHA256)[2:] for a in (0, 4, 8)]
    return chunks, dig, packs


def test_the_model_by_hand_on_a_dozen_digests_over_four_epochs():
    chunks, dig, packs = _dozen()
    stranger = np.zeros((1, 32), dtype=np.uint8)
    st = ag.Store()
    st.add(*packs[0])                                                      # before ageing: 0..3
    assert (st.ageing, st.epoch, st.stamp_bytes()) == (False, 0, 0)
    st.set_epoch(1)                                                        # everything held is stamped 1
    assert (st.ageing, st.epoch, st.stamp_bytes()) == (True, 1, pr.alloc(4096)) and st.stamps(dig[:5]) == [1, 1, 1, 1, ag.NONE]
    st.set_epoch(2)
    st.add(*packs[1])                                                      # 4..7 at epoch 2
    assert st.stamps(dig) == [1] * 4 + [2] * 4 + [ag.NONE] * 4
    # a repeat in a touch counts once in n_refreshed, per row in n_unknown; a digest already at the epoch is not refreshed
    assert st.touch(np.concatenate([dig[[0, 0, 4, 0]], stranger, stranger])) == {"n_rows": 6, "n_unknown": 2, "n_refreshed": 1}
    assert st.stamps(dig[:2]) == [2, 1]
    st.set_epoch(3)
    st.set_epoch(3)                                                        # equal: a no-op
    st.add(*packs[2])                                                      # 8..11 at epoch 3
    st.add(*packs[0])                                                      # a re-add refreshes: the first form stays, the stamp does not
    assert st.stamps(dig) == [3] * 4 + [2] * 4 + [3] * 4 and st.info()["n_digests"] == 12
    st.set_epoch(4)
    assert st.touch(dig[[5, 9, 5]]) == {"n_rows": 3, "n_unknown": 0, "n_refreshed": 2}
    assert st.stamps(dig) == [3, 3, 3, 3, 2, 4, 2, 2, 3, 4, 3, 3]
    for bad in (3, ag.NONE):                                               # the clock never goes back; 0xFFFFFFFF is reserved
        with pytest.raises(ValueError):
            st.set_epoch(bad)
    # a bound equal to a stamp lands in the upper bin
    bins = st.census([3])
    assert [b["n_digests"] for b in bins] == [3, 9]
    assert bins[0] == {"n_digests": 3, "stored_bytes": 24 + 26 + 27, "live_bytes": 96, "chunk_bytes": 24 + 26 + 27}
    assert [b["n_digests"] for b in st.census([1, 2, 3, 4, 5])] == [0, 0, 3, 7, 2, 0]
    assert [b["n_digests"] for b in st.census([4])] == [10, 2]
    assert sum(b["live_bytes"] for b in st.census([2, 4])) == st.usage()["live_bytes"] == 12 * 32
    with pytest.raises(ValueError):
        st.expire(5)                                                       # above the epoch: refused
    # nothing older than 2: nothing changes, the sizes are those of a prune with an empty request
    slots = st.slots
    info = st.expire(2, 1000)
    assert (info["n_rows"], info["n_unknown"], info["n_dropped"]) == (0, 0, 0) and st.slots == slots
    assert info["peak_extra_bytes"] == pr.alloc(0) + pr.alloc(1024) + pr.alloc(4096) + 2 * pr.alloc(4 * 8) + pr.alloc(64)
    # E = 3 drops 4, 6 and 7: pack 1 keeps 32 of 128 bytes and is compacted at 1000, kept whole at 0
    twin = copy.deepcopy(st)
    info = st.expire(3, 1000)
    assert (info["n_rows"], info["n_unknown"], info["n_dropped"], info["dropped_stored_bytes"], info["dropped_chunk_bytes"]) == (0, 0, 3, 77, 77)
    assert (info["n_blobs_freed"], info["n_blobs_compacted"], info["moved_bytes"]) == (2, 1, 32)      # and the re-add's blob, never live
    assert st.stamps(dig) == [3, 3, 3, 3, ag.NONE, 4, ag.NONE, ag.NONE, 3, 4, 3, 3]         # survivors keep their stamps
    info0 = twin.expire(3, 0)
    assert (info0["n_dropped"], info0["n_blobs_freed"], info0["moved_bytes"]) == (3, 1, 0)
    # the formula: the list prune's with n = 0, plus the new stamp array (1 024 slots again)
    table = pr.alloc(1024 * 8) + pr.alloc(1024 * 48)
    want = pr.alloc(0) + pr.alloc(1024) + pr.alloc(4096) + 2 * pr.alloc(4 * 8) + pr.alloc(64) + table + pr.alloc(9 * 48) + pr.alloc(9 + 16) + \
        pr.alloc(9 * 8 + 16) + pr.alloc(64) + pr.alloc(4 * 1024)
    assert info0["peak_extra_bytes"] == want
    assert info["peak_extra_bytes"] == want + pr.alloc(4) + pr.alloc((2 * 1 + 8) * 8) + pr.alloc(32) + pr.alloc(4 * 1 * 8) + pr.alloc(1024 * 8)
    assert st.expire(4, 0)["n_dropped"] == 7 and sorted(st.stamps(dig)) == [4, 4] + [ag.NONE] * 10


@pytest.mark.parametrize("permille", [0, 600, 1000])
def test_the_models_expiry_is_the_list_prune_fed_the_victims(permille):
    a, b, c, _ = pr.three_fates()
    for min_epoch in (1, 2, 3, 4):
        aged, plain = ag.Store(), pr.Store()
        aged.set_epoch(1)
        for epoch, part in ((1, a), (2, b), (3, c)):
            aged.set_epoch(epoch)
            _, _, ze, zb = qc.zpack_of(part, pc.SHA256)
            aged.add(ze, zb)
            plain.add(ze, zb)
        aged.set_epoch(4)
        dig_b = qc.digests_of(b, pc.SHA256)
        aged.touch(dig_b[[0, 2, 4, 6]])                                    # half of b is used again
        victims = aged.victims(min_epoch)
        got = aged.expire(min_epoch, permille)
        want = plain.prune(np.frombuffer(b"".join(victims), dtype=np.uint8).reshape(-1, 32), keep=False, permille=permille)
        addend = pr.alloc(4 * plain.slots) if victims else 0
        assert got == dict(want, n_rows=0, peak_extra_bytes=want["peak_extra_bytes"] - pr.alloc(32 * len(victims)) + pr.alloc(0) + addend)
        assert aged.info() == plain.info() and aged.usage() == plain.usage() and aged.held == plain.held
        assert len(victims) == {1: 0, 2: len(a), 3: len(a) + 4, 4: len(a) + 4 + len(c)}[min_epoch]
