"""Recoding a compressed pack set without a GPU: the header declares and tags the call and the binding covers it, mi_recode_info
has the header's layout, a NULL set is refused without a device, THE RULE (zrecode_cases.recode_form) is pinned by hand, and what
the model holds after a recode of the planted chunks passes the host's mi_zpack_check at both levels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import zpack_cases as zc
import zrecode_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")
FIELDS = ["n_digests", "n_recoded", "n_raw_recoded", "n_undecodable", "stored_before", "stored_after", "live_before", "live_after",
          "n_blobs_rewritten", "n_blobs_freed", "freed_bytes", "new_blob_bytes", "n_rounds", "peak_extra_bytes", "ms_decode", "ms_encode",
          "ms_move", "ms_rebuild", "ms_verify"]


def test_the_header_declares_and_tags_the_call_and_the_binding_covers_it(engine_lib):
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    tags = dict((m.group(2), m.group(1)) for m in
                re.finditer(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b(mi_[a-z0-9_]+)\s*\(", src, flags=re.M))
    assert tags.get("mi_zset_recode") == "MI_BLOCK"
    assert "mi_zset_recode" in engine_lib._mi_symbols and hasattr(engine_lib, "mi_zset_recode")
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M)        # additive: the version stays
    assert re.search(r"^#define\s+MI_ZSET_RECODE_VERIFY\s+0x1u", src, re.M)
    assert re.search(r"typedef struct \{\s*/\* 152 bytes \*/[^}]*\} mi_recode_info;", text)
    import makisu_amd as M
    assert M.ZSET_RECODE_VERIFY == 1 and M.ZPACK_LEVEL2 == 4 and hasattr(M.ZSet, "recode")
    for name in ("RecodeInfo", "ZSET_RECODE_VERIFY"):
        assert name in M.__all__, name


def test_the_struct_layout_matches_the_header(tmp_path):
    import makisu_amd as M
    lines = ['printf("%zu\\n", sizeof(mi_recode_info));'] + ['printf("%%zu\\n", offsetof(mi_recode_info, %s));' % f for f in FIELDS]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "makisu_mi.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    R = M.RecodeInfo
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f in FIELDS]
    assert got[0] == 152 and [n for n, _ in R._fields_] == FIELDS


def test_a_null_set_is_refused_without_a_device(engine_lib):
    import makisu_amd as M
    info = M.RecodeInfo()
    info.n_digests = 9
    assert engine_lib.mi_zset_recode(None, M.ZPACK_LEVEL2, 0, C.byref(info)) == -1 and info.n_digests == 0
    assert engine_lib.mi_zset_recode(None, 0x80, 1 << 20, None) == -1


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def test_the_rule_pinned_by_hand():
    # GOOD_STREAM (31 bytes for 34) decodes to GOOD_PLAIN, and both levels code GOOD_PLAIN to exactly GOOD_STREAM (31 < 34 -
    # (34 >> 4) = 32: the block is kept): the candidate is not SMALLER than the stored form -- the entry keeps its bytes; the raw
    # form of the same chunk is replaced by it
    for level in (1, 2):
        assert rc.coded(zc.GOOD_PLAIN, level) == zc.GOOD_STREAM
        assert rc.recode_form(zc.GOOD_STREAM, 34, level) == zc.GOOD_STREAM
        assert rc.recode_form(zc.GOOD_PLAIN, 34, level) == zc.GOOD_STREAM                    # raw in, a block of 31 bytes out
    # raw to block: 40 bytes of one value.  One literal, a match of offset 1 to n - 5 = 35 (length 34: 15 + extension byte 15),
    # five last literals: token 0x1F, the literal, offset 1 0, extension 15, token 0x50, five literals = 11 bytes
    nines = bytes([9]) * 40
    block = bytes([0x1F, 9, 1, 0, 15, 0x50]) + bytes([9]) * 5
    assert zc.lz4_block_decode(block, 40) == nines
    for level in (1, 2):
        assert rc.recode_form(nines, 40, level) == block
        assert rc.recode_form(block, 40, level) == block                                     # a second call changes nothing
    assert rc.recode_form(bytes(12), 12, 2) == bytes(12)                                     # under 13 bytes: always raw
    # a form that breaks a decoding rule stays as it is
    bad = zc.sequence(bytes(range(100, 120)), 0, 8) + zc.sequence(bytes(range(200, 206)))
    assert rc.plain_of(bad, 34) is None and rc.recode_form(bad, 34, 2) == bad
    assert rc.need(34, 31) == 48 + 64 and rc.need(34, 34) == 64 and rc.need(65536, 65536) == 65824


def test_the_planted_chunks_hold_both_classes():
    names, chunks = rc.planted()
    smaller, same, larger, raw_at_1 = rc.classes()
    assert len(set(chunks)) == len(chunks) and max(len(c) for c in chunks) == 65536
    assert smaller and same and raw_at_1 and set(raw_at_1) <= set(smaller)
    assert len(smaller) + len(same) + len(larger) == len(chunks)
    for i in smaller:
        assert rc.recode_form(rc.coded(chunks[i], 1), len(chunks[i]), 2) == rc.coded(chunks[i], 2)
    for i in same + larger:                                                                  # the reverse direction keeps them all
        assert rc.recode_form(rc.coded(chunks[i], 1), len(chunks[i]), 2) == rc.coded(chunks[i], 1)
    for i in range(len(chunks)):
        if i not in larger:
            assert rc.recode_form(rc.coded(chunks[i], 2), len(chunks[i]), 1) == rc.coded(chunks[i], 2)


@pytest.mark.parametrize("level", [1, 2])
def test_the_models_recoded_set_passes_the_hosts_check(level):
    import makisu_amd as M
    names, chunks = rc.planted()
    a, b = list(range(0, len(chunks), 2)), list(range(1, len(chunks), 2))
    store = rc.Store()
    for g in (a, b):
        store.add(*rc.zpack_at([chunks[i] for i in g], 3 - level))
    before = store.usage()
    info = store.recode(level)
    dig = np.frombuffer(b"".join(zc.sha(c) for c in chunks), dtype=np.uint8).reshape(-1, 32)
    entries, blob = store.cut(dig)
    assert M.zpack_check(blob, entries) is None
    assert [int(x) for x in entries["stored"]] == [min(len(rc.coded(c, 1)), len(rc.coded(c, 2))) for c in chunks]
    assert info["stored_after"] == int(entries["stored"].sum()) <= info["stored_before"] and info["n_undecodable"] == 0
    assert info["live_after"] == len(blob) == store.usage()["live_bytes"]
    if info["n_recoded"]:
        assert info["n_blobs_rewritten"] in (1, 2) and store.usage()["n_blobs"] == 3 - info["n_blobs_rewritten"]
        assert store.usage()["resident_bytes"] == before["resident_bytes"] - info["freed_bytes"] + rc.alloc(info["new_blob_bytes"])
    else:
        assert store.usage() == before
    again = store.recode(level)
    assert again["n_recoded"] == 0 and store.cut(dig)[1] == blob
