"""Zpack level 2 without a GPU: the header defines MI_ZPACK_LEVEL2 and MI_MEMFS_ZPACK_LEVEL2 and the binding exports them, every
block the level-2 model (zpack2_cases.py) makes for its planted chunks decodes with the independent decoder and passes the real
mi_zpack_check, every planted chunk has the sequence list it was planted to have, level 1's model is what it was on level 1's
planted chunks, and over the project's own files level 2 stores less than level 1.  There is NO per-chunk promise: a single
chunk may store more at level 2 (tools/zpack_model_ratio.py, profiles/chunk_zpack_l2_model.txt hold the corpus figures)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import pack_cases as pc
import zpack2_cases as z2
import zpack_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")


@pytest.fixture(scope="module")
def cases():
    return z2.planted_chunks2()


def test_the_header_defines_the_flags_and_the_binding_exports_them(engine_lib):
    import makisu_amd as M
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^#define\s+MI_ZPACK_LEVEL2\s+0x4u", src, re.M) and re.search(r"^#define\s+MI_ZPACK_VERIFY\s+0x1u", src, re.M)
    assert re.search(r"^#define\s+MI_MEMFS_ZPACK_LEVEL2\s+0x10u", src, re.M) and re.search(r"^#define\s+MI_MEMFS_CHUNK_ZPACK\s+0x4u", src, re.M)
    assert M.ZPACK_LEVEL2 == 4 and M.MEMFS_ZPACK_LEVEL2 == 0x10 and M.ZPACK_VERIFY == 1
    for name in ("ZPACK_LEVEL2", "MEMFS_ZPACK_LEVEL2"):
        assert name in M.__all__, name
    assert inspect.signature(M.Pack.compress).parameters["level"].default == 1
    assert list(inspect.signature(M.Batch.zpack_at).parameters) == ["self", "level", "select", "verify"]
    assert inspect.signature(M.MemFS.set_options).parameters["zpack_level"].default == 1
    for bad in (0, 3, None):
        with pytest.raises(ValueError):
            M._zpack_level_flag(bad)
    # additive: no struct changes size, the version stays
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M) and engine_lib.mi_abi_version() == 6
    assert C.sizeof(M.ZPackEntry) == 56 and C.sizeof(M.ZPackInfo) == 80
    # the sentence the issue changes, and the calls that take no level
    assert "pure function of its bytes and the level" in text and "pure function of its bytes (" not in text
    assert "mi_zset_zpack, mi_zset_missing, mi_zset_prune and mi_batch_add_zrecipes take no level flag" in " ".join(text.split()).replace(" * ", " ")
    # the handle takes the option beside the zpack option, alone, and still refuses the bit behind it
    root = os.path.join(ROOT, "tests")
    with M.MemFS(root) as fs:
        L = engine_lib
        assert L.mi_memfs_set_options(fs._h, 0x4 | 0x10) == 0 and L.mi_memfs_set_options(fs._h, 0x10) == 0
        assert L.mi_memfs_set_options(fs._h, 0x2 | 0x4 | 0x10) == -1 and L.mi_memfs_set_options(fs._h, 0x20) == -1
        fs.set_options(chunk_zpack=True, zpack_level=2)
        fs.set_options()


def test_every_planted_block_decodes_and_the_zpack_passes_the_real_check(cases):
    import makisu_amd as M
    chunks = [c for _, c, _ in cases]
    assert len(set(chunks)) == len(chunks)                                                     # distinct: a set holds each
    for name, c, _ in cases:
        stored = z2.compress_chunk2(c)
        if len(stored) < len(c):
            assert zc.lz4_block_decode(stored, len(c)) == c and len(stored) < len(c) - (len(c) >> 4) and len(c) >= 13, name
            at = 0
            seqs = z2.parse2(c)
            assert seqs[-1][0] >= 5 and seqs[-1][1] is None, name                              # the last 5 bytes are literals
            for lit, off, mlen in seqs[:-1]:
                at += lit
                assert at <= len(c) - 12 and 1 <= off <= 65535 and off <= at and mlen >= 4 and at + mlen <= len(c) - 5, name
                at += mlen
        else:
            assert stored == c, name
    for alg in (pc.SHA256, pc.BLAKE2S):
        entries, blob = zc.pack_of(chunks, alg)
        zentries, zblob = z2.model_compress2(entries, blob)
        assert M.zpack_check(zblob, zentries, alg=alg) is None
        plain_e, plain_b = zc.model_expand(zentries, zblob)
        assert plain_b == blob and pc.same_entries(plain_e, entries)
    # a mixed pack at both levels: two stored forms of the same chunks, either passes the check
    design = open(os.path.join(ROOT, "DESIGN.md"), "rb").read()
    entries, blob = zc.pack_of([design[:8192], design[20000:20000 + 65536], zc.text_like(4095, 3)])
    one, two = zc.model_compress(entries, blob), z2.model_compress2(entries, blob)
    assert M.zpack_check(one[1], one[0]) is None and M.zpack_check(two[1], two[0]) is None
    assert int(two[0]["stored"].sum()) < int(one[0]["stored"].sum()) and two[1] != one[1]


def test_the_planted_chunks_have_the_sequences_they_were_planted_with(cases):
    by = {name: (chunk, want) for name, chunk, want in cases}
    for name, chunk, want in cases:
        if want is not None:
            assert z2.parse2(chunk) == want, name
            assert sum(s[0] + (s[2] or 0) for s in want) == len(chunk), name
    assert sorted({len(c) for n, c, _ in cases if n.startswith(("random", "text"))}) == zc.LENGTHS
    for run in zc.LITERAL_RUNS:
        assert by["literal run %d" % run][1][1] == (run, 108 + run - 20, 8)
    for m in zc.MATCH_LENGTHS:
        assert by["match length %d" % m][1][0] == (300, 300, m)
    for off in zc.OFFSETS:
        assert by["offset %d" % off][1][0] == (128, off, 40)
    # the two tables
    c, want = by["the 8-byte table's candidate is longer"]
    assert c[40:44] == c[10:14] == c[150:154] and c[44] != c[154] and want[0] == (150, 140, 20)
    assert z2.parse2(c, two_tables=False, choose=False, backward=False)[0] == (150, 110, 4)    # T4 alone holds 40
    c, want = by["the 4-byte table's candidate is longer"]
    assert c[8:12] == c[30:34] == c[150:154] and z2.hash8_of(c, 8) == z2.hash8_of(c, 150) != z2.hash8_of(c, 30) and want[0] == (150, 120, 7)
    c, want = by["equal lengths: the greater source"]
    assert c[8:12] == c[30:34] == c[150:154] and c[12] != c[154] and c[34] != c[154] and want[0] == (150, 120, 4)
    # the choice
    c, want = by["a later lane inside the first's match wins"]
    assert c[150:156] == c[10:16] and c[152:182] == c[30:60] and want[0] == (152, 122, 30)
    assert z2.parse2(c, choose=False)[0] == (150, 140, 6)
    assert by["a score tie goes to the lower lane"][1][:2] == [(150, 140, 6), (0, 122, 4)]
    assert by["a later lane beyond the first's match does not win"][1][:2] == [(150, 140, 6), (0, 126, 30)]
    for m in z2.CAP_LENGTHS:
        assert by["match length %d, the cap is %d" % (m, z2.CAP)][1][0] == (300, 290, m)
    assert z2.CAP_LENGTHS == [67, 68, 131, 132, 133]
    # backwards
    c, want = by["backwards to a differing byte"]
    assert c[110:140] == c[70:100] and c[109] != c[69] and want[0] == (110, 40, 30) and z2.parse2(c, backward=False)[0] == (128, 40, 12)
    c, want = by["backwards to the anchor: literal run 0"]
    assert want[1] == (0, 128, 30) and c[147] == c[19] and z2.parse2(c, backward=False)[1] == (1, 128, 29)
    c, want = by["backwards stops at source position 0"]
    assert want[0] == (100, 100, 30) and c[99] == c[-1]
    for k in z2.PERIODS:
        c, want = by["period %d, backwards" % k]
        assert want[0] == (120, k, 48) and z2.parse2(c, backward=False)[0] == (128, k, 40)
    # dense insertion: level 1 does not find the source inside the earlier match, level 2 does
    c, want = by["a source inside an earlier match"]
    assert c[300:320] == c[225:245] and want[1] == (72, 75, 20) and zc.parse(c)[1] == (75, 75, 17)
    assert z2.parse2(c, dense=False, backward=False)[1] == (75, 75, 17)                        # (going backwards from 303 makes up for it)
    c, want = by["a longer source inside an earlier match"]
    assert c[300:316] == c[215:231] and c[215:228] == c[97:110] and want[1] == (72, 85, 16)
    assert z2.parse2(c, dense=False)[1] == zc.parse(c)[1] == (72, 203, 13)                     # the older source, 13 long
    # the ends and the raw rule
    c, want = by["match to n - 5"]
    assert want[0][0] + want[0][2] == len(c) - 5 and c[-5:] == c[105:110]
    assert by["match at n - 12"][1][1] == (78, 281, 7) and by["match at n - 11"][1] == [(150, 120, 60), (90, None, None)]
    assert by["zeros"][0] == bytes(65536) and len(z2.compress_chunk2(bytes(65536))) == 267
    for n, stored in ((150, 150), (151, 141)):
        c, want = by["block of 141 for %d" % n]
        block = zc.encode(c, want)
        assert len(block) == 141 and (len(block) < n - (n >> 4)) == (stored == 141) and len(z2.compress_chunk2(c)) == stored


def test_level_1s_model_is_what_it_was_on_level_1s_planted_chunks():
    """zpack_cases.py is not touched: its planted chunks still have the sequence lists they were planted with, their stored
    sizes are the recorded ones, and level 2's frame with every element switched off IS level 1's parse"""
    cases1 = zc.planted_chunks()
    for name, chunk, want in cases1:
        if want is not None:
            assert zc.parse(chunk) == want, name
        if len(chunk) >= zc.MIN_CHUNK:
            assert z2.parse2(chunk, two_tables=False, choose=False, backward=False, dense=False) == zc.parse(chunk), name
    stored = {name: len(zc.compress_chunk(c)) for name, c, _ in cases1}
    assert stored["zeros"] == 267 and stored["period 3"] == 24 and stored["block of 141 for 150"] == 150 and stored["block of 141 for 151"] == 141
    assert stored["random 65536"] == 65536 and stored["text 13"] == 13


def test_level_2_stores_less_than_level_1_over_the_projects_own_files():
    """The condition of DESIGN.md 4.14 -- level 2's TOTAL below level 1's -- on files every checkout has (the corpus of the recorded
    figures is the box's /usr/lib: tools/zpack_model_ratio.py).  8 KiB pieces of the first 128 KiB of each."""
    one = two = 0
    for rel in ("makisu_amd/libmakisu_mi.so", "SURVEY.md", "makisu_amd/csrc/gear_cdc.hip"):
        data = open(os.path.join(ROOT, rel), "rb").read()[:131072]
        pieces = [data[i:i + 8192] for i in range(0, len(data), 8192)]
        a, b = sum(len(zc.compress_chunk(p)) for p in pieces), sum(len(z2.compress_chunk2(p)) for p in pieces)
        print("%s: %d bytes, level 1 %d, level 2 %d (%.4f)" % (rel, len(data), a, b, b / a))
        assert b < a, rel
        one, two = one + a, two + b
    assert two < one
