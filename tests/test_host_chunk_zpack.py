"""The compressed packs without a GPU: the header declares and tags the calls and the binding covers them, mi_zpack_entry and
mi_zpack_info have the header's layout, the model (zpack_cases.py) writes blocks that an independent LZ4 decoder and the real
mi_zpack_check accept, every row of the malformed table is refused with the right entry named, and the model's parse keeps the
ratio DESIGN.md 4.9 states against zlib level 1."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import pack_cases as pc
import zpack_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")
NEW_CALLS = ["mi_pack_compress", "mi_zpack_get_info", "mi_zpack_entries", "mi_zpack_read", "mi_zpack_free", "mi_packset_add_zblob",
             "mi_packset_add_zpack", "mi_zpack_check"]


def test_the_header_declares_and_tags_the_calls_and_the_binding_covers_them(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tags = dict((m.group(2), m.group(1)) for m in
                re.finditer(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b(mi_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name in NEW_CALLS:
        assert tags.get(name) == "MI_BLOCK", (name, tags.get(name))       # the core set stays as it is
        assert name in engine_lib._mi_symbols and hasattr(engine_lib, name), name
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M)        # additive: the version stays
    assert engine_lib.mi_abi_version() == 6
    assert re.search(r"^#define\s+MI_ZPACK_VERIFY\s+0x1u", src, re.M)
    import makisu_amd as M
    assert M.ZPACK_VERIFY == 1
    assert hasattr(M.Pack, "compress") and hasattr(M.PackSet, "add_zblob") and hasattr(M.PackSet, "add_zpack")
    for attr in ("info", "entries", "read"):
        assert hasattr(M.ZPack, attr), attr
    for name in ("ZPACK_VERIFY", "ZPackInfo", "ZPack", "zpack_check"):
        assert name in M.__all__, name


def test_entry_and_info_layouts_match_the_header(tmp_path):
    """sizeof / offsetof from a compiled probe against ctypes and against the model's dtype"""
    import makisu_amd as M
    e_fields = ["digest", "offset", "chunk_index", "length", "stored"]
    i_fields = ["n_entries", "blob_bytes", "chunk_bytes", "stored_bytes", "n_raw", "alg", "verified", "ms_encode", "ms_compact", "ms_verify", "ms_decode"]
    lines = ['printf("%zu %zu\\n", sizeof(mi_zpack_entry), sizeof(mi_zpack_info));']
    lines += ['printf("%%zu\\n", offsetof(mi_zpack_entry, %s));' % f for f in e_fields]
    lines += ['printf("%%zu\\n", offsetof(mi_zpack_info, %s));' % f for f in i_fields]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "makisu_mi.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    E, I = M.ZPackEntry, M.ZPackInfo
    assert got == [C.sizeof(E), C.sizeof(I)] + [getattr(E, f).offset for f in e_fields] + [getattr(I, f).offset for f in i_fields]
    assert got[:2] == [56, 80] and [n for n, _ in E._fields_] == e_fields and [n for n, _ in I._fields_] == i_fields
    assert M.ZPACK_ENTRY_DTYPE.itemsize == zc.ZENTRY_DTYPE.itemsize == M.PACK_ENTRY_DTYPE.itemsize == 56
    for f in e_fields:
        assert M.ZPACK_ENTRY_DTYPE.fields[f][1] == zc.ZENTRY_DTYPE.fields[f][1] == got[2 + e_fields.index(f)], f


@pytest.fixture(scope="module")
def mixed_pack_chunks():
    rng = np.random.default_rng(81)
    design = open(os.path.join(ROOT, "DESIGN.md"), "rb").read()
    return [design[:8192], rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), bytes(65536), b"abc" * 1000, b"x", b"y" * 12, b"z" * 13,
            design[20000:20100], zc.text_like(4095, 3), design[30000:30000 + 65536]]


def test_the_models_blocks_decode_with_an_independent_decoder_and_pass_the_real_check(mixed_pack_chunks):
    import makisu_amd as M
    chunks = mixed_pack_chunks
    for c in chunks:
        stored = zc.compress_chunk(c)
        assert len(stored) <= len(c)
        if len(stored) < len(c):
            assert zc.lz4_block_decode(stored, len(c)) == c and len(stored) < len(c) - (len(c) >> 4) and len(c) >= 13
            seqs = zc.parse(c)
            assert seqs[-1][0] >= 5 and seqs[-1][1] is None                                    # the last 5 bytes are literals
            at = 0
            for lit, off, mlen in seqs[:-1]:
                at += lit
                assert at <= len(c) - 12 and 1 <= off <= 65535 and off <= at and mlen >= 4 and at + mlen <= len(c) - 5
                at += mlen
        else:
            assert stored == c
    assert [len(zc.compress_chunk(c)) < len(c) for c in chunks] == [True, False, True, True, False, False, True, False, True, True]
    for alg in (pc.SHA256, pc.BLAKE2S):
        entries, blob = zc.pack_of(chunks, alg)
        zentries, zblob = zc.model_compress(entries, blob)
        assert M.zpack_check(zblob, zentries, alg=alg) is None
        assert M.zpack_check(zblob, zentries, alg=1 - alg) == 0                                # the other algorithm's digests
        assert len(zblob) == sum(zc.round16(int(s)) for s in zentries["stored"]) < len(blob) // 2
        assert zentries["offset"].tolist() == np.concatenate([[0], np.cumsum((zentries["stored"].astype(np.int64) + 15) // 16 * 16)[:-1]]).tolist()
        # expanded again it is the plain pack, which the existing check accepts
        plain_e, plain_b = zc.model_expand(zentries, zblob)
        assert plain_b == blob and pc.same_entries(plain_e, entries) and M.pack_check(plain_b, plain_e, alg=alg) is None
        # a flipped plain byte in a raw entry, a flipped literal in a coded one: the digest names the entry
        for k in (1, 0):
            hurt = bytearray(zblob)
            hurt[int(zentries["offset"][k]) + 2] ^= 1
            assert M.zpack_check(bytes(hurt), zentries, alg=alg) == k
    assert M.zpack_check(b"", np.zeros(0, dtype=zc.ZENTRY_DTYPE)) is None
    with pytest.raises(M.MiError):
        M.zpack_check(b"", np.zeros(0, dtype=zc.ZENTRY_DTYPE), alg=7)


def test_every_row_of_the_malformed_table_is_refused_with_its_entry_named():
    import makisu_amd as M
    table = zc.malformed_zpacks()
    assert [name for name, _, _ in zc.malformed_table()] == [
        "offset 0", "offset one beyond the bytes produced", "literal run one byte past the stored span",
        "length extension cut off by the span's end", "match one byte past length", "output one byte short", "one stored byte left over",
        "non-zero pad", "stored > length", "stored == 0", "overlap", "off-grid offset"]
    assert len(table) == 24
    for name, entries, blob, bad in table:
        assert M.zpack_check(blob, entries) == bad, name
    # the streams are wrong for the reason their names give: the independent decoder refuses the first seven too, and the good
    # stream they were made from decodes
    assert zc.lz4_block_decode(zc.GOOD_STREAM, 34) == zc.GOOD_PLAIN
    good_e, good_b = zc.build_zpack([zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN)])
    assert M.zpack_check(good_b, good_e) is None and len(good_b) == 32
    for name, specs, _ in zc.malformed_table()[:7]:
        with pytest.raises(ValueError):
            zc.lz4_block_decode(specs[0]["stream"], specs[0]["length"])
    # a decode failure behind a digest failure is the one named: the order the device path finds them in
    rng = np.random.default_rng(82)
    raw = rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    specs = [zc._entry(raw, 40, bytes(40)), zc._entry(zc.GOOD_STREAM, 35)]                     # entry 0: wrong digest; entry 1: short
    entries, blob = zc.build_zpack(specs)
    assert M.zpack_check(blob, entries) == 1
    entries, blob = zc.build_zpack(specs[:1])
    assert M.zpack_check(blob, entries) == 0


def test_null_arguments_are_refused_without_a_ctx(engine_lib):
    L = engine_lib
    out, bad = C.c_void_p(5), C.c_uint64(7)
    assert L.mi_pack_compress(None, 0, C.byref(out)) == -1 and out.value is None
    assert L.mi_pack_compress(None, 0, None) == -1
    assert L.mi_zpack_get_info(None, None) == -1 and L.mi_zpack_entries(None, None, 0) == -1 and L.mi_zpack_read(None, 0, None, 0) == -1
    assert L.mi_packset_add_zblob(None, None, 0, None, 0, 0, C.byref(bad)) == -1 and bad.value == 0
    assert L.mi_packset_add_zpack(None, None, 0) == -1
    assert L.mi_zpack_check(None, 16, None, 0, 0, C.byref(bad)) == -1
    L.mi_zpack_free(None)


def test_the_planted_chunks_have_the_sequences_they_were_planted_with():
    cases = zc.planted_chunks()
    by_name = {name: (chunk, want) for name, chunk, want in cases}
    assert len({c for _, c, _ in cases}) == len(cases)                                          # distinct: a set holds each
    for name, chunk, want in cases:
        if want is not None:
            assert zc.parse(chunk) == want, name
            assert sum(s[0] + (s[2] or 0) for s in want) == len(chunk), name
    assert sorted({len(c) for n, c, _ in cases if n.startswith(("random", "text"))}) == zc.LENGTHS
    for run in zc.LITERAL_RUNS:                                                                 # the run, in front of a match, off the 64-grid
        assert by_name["literal run %d" % run][1][1] == (run, 108 + run - 20, 8)
    for m in zc.MATCH_LENGTHS:
        assert by_name["match length %d" % m][1][0] == (300, 300, m)
    for off in zc.OFFSETS:
        assert by_name["offset %d" % off][1][0] == (128, off, 40)
    chunk, want = by_name["match to n - 5"]
    assert want[0][0] + want[0][2] == len(chunk) - 5 and chunk[-5:] == chunk[105:110]         # the source goes on: the limit ended it
    assert by_name["match at n - 12"][1][1] == (78, 281, 7) and by_name["match at n - 11"][1] == [(150, 120, 60), (90, None, None)]
    assert by_name["candidate in lane 63"][1][0] == (191, 181, 8)
    chunk, want = by_name["two positions in one slot"]
    assert chunk[5:9] == chunk[40:44] == chunk[150:154] and zc.hash_of(chunk, 5) == zc.hash_of(chunk, 40) and want[0] == (150, 110, 4)
    for n, stored in ((150, 150), (151, 141)):
        chunk, want = by_name["block of 141 for %d" % n]
        block = zc.encode(chunk, want)
        assert len(block) == 141 and (len(block) < n - (n >> 4)) == (stored == 141) and len(zc.compress_chunk(chunk)) == stored
    # extension bytes at their edges: 14 none, 15 one byte of 0, 270 two bytes
    assert zc.sequence(bytes(14))[0] == 0xE0 and zc.sequence(bytes(15))[:2] == b"\xf0\x00" and zc.sequence(bytes(270))[:3] == b"\xf0\xff\x00"
    assert zc.sequence(b"", 1, 18)[0] == 14 and zc.sequence(b"", 1, 19) == b"\x0f\x01\x00\x00" and zc.sequence(b"", 1, 274)[3:] == b"\xff\x00"


def test_the_models_parse_keeps_the_ratio_the_design_states():
    """over 8 KiB pieces (the first 1.5 MB of each file) the model stores at most 1.5 x what zlib level 1
    stores for the same pieces -- the starting parse measured 1.31 to 1.43; more than 5 % over the worst of that means matches
    are being lost -- and it saves at least a quarter of each text file."""
    texts = ["SURVEY.md", "oracle/mi_oracle.c", "makisu_amd/csrc/gear_cdc.hip"]
    for rel in texts + ["makisu_amd/libmakisu_mi.so"]:
        data = open(os.path.join(ROOT, rel), "rb").read()[:1_500_000]
        pieces = [data[i:i + 8192] for i in range(0, len(data), 8192)]
        model = sum(len(zc.compress_chunk(p)) for p in pieces)
        yard = sum(len(zlib.compress(p, 1)) for p in pieces)
        print("%s: %d bytes, model %.4f of the input, %.4f x zlib level 1" % (rel, len(data), model / len(data), model / yard))
        assert model <= 1.5 * yard, (rel, model, yard)
        if rel in texts:
            assert model <= 0.75 * len(data), (rel, model, len(data))
