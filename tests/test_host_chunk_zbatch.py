"""Zpacks coded straight from the arena, without a GPU: the header declares and tags the calls and the option and the binding
covers them, NULL arguments are refused without a device, mi_memfs_set_options takes the new option alone and refuses it beside
MI_MEMFS_CHUNK_PACK, the model (zbatch_cases.py: pack_cases' model handed to zpack_cases') is pinned by hand on three chunks, and
the planted inputs of tests/test_gpu_chunk_zbatch.py are what their names say."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pack_cases as pc
import zbatch_cases as bc
import zpack_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")
NEW_CALLS = ["mi_batch_zpack_chunks", "mi_memfs_take_zpack", "mi_zset_missing"]


def test_the_header_declares_and_tags_the_calls_and_the_binding_covers_them(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tags = dict((m.group(2), m.group(1)) for m in
                re.finditer(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b(mi_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name in NEW_CALLS:
        assert tags.get(name) == "MI_BLOCK", (name, tags.get(name))       # the core set stays as it is
        assert name in engine_lib._mi_symbols and hasattr(engine_lib, name), name
    assert tags.get("mi_memfs_set_options") == "MI_CORE"
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M)        # additive: the version stays
    assert engine_lib.mi_abi_version() == 6
    assert re.search(r"^#define\s+MI_MEMFS_CHUNK_ZPACK\s+0x4u", src, re.M)
    assert re.search(r"^#define\s+MI_MEMFS_CHUNK_PACK\s+0x2u", src, re.M)
    import makisu_amd as M
    assert M.MEMFS_CHUNK_ZPACK == 4 and "MEMFS_CHUNK_ZPACK" in M.__all__
    assert hasattr(M.Batch, "zpack") and hasattr(M.MemFS, "take_zpack") and hasattr(M.ZSet, "missing")
    import inspect
    assert "chunk_zpack" in inspect.signature(M.MemFS.set_options).parameters
    assert list(inspect.signature(M.Batch.zpack).parameters) == ["self", "select", "verify"]
    assert list(inspect.signature(M.ZSet.missing).parameters) == list(inspect.signature(M.PackSet.missing).parameters)


def test_null_arguments_are_refused_without_a_device(engine_lib):
    import makisu_amd as M
    L = engine_lib
    out = C.c_void_p(5)
    assert L.mi_batch_zpack_chunks(None, None, 0, 0, C.byref(out)) == -1
    assert L.mi_batch_zpack_chunks(None, None, 0, 0, None) == -1
    assert L.mi_memfs_take_zpack(None, C.byref(out)) == -1 and L.mi_memfs_take_zpack(None, None) == -1
    info = M.WantInfo()
    info.n_rows = info.n_want = 7
    assert L.mi_zset_missing(None, None, None, 0, None, None, 0, C.byref(info)) == -1
    assert (info.n_rows, info.n_want) == (0, 0)                            # zeroed before anything is looked at
    assert L.mi_zset_missing(None, None, None, 0, None, None, 0, None) == -1


def test_set_options_takes_the_option_alone_and_refuses_it_beside_the_plain_pack(engine_lib, tmp_path):
    import makisu_amd as M
    L = engine_lib
    root = tmp_path / "root"
    root.mkdir()
    with M.MemFS(str(root)) as fs:
        assert L.mi_memfs_set_options(fs._h, 0x4) == 0
        assert L.mi_memfs_set_options(fs._h, 0x4 | 0x1) == 0
        assert L.mi_memfs_set_options(fs._h, 0x2 | 0x4) == -1
        assert b"exclude each other" in L.mi_memfs_error(fs._h)
        assert L.mi_memfs_set_options(fs._h, 0x8) == -1
        assert L.mi_memfs_set_options(fs._h, 0x2) == 0                     # the plain pack's option as ever
        with pytest.raises(M.MiError) as ei:
            fs.set_options(chunk_pack=True, chunk_zpack=True)
        assert ei.value.code == -1
        fs.set_options(chunk_zpack=True)
        out = C.c_void_p(5)
        assert L.mi_memfs_take_zpack(fs._h, C.byref(out)) == -6 and out.value is None      # no commit yet
        assert b"mi_memfs_take_zpack" in L.mi_memfs_error(fs._h)
        fs.commit_layer(must_scan=True)                                    # ctx == NULL: the reference's commit, as ever -- no zpack
        assert L.mi_memfs_take_zpack(fs._h, C.byref(out)) == -6


def test_the_model_pinned_by_hand_on_three_chunks():
    """one file cut into a raw chunk of 40 bytes (no four bytes repeat), forty 9s (coded: one literal, a match of 34 at offset 1,
    the last five literals -- 11 bytes) and five bytes (under 13: always raw)"""
    raw40, nines, hello = bytes(range(40, 80)), bytes([9]) * 40, b"hello"
    stream = bytes([0x1F, 9, 1, 0, 15, 0x50, 9, 9, 9, 9, 9])
    assert zc.compress_chunk(nines) == stream and zc.compress_chunk(raw40) == raw40 and zc.compress_chunk(hello) == hello
    assert zc.lz4_block_decode(stream, 40) == nines
    files = [raw40 + nines + hello]
    rows = [(0, 0, 40), (0, 40, 40), (0, 80, 5)]
    entries, blob = bc.model_zpack(rows, files)
    assert entries["chunk_index"].tolist() == [0, 1, 2] and entries["offset"].tolist() == [0, 48, 64]
    assert entries["length"].tolist() == [40, 40, 5] and entries["stored"].tolist() == [40, 11, 5]
    assert [bytes(x) for x in entries["digest"]] == [zc.sha(raw40), zc.sha(nines), zc.sha(hello)]
    assert blob == raw40 + bytes(8) + stream + bytes(5) + hello + bytes(11) and len(blob) == 80
    assert bc.kinds(entries).tolist() == [False, True, False] and bc.tiles_with_both_kinds(entries) == [0]
    entries, blob = bc.model_zpack(rows, files, select=[0x80, 0, 1])       # flags are non-zero bytes; chunk_index is the ROW
    assert entries["chunk_index"].tolist() == [0, 2] and entries["offset"].tolist() == [0, 48] and blob == raw40 + bytes(8) + hello + bytes(11)
    entries, blob = bc.model_zpack(rows, files, select=[0, 0, 0])
    assert len(entries) == 0 and blob == b""
    import makisu_amd as M
    assert M.zpack_check(*reversed(bc.model_zpack(rows, files))) is None
    e2, _ = bc.model_zpack(rows, files, alg=pc.BLAKE2S)
    assert e2["stored"].tolist() == [40, 11, 5] and bytes(e2["digest"][0]) != zc.sha(raw40)


def test_the_planted_inputs_are_what_their_names_say():
    data = bc.mixed_file()
    assert len(data) == 1 << 20
    for k in range(0, 8):
        piece = data[k * bc.PIECE:(k + 1) * bc.PIECE]
        assert (len(zc.compress_chunk(piece)) < len(piece)) == (k % 2 == 1), k     # random pieces stay raw, text pieces are coded
    files = bc.planted_files()
    planted = [c for _, c, _ in zc.planted_chunks()]
    assert files[:-1] == planted and len(files[-1]) == 7 + sum(map(len, planted)) and files[-1][7:7 + len(planted[0])] == planted[0]
    assert min(map(len, planted)) == 1 and max(map(len, planted)) == 65536
