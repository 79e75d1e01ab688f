"""Chunk packs without a GPU: the header declares and tags the calls and the binding covers them, the two structs have the
header's layout, and mi_pack_check -- host logic, what the pulling side runs before it trusts a pack -- accepts the packs the
pure-Python model (pack_cases.py) builds and names the first entry that is wrong for each kind of damage."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pack_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")
NEW_CALLS = ["mi_batch_pack_chunks", "mi_pack_get_info", "mi_pack_entries", "mi_pack_read", "mi_pack_device", "mi_pack_free",
             "mi_pack_check", "mi_memfs_take_pack", "mi_copy_layer_chunks"]


def test_the_header_declares_and_tags_the_calls_and_the_binding_covers_them(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tags = dict((m.group(2), m.group(1)) for m in
                re.finditer(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b(mi_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name in NEW_CALLS:
        assert tags.get(name) == "MI_BLOCK", (name, tags.get(name))       # the core set stays as it is
        assert name in engine_lib._mi_symbols and hasattr(engine_lib, name), name
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M)        # additive: the version stays
    assert re.search(r"^#define\s+MI_PACK_VERIFY\s+0x1u", src, re.M) and re.search(r"^#define\s+MI_MEMFS_CHUNK_PACK\s+0x2u", src, re.M)
    import makisu_amd as M
    assert (M.PACK_VERIFY, M.MEMFS_CHUNK_PACK) == (1, 2)
    for attr in ("pack",):
        assert hasattr(M.Batch, attr)
    for attr in ("info", "entries", "read", "bytes", "close"):
        assert hasattr(M.Pack, attr), attr
    assert hasattr(M.MemFS, "take_pack") and callable(M.pack_check)


def test_pack_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of mi_pack_entry and mi_pack_info from a compiled probe against ctypes, numpy and the model's dtype"""
    import makisu_amd as M
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "makisu_mi.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mi_pack_entry), offsetof(mi_pack_entry, digest), offsetof(mi_pack_entry, offset),
         offsetof(mi_pack_entry, chunk_index), offsetof(mi_pack_entry, length), offsetof(mi_pack_entry, reserved));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mi_pack_info), offsetof(mi_pack_info, n_entries), offsetof(mi_pack_info, blob_bytes),
         offsetof(mi_pack_info, chunk_bytes), offsetof(mi_pack_info, alg), offsetof(mi_pack_info, verified),
         offsetof(mi_pack_info, ms_gather), offsetof(mi_pack_info, ms_verify));
  return 0; }''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    E, I = M.PackEntry, M.PackInfo
    want = [C.sizeof(E), E.digest.offset, E.offset.offset, E.chunk_index.offset, E.length.offset, E.reserved.offset,
            C.sizeof(I), I.n_entries.offset, I.blob_bytes.offset, I.chunk_bytes.offset, I.alg.offset, I.verified.offset,
            I.ms_gather.offset, I.ms_verify.offset]
    assert got == want and got[0] == 56
    for dt in (M.PACK_ENTRY_DTYPE, pc.ENTRY_DTYPE):
        assert dt.itemsize == 56 and [dt.fields[n][1] for n in ("digest", "offset", "chunk_index", "length", "reserved")] == got[1:6]


@pytest.fixture(scope="module")
def packs():
    """alg -> (entries, blob, rows) of a model-built pack: three files cut at random, every third row left out"""
    rng = np.random.default_rng(5)
    files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (5000, 1, 33333)]
    rows = pc.random_cut_rows(rng, files)
    select = [i % 3 != 1 for i in range(len(rows))]
    out = {}
    for alg in (pc.SHA256, pc.BLAKE2S):
        entries, blob = pc.model_pack(rows, files, select, alg)
        assert len(entries) > 60 and len(blob) == sum(pc.round16(int(e["length"])) for e in entries)
        out[alg] = (entries, blob)
    return out


@pytest.mark.parametrize("alg", [pc.SHA256, pc.BLAKE2S])
def test_pack_check_accepts_what_the_model_builds(engine_lib, packs, alg):
    import makisu_amd as M
    entries, blob = packs[alg]
    assert M.pack_check(blob, entries, alg) is None
    # a subset of the entries (the pulling side wants some chunks only) is sound too
    assert M.pack_check(blob, entries[::2], alg) is None
    # the empty pack, and a pack of one 1-byte chunk: a 16-byte unit with 15 zero bytes
    assert M.pack_check(b"", np.zeros(0, dtype=pc.ENTRY_DTYPE), alg) is None
    e1, b1 = pc.model_pack([(0, 0, 1)], [b"\x7f"], None, alg)
    assert b1 == b"\x7f" + b"\0" * 15 and M.pack_check(b1, e1, alg) is None


@pytest.mark.parametrize("alg", [pc.SHA256, pc.BLAKE2S])
def test_pack_check_names_the_first_bad_entry(engine_lib, packs, alg):
    import makisu_amd as M
    entries, blob = packs[alg]
    n = len(entries)
    k = next(i for i in range(n // 2, n) if int(entries[i]["length"]) % 16 and int(entries[i]["length"]) > 16)   # has pad bytes
    off, length = int(entries[k]["offset"]), int(entries[k]["length"])
    # a flipped data byte (first, middle, last byte of the chunk)
    for at in (off, off + length // 2, off + length - 1):
        bad = bytearray(blob)
        bad[at] ^= 0x01
        assert M.pack_check(bytes(bad), entries, alg) == k
    # a non-zero pad byte: the first and the last of the pad
    for at in (off + length, off + pc.round16(length) - 1):
        bad = bytearray(blob)
        assert bad[at] == 0
        bad[at] = 0x80
        assert M.pack_check(bytes(bad), entries, alg) == k
    # an entry off the 16-byte grid (its bytes and digest moved along: only the grid is wrong)
    e = entries.copy()
    e[k]["offset"] += 8
    assert M.pack_check(blob, e, alg) == k
    # overlapping entries: entry k begins inside entry k - 1 (and an entry out of order is the same finding)
    e = entries.copy()
    e[k]["offset"] = int(entries[k - 1]["offset"])
    assert M.pack_check(blob, e, alg) == k
    e = entries.copy()
    e[[k - 1, k]] = e[[k, k - 1]]
    assert M.pack_check(blob, e, alg) == k
    # an entry past the end: beginning there, and reaching there (its pad included)
    e = entries.copy()
    e[n - 1]["offset"] = len(blob) + 16
    assert M.pack_check(blob, e, alg) == n - 1
    assert M.pack_check(blob[:-16], entries, alg) == n - 1
    e = entries.copy()
    e[k]["length"] = 0xFFFFFFF0
    assert M.pack_check(blob, e, alg) == k
    # a wrong alg: the very first chunk does not hash to its digest; an unknown one is refused
    assert M.pack_check(blob, entries, 1 - alg) == 0
    with pytest.raises(M.MiError):
        M.pack_check(blob, entries, 7)
    bad = C.c_uint64(99)
    blob_a = np.frombuffer(blob, dtype=np.uint8)
    ent = np.ascontiguousarray(entries, dtype=M.PACK_ENTRY_DTYPE)
    assert engine_lib.mi_pack_check(blob_a.ctypes.data, len(blob), ent.ctypes.data, n, 7, C.byref(bad)) == -1
    assert engine_lib.mi_pack_check(blob_a.ctypes.data, len(blob), ent.ctypes.data, n, alg, None) == 0          # first_bad is optional
