"""The restore without a GPU: the header declares and tags the calls and the binding covers them, the two structs have the
header's layout, the pure-Python restore model (restore_cases.py) undoes the pack model (pack_cases.py) on rows cut at random,
its count of joined units is what a byte-by-byte count gives, and NULL arguments are refused where no ctx is needed to say so."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import pack_cases as pc
import restore_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")
NEW_CALLS = ["mi_packset_create", "mi_packset_add_blob", "mi_packset_add_pack", "mi_packset_get_info", "mi_packset_free",
             "mi_batch_add_recipes"]


def test_the_header_declares_and_tags_the_calls_and_the_binding_covers_them(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tags = dict((m.group(2), m.group(1)) for m in
                re.finditer(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b(mi_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name in NEW_CALLS:
        assert tags.get(name) == "MI_BLOCK", (name, tags.get(name))       # the core set stays as it is
        assert name in engine_lib._mi_symbols and hasattr(engine_lib, name), name
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M)        # additive: the version stays
    assert engine_lib.mi_abi_version() == 6
    assert re.search(r"^#define\s+MI_PACKSET_VERIFY\s+0x1u", src, re.M) and re.search(r"^#define\s+MI_RECIPE_VERIFY\s+0x1u", src, re.M)
    import makisu_amd as M
    assert (M.PACKSET_VERIFY, M.RECIPE_VERIFY) == (1, 1)
    assert hasattr(M.Engine, "packset") and hasattr(M.Batch, "add_recipes")
    for attr in ("add_blob", "add_pack", "info", "close", "__enter__", "__exit__"):
        assert hasattr(M.PackSet, attr), attr
    for name in ("PackSet", "PackSetInfo", "RecipeStats", "PACKSET_VERIFY", "RECIPE_VERIFY"):
        assert name in M.__all__, name


def test_restore_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of mi_packset_info and mi_recipe_stats from a compiled probe against ctypes"""
    import makisu_amd as M
    info = ["n_packs", "n_entries", "n_digests", "blob_bytes", "alg", "reserved", "ms_upload", "ms_verify", "ms_insert"]
    stats = ["n_files", "n_rows", "bytes", "n_joined_units", "ms_resolve", "ms_assemble", "ms_verify"]
    lines = ['printf("%zu\\n", sizeof(mi_packset_info));'] + ['printf("%%zu\\n", offsetof(mi_packset_info, %s));' % f for f in info] + \
            ['printf("%zu\\n", sizeof(mi_recipe_stats));'] + ['printf("%%zu\\n", offsetof(mi_recipe_stats, %s));' % f for f in stats]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "makisu_mi.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    I, S = M.PackSetInfo, M.RecipeStats
    want = [C.sizeof(I)] + [getattr(I, f).offset for f in info] + [C.sizeof(S)] + [getattr(S, f).offset for f in stats]
    assert got == want and got[0] == 64 and got[len(info) + 1] == 56
    assert [n for n, _ in I._fields_] == info and [n for n, _ in S._fields_] == stats


def _joined_by_bytes(recipes):
    """the definition, byte by byte: a unit of a file (which begins on a 256-byte boundary) that bytes of two rows fall into"""
    total = 0
    for _, lens in recipes:
        owner = np.repeat(np.arange(len(lens)), np.asarray(lens, dtype=np.int64))
        for u in range(0, len(owner), 16):
            total += len(set(owner[u:u + 16].tolist())) > 1
    return total


def test_the_restore_model_undoes_the_pack_model():
    rng = np.random.default_rng(6)
    files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (5000, 0, 1, 33333, 16, 257)]
    for lo, hi in ((1, 700), (1, 40), (1, 3)):
        rows = pc.random_cut_rows(rng, files, lo, hi)
        for alg in (pc.SHA256, pc.BLAKE2S):
            recipes = [rc.recipe_of(rows, files, f, alg) for f in range(len(files))]
            assert [len(r[1]) for r in recipes][1] == 0                    # the empty file: a recipe of no rows
            # one pack of every row; two packs of the even and the odd rows; the second of them added twice
            whole = pc.model_pack(rows, files, None, alg)
            even = pc.model_pack(rows, files, [i % 2 == 0 for i in range(len(rows))], alg)
            odd = pc.model_pack(rows, files, [i % 2 == 1 for i in range(len(rows))], alg)
            assert rc.model_restore([whole], recipes) == files
            assert rc.model_restore([even, odd, odd], recipes) == files
            # recipes may reuse chunks and come in any order
            again = [recipes[3], recipes[0], recipes[3]]
            assert rc.model_restore([odd, even], again) == [files[3], files[0], files[3]]
            assert rc.joined_units(recipes) == _joined_by_bytes(recipes)
    # a digest no pack holds; a digest held with another length
    rows = pc.random_cut_rows(rng, files, 50, 700)
    recipes = [rc.recipe_of(rows, files, f) for f in range(len(files))]
    even = pc.model_pack(rows, files, [i % 2 == 0 for i in range(len(rows))])
    try:
        rc.model_restore([even], recipes)
        raise AssertionError("a recipe over half a store came back")
    except KeyError:
        pass
    dig, lens = recipes[0]
    try:
        rc.model_restore([pc.model_pack(rows, files)], [(dig, lens + 1)])
        raise AssertionError("a wrong length came back")
    except ValueError:
        pass


def test_the_issues_tiny_rows_have_the_mix_the_gpu_test_rests_on():
    """tests/test_gpu_chunk_restore.py walks the joined path with this input: here, without a GPU, what it consists of"""
    import hashlib
    rng = np.random.default_rng(41)
    data = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    rows = pc.random_cut_rows(rng, [data], 1, 40)
    assert len(rows) == 3205
    assert rc.unit_cover_histogram([n for _, _, n in rows]) == {1: 1645, 2: 1980, 3: 412, 4: 53, 5: 5, 6: 1}
    assert len({hashlib.sha256(data[o:o + n]).digest() for _, o, n in rows}) == 3181
    assert rc.unit_cover_histogram([1] * 64 + [15, 16, 17, 31, 32, 33, 1]) == {1: 6, 2: 4, 16: 4}


def test_null_arguments_are_refused_without_a_ctx(engine_lib):
    L = engine_lib
    out, bad = C.c_void_p(), C.c_uint64(7)
    assert L.mi_packset_create(None, 0, C.byref(out)) == -1
    assert L.mi_packset_add_blob(None, None, 0, None, 0, 0, C.byref(bad)) == -1
    assert L.mi_packset_add_pack(None, None, 0) == -1
    assert L.mi_packset_get_info(None, None) == -1
    assert L.mi_batch_add_recipes(None, None, 0, None, None, None, None, 0, None) == -1
    assert L.mi_packset_free(None) is None                                 # NULL is fine, as for mi_pack_free
