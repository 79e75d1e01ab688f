"""The chunk fetch without a GPU: the header declares and tags the two calls and the binding covers them, mi_want_info has the
header's layout, the pure-Python model (fetch_cases.py) cuts packs that the real mi_pack_check accepts and that restore the
files, NULL arguments are refused where no ctx is needed to say so, and the planted inputs of tests/test_gpu_chunk_fetch.py
have the properties those tests rest on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import fetch_cases as fc
import pack_cases as pc
import restore_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")
NEW_CALLS = ["mi_packset_missing", "mi_packset_pack"]


def test_the_header_declares_and_tags_the_calls_and_the_binding_covers_them(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tags = dict((m.group(2), m.group(1)) for m in
                re.finditer(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b(mi_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name in NEW_CALLS:
        assert tags.get(name) == "MI_BLOCK", (name, tags.get(name))       # the core set stays as it is
        assert name in engine_lib._mi_symbols and hasattr(engine_lib, name), name
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M)        # additive: the version stays
    assert engine_lib.mi_abi_version() == 6
    assert re.search(r"^#define\s+MI_SUBPACK_VERIFY\s+0x1u", src, re.M)
    import makisu_amd as M
    assert M.SUBPACK_VERIFY == 1
    for attr in ("missing", "pack"):
        assert hasattr(M.PackSet, attr), attr
    for name in ("WantInfo", "SUBPACK_VERIFY"):
        assert name in M.__all__, name


def test_want_info_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of mi_want_info from a compiled probe against ctypes"""
    import makisu_amd as M
    fields = ["n_rows", "n_distinct", "n_held", "n_want", "held_bytes", "want_bytes", "ms_resolve"]
    lines = ['printf("%zu\\n", sizeof(mi_want_info));'] + ['printf("%%zu\\n", offsetof(mi_want_info, %s));' % f for f in fields]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "makisu_mi.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    W = M.WantInfo
    assert got == [C.sizeof(W)] + [getattr(W, f).offset for f in fields] and got[0] == 56
    assert [n for n, _ in W._fields_] == fields


def test_the_models_subpack_passes_the_real_pack_check_and_restores_the_files():
    import makisu_amd as M
    rng = np.random.default_rng(7)
    files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (5000, 0, 1, 33333, 16, 257)]
    rows = pc.random_cut_rows(rng, files, 1, 700)
    for alg in (pc.SHA256, pc.BLAKE2S):
        recipes = [rc.recipe_of(rows, files, f, alg) for f in range(len(files))]
        packs = [pc.model_pack(rows, files, [i % 3 == k for i in range(len(rows))], alg) for k in range(3)]
        store = rc.chunk_store(packs)
        layer = [r for r in recipes if len(r[1])] + [recipes[3], recipes[0]]                # the recipes end to end, two files twice
        request = np.concatenate([r[0] for r in layer])
        lengths = np.concatenate([r[1] for r in layer])
        entries, blob = fc.model_subpack(store, request, alg)
        assert len(entries) == len(store) <= len(rows) < len(request)
        assert M.pack_check(blob, entries, alg=alg) is None
        assert rc.model_restore([(entries, blob)], recipes) == files
        # ... and every entry sits at its first occurrence, in that order
        first = {}
        for r, d in enumerate(request):
            first.setdefault(bytes(d), r)
        assert entries["chunk_index"].tolist() == sorted(first.values())
        assert [bytes(d) for d in entries["digest"]] == [bytes(request[r]) for r in sorted(first.values())]
        # the shuffled request gives the same chunks in another order, and a blob of the same size
        perm = rng.permutation(len(request))
        e2, b2 = fc.model_subpack(store, request[perm], alg)
        assert M.pack_check(b2, e2, alg=alg) is None and len(b2) == len(blob)
        assert rc.model_restore([(e2, b2)], recipes) == files
        # missing: against a store of one pack of the three
        part = rc.chunk_store(packs[:1])
        held, want, info = fc.model_missing(part, request, lengths)
        assert info["n_held"] + info["n_want"] == info["n_distinct"] == len(store) and info["n_rows"] == len(request)
        assert held.tolist() == [bytes(d) in part for d in request]
        assert [bytes(request[r]) for r in want.tolist()] == [k for k in dict.fromkeys(bytes(d) for d in request) if k not in part]
        assert info["held_bytes"] == sum(len(v) for v in part.values())
        assert info["want_bytes"] == sum(len(v) for k, v in store.items() if k not in part)
        assert fc.model_missing(part, request)[2]["want_bytes"] == 0
        # what the want list asks for, cut from the full store and added to the part, restores everything
        e3, b3 = fc.model_subpack(store, request[want.astype(np.int64)], alg)
        assert rc.model_restore([packs[0], (e3, b3)], recipes) == files
    for bad in (0, lengths[3] + 1):
        wrong = lengths.copy()
        wrong[3] = bad
        key = bytes(request[3])
        try:
            fc.model_missing({key: store[key]}, request, wrong)
            raise AssertionError("a wrong length passed")
        except ValueError as e:
            assert str(e) == "row 3"


def test_null_arguments_are_refused_without_a_ctx(engine_lib):
    L = engine_lib
    out, bad = C.c_void_p(5), C.c_uint64(7)
    import makisu_amd as M
    info = M.WantInfo(9, 9, 9, 9, 9, 9, 9.0)
    assert L.mi_packset_missing(None, None, None, 0, None, None, 0, C.byref(info)) == -1
    assert list(info.as_dict().values()) == [0] * 7                                                # zeroed before anything else
    assert L.mi_packset_missing(None, None, None, 0, None, None, 0, None) == -1
    assert L.mi_packset_pack(None, None, None, 0, 0, C.byref(out), C.byref(bad)) == -1
    assert out.value is None and bad.value == 0
    assert L.mi_packset_pack(None, None, None, 0, 0, None, None) == -1


def test_the_planted_inputs_have_the_properties_the_gpu_tests_rest_on():
    # the tile-edge request (test 2)
    dig, chunks, packs = fc.edge_case()
    store = rc.chunk_store(packs)
    assert len(store) == len(chunks) == len(fc.EDGE_LENGTHS) and [len(store[bytes(d)]) for d in dig] == fc.EDGE_LENGTHS
    entries, blob = fc.model_subpack(store, dig)
    off, ln = entries["offset"].astype(np.int64), entries["length"].astype(np.int64)
    end = off + (ln + 15) // 16 * 16
    assert {int(x) % 16 for x in ln} == set(range(16))                                            # all sixteen length residues
    assert {1, 15, 16, 17, 65536} <= set(ln.tolist())
    assert any(int(o + k) % fc.TILE == 0 and k % 16 == 0 for o, k in zip(off, ln))                # ends on a tile's last byte
    assert any(int(o) % fc.TILE == 0 and o > 0 for o in off)                                      # begins on a tile's first
    per_tile = np.bincount(np.concatenate([np.arange(o // fc.TILE, (e - 1) // fc.TILE + 1) for o, e in zip(off, end)]))
    assert per_tile.max() == fc.TILE_ENTRIES and per_tile.tolist() == [21, 1024, 1, 1, 1, 1, 1]
    assert len(blob) == 98352 and len(blob) % fc.TILE != 0
    # the source: two packs in another order whose pad bytes are NOT zero, so mi_pack_check rejects them; no chunk holds a zero
    import makisu_amd as M
    for en, bl in packs:
        pads = [bl[int(o) + int(k):int(o) + pc.round16(int(k))] for o, k in zip(en["offset"], en["length"])]
        assert all(set(p) <= {0xA5} for p in pads) and sum(len(p) for p in pads) > 0
        assert M.pack_check(bl, en) is not None
    assert all(0 not in c for c in chunks)
    pad_at = np.ones(len(blob), dtype=bool)
    for o, k in zip(off, ln):
        pad_at[o:o + k] = False
    assert pad_at.sum() == len(blob) - sum(fc.EDGE_LENGTHS) == 166 and not np.frombuffer(blob, dtype=np.uint8)[pad_at].any()
    # the tripled request (test 3): every digest exactly three times, and not in three runs
    rng = np.random.default_rng(62)
    d = fc.fake_digests(rng, 500)
    assert len({bytes(x) for x in d}) == 500
    req, src = fc.tripled_request(rng, d)
    assert np.bincount(src).tolist() == [3] * 500 and np.array_equal(req, d[src])
    firsts = [int(np.flatnonzero(src == i)[0]) for i in range(500)]
    assert max(firsts) > 600 and sorted(firsts) != firsts                                          # first occurrences all over the request
    # the plan's boundaries (test 4): one block more than the second-level scan takes at a time
    assert 600_000 // fc.PLAN_BLOCK > 256
