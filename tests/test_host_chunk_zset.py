"""The compressed pack sets without a GPU: the header declares and tags the calls and the binding covers them, mi_zset_info has
the header's layout, NULL arguments are refused without a device, and the cut's model (zset_cases.py) is pinned by hand on a
three-chunk store and held against the coder's model: cutting stored forms gives what compressing the plain sub-pack gives."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import fetch_cases as fc
import pack_cases as pc
import restore_cases as rc
import zpack_cases as zc
import zset_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")
NEW_CALLS = ["mi_zset_create", "mi_zset_add_zblob", "mi_zset_add_zpack", "mi_zset_get_info", "mi_zset_free", "mi_zset_zpack",
             "mi_batch_add_zrecipes"]


def test_the_header_declares_and_tags_the_calls_and_the_binding_covers_them(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tags = dict((m.group(2), m.group(1)) for m in
                re.finditer(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b(mi_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name in NEW_CALLS:
        assert tags.get(name) == "MI_BLOCK", (name, tags.get(name))       # the core set stays as it is
        assert name in engine_lib._mi_symbols and hasattr(engine_lib, name), name
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M)        # additive: the version stays
    assert engine_lib.mi_abi_version() == 6
    assert re.search(r"^#define\s+MI_ZSET_VERIFY\s+0x1u", src, re.M)
    import makisu_amd as M
    assert M.ZSET_VERIFY == 1
    for attr in ("add_zblob", "add_zpack", "info", "zpack", "close"):
        assert hasattr(M.ZSet, attr), attr
    assert hasattr(M.Engine, "zset") and hasattr(M.Batch, "add_zrecipes")
    for name in ("ZSet", "ZSetInfo", "ZSET_VERIFY"):
        assert name in M.__all__, name


def test_the_info_layout_matches_the_header(tmp_path):
    import makisu_amd as M
    fields = ["n_packs", "n_entries", "n_digests", "blob_bytes", "stored_bytes", "chunk_bytes", "alg", "reserved", "ms_upload", "ms_verify",
              "ms_insert"]
    lines = ['printf("%zu %zu %zu\\n", sizeof(mi_zset_info), sizeof(mi_zpack_entry), sizeof(mi_recipe_stats));']
    lines += ['printf("%%zu\\n", offsetof(mi_zset_info, %s));' % f for f in fields]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "makisu_mi.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    I = M.ZSetInfo
    assert got == [C.sizeof(I), C.sizeof(M.ZPackEntry), C.sizeof(M.RecipeStats)] + [getattr(I, f).offset for f in fields]
    assert got[0] == 80 and [n for n, _ in I._fields_] == fields


def test_null_arguments_are_refused_without_a_device(engine_lib):
    L = engine_lib
    out, bad = C.c_void_p(5), C.c_uint64(9)
    assert L.mi_zset_create(None, 0, C.byref(out)) == -1
    assert L.mi_zset_zpack(None, None, None, 0, 0, C.byref(out), C.byref(bad)) == -1 and out.value is None and bad.value == 0
    assert L.mi_zset_zpack(None, None, None, 0, 0, None, None) == -1
    assert L.mi_batch_add_zrecipes(None, None, 0, None, None, None, None, 0, None) == -1
    assert L.mi_zset_add_zblob(None, None, 0, None, 0, 0, C.byref(bad)) == -1
    assert L.mi_zset_add_zpack(None, None, 0) == -1 and L.mi_zset_get_info(None, None) == -1
    L.mi_zset_free(None)


# ---- the cut's model ---------------------------------------------------------------------------------------------------------------
def test_the_cut_model_pinned_by_hand_on_a_three_chunk_store():
    """a raw chunk of 5 bytes, GOOD_STREAM (31 bytes stored for 34) and a chunk held by two packs in two forms: pack A holds it
    raw, pack B coded -- A is added first, so raw is what the set keeps.  The request repeats a digest."""
    raw5, twice = b"hello", bytes([9]) * 40
    coded_twice = zc.compress_chunk(twice)
    assert len(coded_twice) < 40
    a = zc.build_zpack([zc._entry(raw5, 5, raw5), zc._entry(twice, 40, twice, pad=0xA5)])
    b = zc.build_zpack([zc._entry(coded_twice, 40, twice), zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN, pad=0x11)])
    d5, dt, dg = (np.frombuffer(zc.sha(x), dtype=np.uint8) for x in (raw5, twice, zc.GOOD_PLAIN))
    request = np.stack([dg, dt, dg, d5, dt])
    entries, blob = qc.model_cut([a, b], request)
    assert entries["chunk_index"].tolist() == [0, 1, 3] and entries["offset"].tolist() == [0, 32, 80]
    assert entries["length"].tolist() == [34, 40, 5] and entries["stored"].tolist() == [31, 40, 5]
    assert [bytes(x) for x in entries["digest"]] == [bytes(dg), bytes(dt), bytes(d5)]
    assert blob == zc.GOOD_STREAM + b"\0" + twice + bytes(8) + raw5 + bytes(11) and len(blob) == 96
    assert zc.model_expand(entries, blob)[1] == zc.GOOD_PLAIN + bytes(14) + twice + bytes(8) + raw5 + bytes(11)
    # the other order of the packs: the coded form wins
    entries, blob = qc.model_cut([b, a], request)
    assert entries["stored"].tolist() == [31, len(coded_twice), 5] and blob[32:32 + len(coded_twice)] == coded_twice


def test_the_cut_commutes_with_the_coder_on_the_planted_chunks():
    """model_cut over compressed packs == model_compress(model_subpack over the plain packs): what makes the feature exact"""
    chunks = [c for _, c, _ in zc.planted_chunks()]
    dig = qc.digests_of(chunks)
    groups = [list(range(0, 20)), list(range(20, 40)) + [3], list(range(40, len(chunks)))]        # chunk 3 lies in two packs
    plain = [zc.pack_of([chunks[k] for k in g]) for g in groups]
    zpacks = [zc.model_compress(*p) for p in plain]
    request, _ = fc.tripled_request(np.random.default_rng(5), dig)
    want = zc.model_compress(*fc.model_subpack(rc.chunk_store(plain), request, pc.SHA256))
    got = qc.model_cut(zpacks, request)
    assert got[1] == want[1] and all(np.array_equal(got[0][f], want[0][f]) for f in zc.ZENTRY_DTYPE.names)
    assert got[1] == qc.model_cut([(z[0], qc.with_pads(z[0], z[1], 0xA5)) for z in zpacks], request)[1]
    import makisu_amd as M
    assert M.zpack_check(got[1], got[0]) is None


def test_the_planted_restore_rows_are_what_their_names_say():
    rows = qc.restore_rows()
    seen = {"offsets": set(), "runs": set(), "matches": set()}
    for name, chunk, coded in rows:
        stored = zc.compress_chunk(chunk)
        assert (len(stored) < len(chunk)) == coded, name
        if coded:
            for lit, off, mlen in zc.parse(chunk)[:-1]:
                seen["offsets"].add(off), seen["runs"].add(lit), seen["matches"].add(mlen)
    assert sorted(len(c) for n, c, _ in rows if n.startswith("raw ")) == qc.ROW_LENGTHS
    assert sorted(len(c) for n, c, _ in rows if n.startswith("coded ")) == [n for n in qc.ROW_LENGTHS if n >= 13]
    assert seen["offsets"] >= {1, 2, 63, 64, 65} and seen["runs"] >= {269, 270, 271} and seen["matches"] >= {273, 274}
    assert max(seen["matches"]) > qc.LONG_MATCH
    chunks, files = qc.residue_files(rows)
    starts = {}
    for f in files:                                                 # every row begins at each of the 16 residues
        at = 0
        for k in f:
            starts.setdefault(k, set()).add(at % 16)
            at += len(chunks[k])
    assert all(len(starts[k]) == 16 for k in range(len(rows)))
    order = files[0]
    kinds = [rows[k][2] for k in order]
    assert (False, True) in zip(kinds, kinds[1:]) and (True, False) in zip(kinds, kinds[1:]) and len(set(order)) < len(order)
