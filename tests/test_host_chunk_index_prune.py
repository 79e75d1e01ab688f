"""The chunk index's query, prune and retain calls without a GPU: the header declares and tags the four calls and the binding
covers them, mi_index_prune_info has the header's layout, NULL arguments are refused without a device, the model
(index_cases.py) is pinned by hand, its crafted digests are what their names say, and INTEGRATION.md names only declared calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import index_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")
NEW_CALLS = ["mi_index_query", "mi_index_query_batch", "mi_index_prune", "mi_index_retain_zset"]
INFO_FIELDS = ["n_rows", "n_unknown", "n_before", "n_dropped", "n_after", "slots_before", "slots_after", "rebuilt", "peak_extra_bytes",
               "ms_mark", "ms_rebuild"]


def _tags():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return src, dict((m.group(2), m.group(1)) for m in
                     re.finditer(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b(mi_[a-z0-9_]+)\s*\(", src, flags=re.M))


def test_the_header_declares_and_tags_the_calls_and_the_binding_covers_them(engine_lib):
    src, tags = _tags()
    for name in NEW_CALLS:
        assert tags.get(name) == "MI_BLOCK", (name, tags.get(name))
        assert name in engine_lib._mi_symbols and hasattr(engine_lib, name), name
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", src, re.M)        # additive: the version stays
    assert re.search(r"^#define\s+MI_INDEX_PRUNE_KEEP\s+0x1u", src, re.M) and re.search(r"^#define\s+MI_INDEX_PRUNE_DROP\s+0x2u", src, re.M)
    for name in ("mi_index_create", "mi_index_free", "mi_index_count", "mi_index_export", "mi_index_import"):
        assert tags[name] == "MI_CORE", name                               # the core set stays as it is
    import makisu_amd as M
    assert (M.INDEX_PRUNE_KEEP, M.INDEX_PRUNE_DROP) == (1, 2)
    for attr in ("query", "query_batch", "prune", "retain"):
        assert hasattr(M.ChunkIndex, attr), attr
    for name in ("IndexPruneInfo", "INDEX_PRUNE_KEEP", "INDEX_PRUNE_DROP"):
        assert name in M.__all__, name


def test_the_struct_layout_matches_the_header(tmp_path):
    import makisu_amd as M
    lines = ['printf("%zu\\n", sizeof(mi_index_prune_info));']
    lines += ['printf("%%zu\\n", offsetof(mi_index_prune_info, %s));' % f for f in INFO_FIELDS]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "makisu_mi.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    P = M.IndexPruneInfo
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in INFO_FIELDS]
    assert C.sizeof(P) == 88 and [n for n, _ in P._fields_] == INFO_FIELDS == ic.INFO_FIELDS + ["ms_mark", "ms_rebuild"]


def test_null_arguments_are_refused_without_a_device(engine_lib):
    import makisu_amd as M
    L = engine_lib
    info, n = M.IndexPruneInfo(), C.c_uint64(7)
    info.n_rows = 9
    dig = np.zeros((2, 32), dtype=np.uint8)
    assert L.mi_index_query(None, dig.ctypes.data, 2, None, C.byref(n)) == -1 and n.value == 0
    assert L.mi_index_query_batch(None, None, None, 0, None) == -1
    assert L.mi_index_prune(None, dig.ctypes.data, 2, M.INDEX_PRUNE_KEEP, C.byref(info)) == -1 and info.n_rows == 0
    assert L.mi_index_prune(None, None, 0, 3, None) == -1
    assert L.mi_index_retain_zset(None, None, C.byref(info)) == -1 and L.mi_index_retain_zset(None, None, None) == -1


def test_the_integration_text_names_only_declared_calls():
    _, tags = _tags()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    named = set(re.findall(r"\bmi_index_[a-z0-9_]+", doc))
    assert set(NEW_CALLS) - {"mi_index_query"} <= named, sorted(named)     # prune, retain and the dry run are all there
    for name in named - {"mi_index_prune_info"}:                           # (the struct: a type, not a call)
        assert name in tags, name
    assert "MI_INDEX_PRUNE_DROP" in doc and "mi_zset_prune" in doc


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _d(*first, fill=7):
    return bytes(first) + bytes([fill]) * (32 - len(first))


def test_the_table_size_rule_pinned_by_hand():
    assert [ic.table_slots(n) for n in (0, 1, 512, 513, 1024, 1025, 2000, 5000)] == [1024, 1024, 1024, 2048, 2048, 4096, 4096, 16384]
    assert [ic.alloc(n) for n in (0, 1, 256, 257, 64)] == [256, 512, 512, 768, 512]
    assert ic.tag_of(bytes(32)) == 1 and ic.tag_of(_d(1, 0, 0, 0, 0, 0, 0, 0)) == 1 and ic.tag_of(_d(0, 1, 0, 0, 0, 0, 0, 0)) == 256
    assert ic.home(_d(0xFF, 0x03), 1024) == 1023 and ic.home(_d(0xFF, 0x03), 2048) == 1023 and ic.home(_d(0xFF, 0x07), 2048) == 2047


def test_the_prune_model_pinned_by_hand_on_five_digests():
    a, b, c, d, e = (_d(i) for i in range(1, 6))
    stranger = _d(9, 9)
    m = ic.Index()
    assert m.add(ic.rows([a, b, c, d, d])) == 4 and m.add(ic.rows([d, e])) == 1 and m.slots == 1024
    assert m.query(ic.rows([a, stranger, e, e])) == [1, 0, 1, 1]
    # KEEP [a, c, a stranger, a]: b, d, e go.  The first scratch: the request (128 -> 512), marks (1 024 -> 1 280), totals (512);
    # the rebuild: tags (8 192 -> 8 448), digests (32 768 -> 33 024), records (64 -> 512), row states (18 -> 512), row slots
    # (32 -> 512), counters (512)
    info = m.prune(ic.rows([a, c, stranger, a]), keep=True)
    assert info == {"n_rows": 4, "n_unknown": 1, "n_before": 5, "n_dropped": 3, "n_after": 2, "slots_before": 1024, "slots_after": 1024,
                    "rebuilt": 1, "peak_extra_bytes": (512 + 1280 + 512) + (8448 + 33024 + 512 + 512 + 512 + 512)}
    assert m.held == {a, c} and stranger not in m.held                                # a prune never adds
    # nothing to drop: only the first scratch, the table is not touched
    info = m.prune(ic.rows([stranger]), keep=False)
    assert info == {"n_rows": 1, "n_unknown": 1, "n_before": 2, "n_dropped": 0, "n_after": 2, "slots_before": 1024, "slots_after": 1024,
                    "rebuilt": 0, "peak_extra_bytes": 512 + 1280 + 512}
    assert m.prune(ic.rows([]), keep=False)["peak_extra_bytes"] == 256 + 1280 + 512
    # a dropped digest is one that was never added
    assert m.add(ic.rows([b, a])) == 1 and m.held == {a, b, c}
    # KEEP nothing empties it
    info = m.prune(ic.rows([]), keep=True)
    assert (info["n_dropped"], info["n_after"], info["slots_after"], info["rebuilt"]) == (3, 0, 1024, 1) and not m.held
    assert info["peak_extra_bytes"] == (256 + 1280 + 512) + (8448 + 33024 + 256 + 512 + 512 + 512)


def test_the_table_shrinks_and_regrows_in_the_model():
    rng = np.random.default_rng(5)
    dig = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
    m = ic.Index()
    assert m.add(dig) == 3000 and m.slots == 8192
    info = m.prune(dig[:600], keep=True)
    assert (info["slots_before"], info["slots_after"], info["n_dropped"]) == (8192, 2048, 2400) and m.slots == 2048
    assert m.add(dig) == 2400 and m.slots == 8192                       # (600 + 3 000 rows) x 2 = 7 200


def test_the_retain_model_pinned_by_hand():
    a, b, c = (_d(i) for i in range(1, 4))
    m = ic.Index()
    m.add(ic.rows([a, b, c]))
    # the exported digests (96 -> 512), three answers a row (24 -> 512 each), flags (3 -> 512), totals (512); then the rebuild for one
    info = m.retain({b, _d(8)})
    assert info == {"n_rows": 0, "n_unknown": 0, "n_before": 3, "n_dropped": 2, "n_after": 1, "slots_before": 1024, "slots_after": 1024,
                    "rebuilt": 1, "peak_extra_bytes": 6 * 512 + (8448 + 33024 + 4 * 512)}
    assert m.held == {b}
    info = m.retain({b})
    assert (info["rebuilt"], info["n_dropped"], info["peak_extra_bytes"]) == (0, 0, 6 * 512)
    assert ic.Index().retain({a}) == {"n_rows": 0, "n_unknown": 0, "n_before": 0, "n_dropped": 0, "n_after": 0, "slots_before": 1024,
                                      "slots_after": 1024, "rebuilt": 0, "peak_extra_bytes": 0}


def test_the_crafted_digests_are_what_their_names_say():
    rng = np.random.default_rng(6)
    sizes = [1 << k for k in range(10, 17)]
    a = ic.same_first8(5, rng)
    assert len(set(ic.keys(a))) == 5 and len({bytes(x[:8]) for x in a}) == 1
    b = ic.same_home(6, rng)
    assert len({ic.tag_of(x) for x in b}) == 6 and all(len({ic.home(x, s) for x in b}) == 1 for s in sizes)
    c = ic.last_slot(4, rng)
    assert len({ic.tag_of(x) for x in c}) == 4 and all(ic.home(x, s) == s - 1 for x in c for s in sizes)
    z, o = ic.zero_and_one(rng)
    assert bytes(z[:8]) == bytes(8) and bytes(o[:8]) == b"\x01" + bytes(7) and ic.tag_of(z) == ic.tag_of(o) == 1 and bytes(z) != bytes(o)
