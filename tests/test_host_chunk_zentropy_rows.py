"""The inputs of tests/test_gpu_chunk_zentropy_rows.py without a GPU: every condition the GPU tests rely on is proved here from
the model alone (zentropy_cases.py through zentropy_rows_cases.py) -- the many rows' forms, where they stand and that no two
chunks are equal; the hand-built edge forms through mi_zpack_check and the model's decoder; the keep rule's chunks on their
line; the wrong digest under a sound form H.  Bit for bit: there are no tolerances."""
import collections
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import pack_cases as pc  # noqa: E402
import zentropy_cases as ze  # noqa: E402
import zentropy_rows_cases as zr  # noqa: E402
import zpack_cases as zc  # noqa: E402


@pytest.fixture(scope="module")
def rows():
    t = time.time()
    r = zr.many_rows()
    print("the model of %d rows: %.1f s (0 if another module computed it)" % (zr.N_ROWS, time.time() - t))
    return r


def _lens_of(data):
    return ze.code_lengths(np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256))


# ---- 1. many rows ---------------------------------------------------------------------------------------------------------------------
def test_the_many_rows_hold_all_four_forms_where_the_tiles_and_the_second_trip_need_them(rows):
    r = rows
    n, grid, tile = zr.N_ROWS, zr.UNWRAP_GRID, zr.PLAN_TILE
    assert len(r.chunks) == n == grid + 2 * tile + 5 and n < 2 * grid
    assert all(cnt > 0 for cnt, _ in r.census), r.census                                      # all four forms occur
    assert [cnt for cnt, _ in r.census] == [int((r.forms == f).sum()) for f in range(4)]
    assert int(r.is_h.sum()) >= tile + 1                                                       # more than one tile of form H rows
    both_trips = [k for k in range(grid, n) if r.is_h[k] and r.is_h[k - grid]]                 # a wave unwraps one, then the other
    assert len(both_trips) >= 2000
    assert {int(r.forms[k]) for k in both_trips} == {2, 3} == {int(r.forms[k - grid]) for k in both_trips}
    assert {int(f) for f in r.forms[grid:]} == {0, 1, 2, 3} == {int(f) for f in r.forms[:2 * tile]}
    for t in range(tile, n, tile):                                                             # every tile boundary: form H on both sides
        assert r.is_h[t - 1] and r.is_h[t] and r.is_h[t + 1], t
    assert n // tile == 34 and n % tile                                                        # 35 blocks, the last one partial
    assert len({bytes(d) for d in r.entries["digest"]}) == n                                   # the digests are all distinct
    needs = [zc.round16(len(u)) for u, h in zip(r.under, r.is_h) if h]                         # what zh_place_kernel sums up
    assert len(set(needs)) >= 32 and len({x % 64 for x in needs}) == 4
    between = r.forms[2 * tile + 2:grid - 1]
    assert 0 < int((between >= 2).sum()) == 3 * (grid // tile - 2) - 3                         # only the boundary rows, between the zones
    assert int((between == 0).sum()) > 10000 and int((between == 1).sum()) > 10000


def test_the_many_rows_model_is_the_models_layout_and_the_host_check_takes_it(rows):
    r = rows
    head_e, head_b = ze.model_compress_h(r.entries[:200], r.blob, 1)                            # the layout built here IS model_compress_h's
    assert head_e.tobytes() == r.zentries[:200].tobytes() and r.zblob[:len(head_b)] == head_b
    assert int(r.zentries["offset"][-1]) + zc.round16(int(r.zentries["stored"][-1])) == len(r.zblob)
    assert M.zpack_check(r.zblob, r.zentries) is None                                          # every row decodes and hashes, natively
    assert M.zpack_check(r.zb1, r.ze1) is None
    picks = [k for k in range(0, zr.N_ROWS, 997)] + [k for k in range(zr.UNWRAP_GRID, zr.N_ROWS, 211)]
    for k in picks:                                                                            # the form under form H is level 1's own
        assert r.under[k] == zc.compress_chunk(r.chunks[k]), k
        assert ze.expand_chunk(r.stored[k], r.lengths[k]) == r.chunks[k], k
    assert sum(map(len, r.stored)) == sum(s for _, s in r.census) < sum(map(len, r.under))
    assert ze.count_forms(r.ze1, r.zb1)[2:] == [[0, 0], [0, 0]]


def test_the_level_2_rows_hold_form_h_of_both_kinds():
    chunks, entries, blob, want_e, want_b = zr.level2_rows()
    census = ze.count_forms(want_e, want_b)
    assert len(chunks) == zr.LEVEL2_ROWS and all(cnt > 0 for cnt, _ in census), census
    assert M.zpack_check(want_b, want_e) is None


@pytest.mark.parametrize("how", sorted(zr.DAMAGE))
def test_the_damaged_rows_lie_on_the_second_trip_and_the_first_is_named(rows, how):
    r = rows
    zentries, blob, a, b, rule = zr.damaged(r, how)
    assert zr.UNWRAP_GRID + 100 <= a < b < zr.N_ROWS and r.is_h[a] and r.is_h[b] and rule == zr.DAMAGE[how]
    assert r.is_h[a - zr.UNWRAP_GRID] and r.is_h[b - zr.UNWRAP_GRID]                            # their waves have unwrapped a row before
    forms = [bytes(blob[int(en["offset"]):int(en["offset"]) + int(en["stored"])]) for en in zentries[[a, b]]]
    assert [ze.chunk_rule(f, r.lengths[k])[0] for f, k in zip(forms, (a, b))] == [rule, ze.RULE_CODE]
    assert all(int(zentries["stored"][k]) < r.lengths[k] for k in (a, b))                      # the structural check lets both through
    same = np.flatnonzero(zentries["stored"] == r.zentries["stored"])
    assert len(same) >= zr.N_ROWS - 1 and np.array_equal(zentries["digest"], r.zentries["digest"])
    if how != "unassigned code":                                                                # nothing else was touched
        differ = np.flatnonzero(np.frombuffer(blob, dtype=np.uint8) != np.frombuffer(r.zblob, dtype=np.uint8))
        assert {int(np.searchsorted(r.zentries["offset"], d, side="right")) - 1 for d in differ} == {a, b}
    assert ze.first_refused(zentries[zr.UNWRAP_GRID:], blob) == (a - zr.UNWRAP_GRID, rule)
    assert M.zpack_check(blob, zentries) == a


def test_the_unassigned_code_is_refused_by_a_cleared_table_only(rows):
    """what the row of "unassigned code" is FOR: the row its wave unwrapped before has a complete code, and a decoder that left
    that row's table in place would accept the damaged form -- so only the per-row clearing of the table refuses it"""
    r = rows
    zentries, blob, a, _, _ = zr.damaged(r, "unassigned code")
    at = int(zentries["offset"][a])
    form, prev = blob[at:at + int(zentries["stored"][a])], r.stored[a - zr.UNWRAP_GRID]
    assert r.forms[a - zr.UNWRAP_GRID] == 3 and sum(1 << (11 - l) for l in zr.form_lens(prev) if l) == 2048
    before = zr.decode_table(zr.form_lens(prev))
    assert all(l for _, l in before)                                                            # every entry is somebody's
    assert zr.table_decode(prev, before) == r.chunks[a - zr.UNWRAP_GRID]                        # (the table decoder decodes)
    assert zr.table_decode(form, zr.decode_table(zr.form_lens(form))) is None                   # cleared: refused
    stale = zr.table_decode(form, zr.decode_table(zr.form_lens(form), before))
    assert stale is not None and len(stale) == r.lengths[a] and stale.count(7) == len(stale) - 1
    longer = form[:ze.HEAD] + (int.from_bytes(form[ze.HEAD:ze.HEAD + 2], "little") + 1).to_bytes(2, "little") + form[ze.HEAD + 2:] + bytes(1)
    assert ze.chunk_rule(longer, r.lengths[a])[0] == ze.RULE_BITS                               # refused whatever the stream's size


# ---- 2. a good form H under the wrong digest ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", [pc.SHA256, pc.BLAKE2S])
def test_the_host_check_hashes_what_form_h_decodes_to(alg):
    for name, entries, blob, bad in zr.wrong_digest_zpacks(alg):
        assert ze.first_refused(entries, blob) is None, name                                    # every form is sound ...
        assert M.zpack_check(blob, entries, alg=alg) == bad, name                               # ... the entry is named as an LZ4 one would be
        honest = entries.copy()
        at, stored, n = int(entries["offset"][bad]), int(entries["stored"][bad]), int(entries["length"][bad])
        honest["digest"][bad] = np.frombuffer(pc.HASHES[alg](ze.expand_chunk(blob[at:at + stored], n)).digest(), dtype=np.uint8)
        assert M.zpack_check(blob, honest, alg=alg) is None, name


# ---- 4. edge forms -------------------------------------------------------------------------------------------------------------------------
def test_every_edge_form_is_accepted_by_the_host_check_and_the_models_decoder():
    forms = zr.edge_forms()
    assert len(forms) == 13
    for name, form, chunk in forms:
        assert ze.chunk_rule(form, len(chunk)) == (0, chunk), name
        kind, inner = ze.huff_decode(form, len(chunk))
        assert (kind == 2 and inner == chunk) or (kind == 1 and zc.lz4_block_decode(inner, len(chunk)) == chunk), name
    for alg in (pc.SHA256, pc.BLAKE2S):
        for name, entries, blob, chunks in zr.edge_zpacks(alg):
            assert M.zpack_check(blob, entries, alg=alg) is None and ze.first_refused(entries, blob) is None, name
            assert [int(n) for n in entries["length"]] == [len(c) for c in chunks]
    assert len(zr.edge_zpacks()[-1][3]) == 10


def _stream_sizes(form):
    s = form[2] + 1
    return [int.from_bytes(form[ze.HEAD + 2 * i:ze.HEAD + 2 * i + 2], "little") for i in range(s)]


def test_the_empty_stream_forms_are_what_they_are_named():
    forms = {name: (form, chunk) for name, form, chunk in zr.edge_forms()}
    f, c = forms["zeros over 64 streams"]
    assert c == bytes(1000) and len(zc.compress_chunk(c)) == 14 and len(f) == 278
    for s in (64, 33, 32):
        f, _ = forms["zeros over %d streams" % s]
        sizes = _stream_sizes(f)
        assert f[1] == 1 and len(sizes) == s and all(sizes[:14]) and sizes[14:] == [0] * (s - 14)
    for s in (32, 64):
        for inner in (s - 1, s, s + 1):
            f, c = forms["a block of %d bytes over %d streams" % (inner, s)]
            sizes = _stream_sizes(f)
            assert int.from_bytes(f[4:8], "little") == inner == len(zc.compress_chunk(c)) and f[1] == 1
            assert sum(1 for x in sizes if x == 0) == max(0, s - inner) and len(sizes) == s
    # no coder here makes any of them: a block this short never pays for form H's header
    assert all(ze.form_of(ze.compress_chunk_h(c, 1), len(c)) == 1 for name, (_, c) in forms.items() if "streams" in name and "one symbol" not in name)


def test_the_deep_code_is_clamped_from_twenty_one_bits():
    fib = zr.fibonacci_chunk()
    counts = np.bincount(np.frombuffer(fib, dtype=np.uint8), minlength=256)
    assert len(fib) == 46367 and int((counts > 0).sum()) == 22
    assert max(ze.code_lengths(counts, 64)) == 21
    lens = ze.code_lengths(counts)
    assert sorted(l for l in lens if l) == [1, 2, 3, 4, 5, 6, 7, 10] + [11] * 14
    assert sum(1 << (11 - l) for l in lens if l) == 2048
    form = dict((name, f) for name, f, _ in zr.edge_forms())["a code clamped from 21 bits"]
    assert len(form) == 15584 == ze.huff_size(fib) and form[1] == 2 and ze.huff_decode(form, len(fib)) == (2, fib)
    for level in (1, 2):                                           # decoder-only: the coder keeps an LZ4 block for this chunk
        assert len(ze.under_form(fib, level)) < len(fib) and ze.compress_chunk_h(fib, level) != form


def test_the_flat_code_fills_the_table_and_the_form_is_smaller_than_the_chunk():
    flat = zr.flat_chunk()
    lens = _lens_of(flat)
    assert len(flat) == 65536 and all(lens) and collections.Counter(lens) == {7: 64, 8: 64, 9: 128}
    assert sum(1 << (11 - l) for l in lens) == 2048                 # complete: no table entry is unassigned
    assert ze.huff_size(flat) == 63700 < 65536                      # (63 488 bytes of codes, 12 of the streams' last bytes, 200 of header)
    assert zr.flat_uniform_size() == 65736 > 65536                  # uniformly random bytes: 8 bits each, no smaller form exists
    for level in (1, 2):                                           # decoder-only: not a sixteenth under the chunk
        assert ze.compress_chunk_h(flat, level) == flat


def test_the_one_symbol_forms_are_all_zero_bits():
    forms = {name: (form, chunk) for name, form, chunk in zr.edge_forms()}
    for s, size in ((32, 200 + 32 * 8), (1, 138 + 250)):
        f, c = forms["one symbol over %d streams" % s]
        assert c == b"\x07" * 2000 and len(f) == size and f[1] == 2
        assert {i: l for i, l in enumerate(_lens_of(c)) if l} == {7: 1}
        assert f[ze.HEAD + 2 * s:] == bytes(len(f) - ze.HEAD - 2 * s)
    assert forms["one symbol over 1 streams"][0] != ze._unassigned_form()[0]                 # the base of the malformed table's row


# ---- 5. the keep rule ----------------------------------------------------------------------------------------------------------------------
def test_the_keep_rules_chunks_stand_on_the_bound_and_one_under_it():
    cases = zr.edge_chunks_h()
    by = dict((name, (c, m)) for name, c, m in cases)
    on, under = by["raw, on the bound"][0], by["raw, one under the bound"][0]
    assert (len(on), len(under)) == (3331, 3332) and under[:3331] == on
    for level in (1, 2):
        assert ze.under_form(on, level) == on and ze.under_form(under, level) == under        # both parses leave them raw
        assert (zr.keep_margin(on, level), zr.keep_margin(under, level)) == (0, -1)
        assert ze.compress_chunk_h(on, level) == on
        assert len(ze.compress_chunk_h(under, level)) == 3123 and ze.form_of(ze.compress_chunk_h(under, level), 3332) == 3
    lz_on, lz_under, tried = zr.edge_lz4_pair()
    assert tried <= zr.EDGE_LZ4_MAX and (lz_on[1], lz_under[1]) == (0, -1)
    assert by["lz4, on the bound"] == lz_on and by["lz4, under the bound"] == lz_under
    for (c, m), form in ((lz_on, 1), (lz_under, 2)):
        assert len(zc.compress_chunk(c)) < len(c) and zr.keep_margin(c, 1) == m
        assert ze.form_of(ze.compress_chunk_h(c, 1), len(c)) == form
    # at level 2 the denser parse moves both by one byte: the pair stands at +1 and 0, and both stay LZ4
    assert [zr.keep_margin(c, 2) for c, _ in (lz_on, lz_under)] == [1, 0]
    assert [ze.form_of(ze.compress_chunk_h(c, 2), len(c)) for c, _ in (lz_on, lz_under)] == [1, 1]
    for name, c, m in cases:
        for level in (1, 2):
            assert ze.expand_chunk(ze.compress_chunk_h(c, level), len(c)) == c, name
