"""The planted members of tests/inflate_cases.py (planted_streams: deflate streams written by hand, block by block, so that every branch
of the device inflate's decoder is taken on purpose) without a GPU: zlib inflates each to its data and the model says DONE with the
same bytes; trace() reaches every label a member is there for, and between them the members reach the whole list; every subtly wrong
decoder is told from the right one by a member that is named; the members written by zlib and by the deflate leg reach none of the
staging ring's labels (the finding that made these members necessary); every byte offset the GPU test starts a decode from ends in
the model."""
import gzip
import os
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_cases as dc  # noqa: E402
import inflate_cases as ic  # noqa: E402


@pytest.fixture(scope="module")
def planted():
    return ic.planted_streams()


@pytest.fixture(scope="module")
def traced(planted):
    """name -> (the labels its candidates reach, its candidates' rows)"""
    return {name: ic.member_labels(gz) for name, (gz, _, _) in planted.items()}


def test_zlib_and_the_model_inflate_every_planted_member(planted):
    for name, (gz, data, _) in planted.items():
        assert ic.zlib_inflates(gz) == data, name
        p = ic.plan(gz)
        assert p["result"] == ic.DONE and p["out"] == data, (name, p["result"], p["rule"], p["at_in"])
        assert sum(p["sizes"]) == len(data) and p["n_segments"] == len(p["sizes"]) <= p["n_candidates"], name
        assert len(gz) < 34000, name                     # a few KB, or 32 KB of history and a little


def test_every_member_reaches_its_labels_and_together_the_whole_list(planted, traced):
    named = set()
    for name, (_, _, labels) in planted.items():
        assert labels <= traced[name][0], (name, sorted(labels - traced[name][0], key=str))
        named |= labels
    assert named == ic.required_labels(), (sorted(named ^ ic.required_labels(), key=str))


def test_the_planted_members_are_what_their_names_say(planted, traced):
    gz, data, _ = planted["far_first"]
    assert gz[10] & 0xF8 == 0b10101 << 3 and len(data) > 32768 + 258     # the stored block's pad bits
    # the dead headers: three dead candidates, each NO_END_OF_BLOCK
    dead = [r for c, r in traced["dead_headers"][1] if c != 10]
    assert [(r["status"], r["rule"]) for r in dead] == [(ic.SEG_BROKEN, ic.NO_END_OF_BLOCK)] * 3
    # the tiles' edges: the live chain's ends and the dead markers lie where they were planted, at every residue
    gz, _, _ = planted["tile_edges"]
    rows = dict(traced["tile_edges"][1])
    live = [r["end"] for c, r in sorted(rows.items()) if r["status"] == ic.SEG_ENDS and (c == 10 or c in ic.LIVE_TILE_ENDS)]
    assert live == ic.LIVE_TILE_ENDS and ic.plan(gz)["n_segments"] == len(live) + 1
    assert {p % 2048 for p in live} == set(range(2044, 2048)) | set(range(5)) and {p % 8 for p in live} == set(range(8))
    assert len({p // 2048 for p in live}) >= 3
    dead = [c for c in rows if c != 10 and c not in live]
    assert dead[:-1] == ic.DEAD_TILE_ENDS and {p % 2048 for p in dead[:-1]} == {p % 2048 for p in live}
    assert gz[dead[0] - 4:dead[0] + 8] == ic.MARKER * 3 and gz[dead[-1] - 5:dead[-1]] == b"\x00" + ic.MARKER
    assert all(rows[c]["status"] == ic.SEG_BROKEN for c in dead)
    # n - 8 counts, n - 7 does not
    gz, _, _ = planted["marker_at_n_minus_8"]
    assert gz[-12:-8] == ic.MARKER and [c for c, _ in traced["marker_at_n_minus_8"][1]] == [10, len(gz) - 8]
    gz, _, _ = planted["marker_at_n_minus_7"]
    assert gz[-11:-7] == ic.MARKER and [c for c, _ in traced["marker_at_n_minus_7"][1]] == [10]
    # the empty segments, and the rounds for a window of 1 MiB: the empty ones close the round the full segment opened
    p = ic.plan(planted["empty_segments"][0], 1 << 20)
    assert (p["n_candidates"], p["n_segments"], p["n_rounds"], p["sizes"]) == (ic.N_EMPTY + 1, ic.N_EMPTY + 1, 1, [0] * (ic.N_EMPTY + 1))
    p = ic.plan(planted["empty_segments_between"][0], 1 << 20)
    assert p["sizes"] == [1 << 20] + [0] * (ic.N_EMPTY - 1) + [100] and p["n_rounds"] == 2 == ic.rounds(p["sizes"], 1 << 20)
    assert ic.plan(planted["empty_segments_between"][0])["n_rounds"] == 1


def test_decode_segment_and_trace_are_one_decode(planted):
    for name in ("lengths", "dead_headers", "source_across", "stored_offsets"):
        gz = planted[name][0]
        for c in ic.candidates(gz, 10):
            row, out, _ = ic.trace(gz, c)
            assert (row, out) == ic.decode_segment(gz, c), (name, c)


@pytest.mark.parametrize("wrong", ic.WRONGS)
def test_a_subtly_wrong_decoder_is_told_by_a_named_member(planted, wrong):
    teller = {"sym285": "lengths", "last_dist_base": "far_first", "no_mod": "source_across", "clip_repeat": "repeats_across", "walk14": "long_literals"}[wrong]
    gz, data, _ = planted[teller]
    p = ic.plan(gz, wrong=(wrong,))
    assert p["result"] != ic.DONE or p["out"] != data, (wrong, teller)
    told = [name for name, (gz, data, _) in planted.items() if len(data) <= 100000 and (lambda p: p["result"] != ic.DONE or p["out"] != data)(ic.plan(gz, wrong=(wrong,)))]
    assert teller in told
    # ... and on the corruption tests' base the wrong decoder and the right one agree (but for the plain copy: every compressor writes
    # overlapping matches): it takes a planted member to tell them
    gz, data = ic.two_piece()
    assert (ic.plan(gz, wrong=(wrong,))["out"] == data) == (wrong != "no_mod")


def present_members():
    """the members the other inflate tests decode, up to the size the model is asked for there"""
    out = []
    for n in (0, 1, 12, 13, 63, 64, 65, 65535, 65536, 65537):
        out += [dc.gzip_member(dc.text(n, 51)), dc.gzip_member(dc.random_bytes(n, 52)), dc.gzip_member(dc.symbols(n, 4, 53))]
    out += [dc.gzip_member(d) for d in (dc.no_match(), dc.one_distance(), dc.one_distance(65536 + 700))]
    mixed = dc.text(100000, 54) + bytes(30000) + dc.random_bytes(40000, 55) + dc.symbols(60000, 7, 56)
    out += [ic.host_leg(mixed, level, 1 << 16) for level in (1, 6, 9)]
    x = dc.text(200000, 63)
    out += [ic.one_stream(x[:30000], 6, zlib.Z_FIXED), ic.one_stream(x[:140000], 0), ic.one_stream(x[:30000], 6, zlib.Z_HUFFMAN_ONLY),
            ic.one_stream(bytes(100000), 6, zlib.Z_RLE), ic.one_stream(ic.repeat_at(32768), 9), ic.source_at_start()[0], gzip.compress(x),
            ic.two_piece()[0]]
    out += [gz for gz, _ in ic.planted_cases().values()]
    return out


def test_the_present_members_reach_none_of_the_rings_labels():
    """what zlib and the deflate leg write never puts an overlapping match's source across the flushed line, never fills the ring to 511
    or 512 and never brings a stored block while the ring holds bytes; no match of theirs has distance 32 768 either (zlib's longest is
    32 768 - 262).  If an input changes so that it does, this fails and the list of what only the planted members reach gets shorter"""
    reached = set()
    for gz in present_members():
        at = ic.gzip_header(gz)
        while True:                                      # the live chain
            row, _, labels = ic.trace(gz, at)
            reached |= labels
            if row["status"] != ic.SEG_ENDS:
                assert row["status"] == ic.SEG_FINAL
                break
            at = row["end"]
    assert not reached & ic.ring_labels(), sorted(reached & ic.ring_labels(), key=str)
    assert not reached & {("far", 0), ("far", 1), ("dist", 29, "max"), ("lit_bits", 15), ("dist_bits", 14), ("dist_bits", 15), ("hclen", 4), ("hclen", 19),
                          ("lit_incomplete",), ("len", 284, "max")}
    assert not any(l[0] == "repeat" and (l[2] or (l[3] and l[1] != 16)) for l in reached)


def test_the_model_ends_on_every_start_the_gpu_test_gives_it(planted):
    """every byte offset of three small members as a start, under a window of 64 KiB: mostly garbage, and every way a decode can end"""
    statuses, rules = set(), set()
    for gz in (ic.two_piece()[0], planted["lengths"][0], planted["long_run"][0]):
        for start in range(len(gz)):
            row, _ = ic.decode_segment(gz, start, 65536)
            assert row["bit"] <= 8 * len(gz) + 64 and row["out_bytes"] <= 65536
            statuses.add(row["status"])
            rules.add(row["rule"])
    assert statuses == {ic.SEG_ENDS, ic.SEG_FINAL, ic.SEG_BROKEN, ic.SEG_TOO_LONG} and ic.BEYOND_WINDOW in rules and len(rules) >= 8
