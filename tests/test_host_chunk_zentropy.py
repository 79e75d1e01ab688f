"""The zpack entropy stage without a GPU: the model of zentropy_cases.py pinned byte for byte on hand-built inputs, its round trip
on the planted chunks, and mi_zpack_check (csrc/host_huff.h behind it) held against the model's decoder on every row of the
malformed table -- the entry AND the rule, which the library's rule names spell out.  Bit for bit: there are no tolerances."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import pack_cases as pc  # noqa: E402
import zentropy_cases as ze  # noqa: E402
import zpack_cases as zc  # noqa: E402

TWO = bytes(0x41 if (i * i) % 7 < 3 else 0x42 for i in range(400))
ONE = b"\x07" * 40
SMALL = bytes((i * 37) % 5 + 0x30 for i in range(20))
ODD = bytes((i * i * 11) % 9 + 0x61 for i in range(77))


def _lens(inner):
    lens = ze.code_lengths(np.bincount(np.frombuffer(inner, dtype=np.uint8), minlength=256))
    return {s: l for s, l in enumerate(lens) if l}


# ---- 1. the model's forms, pinned ----------------------------------------------------------------------------------------------------
def test_a_two_symbol_chunk_codes_to_one_bit_a_symbol():
    f = ze.huff_form(TWO, 2)
    assert _lens(TWO) == {0x41: 1, 0x42: 1}
    assert len(f) == 264 and f[:8].hex() == "00021f0090010000"
    assert f[8:136] == bytes(32) + bytes([0x10, 0x01]) + bytes(94)       # symbol 0x41: byte 32's high nibble; 0x42: byte 33's low one
    assert f[136:200] == bytes([2, 0]) * 32                               # 400 symbols over 32 streams: 12 or 13 bits, 2 bytes each
    assert f[200:].hex() == ("180c0603c10030180c0683016010180c0603c10030180c0683016010180c0603c10030080c0683016000180c0603c10030080c0683016000"
                             "180c0603c1003008")
    assert ze.huff_decode(f, 400) == (2, TWO)


def test_a_single_symbol_inner_form_gets_length_one_and_an_incomplete_code():
    f = ze.huff_form(ONE, 2)
    assert _lens(ONE) == {7: 1}
    assert len(f) == 232 and f[:8].hex() == "00021f0028000000" and f[8 + 3] == 0x10 and sum(f[8:136]) == 0x10
    assert f[136:200] == bytes([1, 0]) * 32 and f[200:] == bytes(32)     # 40 symbols: 2 or 1 zero bits a stream, one byte each
    assert ze.huff_decode(f, 40) == (2, ONE)


def test_an_inner_length_below_the_stream_count_leaves_empty_streams():
    f = ze.huff_form(SMALL, 1)
    assert _lens(SMALL) == {0x30: 3, 0x31: 3, 0x32: 2, 0x33: 2, 0x34: 2}
    assert len(f) == 220 and f[:8].hex() == "00011f0014000000"
    assert f[136:200] == bytes([1, 0]) * 20 + bytes(24)                   # streams 20..31 hold nothing: size 0
    assert f[200:].hex() == "0300010702030001070203000107020300010702"
    assert ze.huff_decode(f, 21) == (1, SMALL)


def test_an_inner_length_that_is_no_multiple_of_the_stream_count():
    f = ze.huff_form(ODD, 1)
    assert _lens(ODD) == {0x61: 2, 0x63: 2, 0x66: 2, 0x69: 2}
    assert len(f) == 232 and f[:8].hex() == "00011f004d000000" and f[136:200] == bytes([1, 0]) * 32
    assert f[200:].hex() == "24320f1811093c230624320f1801090c030604020f0801090c030604020f0801"     # 13 streams of 3 symbols, 19 of 2
    assert ze.huff_decode(f, 78) == (1, ODD)


def test_fibonacci_counts_are_clamped_to_eleven_bits_and_the_kraft_sum_is_repaired():
    inner = ze.fibonacci_inner()
    counts = np.bincount(np.frombuffer(inner, dtype=np.uint8), minlength=256)
    free = ze.code_lengths(counts, 64)
    assert [free[7 * i + 3] for i in range(24)] == [23, 23] + list(range(22, 0, -1))
    lens = ze.code_lengths(counts)
    # the clamp alone leaves 17 + 2 symbols at 11 and a Kraft sum above 2^11; the repair lengthens the longest of the shorter ones
    assert [lens[7 * i + 3] for i in range(24)] == [11] * 17 + [8, 6, 5, 4, 3, 2, 1]
    assert sum(1 << (11 - l) for l in lens if l) == 2041
    f = ze.huff_form(inner, 2)
    assert len(f) == 40987 and hashlib.sha256(f).hexdigest() == "fd0a1836a59dab680560c33aff8ea18b660f51fdde005efa27c482582d2372fa"
    assert ze.huff_size(inner) == len(f) and ze.huff_size(inner, 32, None) == 39936


def test_ties_in_the_merge_go_to_the_leaf_and_in_the_order_to_the_lower_symbol():
    counts = [0] * 256
    for s in (9, 5, 200, 77):
        counts[s] = 3                                              # four equal counts: a full tree of depth 2 whatever the order
    counts[1] = 6                                                  # ... and one as heavy as two of them
    lens = ze.code_lengths(counts)
    # leaves (3,5) (3,9) (3,77) (3,200) (6,1): 5+9 -> 6, 77+200 -> 6; then the LEAF (6,1) and the first merged 6 -> 12; 6 + 12
    assert {s: lens[s] for s in (5, 9, 77, 200, 1)} == {5: 3, 9: 3, 77: 1 + 1, 200: 2, 1: 2}
    codes = ze.canonical_codes(lens)
    assert [codes[s] for s in (1, 77, 200, 5, 9)] == [0b00, 0b10, 0b01, 0b011, 0b111]     # by (length, symbol), bit-reversed


# ---- 2. round trips -------------------------------------------------------------------------------------------------------------------
def test_the_planted_chunks_round_trip_and_hold_all_four_forms_at_both_levels():
    cases = ze.planted_chunks_h()
    for level in (1, 2):
        forms = set()
        for name, chunk in cases:
            stored = ze.compress_chunk_h(chunk, level)
            under = ze.under_form(chunk, level)
            assert 0 < len(stored) <= len(under) <= len(chunk), name
            assert ze.expand_chunk(stored, len(chunk)) == chunk, name
            form = ze.form_of(stored, len(chunk))
            forms.add(form)
            if form >= 2:                                          # the rule that keeps it, and the limit
                assert len(stored) < len(under) - (len(under) >> 4) and len(chunk) <= ze.MAX_CHUNK, name
                assert stored[2] == ze.STREAMS - 1 and (form == 2) == (len(under) < len(chunk)), name
            if name.startswith("random") or len(chunk) > ze.MAX_CHUNK:
                assert form < 2, name
        assert forms == {0, 1, 2, 3}
    by_name = dict(cases)
    assert ze.form_of(ze.compress_chunk_h(by_name["four symbols"], 1), 320) == 3
    assert ze.form_of(ze.compress_chunk_h(by_name["text 65536"], 1), 65536) == 2
    assert ze.form_of(ze.compress_chunk_h(by_name["text 65537"], 1), 65537) == 1
    assert ze.form_of(ze.compress_chunk_h(by_name["zeros"], 2), 65536) == 2


def test_the_decoder_takes_one_to_sixty_four_streams():
    inner = zc.compress_chunk(zc.text_like(3000, 5))
    for streams in (1, 2, 31, 33, 64):
        f = ze.huff_form(inner, 1, streams)
        assert f[2] == streams - 1 and ze.expand_chunk(f, 3000) == zc.text_like(3000, 5)
        entries, blob = zc.build_zpack([zc._entry(f, 3000, zc.text_like(3000, 5))])
        assert M.zpack_check(blob, entries) is None


# ---- 3. mi_zpack_check against the model's decoder --------------------------------------------------------------------------------------
def test_the_malformed_table_names_every_rule_and_branch():
    rules = [rule for _, _, _, rule in ze.malformed_table()]
    assert set(rules) == {2, 6, 7, 8, 9, 10, 11}
    assert rules.count(8) == 11 and rules.count(9) == 3 and rules.count(10) == 2 and rules.count(11) == 4


@pytest.mark.parametrize("alg", [pc.SHA256, pc.BLAKE2S])
def test_zpack_check_and_the_model_agree_on_every_malformed_row(alg):
    good_e, good_b = ze.good_zpack(alg)
    assert ze.first_refused(good_e, good_b) is None and M.zpack_check(good_b, good_e, alg=alg) is None
    assert [row[0] for row in ze.count_forms(good_e, good_b)] == [1, 1, 1, 1]
    for name, entries, blob, bad, rule in ze.malformed_zpacks(alg):
        assert ze.first_refused(entries, blob) == (bad, rule), name
        assert M.zpack_check(blob, entries, alg=alg) == bad, name


def test_the_librarys_rule_names_continue_the_lz4_decoders():
    text = open(os.path.join(ROOT, "makisu_amd", "csrc", "host_huff.h")).read()
    for rule, word in ((8, "kHuffHeader = 8"), (9, "kHuffCode = 9"), (10, "kHuffSizes = 10"), (11, "kHuffBits = 11")):
        assert word in text
    assert "kLz4PadNotZero = 7" in open(os.path.join(ROOT, "makisu_amd", "csrc", "host_lz4.h")).read()


def test_a_digest_that_differs_is_found_behind_a_form_h_that_decodes():
    entries, blob = ze.good_zpack()
    entries = entries.copy()
    entries["digest"][3][0] ^= 1
    assert M.zpack_check(blob, entries) == 3
    hurt = bytearray(blob)
    off = int(entries["offset"][1])
    hurt[off + 300] ^= 0x10                                        # a bit inside a stream: decodes to other bytes, or breaks rule 11
    assert M.zpack_check(bytes(hurt), ze.good_zpack()[0]) == 1
