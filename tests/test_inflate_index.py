"""CPU tests of the index of checkpoints (csrc/host_inflate_index.h behind mi_inflate_index_build / _check): the C
builder's index equals the model's (tests/inflate_index_cases.py) byte for byte, the model's spans put together are zlib's output,
the planted member holds what it was written to hold, every numbered refusal of the checker, and the builder's own refusals."""
import hashlib
import os
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import inflate_cases as ic  # noqa: E402
import inflate_index_cases as xc  # noqa: E402

SPACINGS = (1, 65536, 0)


@pytest.fixture(scope="module")
def members():
    return xc.members()


@pytest.mark.parametrize("name", ["one_stream_1", "one_stream_6", "one_stream_9", "one_stream_fixed", "no_reset", "host_leg", "stored_only", "planted"])
def test_the_builders_index_is_the_models_byte_for_byte(members, name):
    gz, data = members[name]
    assert zlib.decompress(gz, 31) == data
    for spacing in SPACINGS:
        want = xc.index(gz, spacing)
        got, info = M.inflate_index_build(gz, spacing, want_digest=True)
        assert got == want, (name, spacing, len(got), len(want))
        h = xc.parse(got)
        assert (info["n_points"], info["out_bytes"], info["windows_bytes"], info["spacing"]) == \
               (h["n_points"], len(data), h["windows_bytes"], spacing or xc.SPACING)
        assert info["n_blocks"] == sum(1 for _, _, bfinal in xc.boundaries(gz)[0] if not bfinal)
        assert info["tar_digest"].hex() == hashlib.sha256(data).hexdigest()
        assert M.inflate_index_check(got, gz)[0] == 0 and M.inflate_index_check(got)[0] == 0
        assert len(got) == 64 + 32 * h["n_points"] + h["windows_bytes"] and h["points"][0] == dict(in_bit=80, out_at=0, win_at=0, win_bytes=0)
    assert xc.parse(xc.index(gz, 1))["n_points"] >= (2 if name != "planted" else 20)


@pytest.mark.parametrize("name", ["one_stream_6", "no_reset", "host_leg", "stored_only", "planted"])
def test_the_models_spans_put_together_are_zlibs_output(members, name):
    gz, data = members[name]
    for spacing in (1, 65536):
        out = b""
        for s in xc.spans(xc.index(gz, spacing)):
            row, got = xc.decode_span(gz, s["in_bit"], s["end_bit"], s["hist"], s["out_bytes"])
            assert row["status"] in (ic.SEG_ENDS, ic.SEG_FINAL) and row["rule"] == 0 and len(got) == s["out_bytes"], (name, s["in_bit"], row)
            assert (row["status"] == ic.SEG_FINAL) == (s["end_bit"] == 0)
            out += got
        assert out == data == zlib.decompress(gz, 31)


def test_the_planted_member_holds_what_it_was_written_to_hold():
    gz, data, what = xc.planted_member()
    assert ic.zlib_inflates(gz) == data
    sp = xc.spans(xc.index(gz, 1))
    by_out = {s["out_at"]: s for s in sp}
    assert {s["in_bit"] % 8 for s in sp} == set(range(8))                  # a condition, not a hope: a point at every bit offset
    assert set(what.values()) <= set(by_out), sorted(set(what.values()) - set(by_out))

    # the spans' first tokens, as written: each reads the window the way its name says
    s = by_out[what["inside_window"]]
    assert s["win_bytes"] == 1000 == s["out_at"] and len(s["hist"]) == 1000               # a short window
    assert data[1000:1010] == data[500:510] and data[1010:1268] == data[10:268]
    s = by_out[what["short_window_first_byte"]]
    assert s["win_bytes"] == s["out_at"] < 32768 and data[s["out_at"]:s["out_at"] + 40] == data[0:40]
    for name in ("straddle_plain", "straddle_overlap", "overlap_from_window", "far", "far_second", "empty_stored_first"):
        s = by_out[what[name]]
        # without its window the span breaks the distance rule; with one byte less than it needs, too
        assert xc.decode_span(gz, s["in_bit"], s["end_bit"], b"", s["out_bytes"])[0]["rule"] == ic.DISTANCE, name
        assert xc.decode_span(gz, s["in_bit"], s["end_bit"], s["hist"], s["out_bytes"])[0]["rule"] == 0, name
    for name, unread in (("far", 0), ("far_second", 1)):               # distance 32 768 at op 0 reads hist[0], at op 1 hist[1]
        s = by_out[what[name]]
        assert s["win_bytes"] == 32768
        assert xc.decode_span(gz, s["in_bit"], s["end_bit"], s["hist"][unread:], s["out_bytes"])[0]["rule"] == 0, name
        assert xc.decode_span(gz, s["in_bit"], s["end_bit"], s["hist"][unread + 1:], s["out_bytes"])[0]["rule"] == ic.DISTANCE, name
    s = by_out[what["far"]]
    assert data[s["out_at"]:s["out_at"] + 258] == s["hist"][:258]
    s = by_out[what["overlap_from_window"]]
    assert data[s["out_at"]:s["out_at"] + 258] == (s["hist"][-3:] * 86)                   # dist 3 < len 258, from inside the window
    s = by_out[what["straddle_overlap"]]
    assert data[s["out_at"] + 5:s["out_at"] + 25] == (s["hist"][-10:] + data[s["out_at"]:s["out_at"] + 5]) * 1 + data[s["out_at"] + 5:s["out_at"] + 10]
    # the span that begins with an empty stored block: 00 00 FF FF lies right behind the point's byte, and the span goes on behind it
    s = by_out[what["empty_stored_first"]]
    byte = (s["in_bit"] + 3 + 7) // 8
    assert gz[byte:byte + 4] == ic.MARKER and s["out_bytes"] >= 31
    assert ic.decode_segment(gz, s["in_bit"] // 8)[0]["status"] != ic.SEG_FINAL


def _refused(ix, gz=None):
    return M.inflate_index_check(ix, gz)[0]


def test_every_numbered_refusal_of_the_checker(members):
    gz, _ = members["planted"]
    other, _ = members["no_reset"]
    ix = xc.index(gz, 1)
    h = xc.parse(ix)
    p = h["points"]
    assert h["n_points"] >= 6 and _refused(ix, gz) == 0
    R = xc
    cases = [
        (R.R_MAGIC, ix[:63], gz), (R.R_MAGIC, b"", gz), (R.R_MAGIC, b"MIGZIX02" + ix[8:], gz),
        (R.R_SIZES, ix[:-1], gz), (R.R_SIZES, ix + b"\x00", gz), (R.R_SIZES, xc.patch(ix, 40, 0), gz), (R.R_SIZES, xc.patch(ix, 40, 1 << 60), gz),
        (R.R_SIZES, xc.patch(ix, 56, h["windows_bytes"] + 16), gz), (R.R_SIZES, xc.patch(ix, 48, 0), gz),
        (R.R_SIZES, xc.patch(ix, 28, h["isize"] ^ 1, 4), gz), (R.R_SIZES, xc.patch(ix, 32, h["n"]), gz),
        (R.R_FIRST, xc.patch(ix, xc.row_at(0, "in_bit"), 81), gz), (R.R_FIRST, xc.patch(ix, xc.row_at(0, "out_at"), 1), gz),
        (R.R_FIRST, xc.patch(ix, xc.row_at(0, "win_bytes"), 16, 4), gz),
        (R.R_IN_BIT, xc.patch(ix, xc.row_at(3, "in_bit"), p[2]["in_bit"]), gz), (R.R_IN_BIT, xc.patch(ix, xc.row_at(1, "in_bit"), 80), gz),
        (R.R_OUT_AT, xc.patch(ix, xc.row_at(3, "out_at"), p[2]["out_at"]), gz),
        (R.R_IN_END, xc.patch(ix, xc.row_at(h["n_points"] - 1, "in_bit"), 8 * (h["n"] - 8)), gz),
        (R.R_OUT_END, xc.patch(ix, xc.row_at(h["n_points"] - 1, "out_at"), h["out_bytes"]), gz),
        (R.R_WIN_BYTES, xc.patch(ix, xc.row_at(2, "win_bytes"), p[2]["win_bytes"] - 1, 4), gz),
        (R.R_WIN_BYTES, xc.patch(ix, xc.row_at(2, "zero"), 1, 4), gz),
        (R.R_WIN_BYTES, xc.patch(ix, xc.row_at(h["n_points"] - 1, "win_bytes"), 32769, 4), gz),
        (R.R_WINDOW, xc.patch(ix, xc.row_at(2, "win_at"), p[2]["win_at"] + 8), gz),             # not aligned
        (R.R_WINDOW, xc.patch(ix, xc.row_at(2, "win_at"), p[1]["win_at"]), gz),                 # overlapping the one in front
        (R.R_WINDOW, xc.patch(ix, xc.row_at(h["n_points"] - 1, "win_at"), h["windows_bytes"] - 16), gz),   # out of bounds
        (R.R_MEMBER, ix, other), (R.R_MEMBER, ix, gz[:-1]), (R.R_MEMBER, ix, gz[:-8] + bytes(4) + gz[-4:]),
        (R.R_MEMBER, ix, ic.with_fname(gz, 3)[:len(gz)]), (R.R_MEMBER, xc.patch(ix, 8, h["n"] + 1), gz),
    ]
    seen = set()
    for k, (want, bad, member) in enumerate(cases):
        got, text = M.inflate_index_check(bad, member)
        assert got == want and text and text != "?" and (text == "ok") == (got == 0), (k, want, got, text)
        seen.add(got)
    assert seen == set(xc.REFUSALS) - {0}
    assert _refused(xc.patch(ix, 8, h["n"] + 1)) == 0                     # without the member nothing holds n
    assert len({M.load_library().mi_inflate_index_refusal(r) for r in xc.REFUSALS}) == len(xc.REFUSALS)      # each number has a text of its own


def test_the_builders_refusals(members):
    gz, data = members["no_reset"]
    for bad, text in ((gz + gz, "a second member"), (gz + b"\x00", "trailing bytes"), (gz[:-8] + bytes((gz[-8] ^ 1,)) + gz[-7:], "CRC-32"),
                      (gz[:-4] + bytes((gz[-4] ^ 1,)) + gz[-3:], "the trailer states"), (gz[:len(gz) // 2], "corrupt deflate stream"),
                      (gz[:300] + bytes((gz[300] ^ 0x10,)) + gz[301:], ""), (b"\x1f\x8b\x07" + gz[3:], "no gzip header"), (gz[:12], "")):
        with pytest.raises(M.MiError) as e:
            M.inflate_index_build(bad, 1)
        assert e.value.code == -1 and text in str(e.value), (text, str(e.value))
    assert M.inflate_index_build(gz, 1)[0] == xc.index(gz, 1)
