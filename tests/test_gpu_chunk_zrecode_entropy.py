"""GPU tests of mi_zset_recode with the entropy stage (MI_ZPACK_ENTROPY): a level-1 set recoded with the flag,
without and with MI_ZPACK_LEVEL2 and MI_ZSET_RECODE_VERIFY, holds the forms the model of zrecode_h_cases.py predicts byte for
byte; no entry grows, a second call replaces nothing, a plain level-2 recode afterwards replaces what the model says (nothing, on
these chunks); a set that already holds form H is decoded through the unwrap by a recode WITHOUT the flag; a malformed form H in
an unverified set is counted, kept verbatim and named with its rule under VERIFY.  Bit for bit: there are no tolerances."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import zentropy_cases as ze  # noqa: E402
import zpack_cases as zc  # noqa: E402
import zrecode_h_cases as zh  # noqa: E402

pytestmark = pytest.mark.gpu


def _forms(f):
    return [[int(f.n[i]), int(f.stored[i])] for i in range(4)]


@pytest.fixture(scope="module")
def level1_set():
    """the planted chunks as a level-1 zpack WITHOUT the stage, and what the model holds after each recode, computed once"""
    chunks = [c for _, c in ze.planted_chunks_h()]
    entries, blob = zc.pack_of(chunks)
    ze1, zb1 = zc.model_compress(entries, blob)
    lengths = [len(c) for c in chunks]
    forms = zh.forms_of(ze1, zb1)
    after = dict((level, zh.recode_forms(forms, lengths, level, True)) for level in (1, 2))
    return chunks, ze1, zb1, lengths, forms, after


def _held(zs, digests, lengths, forms):
    """the set holds exactly these forms: the cut of everything, byte for byte"""
    want_e, want_b = zh.cut_of(digests, lengths, forms)
    with zs.zpack(digests, np.asarray(lengths, dtype=np.uint32), verify=True) as z:
        got_e = z.entries()
        assert np.array_equal(got_e["stored"], want_e["stored"]) and np.array_equal(got_e["offset"], want_e["offset"])
        assert z.read() == want_b
    assert _forms(zs.count_forms()) == zh.census(forms, lengths)


@pytest.mark.parametrize("level,verify", [(1, False), (2, False), (2, True), (1, True)])
def test_a_level_1_set_recoded_with_the_stage_holds_the_models_forms(level1_set, level, verify):
    chunks, ze1, zb1, lengths, forms, after = level1_set
    want, n_replaced, n_undecodable = after[level]
    assert n_undecodable == 0 and n_replaced > 10 and {ze.form_of(f, n) for f, n in zip(want, lengths)} == {0, 1, 2, 3}
    assert all(len(a) <= len(b) for a, b in zip(want, forms))                         # the rule: no entry grows
    dig = np.ascontiguousarray(ze1["digest"])
    with M.Engine(max_size=262144) as e, e.zset() as zs:
        zs.add_zblob(zb1, ze1, verify=True)
        _held(zs, dig, lengths, forms)
        info = zs.recode(level=level, verify=verify, entropy=True)
        assert (info.n_digests, info.n_recoded, info.n_undecodable) == (len(chunks), n_replaced, 0)
        assert (info.stored_before, info.stored_after) == (sum(map(len, forms)), sum(map(len, want))) and zs.info.stored_bytes == info.stored_after
        _held(zs, dig, lengths, want)
        again = zs.recode(level=level, verify=verify, entropy=True)                     # a second call changes nothing
        assert again.n_recoded == 0 and again.stored_after == info.stored_after and again.n_undecodable == 0
        # a recode WITHOUT the flag decodes the form H rows through the unwrap and replaces what the model says
        want2, n2, u2 = zh.recode_forms(want, lengths, 2, False)
        assert u2 == 0 and (n2 == 0 or level == 1)                                    # (after ENTROPY | LEVEL2: nothing; after level 1: one LZ4 row)
        plain2 = zs.recode(level=2, verify=True)
        assert (plain2.n_recoded, plain2.n_undecodable, plain2.stored_after) == (n2, 0, sum(map(len, want2)))
        _held(zs, dig, lengths, want2)
        with e.batch() as b:                                                           # ... and the set still restores its chunks
            keep = [k for k, n in enumerate(lengths) if n <= 8192]
            b.add_zrecipes(zs, [(dig[keep], np.asarray([lengths[k] for k in keep], dtype=np.uint32))], verify=True)
            b.run()
            body = b"".join(chunks[k] for k in keep)
            assert b.read_file(0, 0, len(body)) == body


def test_small_rounds_give_the_same_forms(level1_set):
    chunks, ze1, zb1, lengths, forms, after = level1_set
    want, n_replaced, _ = after[1]
    dig = np.ascontiguousarray(ze1["digest"])
    with M.Engine(max_size=262144) as e, e.zset() as zs:
        zs.add_zblob(zb1, ze1)
        info = zs.recode(level=1, verify=True, entropy=True, scratch_bytes=100_000)      # a 64 KiB chunk exceeds it alone
        assert info.n_rounds > 5 and info.n_recoded == n_replaced
        _held(zs, dig, lengths, want)


def test_a_set_of_form_h_from_compress_recodes_to_the_same_forms(level1_set):
    """whichever way form H came in -- mi_pack_compress with the flag, or a recode -- the held forms are the model's"""
    chunks, ze1, zb1, lengths, forms, after = level1_set
    entries, blob = zc.pack_of(chunks)
    he, hb = ze.model_compress_h(entries, blob, 1)
    held = zh.forms_of(he, hb)
    assert held == after[1][0]                                    # compress_chunk_h IS the candidate, and it won wherever it is smaller
    dig = np.ascontiguousarray(he["digest"])
    with M.Engine(max_size=262144) as e, e.zset() as zs:
        zs.add_zblob(hb, he, verify=True)
        for level in (1, 2):
            want, n, u = zh.recode_forms(held, lengths, level, True)
            info = zs.recode(level=level, verify=True, entropy=True)
            assert (info.n_recoded, info.n_undecodable) == (n, u) and u == 0
            _held(zs, dig, lengths, want)
            held = want


def test_the_census_counts_a_form_h_with_a_bad_kind_as_the_model_does():
    """found by the store walks (test_gpu_chunk_store_walk.py, the damaged kind): a span that begins like form H with a kind byte
    that is neither 1 nor 2 -- only an unverified add brings one -- was counted under [2] by the device and under [3] by
    zentropy_cases.form_of.  The header now says [3]; the set's census and the cut's agree with the model"""
    rows = [(entries, blob) for name, entries, blob, _, _ in ze.malformed_zpacks() if name in ("kind 0, behind good entries", "kind 3, behind good entries")]
    assert len(rows) == 2
    with M.Engine() as e:
        for entries, blob in rows:
            want = ze.count_forms(entries, blob)
            assert want[3][0] == 2 and want[2][0] == 0                              # the good form H over plain, and the bad kind
            with e.zset() as zs:
                zs.add_zblob(blob, entries)
                assert _forms(zs.count_forms()) == want
                with zs.zpack(np.ascontiguousarray(entries["digest"])) as z:
                    assert _forms(z.count_forms()) == want
        # one stored byte, 0x00, for a chunk of 5: there is no kind byte at all (form_of has no answer); the header says [3]
        entries, blob = zc.build_zpack([zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN), zc._entry(b"\0", 5)])
        with e.zset() as zs:
            zs.add_zblob(blob, entries)
            assert _forms(zs.count_forms()) == [[0, 0], [1, 31], [0, 0], [1, 1]]


def test_a_malformed_form_h_in_an_unverified_set_is_counted_kept_and_named_under_verify():
    words = {8: "an entropy form with a bad header", 9: "an entropy form whose code lengths", 10: "an entropy form whose stream sizes",
             11: "an entropy form with a stream that ends early", 7: "a pad byte behind the stored span", 2: "a match offset beyond", 6: "short of the chunk's length"}
    picked = {}
    for name, entries, blob, bad, rule in ze.malformed_zpacks():
        if name.endswith("behind good entries") and rule not in picked and len(entries[bad:bad + 1]) and int(entries["length"][bad]) <= 65536:
            picked[rule] = (name, entries, blob, bad)
    assert sorted(picked) == [2, 6, 7, 8, 9, 10, 11]
    with M.Engine() as e:
        for rule, (name, entries, blob, bad) in sorted(picked.items()):
            dig = np.ascontiguousarray(entries["digest"])
            lengths = [int(n) for n in entries["length"]]
            with e.zset() as zs:
                zs.add_zblob(blob, entries)
                before = zs.info.as_dict()
                with pytest.raises(M.MiError) as ei:
                    zs.recode(level=1, verify=True, entropy=True)
                assert ei.value.code == -5 and words[rule] in str(ei.value) and "unchanged" in str(ei.value), (name, str(ei.value))
                assert {k: v for k, v in zs.info.as_dict().items() if not k.startswith("ms_")} == {k: v for k, v in before.items() if not k.startswith("ms_")}
                info = zs.recode(level=1, entropy=True)
                pads_ok = [not any(blob[int(en["offset"]) + int(en["stored"]):int(en["offset"]) + zc.round16(int(en["stored"]))]) for en in entries]
                want, n, u = zh.recode_forms(zh.forms_of(entries, blob), lengths, 1, True, pads_ok)
                assert (info.n_undecodable, info.n_recoded) == (u, n) == (1, n), name
                with zs.zpack(dig) as z:                                # the damaged form is kept verbatim
                    got = zh.forms_of(z.entries(), z.read())
                assert got == want and got[bad] == zh.forms_of(entries, blob)[bad], name
