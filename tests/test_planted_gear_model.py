"""The planted-candidate scenarios (tests/planted_gear.py) on the CPU: for every row of the table the planted set IS
the oracle's candidate set, the plain-Python selection equals the oracle's chunkers, and the model of the kernel's
passes reports the branch the row is named for -- so that tests/test_gpu_gear_planted.py, which runs the same rows on
the GPU, provably walks those branches.  No GPU use.  Cut points: parity UNPINNED w.r.t. the reference (it has no CDC).
"""
import numpy as np
import pytest

import planted_gear as P

NAMES = list(P.SCENARIOS)


def _oracle_params(oracle, p):
    return oracle.CdcParams(p.seed, p.mask_bits, p.min_size, p.max_size)


# ---- the tools themselves ------------------------------------------------------------------------------------------

def test_a_stone_in_filler_is_one_candidate(oracle):
    st = P.stones()
    assert st.shape == (48, 64) and len({s.tobytes() for s in st}) == 48
    fill = bytes([P.FILL]) * 200
    for s in st:
        assert oracle.gear_candidates(fill + s.tobytes() + fill, P.SEED, 13).tolist() == [264]
    for s in P.salts():
        assert oracle.gear_candidates(fill + s.tobytes() + fill, P.SEED, 13).size == 0
    assert oracle.gear_candidates(bytes([P.FILL]) * 5000, P.SEED, 13).size == 0


def test_stones_for_another_mask_and_filler(oracle):
    st = P.stones(P.SEED, 10, 0x00, 8)
    fill = bytes(200)
    for s in st:
        assert oracle.gear_candidates(fill + s.tobytes() + fill, P.SEED, 10).tolist() == [264]


def test_plant_is_exact_and_varied(oracle):
    ends = [64, 128, 192, 5000, 5064, 40000, 65536]
    data = P.plant(65536, ends)
    assert len(data) == 65536
    assert oracle.gear_candidates(data, P.SEED, 13).tolist() == ends
    assert P.plant(65536, ends) == data                                  # the same bytes every time
    assert P.plant(65536, ends, seed=1) != data
    assert len({data[e - 64:e] for e in ends}) > 1                       # not one stone everywhere
    assert P.plant(0, []) == b"" and P.plant(10, []) == bytes([P.FILL]) * 10
    sixteen = list(range(1024 + 64, 1024 + 64 * 17, 64))                 # 16 stones back to back in one run
    assert oracle.gear_candidates(P.plant(4096, sixteen), P.SEED, 13).tolist() == sixteen


@pytest.mark.parametrize("size,ends", [(1000, [63]), (1000, [100, 163]), (1000, [1001])])
def test_plant_refuses_what_it_cannot_do(size, ends):
    with pytest.raises(ValueError):
        P.plant(size, ends)


def test_select_by_hand():
    """Worked from the spec's sentence, not from code: min 10, max 50."""
    assert P.select([], 0, 10, 50) == []
    assert P.select([], 7, 10, 50) == [7]
    assert P.select([], 120, 10, 50) == [50, 100, 120]
    assert P.select([9, 10, 19, 20, 61, 62], 70, 10, 50) == [10, 20, 61, 70]      # 9: too close; 19: 9 from 10
    assert P.select([5, 60, 70], 70, 10, 50) == [50, 60, 70]                      # forced at 50, 60 is 10 from it
    assert P.select([51], 100, 10, 50) == [50, 100]                               # 51 is 1 from the forced cut
    assert P.select([50], 100, 10, 50) == [50, 100]
    assert P.select([100], 100, 10, 50) == [50, 100]
    assert P.select([95], 100, 10, 50) == [50, 95, 100]                           # the end cuts however close


def test_classify_by_hand():
    """Two groups and a bit, worked from the header comment of gear_cdc.hip."""
    G, T = P.G, P.T
    # G+1000 is too close to a cut assumed at G, but 2900 behind group 0's last cut; G+2500 is the other way round:
    # group 1's speculation and its validation run 1500 bytes apart on forced cuts and never meet
    ends = [3000, G - 1900, G + 1000, G + 2500, 2 * G + 3000]
    cls = P.classify(ends, 2 * G + 5000)
    g0, g1, g2 = cls["groups"]
    assert g0["spec"] == [3000, 3000 + 65536, 3000 + 2 * 65536, 3000 + 3 * 65536, G - 1900]
    assert g1["spec"] == [G + 2500 + 65536 * k for k in range(4)] and g1["assumed"] == G - 1900
    assert (g1["meet"], g1["prefix_n"], g1["redo"]) == ("never", 4, False)
    assert g1["cuts"] == [G + 1000 + 65536 * k for k in range(4)]
    # group 2 was validated from group 1's speculative exit G+199108, which forces a cut at 2G+2500; the true exit
    # G+197608 forces one at 2G+1000.  Either leaves 2G+3000 too close: both meet the speculation only at the file end
    assert g2["spec"] == [2 * G + 3000, 2 * G + 5000] and g2["assumed"] == G + 199108 and g2["meet"] == 1
    assert (g2["redo"], g2["redo_meet"], g2["cuts"]) == (True, 1, [2 * G + 1000, 2 * G + 5000])
    assert cls["cuts"] == P.select(ends, 2 * G + 5000, 2048, 65536)
    assert [t["count"] for t in cls["tiles"]] == [1, 0, 0, 1, 2, 0, 0, 0, 1]
    small = P.classify([100, 200, 300, 400, 500, 600, 700, 5000], T)
    assert not small["large"] and small["tiles"][0] == dict(count=8, max_run=7, top_run=0, dense=True, listable=True)
    assert small["cuts"] == [5000, T]


# ---- every scenario ------------------------------------------------------------------------------------------------

def test_the_table_names_every_branch():
    says = " | ".join(s.says for s in P.SCENARIOS.values())
    for words in ("pack overflows", "exactly 64", "65 candidates in a tile", "index 63 of", "index 64 of", "index 65 of",
                  "never meets", "cascades over three groups", "63, 64, 65, 255, 256, 257", "R-1 = 129",
                  "c+min_minus_1", "c+min,", "c+max,", "c+max_plus_1", "tile_first", "group_last",
                  "forced cut lands on tile end", "exactly full", "the bitmap is searched", "halo"):
        assert words in says, words
    assert len(NAMES) == len(set(NAMES)) >= 100
    # the one kind of selection row that no off-by-one selection can tell apart is the candidate just inside max_size
    assert [n for n in NAMES if n.startswith(("select_", "forced_")) and not P.SCENARIOS[n].variants] == \
        ["select_max_minus_1_at_" + pos for pos in ("mid", "tile_first", "tile_last", "group_first", "group_last")]


@pytest.mark.parametrize("name", NAMES)
def test_planted_set_is_the_candidate_set(oracle, name):
    b = P.built(name)
    p = b["sc"].params
    got = oracle.gear_candidates(b["data"], p.seed, p.mask_bits)
    assert len(b["data"]) == b["size"]
    assert np.array_equal(got, np.asarray(b["ends"], dtype=np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_select_is_the_oracles_selection(oracle, name):
    b = P.built(name)
    p = b["sc"].params
    op = _oracle_params(oracle, p)
    a = np.frombuffer(b["data"], dtype=np.uint8)
    want = np.asarray(b["cuts"], dtype=np.uint64)
    assert np.array_equal(oracle.cdc_classic(a, op), want)
    assert np.array_equal(oracle.cdc_two_phase(a, op), want)
    assert np.array_equal(oracle.cdc_select(b["ends"], b["size"], p.min_size, p.max_size), want)


@pytest.mark.parametrize("name", NAMES)
def test_classify_reports_the_branch(name):
    b = P.built(name)
    assert P.observed(b) == b["sc"].expect, b["sc"].says
    assert b["cls"]["cuts"] == b["cuts"]                 # the model of the passes ends at the spec's cuts
    assert b["cls"]["large"] == (b["size"] > P.T)
    for g in b["cls"]["groups"]:                         # a group's two regions of ends32 hold what the passes write
        assert len(g["spec"] or []) <= P.region(b["sc"].params) and g["prefix_n"] <= P.region(b["sc"].params)


@pytest.mark.parametrize("name,variant", [(n, v) for n in NAMES for v in P.SCENARIOS[n].variants])
def test_boundary_input_tells_an_off_by_one_apart(name, variant):
    b = P.built(name)
    p = b["sc"].params
    assert P.select(b["ends"], b["size"], p.min_size + variant[0], p.max_size + variant[1]) != b["cuts"]


@pytest.mark.parametrize("name", [n for n in NAMES if P.SCENARIOS[n].parts])
def test_parts_need_more_than_one_round(name):
    """Some halo leaves on the wrong phase: the first exchange changes an entry.  The entries the exchange settles on are
    the cuts select() puts at or before the parts' first bytes."""
    b = P.built(name)
    bounds = b["sc"].parts
    assert bounds[0][0] == 0 and bounds[-1][1] == b["size"] and all(lo % P.G == 0 for lo, _ in bounds)
    assert all(a[1] == c[0] for a, c in zip(bounds, bounds[1:]))
    rounds, entries = P.part_rounds(b["ends"], b["size"], bounds, b["sc"].params)
    assert rounds > 1
    assert entries == [max([0] + [c for c in b["cuts"] if c <= lo]) for lo, _ in bounds]


def test_chunks_of_a_planted_file_differ(oracle):
    """dup_of has to be worth checking: most chunks of a lattice file are unique, a few are not."""
    b = P.built("rejoin_never_chain_2")
    _, rc = oracle.scan_batch(np.frombuffer(b["data"], dtype=np.uint8), np.array([0], dtype=np.uint64),
                              np.array([b["size"]], dtype=np.uint64), _oracle_params(oracle, b["sc"].params))
    assert (rc["dup_of"] < 0).sum() > 0.9 * len(rc)
