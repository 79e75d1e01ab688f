"""Planted Gear candidates: files whose candidate set is chosen, not drawn ("Planting
candidates").  Test infrastructure only: numpy and the CPU oracle, no GPU.

h_i depends only on the 64 bytes ending at i.  A 64-byte STONE whose hash has mask_bits zero top bits, laid into a
constant filler, puts a candidate exactly at the stone's end and nowhere else -- provided no window that mixes stone
and filler is a candidate too, which stones() checks.  plant() lays stones at the wanted ends, sprinkles SALTS (short
strings checked to add no candidate) into the filler so that chunks differ, and verifies the result against the oracle.

    stones(), plant()   content with exactly the wanted candidates
    select()            the spec's selection (DESIGN.md "Gear-CDC spec") in plain Python: a third opinion beside the
                        oracle's two chunkers
    classify()          a model of what gear_cdc.hip's passes do with a candidate set (from that file's header
                        comment): which tiles are dense, what a group speculates, where validation meets the
                        speculation, which groups the per-file pass redoes.  It lets a test state on the CPU that an
                        input forces the branch the test is named after.
    SCENARIOS           the table tests/test_planted_gear_model.py (CPU) and tests/test_gpu_gear_planted.py share
"""
import bisect
import collections
import functools

import numpy as np

from oracle import mi_oracle as O

SEED = 0x4D414B49
T = 64 * 1024            # tile: one wave marks it
RUN = 1024               # a lane's run of a tile
G = 4 * T                # group: four tiles, cut speculatively
LIST = 64                # entries of a tile's candidate list
PACK = 6                 # candidates a lane packs per run
W = 64                   # bytes of the hash window = length of a stone

Params = collections.namedtuple("Params", "seed mask_bits min_size max_size")
DEFAULT = Params(SEED, 13, 2048, 65536)
FILL = 0x5A
SALT_LEN = 8
SALT_STRIDE = 512


def region(params=DEFAULT):
    """Entries of a group's spec list and of its prefix list in ends32."""
    return G // params.min_size + 2


# ---- stones and salts ------------------------------------------------------------------------------------------

def _is_cand(h, mask_bits):
    return (h >> np.uint64(64 - mask_bits)) == 0 if mask_bits else np.ones(h.shape, dtype=bool)


def _fill_ok(table, mask_bits, fill):
    """No candidate in a file of `fill` bytes only: neither in the partial windows of its first 63 bytes nor later."""
    h = np.zeros(1, dtype=np.uint64)
    for _ in range(2 * W):
        h = (h << np.uint64(1)) + table[fill]
        if _is_cand(h, mask_bits)[0]:
            return False
    return True


def _search(seed, mask_bits, fill, length, n, want_end, rng):
    """n strings of `length` bytes such that fill*64 + string + fill*64 has exactly one candidate, at the string's last
    byte (want_end), or none at all."""
    table = O.gear_table(seed)
    if not _fill_ok(table, mask_bits, fill):
        raise ValueError("filler byte 0x%02x makes candidates by itself" % fill)
    found = []
    one = np.uint64(1)
    while sum(len(f) for f in found) < n:
        batch = 100000 if want_end else 4 * n
        s = rng.integers(0, 256, (batch, length), dtype=np.uint8)
        h = np.zeros(batch, dtype=np.uint64)
        for _ in range(W):
            h = (h << one) + table[fill]
        stray = np.zeros(batch, dtype=bool)
        at_end = np.zeros(batch, dtype=bool)
        for j in range(length + W - 1):                  # every window that holds a byte of the string
            h = (h << one) + (table[s[:, j]] if j < length else table[fill])
            c = _is_cand(h, mask_bits)
            if j == length - 1:
                at_end = c
            else:
                stray |= c
        keep = ~stray & (at_end if want_end else ~at_end)
        found.append(s[keep])
    return np.concatenate(found)[:n].copy()


@functools.lru_cache(maxsize=None)
def stones(seed=SEED, mask_bits=13, fill=FILL, n=48):
    """(n, 64) u8: stones for this table, mask and filler.  Fixed RNG: the same stones in every process."""
    return _search(seed, mask_bits, fill, W, n, True, np.random.default_rng([0x570E, seed, mask_bits, fill]))


@functools.lru_cache(maxsize=None)
def salts(seed=SEED, mask_bits=13, fill=FILL, n=8):
    return _search(seed, mask_bits, fill, SALT_LEN, n, False, np.random.default_rng([0x5A17, seed, mask_bits, fill]))


def plant(size, ends, fill=FILL, params=DEFAULT, seed=0):
    """bytes of length `size` whose candidate set (cut END offsets, oracle.gear_candidates) is exactly `ends`.
    Ends are >= 64 and at least 64 apart.  Stones and salts are drawn per position, so chunks differ; a draw that
    makes a stray candidate (two stones back to back can) is drawn again.  Raises if it cannot be done."""
    e = np.asarray(sorted(int(x) for x in ends), dtype=np.int64)
    if e.size:
        if e[0] < W or e[-1] > size or (np.diff(e) < W).any():
            raise ValueError("planted ends must be >= 64, <= size and 64 apart")
    st, sa = stones(params.seed, params.mask_bits, fill), salts(params.seed, params.mask_bits, fill)
    # gaps of pure filler: [lo, hi); a salt keeps 64 bytes away from the stones on both sides
    lo = np.concatenate([[0], e])
    hi = np.concatenate([e - W, [size]])
    first = lo + W
    room = hi - W - SALT_LEN - first
    n_s = np.where(room >= 0, room // SALT_STRIDE + 1, 0)
    k = np.arange(int(n_s.sum())) - np.repeat(np.cumsum(n_s) - n_s, n_s)
    spos = np.repeat(first, n_s) + SALT_STRIDE * k
    for attempt in range(8):
        rng = np.random.default_rng([0x91A7, seed, attempt, size, e.size])
        buf = np.full(size, fill, dtype=np.uint8)
        if e.size:
            buf[(e - W)[:, None] + np.arange(W)] = st[rng.integers(0, len(st), e.size)]
        if spos.size:
            buf[spos[:, None] + np.arange(SALT_LEN)] = sa[rng.integers(0, len(sa), spos.size)]
        got = O.gear_candidates(buf, params.seed, params.mask_bits).astype(np.int64) if size else e[:0]
        if np.array_equal(got, e):
            return buf.tobytes()
    raise RuntimeError("could not plant exactly these candidates: %d wanted, %d found" % (e.size, got.size))


# ---- the spec's selection -----------------------------------------------------------------------------------------

def select(ends, size, min_size, max_size):
    """Chunk ends of a file with these candidates.  DESIGN.md: from the previous cut L, skip candidates with
    e - L < min_size, force a cut at L + max_size, the file end always cuts."""
    cuts, last, i = [], 0, 0
    while last < size:
        while i < len(ends) and ends[i] - last < min_size:
            i += 1
        cut = ends[i] if i < len(ends) and ends[i] - last <= max_size else last + max_size
        last = min(cut, size)
        cuts.append(last)
    return cuts


# ---- a model of the kernel's passes -------------------------------------------------------------------------------

def _walk(cands, last, floor, stop, p):
    """Cuts in (floor, stop] selected from `last` (<= floor): candidates first, a forced cut only if it still lies
    inside -- what the kernel's tile-by-tile selection amounts to over a stretch of tiles."""
    while True:
        lo, hi = max(last + p.min_size, floor + 1), min(last + p.max_size, stop)
        j = bisect.bisect_left(cands, lo)
        if lo <= hi and j < len(cands) and cands[j] <= hi:
            last = cands[j]
        elif last + p.max_size <= stop:
            last += p.max_size
        else:
            return
        yield last


def classify(ends, size, params=DEFAULT, open_end=False):
    """What the passes of gear_cdc.hip do with candidate set `ends` in a file of `size` bytes.

    -> dict: large (bool), tiles [dict(count, max_run, dense, listable)], groups [dict(...)], cuts.
    A tile is DENSE under the marking kernels' rule: more than 64 candidates, or more than 6 in one 1 KiB run;
    listable: the per-file pass can still build its 64-entry list from the bitmap (<= 64 candidates).
    A group: dense (some tile is), spec (the speculative cuts from a cut assumed at its first byte; None if dense),
    assumed (the entry validation used: the previous group's speculative exit; None if validation skipped it),
    meet (spec index where validation met the spec list, "never", or None), redo (the per-file pass re-selected it),
    redo_meet (the same for that re-selection), entry (true), cuts (final, absolute), exit."""
    cands = sorted(int(x) for x in ends)
    idx = np.asarray(cands, dtype=np.int64) - 1                  # byte index of a candidate: bit idx <-> end idx + 1
    n_tiles = -(-size // T)
    count = np.bincount(idx // T, minlength=n_tiles) if n_tiles else np.zeros(0, dtype=np.int64)
    per_run = np.bincount(idx // RUN, minlength=n_tiles * (T // RUN)).reshape(n_tiles, T // RUN)
    tiles = [dict(count=int(count[t]), max_run=int(per_run[t].max()), top_run=int(per_run[t].argmax()),
                  dense=bool(count[t] > LIST or per_run[t].max() > PACK), listable=bool(count[t] <= LIST))
             for t in range(n_tiles)]
    if size <= T:                                                # one wave, one tile, no speculation
        cuts = list(_walk(cands, 0, 0, size, params))
        if size and (not cuts or cuts[-1] < size):
            cuts.append(size)
        return dict(large=False, tiles=tiles, groups=[], cuts=cuts)

    def reselect(g, entry):
        assert entry <= g["g0"] < entry + params.max_size
        where = {c: i for i, c in enumerate(g["spec"] or [])}
        prefix, last, meet = [], entry, "never"
        for c in _walk(cands, entry, g["g0"], g["gend"], params):
            if c in where:
                meet = where[c]
                break
            prefix.append(c)
            last = c
        if meet == "never" and g["last"] and not open_end and size > last:
            if size in where:
                meet = where[size]
            else:
                prefix.append(size)
                last = size
        tail = [] if meet == "never" else g["spec"][meet:]
        return meet, prefix + tail, (last if meet == "never" else g["spec_exit"]), len(prefix)

    groups = []
    for gi in range(-(-size // G)):
        g0, gend = gi * G, min(gi * G + G, size)
        g = dict(g0=g0, gend=gend, last=gend == size, dense=any(t["dense"] for t in tiles[4 * gi:4 * gi + 4]),
                 spec=None, spec_exit=None, assumed=None, meet=None, prefix_n=0, valid=False, redo=False,
                 redo_meet=None)
        if not g["dense"]:                                       # A2: speculate
            spec = list(_walk(cands, g0, g0, gend, params))
            if g["last"] and not open_end and size > (spec[-1] if spec else g0):
                spec.append(size)
            g["spec"], g["spec_exit"] = spec, spec[-1] if spec else g0
            if gi == 0:
                g.update(valid=True, assumed=0, cuts=spec, exit=g["spec_exit"])
        groups.append(g)
    for gi, g in enumerate(groups):                              # B: validate against the previous group's speculation
        if gi and not g["dense"] and not groups[gi - 1]["dense"]:
            g["assumed"] = groups[gi - 1]["spec_exit"]
            g["meet"], g["cuts"], g["exit"], g["prefix_n"] = reselect(g, g["assumed"])
            g["valid"] = True
    prev_exit = 0
    for g in groups:                                             # C: per file, in order
        if not g["valid"] or g["assumed"] != prev_exit:
            g["redo"] = True
            g["redo_meet"], g["cuts"], g["exit"], g["prefix_n"] = reselect(g, prev_exit)
        g["entry"] = prev_exit
        prev_exit = g["exit"]
    return dict(large=True, tiles=tiles, groups=groups, cuts=[c for g in groups for c in g["cuts"]])



def part_rounds(ends, size, bounds, params=DEFAULT):
    """What the exchange of include/makisu_mi.h "parts" does: every part is cut behind a halo of whole groups as if a
    cut fell on the halo's first byte; then, round by round, a part whose entry is not its predecessor's exit takes that
    exit and is cut again.  -> (rounds, the parts' final entries)."""
    cands = sorted(int(x) for x in ends)
    halo = -(-params.max_size // G) * G

    def exit_of(entry, lo, hi):
        cuts = list(_walk(cands, entry, lo, hi, params))
        return size if hi == size else (cuts[-1] if cuts else entry)
    entries = [0 if lo == 0 else exit_of(max(lo - halo, 0), max(lo - halo, 0), lo) for lo, hi in bounds]
    rounds = 0
    while True:
        rounds += 1
        exits = [exit_of(e, lo, hi) for e, (lo, hi) in zip(entries, bounds)]
        want = [0] + exits[:-1]
        if want == entries:
            return rounds, entries
        entries = want


# ---- scenarios ----------------------------------------------------------------------------------------------------
# One table for the CPU model tests and the GPU tests.  A scenario names the branch it is built for (`says`), makes
# (size, ends), and states what classify()/select() must report for it: observe(cls, ends, size, cuts) == expect.
# variants: off-by-one selections (min_size + a, max_size + b) that MUST cut this input differently from the spec.
# parts: byte ranges the file is split into (a parts scenario).  Built lazily, once per process: built(name).

Scenario = collections.namedtuple("Scenario", "name says params make observe expect variants parts")
SCENARIOS = collections.OrderedDict()
MIN, MAX = DEFAULT.min_size, DEFAULT.max_size


def _add(name, says, make, observe, expect, params=DEFAULT, variants=(), parts=None):
    assert name not in SCENARIOS
    SCENARIOS[name] = Scenario(name, says, params, make, observe, expect, tuple(variants), parts)


BIG = 8 << 20
_built, _built_big = {}, {}


def built(name):
    """-> dict(sc, size, ends, data, cls, cuts): the scenario's file, planted and verified.  Kept for the process; of
    the files of many groups only the last one made (both test files walk the table in order)."""
    b = _built.get(name) or _built_big.get(name)
    if b is None:
        sc = SCENARIOS[name]
        size, ends = sc.make()
        ends = sorted(ends)
        b = dict(sc=sc, size=size, ends=ends, data=plant(size, ends, params=sc.params, seed=len(name)),
                 cls=classify(ends, size, sc.params), cuts=select(ends, size, sc.params.min_size, sc.params.max_size))
        if size >= BIG:
            _built_big.clear()
            _built_big[name] = b
        else:
            _built[name] = b
    return b


def observed(b):
    return b["sc"].observe(b["cls"], b["ends"], b["size"], b["cuts"])


def _lat(start, stop, step=3000):
    return list(range(start, stop, step))


# group recipes (gi: group index).  S: one phase -- candidates 3000 apart, the first 2100 into the group: every one is
# a cut whatever the entry, so speculation always holds.  P2: two phases -- 1500 apart, selection takes every second
# one; a selection on the other phase never comes back unless a candidate is missing: dropping candidate 2m merges
# the even phase into the odd one at the odd phase's m-th cut.
def S(gi, n=87):
    return [gi * G + 2100 + 3000 * k for k in range(n)]


def P2(gi, off=600, drop=()):
    return [gi * G + off + 1500 * k for k in range((G - off) // 1500 + 1) if k not in drop]


def D(gi, t, n=65, tiles=4, rest=3000):
    """A group whose tile t holds n candidates, one per 1 KiB run (two in run 10 for the 65th); its other tiles sparse."""
    ts = gi * G + t * T
    dense = [ts + RUN * r + 501 for r in range(min(n, 64))] + [ts + RUN * 10 + 801] * (n - 64)
    return sorted(dense + [e for e in _lat(gi * G + 2100 - rest, gi * G + tiles * T - 64, rest)
                           if e > gi * G + W and not ts - 64 < e <= ts + T + 64])


def _tile(t):
    return lambda cls, ends, size, cuts: {k: cls["tiles"][t][k] for k in ("count", "max_run", "top_run", "dense")}


def _groups(*gis, keys=("dense", "meet", "redo", "redo_meet")):
    def obs(cls, ends, size, cuts):
        out = {gi: tuple(cls["groups"][gi][k] for k in keys) for gi in gis}
        out["redone"] = [i for i, g in enumerate(cls["groups"]) if g["redo"]]
        return out
    return obs


def _both(*observers):
    def obs(cls, ends, size, cuts):
        out = {}
        for o in observers:
            out.update(o(cls, ends, size, cuts))
        return out
    return obs


# -- packing and lists: as a small file (one tile) and as tile 6 (group 1, tile 2) of a large file
LARGE_TILE = 6


def _small(local):
    return lambda: (T, list(local))


def _in_large(local, tile=LARGE_TILE, size=3 * G + 777):
    base = tile * T
    return lambda: (size, _lat(3000, base - 64) + [base + x for x in local] + _lat(base + T + 2000, size - 64))


def _pack(name, says, local, expect_tile, large_group=None, small=True):
    """expect_tile: count, max_run, top_run, dense of the tile; large_group: what group 1 of the large file does"""
    exp = dict(zip(("count", "max_run", "top_run", "dense"), expect_tile))
    if small:
        _add(name + "_small", says + " (a small file)", _small(local), _tile(0), exp)
    gexp = dict(exp)
    gexp[1] = large_group or (exp["dense"], None if exp["dense"] else 0, exp["dense"], "never" if exp["dense"] else None)
    gexp["redone"] = [1, 2] if exp["dense"] else []
    _add(name + "_large", says + " (tile 2 of group 1 of a large file)", _in_large(local),
         _both(_tile(LARGE_TILE), _groups(1)), gexp)


_REST = [r * RUN + 501 for r in (8, 24, 40, 56)]
for _k in (3, 4, 6, 7):
    for _lane in (0, 31, 63):
        _pack("pack_%d_in_run_lane%d" % (_k, _lane),
              "%d candidates in the 1 KiB run of lane %d, the rest of the tile sparse: %s" %
              (_k, _lane, "the lane's pack overflows, the tile is dense with %d candidates and its list is rebuilt "
               "from the bitmap" % (_k + 4) if _k > PACK else "packed in the lane's two registers"),
              [_lane * RUN + 101 + 128 * j for j in range(_k)] + _REST, (_k + 4, _k, _lane, _k > PACK))
_pack("tile_64", "exactly 64 candidates in a tile, one per run: the list is full, not dense",
      [r * RUN + 501 for r in range(64)], (64, 1, 0, False))
_pack("tile_65", "65 candidates in a tile, at most 2 per run: one more than the list holds, dense",
      [r * RUN + 501 for r in range(64)] + [10 * RUN + 801], (65, 2, 10, True))
_SEVEN = [5 * RUN + 101 + 128 * j for j in range(7)]
_pack("overflow_and_64", "7 candidates in one run and 64 in the tile: the list rebuilt from the bitmap is exactly full",
      _SEVEN + [r * RUN + 501 for r in range(6, 63)], (64, 7, 5, True))
_pack("overflow_and_65", "7 candidates in one run and 65 in the tile: the list cannot be rebuilt, the bitmap is searched",
      _SEVEN + [r * RUN + 501 for r in range(6, 64)], (65, 7, 5, True))


def _run_index(cls, ends, size, cuts, tile=0):
    return {"index_in_run": [(e - 1) % RUN for e in ends if (e - 1) // T == tile],
            "stone_starts_in_run": [((e - W) % T) // RUN for e in ends if (e - 1) // T == tile],
            "run": [((e - 1) % T) // RUN for e in ends if (e - 1) // T == tile]}


_add("run_index_0_and_1023_small", "candidates at byte 0 and byte 1023 of a run, and at the tile's last byte",
     _small([5 * RUN + 1, 9 * RUN, T]), _run_index,
     {"index_in_run": [0, 1023, 1023], "stone_starts_in_run": [4, 8, 63], "run": [5, 8, 63]})
_add("run_index_0_and_1023_large", "candidates at byte 0 and 1023 of a run, at a tile's first and last byte",
     _in_large([1, 5 * RUN + 1, 9 * RUN, T]), functools.partial(_run_index, tile=LARGE_TILE),
     {"index_in_run": [0, 0, 1023, 1023], "stone_starts_in_run": [63, 4, 8, 63], "run": [0, 5, 8, 63]})
_STRADDLE = [10 * RUN + 1, 20 * RUN + 32, 30 * RUN + 63, 40 * RUN + 64]
_add("straddle_run_small", "stones across a run boundary: the candidate 1, 32, 63, 64 bytes into the next run",
     _small(_STRADDLE), _run_index,
     {"index_in_run": [0, 31, 62, 63], "stone_starts_in_run": [9, 19, 29, 40], "run": [10, 20, 30, 40]})
_add("straddle_run_large", "stones across a run boundary: the candidate 1, 32, 63, 64 bytes into the next run",
     _in_large(_STRADDLE), functools.partial(_run_index, tile=LARGE_TILE),
     {"index_in_run": [0, 31, 62, 63], "stone_starts_in_run": [9, 19, 29, 40], "run": [10, 20, 30, 40]})
_add("straddle_tile_and_group", "stones across a tile boundary (5T, 6T, 7T) and a group boundary (G, 2G)",
     lambda: (3 * G + 777, sorted(set(_lat(3000, 3 * G, 9000)) | {5 * T + 1, 6 * T + 32, 7 * T + 63, G + 1, 2 * G + 32})),
     lambda cls, ends, size, cuts: {"first_in_tile": {(e - 1) // T: (e - 1) % T for e in ends if (e - 1) % T < 63}},
     {"first_in_tile": {5: 0, 6: 31, 7: 62, 4: 0, 8: 31}})
for _tag, _sz in (("small", 50000), ("large", 2 * G + 12345)):
    for _nm, _d in (("last_byte", 0), ("byte_before_last", 1)):
        _add("candidate_at_%s_%s" % (_nm, _tag), "a candidate whose end is the file's %s" % _nm.replace("_", " "),
             (lambda sz=_sz, d=_d: (sz, _lat(3000, sz - 3000) + [sz - d])),
             lambda cls, ends, size, cuts: {"from_end": size - ends[-1], "last_chunk": cuts[-1] - cuts[-2]},
             {"from_end": _d, "last_chunk": (_sz - _d) - _lat(3000, _sz - 3000)[-1] if _d == 0 else 1})


# -- selection boundaries: the previous cut is c, the candidate (or the forced cut) at e = c + delta
def _boundary(e, delta, cand=True, size=2 * G + 5000):
    c = e - delta
    return lambda: (size, _lat(c % 3000 + 3000, c + 1) + ([e] if cand else []) + _lat(e + 3000, size - 64))


def _boundary_obs(e, delta):
    c = e - delta
    return lambda cls, ends, size, cuts: {"c_cut": c in cuts, "e_cut": e in cuts, "forced": c + MAX in cuts,
                                          "e_in_tile": (e - 1) % T, "tiles_back": (e - 1) // T - (c - 1) // T}


_POS = collections.OrderedDict([("mid", 2 * T + 30000), ("tile_first", 3 * T + 1), ("tile_last", 3 * T),
                                ("group_first", G + 1), ("group_last", G)])
# delta -> (name, e is a cut, a forced cut falls at c + max, the variants that must differ)
_DELTA = [(MIN - 1, "min_minus_1", False, False, [(-1, 0)]), (MIN, "min", True, False, [(1, 0)]),
          # a candidate at c + max - 1 is taken by every off-by-one selection as well: the control of the set
          (MAX - 1, "max_minus_1", True, False, []), (MAX, "max", True, True, [(0, -1)]),
          (MAX + 1, "max_plus_1", False, True, [(0, 1)])]
for _pn, _e in _POS.items():
    for _delta, _dn, _ecut, _forced, _var in _DELTA:
        _add("select_%s_at_%s" % (_dn, _pn), "a candidate at c+%s, at %s" % (_dn, _pn), _boundary(_e, _delta),
             _boundary_obs(_e, _delta),
             {"c_cut": True, "e_cut": _ecut, "forced": _forced, "e_in_tile": (_e - 1) % T,
              "tiles_back": (_e - 1) // T - (_e - _delta - 1) // T}, variants=_var)
for _pn, _e in (("tile_end", 3 * T), ("tile_end_plus_1", 3 * T + 1), ("group_end", G), ("group_end_plus_1", G + 1)):
    _add("forced_cut_at_" + _pn, "no candidate for max_size bytes: the forced cut lands on " + _pn.replace("_", " "),
         _boundary(_e, MAX, cand=False), _boundary_obs(_e, MAX),
         {"c_cut": True, "e_cut": True, "forced": True, "e_in_tile": (_e - 1) % T, "tiles_back": 1},
         variants=[(0, -1), (0, 1)])
_add("empty_tile_carried", "tile 2 has no candidate: the cut before it is carried in and forces a cut inside it",
     _boundary(3 * T - 1000, MAX, cand=False),
     _both(_tile(2), lambda cls, ends, size, cuts: {"forced_in_tile_2": 3 * T - 1000 in cuts}),
     {"count": 0, "max_run": 0, "top_run": 0, "dense": False, "forced_in_tile_2": True})


# -- speculation
def _file(groups, tail=1234):
    return lambda: (len(groups) * G + tail, [e for g in groups for e in g])


for _m, _nm in ((0, "0"), (1, "1"), (63, "63"), (64, "64"), (65, "65"), (86, "last_cut")):
    _add("rejoin_at_" + _nm, "group 1 validates on the other phase and meets its spec list at index %d of 87" % _m,
         _file([S(0), P2(1, drop=(2 * _m,)), S(2)]), _groups(1, keys=("meet", "prefix_n", "redo")),
         {1: (_m, _m, False), "redone": []})
_add("rejoin_never_chain_1", "group 1 never meets its spec list: group 2's entry is wrong, its repair holds",
     _file([S(0), P2(1), S(2), S(3)]), _groups(1, 2, 3),
     {1: (False, "never", False, None), 2: (False, 0, True, 0), 3: (False, 0, False, None), "redone": [2]})
_add("rejoin_never_chain_2", "groups 1 and 2 never rejoin (2 in its repair): the repair cascades to group 3 and holds",
     _file([S(0), P2(1), P2(2, off=1600), S(3), S(4)]), _groups(1, 2, 3, 4),
     {1: (False, "never", False, None), 2: (False, "never", True, "never"), 3: (False, 0, True, 0),
      4: (False, 0, False, None), "redone": [2, 3]})
_add("rejoin_never_chain_3", "groups 1, 2, 3 never rejoin: the repair cascades over three groups and then holds",
     _file([S(0), P2(1), P2(2, off=1600), P2(3), S(4), S(5)]), _groups(1, 2, 3, 4, 5),
     {1: (False, "never", False, None), 2: (False, "never", True, "never"), 3: (False, 0, True, "never"),
      4: (False, 0, True, 0), 5: (False, 0, False, None), "redone": [2, 3, 4]})
_add("rejoin_at_file_end", "the file's last group validates on the other phase until the file end, its last spec cut",
     _file([S(0), P2(1)], tail=0), _groups(1, keys=("meet", "prefix_n", "redo")), {1: (87, 88, False), "redone": []})
# the second candidate of group 1's lattice lies min_size behind the true cut (min_size - 1 behind it for g0+1): the
# true selection and the speculation from g0 disagree about it unless the true cut IS g0
for _d, _nm, _off, _meet, _taken in ((0, "g0", 548, 0, True), (-1, "g0_minus_1", 547, "never", True),
                                     (1, "g0_plus_1", 548, "never", False)):
    _add("true_cut_at_" + _nm, "a true cut at %s, then a two-phase group whose second candidate is %d bytes behind it"
         % (_nm, _off + 1500 - _d),
         _file([S(0, 86) + [G + _d], P2(1, off=_off), S(2)]),
         _both(_groups(1, keys=("meet", "redo")),
               lambda cls, ends, size, cuts, d=_d, o=_off: {"cut": G + d in cuts, "second": G + o + 1500 in cuts}),
         {1: (_meet, False), "redone": [] if _meet == 0 else [2], "cut": True, "second": _taken})


def _spacing_1024():
    return 6 * G, _lat(3 * RUN, 6 * G + 1, RUN)


_add("spacing_1024_full_regions", "candidates 1 KiB apart: 64 per tile, two phases at min_size; every group from 2 "
     "on is repaired on the wrong phase; the last holds R-1 = 129 cuts behind a prefix of 128",
     _spacing_1024,
     lambda cls, ends, size, cuts: {"tile_counts": sorted(set(t["count"] for t in cls["tiles"][1:])),
                                    "redone": [i for i, g in enumerate(cls["groups"]) if g["redo"]],
                                    "last": tuple(cls["groups"][5][k] for k in ("redo_meet", "prefix_n")),
                                    "last_cuts": len(cls["groups"][5]["cuts"]), "R": region()},
     {"tile_counts": [64], "redone": [2, 3, 4, 5], "last": (127, 128), "last_cuts": 129, "R": 130})
BIG_MAX = Params(SEED, 13, 2048, 1 << 20)
_add("groups_without_a_cut", "max_size 1 MiB: groups 1 and 2 hold no cut at all",
     lambda: (6 * G + 100, [3000, 3 * G + 50000] + _lat(3 * G + 53000, 6 * G)),
     lambda cls, ends, size, cuts: {"cuts_in": [len(cls["groups"][i]["cuts"]) for i in (1, 2)],
                                    "redone": [i for i, g in enumerate(cls["groups"]) if g["redo"]]},
     {"cuts_in": [0, 0], "redone": [2, 3]}, params=BIG_MAX)
for _t in range(4):
    _add("dense_tile_%d_of_group" % _t, "65 candidates in tile %d of group 1: no speculation, re-marked and repaired" % _t,
         _file([S(0), D(1, _t), S(2), S(3)]), _both(_tile(4 + _t), _groups(1, 2, 3)),
         {"count": 65, "max_run": 2, "top_run": 10, "dense": True, 1: (True, None, True, "never"),
          2: (False, None, True, 0), 3: (False, 0, False, None), "redone": [1, 2]})
_add("dense_only_group", "a dense tile in a file of one partial group",
     lambda: (3 * T + 100, D(0, 1, tiles=3)), _groups(0), {0: (True, None, True, "never"), "redone": [0]})
_add("dense_last_partial_group", "a dense tile in the file's last, partial group",
     lambda: (2 * G + T + 5000, S(0) + S(1) + D(2, 0, tiles=1)), _groups(1, 2),
     {1: (False, 0, False, None), 2: (True, None, True, "never"), "redone": [2]})
_add("dense_two_in_a_row", "two dense groups in a row",
     _file([S(0), D(1, 1), D(2, 2), S(3), S(4)]), _groups(1, 2, 3, 4),
     {1: (True, None, True, "never"), 2: (True, None, True, "never"), 3: (False, None, True, 0),
      4: (False, 0, False, None), "redone": [1, 2, 3]})
_add("dense_then_speculation_fails", "a dense group, then a group whose repair never meets its speculation",
     _file([S(0), D(1, 3), P2(2), S(3), S(4)]), _groups(1, 2, 3, 4),
     {1: (True, None, True, "never"), 2: (False, None, True, "never"), 3: (False, 0, True, 0),
      4: (False, 0, False, None), "redone": [1, 2, 3]})


def _many_groups():
    gs = [S(i) for i in range(260)]
    for a in (62, 254):
        gs[a], gs[a + 1], gs[a + 2] = P2(a), P2(a + 1, off=1600), P2(a + 2)
    return _file(gs)()


MANY = "fix_pass_at_63_64_65_and_255_256_257"
_add(MANY, "260 groups: the per-file pass has to redo groups 63, 64, 65, 255, 256, 257 and no other",
     _many_groups, _groups(62, 63, 64, 65, 66),
     {62: (False, "never", False, None), 63: (False, "never", True, "never"), 64: (False, 0, True, "never"),
      65: (False, 0, True, 0), 66: (False, 0, False, None), "redone": [63, 64, 65, 255, 256, 257]})



def _first_bad(n_groups, *bad):
    """Every group holds but those in `bad`: the group before a bad one never rejoins, the bad one's repair holds."""
    def make():
        gs = [S(i) for i in range(n_groups)]
        for x in bad:
            gs[x - 1] = P2(x - 1)
        return _file(gs)()
    return make


# the per-file pass reads 256 records per round, 64 per ballot, and starts over behind a group it has redone: these put
# the FIRST bad group of a round at index 64 (second ballot, lane 0), 255 (fourth ballot, lane 63), 256 and 257 (the
# next round's lanes 0 and 1)
for _nm, _n, _bad in (("64_then_255_later", 330, (64, 65 + 255)), ("256", 260, (256,)), ("257", 260, (257,))):
    _add("fix_pass_first_bad_at_" + _nm, "the per-file pass skips ahead over good groups to groups %s only" % (_bad,),
         _first_bad(_n, *_bad), _groups(_bad[0] - 1, _bad[0]),
         {_bad[0] - 1: (False, "never", False, None), _bad[0]: (False, 0, True, 0), "redone": list(_bad)})

# -- parts
_add("parts_two_phase_lattice", "a two-phase lattice across the part boundaries: the halos speculate on the wrong phase",
     _file([S(0)] + [P2(i, off=600 if i % 2 else 1600) for i in range(1, 7)] + [S(7)]),
     _groups(1, 2, keys=("meet", "redo_meet")), {1: ("never", None), 2: ("never", "never"), "redone": [2, 3, 4, 5, 6, 7]},
     parts=[(0, 2 * G), (2 * G, 4 * G), (4 * G, 6 * G), (6 * G, 8 * G + 1234)])
_add("parts_dense_group_in_halo", "a dense group as the halo of a part, two phases around its dense tile",
     _file([S(0), P2(1), D(2, 0, rest=1500), P2(3), S(4), S(5)]), _groups(2, keys=("dense", "redo")),
     {2: (True, True), "redone": [2, 3, 4]},
     parts=[(0, G), (G, 3 * G), (3 * G, 6 * G + 1234)])
