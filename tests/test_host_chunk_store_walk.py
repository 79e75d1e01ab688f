"""The chunk store's walks on the model alone (store_walk_cases.py): the population holds what the walks need, the remembered
coder and decoder are the rule functions of zrecode_h_cases.py, every walk the GPU module runs is executed by the model with
every held good form decoded and hashed and the cut of everything passed through the host's mi_zpack_check after every step,
the coverage conditions hold per kind over its seeds, and the per-step comparison sees four planted model bugs.

MEASURED (one CPU core, this module alone): coding the population of 1 527 chunks at the four coded levels 13.8 s (6.7 s on the
GPU machine's host, where it is the GPU module's fixture) -- zpack2_cases.parse2 is most of it; drawing a walk and running it on
the model with the checks above 0.4 to 3.4 s a walk, 14 s for the nine; the four planted bugs 4 s; the whole module 35 s."""
import time

import numpy as np
import pytest

import pack_cases as pc
import store_walk_cases as sw
import zentropy_cases as ze
import zpack_cases as zc
import zprune_cases as pr
import zrecode_h_cases as zh

TIMES = {}


@pytest.fixture(scope="module")
def coded_population():
    t = time.perf_counter()
    forms = [[sw.form_of_chunk(c, k) for k in range(5)] for c in sw.population()]
    TIMES["coding"] = time.perf_counter() - t
    return forms


def test_the_population_holds_what_the_walks_need(coded_population):
    chunks = sw.population()
    assert len(set(chunks)) == len(chunks) and len(chunks) >= 1400 and max(map(len, chunks)) <= 65537
    planted = set(sw.zr.planted()[1]) | {c for _, c in ze.planted_chunks_h()}
    assert planted <= set(chunks)
    by_form = [0, 0, 0, 0]
    for c, f in zip(chunks, coded_population):
        by_form[ze.form_of(f[3], len(c))] += 1
        assert f[0] == c and all(len(f[k]) <= len(c) for k in range(5))
    assert min(by_form) >= 50, by_form
    assert sum(1 for f in coded_population if len(f[2]) < len(f[1])) >= 18
    assert sum(1 for c in chunks if len(c) < 13) >= 20
    print("forms under level 1 + stage %r, coded in %.1f s" % (by_form, TIMES["coding"]))


def test_the_remembered_coder_and_decoder_are_the_rule_functions(coded_population):
    chunks = sw.population()
    picks = [i for i in range(0, len(chunks), 23) if len(chunks[i]) <= 4096]
    assert len(picks) > 40
    for i in picks:
        c, f = chunks[i], coded_population[i]
        assert f[1:] == [sw.zr.coded(c, 1), sw.zr.coded(c, 2), ze.compress_chunk_h(c, 1), ze.compress_chunk_h(c, 2)]
        for held in f:
            assert sw.decoded(held, len(c))[1] == zh.plain_of(held, len(c)) == c
            for level in (1, 2):
                for entropy in (False, True):
                    assert sw.recode_form(held, len(c), level, entropy) == zh.recode_form(held, len(c), level, entropy)
    for name, spec, rule, _ in sw.damaged():
        assert sw.recode_form(spec["stream"], spec["length"], 2, True) == zh.recode_form(spec["stream"], spec["length"], 2, True), name


def test_the_damaged_entries_pass_the_structural_check_and_break_the_stated_rules():
    import makisu_amd as M
    dmg = sw.damaged()
    stated = {name: rule for name, _, _, rule in ze.malformed_table()}
    assert {d[2] for d in dmg} == set(range(1, 12)) and len({d[3] for d in dmg}) == len(dmg)
    for name, spec, rule, _ in dmg:
        assert rule == stated.get(name, rule), name
        entries, blob = zc.build_zpack([zc._entry(zc.GOOD_STREAM, 34, zc.GOOD_PLAIN), dict(spec)])
        assert M.zpack_check(blob, entries) == 1 and ze.first_refused(entries, blob) == (1, rule), name


# ---- the walks on the model ---------------------------------------------------------------------------------------------------------------
_CHECKED = set()


def _decodes_and_hashes(store, alg, damaged_keys):
    """every held good form decodes (zentropy_cases.expand_chunk itself, once per form) to bytes that hash to its digest"""
    for k, (length, span, stored, _) in store.held.items():
        if (k, span) in _CHECKED:
            continue
        _CHECKED.add((k, span))
        if k in damaged_keys:
            assert store.rule(k)
            continue
        plain = ze.expand_chunk(span[:stored], length)
        assert len(plain) == length and pc.HASHES[alg](plain).digest() == k and not any(span[stored:])


def _host_check(store, alg, damaged_keys):
    """the cut of everything passes mi_zpack_check; one that holds damaged entries is refused at the entry the model names: the
    first that does not decode, else (the cut's pads are zero) the first that does not hash"""
    import makisu_amd as M
    every = sorted(store.held)
    entries, blob = store.cut(sw._as_array(every))
    undecodable = [i for i, k in enumerate(every) if sw.decoded(store.held[k][1][:store.held[k][2]], store.held[k][0])[0]]
    unhashed = [i for i, k in enumerate(every) if k in damaged_keys]
    want = undecodable[0] if undecodable else unhashed[0] if unhashed else None
    assert M.zpack_check(blob, entries, alg) == want


def _run(kind, alg, seed):
    """-> (records, per-step facts): the walk generated and executed on a fresh model, checked after every step"""
    t = time.perf_counter()
    recs = sw.walk(kind, seed)
    ctx = sw.Ctx(kind, alg)
    damaged_keys = {d[3] for d in ctx.dmg}
    facts = []
    for step, rec in enumerate(recs):
        out = sw.apply(ctx, rec)
        for store in ctx.stores:
            u = store.usage()
            assert u["resident_bytes"] < 16 << 20
            _decodes_and_hashes(store, alg, damaged_keys)
            _host_check(store, alg, damaged_keys)
        facts.append({"rec": rec, "fails": out["fails"], "usage": [s.usage() for s in ctx.stores],
                      "gen": [max(s.gen.values(), default=0) for s in ctx.stores], "n_events": [len(s.events) for s in ctx.stores],
                      "rules": {ctx.stores[0].rule(k) for k in ctx.stores[0].held if k in damaged_keys}})
    TIMES.setdefault("walks", []).append(time.perf_counter() - t)
    return recs, facts, ctx


_RUNS = {}


def _ran(kind, alg, seed):
    if (kind, alg, seed) not in _RUNS:
        _RUNS[(kind, alg, seed)] = _run(kind, alg, seed)
    return _RUNS[(kind, alg, seed)]


@pytest.mark.parametrize("kind,alg,seed", sw.WALKS)
def test_the_model_executes_the_walk_and_the_host_accepts_every_state(kind, alg, seed):
    recs, facts, ctx = _ran(kind, alg, seed)
    assert len(recs) == sw.STEPS and recs[:7] == sw.walk(kind, seed, 7)              # a prefix replays
    failing = [f["rec"]["op"] for f in facts if f["fails"]]
    assert bool(failing) == (kind == "damaged")              # (WHICH ops fail over the kind's seeds: the coverage conditions below)


def _outlived(facts, op):
    """the most prunes and recodes that ran (on the same set) while one kept-open cut or batch of it was open -> (prunes, recodes)"""
    best = (0, 0)
    for i, f in enumerate(facts):
        r = f["rec"]
        if r["op"] == op and r.get("open") and not f["fails"]:
            later = [g["rec"] for g in facts[i + 1:] if g["rec"].get("set", 0) == r.get("set", 0) and not g["fails"]]
            got = (sum(1 for x in later if x["op"] == "prune"), sum(1 for x in later if x["op"] == "recode"))
            best = max(best, got, key=lambda v: (min(v[0], 2), min(v[1], 1)))
    return best


def coverage(kind, alg, seed):
    """-> the names of the coverage conditions this walk meets"""
    recs, facts, ctx = _ran(kind, alg, seed)
    met = set()
    events = [e for s in ctx.stores for e in s.events]
    for s in range(len(ctx.stores)):
        slots = [f["usage"][s]["table_slots"] for f in facts]
        moves = [b - a for a, b in zip(slots, slots[1:]) if a != b]
        if len(set(slots)) >= 3 and max(slots) >= 4096 and any(m > 0 for m in moves) and any(m < 0 for m in moves):
            met.add("table")
        if max(f["usage"][s]["n_blobs"] for f in facts) >= 8:
            met.add("8 blobs")
        if max(f["gen"][s] for f in facts) >= 2:
            met.add("third generation")
    for s in ctx.stores:
        recodes = [e for e in s.events if e["op"] == "recode"]
        for e in s.events:
            if e["op"] == "prune" and e["compacted"] and {2, 3} <= e["forms_before"] and {2, 3} <= e["forms_moved"]:
                met.add("prune moves form H")
            if e["op"] == "recode" and e["entropy"] and e["n_blobs"] >= 4 and e["untouched"] >= 1 and e["n_recoded"] >= 20:
                met.add("stage recode of 4 blobs")
            if e["op"] == "recode" and not e["entropy"] and e["forms_before"] & {2, 3}:
                met.add("plain recode over form H")
        for i, a in enumerate(recodes):                                               # (later on the same set, not necessarily next)
            for b in recodes[i + 1:]:
                if (a["level"], a["entropy"], b["level"], b["entropy"]) == (1, True, 2, False):
                    met.add("level 2 after level 1 + stage")
                if (a["level"], a["entropy"], b["level"], b["entropy"]) == (2, False, 1, True):
                    met.add("level 1 + stage after level 2")
        if any(e["op"] == "prune" and e["compacted"] and e["damaged_moved"] for e in s.events) and \
                any(e["op"] == "recode" and e["damaged_moved"] for e in s.events):
            met.add("damaged moved both ways")
    if sum(e["first_form_won"] for e in events if e["op"] == "add") >= 30:
        met.add("first form wins 30")
    codings = [r["items"][0][1] if r["op"] == "add_blob" else r["level"] + 2 * r["entropy"]
               for r, f in zip(recs, facts) if r["op"] in ("add_blob", "add_engine_zpack") and not f["fails"] and (r["op"] != "add_blob" or r["items"])]
    if all(codings.count(c) >= 2 for c in range(5)):
        met.add("five codings twice")
    if all(_outlived(facts, op)[0] >= 2 and _outlived(facts, op)[1] >= 1 for op in ("cut", "restore")):
        met.add("open cut and batch outlive")
    met |= {"refused: " + f["rec"]["op"] for f in facts if f["fails"]}
    if set().union(*[f["rules"] for f in facts]) >= {d[2] for d in ctx.dmg}:
        met.add("every rule held")
    return met


CONDITIONS = ["table", "8 blobs", "third generation", "prune moves form H", "stage recode of 4 blobs", "plain recode over form H",
              "level 2 after level 1 + stage", "level 1 + stage after level 2", "first form wins 30", "five codings twice",
              "open cut and batch outlive"]


@pytest.mark.parametrize("kind", sw.KINDS)
def test_the_walks_of_a_kind_reach_every_state_they_exist_for(kind):
    met = {}
    for k, alg, seed in sw.WALKS:
        if k == kind:
            met[(alg, seed)] = coverage(k, alg, seed)
            print(kind, alg, seed, sorted(met[(alg, seed)]))
    want = CONDITIONS + (["every rule held", "damaged moved both ways", "refused: add_blob", "refused: recode", "refused: restore", "refused: cut"]
                         if kind == "damaged" else [])
    missing = [c for c in want if not any(c in m for m in met.values())]
    assert not missing, missing


# ---- the comparison's teeth -------------------------------------------------------------------------------------------------------------
class ZeroedPads(sw.WalkStore):
    """a compaction that zeroes pads"""

    def prune(self, digests, keep=True, permille=0):
        blobs = set(self.blobs)
        info = sw.WalkStore.prune(self, digests, keep, permille)
        for k, v in self.held.items():
            if v[3] not in blobs:
                self.held[k] = (v[0], v[1][:v[2]] + bytes(len(v[1]) - v[2]), v[2], v[3])
        return info


class ForgetsABlob(sw.WalkStore):
    """a recode with the stage that forgets a blob that had no replaced entry"""
    forgotten = ()

    def recode(self, level, verify=False, scratch_bytes=0, entropy=False):
        blobs = set(self.blobs)
        info = sw.WalkStore.recode(self, level, verify, scratch_bytes, entropy)
        left = [b for b in self.blobs if b in blobs]
        if entropy and info["n_recoded"] and left:
            self.forgotten = tuple(self.forgotten) + (left[0],)
        return info

    def usage(self):
        u = sw.WalkStore.usage(self)
        gone = [b for b in self.forgotten if b in self.blobs]
        return dict(u, n_blobs=u["n_blobs"] - len(gone), resident_bytes=u["resident_bytes"] - sum(pr.alloc(self.blobs[b]) for b in gone))


class LastFormWins(sw.WalkStore):
    """an add whose forms replace the held ones: the set points at the new blob's span, the accounting follows"""

    def add(self, zentries, zblob):
        nb = self.next_blob
        sw.WalkStore.add(self, zentries, zblob)
        if self.next_blob > nb:
            for en in zentries:
                at, stored = int(en["offset"]), int(en["stored"])
                self.held[bytes(en["digest"])] = (int(en["length"]), bytes(zblob[at:at + zc.round16(stored)]), stored, nb)


class StaleCapacity(sw.WalkStore):
    """the table after a prune sized by the count before it"""

    def prune(self, digests, keep=True, permille=0):
        before = len(self.held)
        info = sw.WalkStore.prune(self, digests, keep, permille)
        if info["n_dropped"]:
            self.slots = 1024
            while self.slots < 2 * before:
                self.slots *= 2
            self.table_bytes = pr.alloc(self.slots * 8) + pr.alloc(self.slots * 48)
        return info


def first_difference(kind, seed, mutant):
    """the first step at which the GPU module's comparison (store_walk_cases.diff_counters over the op's counters, diff_states over
    the whole state), fed the unmutated model as what was got, reports a difference from the mutant -> (step, the names)"""
    recs = sw.walk(kind, seed)
    good, bad = sw.Ctx(kind), sw.Ctx(kind, store=mutant)
    for step, rec in enumerate(recs):
        got, want = sw.apply(good, rec), sw.apply(bad, rec)
        diff = sw.diff_counters(got["info"], want["info"]) if got.get("info") and want.get("info") else []
        for a, b in zip(good.stores, bad.stores):
            diff += sw.diff_states(sw.state_of_model(a), sw.state_of_model(b))
        if diff:
            return step, diff
    return None


@pytest.mark.parametrize("mutant,kind,names", [(ZeroedPads, "damaged", {"n_undecodable"}), (ForgetsABlob, "clean", {"usage.n_blobs"}),
                                               (LastFormWins, "clean", {"entries", "cut_blob"}), (StaleCapacity, "clean", {"usage.table_slots"})])
def test_the_per_step_comparison_sees_a_planted_model_bug(mutant, kind, names):
    """the names are diff_states' and diff_counters' own, and among them is the field the planted bug is about"""
    seed = [s for k, _, s in sw.WALKS if k == kind][0]
    found = first_difference(kind, seed, mutant)
    assert found is not None, mutant.__name__
    assert names & set(found[1]), (mutant.__name__, found)
    print(mutant.__name__, "seen at step %d in %r" % found)


def test_the_measured_times():
    """printed, not asserted: what this module's docstring states"""
    for kind, alg, seed in sw.WALKS:
        _ran(kind, alg, seed)
    print("coding %.1f s; walks %s" % (TIMES.get("coding", 0), ", ".join("%.1f" % t for t in TIMES["walks"])))
    assert np.isfinite(sum(TIMES["walks"]))
