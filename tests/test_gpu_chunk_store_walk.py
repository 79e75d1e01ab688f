"""GPU tests of the compressed chunk store as a whole: long deterministic walks over every call (adds of model-coded and
engine-coded zpacks, cuts, want lists, prunes, recodes with and without the entropy stage, restores, an index that follows the
set, two sets that feed each other), drawn by store_walk_cases.py from ONE model of the store.  After EVERY step the set is held
against that model through public calls only -- mi_zset_get_info, mi_zset_get_usage, mi_zset_entries, mi_zset_count_forms and the
cut of ALL held digests in sorted order, entries and blob -- and every counter the model predicts of mi_prune_info and
mi_recode_info is compared; an op that must fail is held to its code and words and must leave all of that as it was; every cut
and batch kept open is read again after every prune and recode.  Bit for bit: there are no tolerances.

A failure names the kind, the seed, the step and the op: store_walk_cases.walk(kind, seed, step + 1) replays it on the model."""
import contextlib
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
import store_walk_cases as sw  # noqa: E402
import zpack_cases as zc  # noqa: E402
import zprune_cases as pr  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ("digest", "offset", "chunk_index", "length", "stored")


@pytest.fixture(scope="module", autouse=True)
def coded_population():
    """the population's forms, coded once by the models for every walk of the module"""
    for c in sw.population():
        for coding in range(5):
            sw.form_of_chunk(c, coding)


def _counts(info):
    return {k: v for k, v in info.as_dict().items() if not k.startswith("ms_")}


def _entries_bytes(e):
    out = np.zeros(len(e), dtype=zc.ZENTRY_DTYPE)
    for f in FIELDS:
        out[f] = e[f]
    return out.tobytes()


def _read(z):
    return (_entries_bytes(z.entries()), z.read()) if len(z) else (b"", b"")


def _state(zs):
    """everything the public calls say about a set, in store_walk_cases.state_of_model's shape"""
    d, ln, st = zs.entries()
    held = {bytes(d[i]): (int(ln[i]), int(st[i])) for i in range(len(d))}
    with zs.zpack(sw._as_array(sorted(held))) as z:
        e, b = _read(z)
    f = zs.count_forms()
    return {"info": _counts(zs.info), "usage": zs.usage().as_dict(), "entries": held,
            "census": [[int(f.n[i]), int(f.stored[i])] for i in range(4)], "cut_entries": e, "cut_blob": b}


def _raises(fails, call):
    code, needles, first_bad = fails
    with pytest.raises(M.MiError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for needle in needles:
        assert needle in str(ei.value), (needle, str(ei.value))
    if first_bad is not None:
        assert ei.value.first_bad == first_bad, (ei.value.first_bad, first_bad, str(ei.value))
    return str(ei.value)


def _brief(rec):
    return {k: (v if not isinstance(v, list) or len(v) <= 8 else "%d items, first %r" % (len(v), v[:4])) for k, v in rec.items()}


class Driver:
    """the engine's side of a walk"""

    def __init__(self, stack, kind, alg):
        self.ctx = sw.Ctx(kind, alg)
        self.e = stack.enter_context(M.Engine(max_size=262144, flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0))
        self.stack = stack
        self.sets = [stack.enter_context(self.e.zset()) for _ in self.ctx.stores]
        self.index = stack.enter_context(self.e.index())
        self.every = sorted(self.ctx.ref)
        self.index.load(b"".join(self.every))
        self.cuts, self.batches = {}, {}

    def compare(self):
        for zs, store in zip(self.sets, self.ctx.stores):
            diff = sw.diff_states(_state(zs), sw.state_of_model(store))
            assert not diff, "the set differs from the model in %r" % (diff,)

    def still_open(self):
        """every cut and batch kept open reads as it did when it was made"""
        for cid, (z, want) in self.cuts.items():
            assert _read(z) == want, "the open cut of step %d changed" % cid
        for bid, (b, files) in self.batches.items():
            for i, want in enumerate(files):
                assert b.read_file(i, 0, len(want)) == want, "file %d of the open batch of step %d changed" % (i, bid)

    def follow(self):
        """the index that follows set 0 answers for every digest of the population as the model does"""
        got = self.index.query(sw._as_array(self.every))
        assert [int(x) for x in got] == [1 if k in self.ctx.index else 0 for k in self.every], "the index differs from the model"

    def step(self, rec):
        ctx, e = self.ctx, self.e
        op, s = rec["op"], rec.get("set", 0)
        zs = self.sets[s]
        if op == "prune" and rec.get("other"):                                        # keep = the other set's entries(), as it gives them
            theirs = self.sets[1 - s].entries()[0]
        before = zs.usage()
        out = sw.apply(ctx, rec)
        fails = out["fails"]
        if op == "add_blob":
            entries, blob = out["zpack"]
            call = lambda: zs.add_zblob(blob, entries, verify=rec["verify"])            # noqa: E731
            _raises(fails, call) if fails else call()
        elif op == "add_engine_zpack":
            pe, pb, (want_e, want_b) = out["plain"]
            if rec["route"] == "batch":                                               # the arena's coder: one file, one chunk, one entry
                chunks = [ctx.chunks[i] for i in rec["chunks"]]
                with e.batch() as b:
                    for k, c in enumerate(chunks):
                        b.add_bytes(c, k)
                    b.run()
                    assert [int(n) for n in b.chunks()["length"]] == [len(c) for c in chunks], "a file of the batch is not one chunk"
                    with b.zpack_at(rec["level"], verify=rec["verify"]) as z:
                        assert _read(z) == (want_e.tobytes(), want_b), "the arena's coder and the model's differ"
                        zs.add_zpack(z, verify=rec["verify"])
            else:
                with e.packset() as ps:
                    ps.add_blob(pb, pe, verify=True)
                    with ps.pack(np.ascontiguousarray(pe["digest"])) as p, \
                            p.compress(verify=rec["verify"], level=rec["level"], entropy=rec["entropy"]) as z:
                        assert _read(z) == (want_e.tobytes(), want_b), "the engine's coder and the model's differ"
                        zs.add_zpack(z, verify=rec["verify"])
        elif op == "add_cut_of_other":
            want_e, want_b = out["zpack"]
            with self.sets[1 - s].zpack(out["request"]) as z:
                assert _read(z) == (want_e.tobytes(), want_b), "the cut differs from the model's"
                zs.add_zpack(z, verify=rec["verify"])
        elif op == "add_open_cut":
            zs.add_zpack(self.cuts[rec["cut"]][0], verify=rec["verify"])
        elif op == "cut":
            call = lambda: zs.zpack(out["request"], out["lengths"], verify=rec["verify"])   # noqa: E731
            if fails:
                _raises(fails, call)
            else:
                z = call()
                want = (out["zpack"][0].tobytes(), out["zpack"][1])
                try:
                    assert _read(z) == want, "the cut differs from the model's"
                finally:
                    if rec["open"]:
                        self.cuts[rec["id"]] = (self.stack.enter_context(z), want)
                    else:
                        z.close()
        elif op == "missing":
            held, want_rows, info = zs.missing(out["request"], out["lengths"])
            m_held, m_want, m_info = out["answer"]
            assert [int(x) for x in held] == m_held and [int(x) for x in want_rows] == m_want
            assert not sw.diff_counters(info.as_dict(), m_info), (info.as_dict(), m_info)
        elif op == "prune":
            request = np.ascontiguousarray(theirs) if rec.get("other") else out["request"]
            info = zs.prune(request, keep=rec["keep"], min_live_permille=rec["permille"])
            diff = sw.diff_counters(_counts(info), out["info"])
            assert not diff, "mi_prune_info differs in %r: %r, the model %r" % (diff, _counts(info), out["info"])
            if s == 0:
                self.index.retain(zs)
        elif op == "recode":
            call = lambda: zs.recode(level=rec["level"], verify=rec["verify"], scratch_bytes=rec["scratch"], entropy=rec["entropy"])  # noqa: E731
            if fails:
                said = _raises(fails, call)
                assert any(k.hex() in said for k in out["bad"]), said
            else:
                info = call()
                diff = sw.diff_counters(_counts(info), out["info"])
                assert not diff, "mi_recode_info differs in %r: %r, the model %r" % (diff, _counts(info), out["info"])
                assert info.n_rounds >= out["min_rounds"]
                after = zs.usage()
                assert after.live_bytes == info.live_after
                assert after.resident_bytes == before.resident_bytes - info.freed_bytes + (pr.alloc(info.new_blob_bytes) if info.n_recoded else 0)
        elif op == "restore":
            b = e.batch()
            try:
                call = lambda: b.add_zrecipes(zs, out["recipes"], verify=rec["verify"])   # noqa: E731
                if fails:
                    counts = b.counts()
                    _raises(fails, call)
                    assert b.counts() == counts, "a refused restore changed the batch"
                else:
                    call()
                    b.run()
                    for i, want in enumerate(out["files"]):
                        assert b.read_file(i, 0, len(want)) == want, "file %d differs from the model's bytes" % i
            finally:
                if rec["open"] and not fails and rec["id"] in ctx.open_batches:
                    self.batches[rec["id"]] = (self.stack.enter_context(b), out["files"])
                else:
                    b.free()
        else:
            raise ValueError(op)
        if op.startswith("add") and not fails and s == 0 and len(out["zpack"][0]):       # the index takes what the set took
            self.index.load(out["zpack"][0]["digest"].tobytes())
        self.compare()                                                                # (an op that failed: the model did not move)
        if op in ("prune", "recode"):
            self.still_open()
        if op == "prune" or op.startswith("add"):
            self.follow()


@pytest.mark.parametrize("kind,alg,seed", sw.WALKS)
def test_the_store_holds_the_model_after_every_step_of_a_walk(kind, alg, seed):
    t = time.perf_counter()
    recs = sw.walk(kind, seed)
    t_model = time.perf_counter() - t
    with contextlib.ExitStack() as stack:
        driver = Driver(stack, kind, alg)
        for step, rec in enumerate(recs):
            try:
                driver.step(rec)
            except (Exception, pytest.fail.Exception) as err:
                raise AssertionError("walk(%r, seed %d), alg %d, step %d, %r: %s: %s"
                                     % (kind, seed, alg, step, _brief(rec), type(err).__name__, err)) from err
    print("walk %s/%d/%d: %d steps, drawn in %.1f s, run in %.1f s" % (kind, alg, seed, len(recs), t_model, time.perf_counter() - t - t_model))
