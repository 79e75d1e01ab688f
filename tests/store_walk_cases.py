"""One model of the compressed chunk store and one generator of long walks over every call of it (mi_zset_*, the cuts, the
restores, the index that follows a set), in pure Python over zprune_cases.py, zrecode_cases.py, zrecode_h_cases.py and
zentropy_cases.py -- which stay as they are.  No engine code is involved.

WalkStore is zrecode_cases.Store with the entropy stage's recode (THE RULE: zrecode_h_cases.recode_form), the census, the want
list, the restore and a cut that takes repeats.  population() is the fixed set U of chunks the walks draw from, damaged() the
rule-breaking entries only an unverified add brings in.  walk(kind, seed, n_steps) draws plain op records -- after four adds that
build the set, WHICH op comes next is drawn from the seed by weights, among the ops that mean something in the model's state;
apply(ctx, rec) executes one on the model and says what the engine must answer; state_of_model / diff_states are the per-step
comparison tests/test_gpu_chunk_store_walk.py holds the engine against.

NOT DRAWN: one digest twice in ONE add under two different forms while the set does not hold it yet.  Which of the two rows
claims the slot is decided by a compare-and-swap between lanes of one launch (tests/test_gpu_chunk_zset.py says so for two
lengths); the header states "the first form wins" for a digest the set holds ALREADY.  The walks repeat a digest inside one add
with two forms only where the set holds it (both lose), and with one form where it does not (either copy is the same bytes)."""
import hashlib

import numpy as np

import pack_cases as pc
import zentropy_cases as ze
import zpack_cases as zc
import zprune_cases as pr
import zrecode_cases as zr

TILE = pr.TILE
alloc = pr.alloc
CODINGS = ("raw", "level 1", "level 2", "level 1 + stage", "level 2 + stage")
KINDS = ("clean", "damaged", "two_sets")
STEPS = 40
# (kind, digest algorithm, seed): the walks both test modules run.  The seeds were picked by running walks on the model until
# every coverage condition of tests/test_host_chunk_store_walk.py is met by some walk of each kind (clean 3 and 19 meet all alone)
WALKS = [("clean", pc.SHA256, 3), ("clean", pc.SHA256, 19), ("clean", pc.SHA256, 2), ("clean", pc.BLAKE2S, 4), ("clean", pc.BLAKE2S, 14),
         ("damaged", pc.SHA256, 10), ("damaged", pc.SHA256, 20), ("two_sets", pc.SHA256, 12), ("two_sets", pc.SHA256, 18)]
N_GENERATED = 1400
POP_SEED = 20261
NEVER = 1 << 20                                        # refs from here on: digests no add ever brings
RULE_WORDS = {1: "a match offset of 0", 2: "a match offset beyond", 3: "a literal run that leaves", 4: "a length extension or an offset cut off",
              5: "output that passes", 6: "short of the chunk's length", 7: "a pad byte behind the stored span",
              8: "an entropy form with a bad header", 9: "an entropy form whose code lengths", 10: "an entropy form whose stream sizes",
              11: "an entropy form with a stream that ends early"}
STRUCTURAL = ("stored > length", "stored == 0", "overlap", "off-grid offset")


# ---- the coder and the decoder, remembered ----------------------------------------------------------------------------------------------
_CODED = {}
_DECODED = {}


def coded_form(plain, level, entropy):
    """zrecode_h_cases.candidate, remembered; level 0: the bytes as they are.  What the model's coder made decodes to what it was
    made from: that is remembered too (tests/test_host_chunk_store_walk.py decodes every held form for itself)"""
    if level == 0:
        return plain
    key = (plain, level, entropy)
    form = _CODED.get(key)
    if form is None:
        form = zr.coded(plain, level)
        if entropy and len(plain) <= ze.MAX_CHUNK and ze.huff_size(form) < len(form) - (len(form) >> 4):
            form = ze.huff_form(form, 1 if len(form) < len(plain) else 2)   # zentropy_cases.compress_chunk_h, the parse taken once
        _CODED[key] = form
        _DECODED.setdefault((form, len(plain)), (0, plain))
    return form


def decoded(form, length):
    """zentropy_cases.chunk_rule, remembered -> (rule, plain or None)"""
    key = (form, length)
    got = _DECODED.get(key)
    if got is None:
        got = _DECODED[key] = ze.chunk_rule(form, length)
    return got


def recode_form(form, length, level, entropy):
    """zrecode_h_cases.recode_form over the remembered coder and decoder (held equal to it in the host tests)"""
    rule, plain = decoded(form, length)
    if rule:
        return form
    cand = coded_form(plain, level, entropy)
    return cand if len(cand) < len(form) else form


# ---- the population -------------------------------------------------------------------------------------------------------------------
_WORDS = [w.encode() for w in ("layer chunk digest store blob table slot prune recode stream offset match literal token block level "
                               "stage entropy huffman code length symbol span pad unit live dead move copy cut keep drop want held "
                               "index batch file recipe arena wave lane scan plan sum carry round scratch verify").split()]


def _word_text(rng, n):
    out = bytearray()
    while len(out) < n:
        out += _WORDS[int(rng.integers(0, len(_WORDS)))] + (b" " if rng.integers(0, 9) else b".\n")
    return bytes(out[:n])


def _generated(rng, n_generated):
    out = []
    share = lambda permille: n_generated * permille // 1000                              # noqa: E731
    sizes = lambda n, lo, hi: (np.exp(rng.uniform(np.log(lo), np.log(hi), n))).astype(int)  # noqa: E731
    for k, n in enumerate(sizes(share(170), 13, 3000)):                                  # random bytes: stay raw; three of them 16 384 long
        out.append(rng.integers(0, 256, 16384 if k < 3 else int(n), dtype=np.uint8).tobytes())
    for k, n in enumerate(sizes(share(200), 30, 1500)):                                  # a phrase with a counter: one LZ4 block
        out.append(zc.text_like(int(n), 1000 + k))
    for k, n in enumerate(sizes(share(200), 500, 3000)):                                # 4 and 16 symbols
        base = (4, 0x41) if k % 5 == 0 else (16, 0x30 + k % 64)
        out.append((rng.integers(0, base[0], int(n), dtype=np.uint8) + base[1]).astype(np.uint8).tobytes())
    for n in sizes(share(110), 1200, 6000):                                             # long text: words, so literals stay
        out.append(_word_text(rng, int(n)))
    for n in sizes(share(170), 13, 2000):                                                # short periods
        unit = rng.integers(0, 256, int(rng.integers(1, 8)), dtype=np.uint8).tobytes()
        out.append((unit * (int(n) // len(unit) + 1))[:int(n)])
    for k in range(share(60)):                                                           # 1 to 12 bytes
        out.append(rng.integers(0, 256, 1 + k % 12, dtype=np.uint8).tobytes() if k >= 24 else bytes([k + 1]) * (1 + k % 12))
    while len(out) < n_generated:                                                        # text with a far copy: work for level 2
        n = int(rng.integers(200, 2000))
        buf = bytearray(_word_text(rng, n))
        a, b = sorted(int(x) for x in rng.integers(0, n - 40, 2))
        buf[b:b + 40] = buf[a:a + 40]
        out.append(bytes(buf))
    return out


_POPULATION = {}


def population(n_generated=N_GENERATED, seed=POP_SEED):
    """U -> a tuple of distinct chunks: the planted ones of zrecode_cases and zentropy_cases, then the generated ones"""
    key = (n_generated, seed)
    if key not in _POPULATION:
        chunks, seen = [], set()
        for c in list(zr.planted()[1]) + [c for _, c in ze.planted_chunks_h()] + _generated(np.random.default_rng(seed), n_generated):
            if c and c not in seen:
                seen.add(c)
                chunks.append(bytes(c))
        _POPULATION[key] = tuple(chunks)
    return _POPULATION[key]


def form_of_chunk(chunk, coding):
    """the stored form of a chunk under one of CODINGS"""
    return coded_form(chunk, (0, 1, 2, 1, 2)[coding], coding >= 3)


_DIGESTS = {}


def digests(alg=pc.SHA256, n_generated=N_GENERATED):
    key = (alg, n_generated)
    if key not in _DIGESTS:
        _DIGESTS[key] = [pc.HASHES[alg](c).digest() for c in population(n_generated)]
    return _DIGESTS[key]


_DAMAGED = []


def damaged():
    """-> [(name, entry spec, rule, digest)]: the entries of both malformed tables that pass the structural host check, each under
    a digest of its own (nothing hashes to it)"""
    if not _DAMAGED:
        rows = [(name, specs[bad]) for name, specs, bad in zc.malformed_table() if name not in STRUCTURAL]
        rows += [(name, specs[bad]) for name, specs, bad, _ in ze.malformed_table()]
        for k, (name, spec) in enumerate(rows):
            form, length = spec["stream"], spec["length"]
            assert spec["stored"] == len(form) and 0 < len(form) <= length and spec["offset"] is None, name
            rule = decoded(form, length)[0] or (ze.RULE_PAD if spec["pad"] and len(form) % 16 else 0)
            assert rule, name
            _DAMAGED.append((name, dict(spec), rule, hashlib.sha256(b"damaged entry %d" % k).digest()))
    return _DAMAGED


def never_digest(n):
    return hashlib.sha256(b"a digest no add ever brings %d" % n).digest()


# ---- the model --------------------------------------------------------------------------------------------------------------------------
class WalkStore(zr.Store):
    """zrecode_cases.Store with the entropy stage's recode, the census, the want list, the restore and a cut with repeats; it
    remembers every blob's generation (0: added, else one more than the oldest blob it was made of) and what each call did"""

    def __init__(self, hint=0):
        zr.Store.__init__(self, hint)
        self.gen = {}
        self.events = []

    def rule(self, k):
        """the rule a reader refuses the held entry with, 0 for none"""
        length, span, stored, _ = self.held[k]
        return decoded(span[:stored], length)[0] or (ze.RULE_PAD if any(span[stored:]) else 0)

    def forms_held(self):
        return {ze.form_of(v[1][:v[2]], v[0]) for v in self.held.values()}

    def add(self, zentries, zblob):
        nb, decided = self.next_blob, set()
        for en in zentries:
            k, at, stored = bytes(en["digest"]), int(en["offset"]), int(en["stored"])
            if k in self.held and self.held[k][1][:self.held[k][2]] != bytes(zblob[at:at + stored]):
                decided.add(k)
        zr.Store.add(self, zentries, zblob)
        if self.next_blob > nb:
            self.gen[nb] = 0
        self.events.append({"op": "add", "first_form_won": len(decided)})

    def prune(self, digests, keep=True, permille=0):
        blobs, where = set(self.blobs), {k: v[3] for k, v in self.held.items()}
        forms_before = self.forms_held()
        info = zr.Store.prune(self, digests, keep, permille)
        new = [b for b in self.blobs if b not in blobs]
        moved = [k for k, v in self.held.items() if v[3] in new]
        if new:
            self.gen[new[0]] = 1 + max(self.gen[where[k]] for k in moved)
        for b in blobs - set(self.blobs):
            del self.gen[b]
        self.events.append({"op": "prune", "compacted": bool(new), "forms_before": forms_before, "n_dropped": info["n_dropped"],
                            "forms_moved": {ze.form_of(self.held[k][1][:self.held[k][2]], self.held[k][0]) for k in moved},
                            "damaged_moved": sum(1 for k in moved if self.rule(k))})
        return info

    def recode(self, level, verify=False, scratch_bytes=0, entropy=False):
        """-> every field of mi_recode_info but the times.  Bookkeeping AND THE SIZES OF peak_extra_bytes: zrecode_cases.Store.recode's,
        line for line (that one asserts a single round and may not be edited) -- the two must change together; the GPU walks fail
        if they drift apart, since both are held against the same engine.  n_rounds and peak_extra_bytes are None unless that model
        covers the call: one round, no stage, no form H held"""
        n, cap, n_blobs = len(self.held), self.slots, len(self.blobs)
        info = dict.fromkeys(["n_digests", "n_recoded", "n_raw_recoded", "n_undecodable", "stored_before", "stored_after", "live_before",
                              "live_after", "n_blobs_rewritten", "n_blobs_freed", "freed_bytes", "new_blob_bytes", "n_rounds",
                              "peak_extra_bytes"], 0)
        info["n_digests"] = n
        info["stored_before"] = info["stored_after"] = sum(v[2] for v in self.held.values())
        event = {"op": "recode", "level": level, "entropy": entropy, "n_blobs": n_blobs, "untouched": n_blobs, "n_recoded": 0,
                 "forms_before": self.forms_held(), "damaged_moved": 0}
        self.events.append(event)
        if n == 0:
            return info
        info["live_before"] = info["live_after"] = sum(len(v[1]) for v in self.held.values())
        covered = self.total_need() <= (scratch_bytes or zr.DEFAULT_SCRATCH) and not entropy and not event["forms_before"] & {2, 3}
        info["n_rounds"] = 1 if covered else None
        new = {}
        for k, (length, span, stored, bid) in self.held.items():
            if self.rule(k):
                info["n_undecodable"] += 1
                continue
            now = recode_form(span[:stored], length, level, entropy)
            if len(now) < stored:
                new[k] = now
        nb = (cap + TILE - 1) // TILE
        extra = alloc(n_blobs * 8) + alloc(n_blobs) + alloc(128) + alloc(2 * nb * 8) + alloc(5 * n * 8) + 4 * alloc(n * 4) + alloc(n * 8)
        if verify:
            extra += alloc(2 * n * 8) + alloc(n * 32)
        extra += alloc(self.total_need())
        info["peak_extra_bytes"] = extra if covered else None
        if not new:
            return info
        staged = sum(zc.round16(len(f)) for f in new.values())
        rewritten = sorted({self.held[k][3] for k in new})
        moved = [k for k, v in self.held.items() if v[3] in rewritten]
        event["damaged_moved"] = sum(1 for k in moved if self.rule(k))
        for k, f in new.items():
            length, _, stored, bid = self.held[k]
            info["n_raw_recoded"] += 1 if stored == length else 0
            self.held[k] = (length, f + bytes(zc.round16(len(f)) - len(f)), len(f), bid)
        blob_bytes = sum(len(self.held[k][1]) for k in moved)
        new_cap = 1024
        while new_cap < 2 * n:
            new_cap *= 2
        table = alloc(new_cap * 8) + alloc(new_cap * 48)
        nb2 = (n + TILE - 1) // TILE
        extra += alloc(staged) + alloc(2 * nb2 * 8) + alloc(blob_bytes) + alloc(4 * len(moved) * 8) + alloc(n * 8)
        extra += table + alloc(n * 48) + alloc(n + 16) + alloc(n * 8 + 16) + alloc(64)
        if verify:
            extra += alloc(2 * len(new) * 8) + alloc(len(new) * 32)
        info["peak_extra_bytes"] = extra if covered else None
        info["n_recoded"] = len(new)
        info["stored_after"] = sum(v[2] for v in self.held.values())
        info["live_after"] = sum(len(v[1]) for v in self.held.values())
        info["n_blobs_rewritten"] = info["n_blobs_freed"] = len(rewritten)
        info["freed_bytes"] = sum(alloc(self.blobs[b]) for b in rewritten)
        info["new_blob_bytes"] = blob_bytes
        self._rewritten(rewritten, blob_bytes, moved)
        self.slots, self.table_bytes = new_cap, table
        event.update(untouched=n_blobs - len(rewritten), n_recoded=len(new))
        return info

    def _rewritten(self, rewritten, blob_bytes, moved):
        gen = 1 + max(self.gen[b] for b in rewritten)
        for b in rewritten:
            del self.blobs[b]
            del self.gen[b]
        bid = self.next_blob
        self.next_blob += 1
        self.blobs[bid], self.gen[bid] = blob_bytes, gen
        for k in moved:
            v = self.held[k]
            self.held[k] = (v[0], v[1], v[2], bid)

    def census(self):
        """-> the four [n, stored] pairs of mi_zset_count_forms"""
        out = [[0, 0] for _ in range(4)]
        for length, span, stored, _ in self.held.values():
            f = ze.form_of(span[:stored], length)
            out[f][0] += 1
            out[f][1] += stored
        return out

    def missing(self, digests, lengths=None):
        """-> (held flags, want rows, every field of mi_want_info but the time)"""
        keys = pr._keys(digests)
        held = [1 if k in self.held else 0 for k in keys]
        seen, want = set(), []
        for r, k in enumerate(keys):
            if k not in seen and k not in self.held:
                want.append(r)
            seen.add(k)
        n_held = sum(1 for k in seen if k in self.held)
        return held, want, {"n_rows": len(keys), "n_distinct": len(seen), "n_held": n_held, "n_want": len(want),
                            "held_bytes": sum(self.held[k][0] for k in seen if k in self.held),
                            "want_bytes": 0 if lengths is None else sum(int(lengths[r]) for r in want)}

    def restore(self, order):
        """the bytes of a file made of these digests"""
        out = []
        for k in pr._keys(order):
            length, span, stored, _ = self.held[k]
            rule, plain = decoded(span[:stored], length)
            assert rule == 0
            out.append(plain)
        return b"".join(out)

    def cut(self, digests):
        """zrecode_cases.Store.cut for a request with repeats: every distinct digest once, in order of first occurrence,
        chunk_index = the row of that occurrence"""
        rows, seen = [], set()
        for r, k in enumerate(pr._keys(digests)):
            if k not in seen:
                seen.add(k)
                rows.append((r, k))
        entries = np.zeros(len(rows), dtype=zc.ZENTRY_DTYPE)
        parts, at = [], 0
        for i, (r, k) in enumerate(rows):
            length, span, stored, _ = self.held[k]
            entries["digest"][i] = np.frombuffer(k, dtype=np.uint8)
            entries["offset"][i], entries["chunk_index"][i], entries["length"][i], entries["stored"][i] = at, r, length, stored
            parts.append(span[:stored] + bytes(len(span) - stored))
            at += len(span)
        return entries, b"".join(parts)


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------
def _as_array(keys):
    return np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(-1, 32) if keys else np.zeros((0, 32), dtype=np.uint8)


def state_of_model(store):
    """everything the public calls say about a set, from the model: info without times, usage, the entries, the census and the
    cut of ALL held digests in sorted digest order"""
    every = sorted(store.held)
    e, b = store.cut(_as_array(every))
    return {"info": store.info(), "usage": store.usage(), "entries": {k: (v[0], v[2]) for k, v in store.held.items()},
            "census": store.census(), "cut_entries": e.tobytes(), "cut_blob": b}


def diff_states(got, want):
    """-> the names of what differs (empty: the states are equal)"""
    out = []
    for name in ("info", "usage"):
        out += ["%s.%s" % (name, f) for f in want[name] if got[name].get(f) != want[name][f]]
    out += [name for name in ("entries", "census", "cut_entries", "cut_blob") if got[name] != want[name]]
    return out


def diff_counters(got, want):
    """an op's counters against the model's; a None of the model is not compared"""
    return [f for f, v in want.items() if v is not None and got.get(f) != v]


# ---- the walks ----------------------------------------------------------------------------------------------------------------------------
class Ctx:
    """what a walk runs on: one or two stores, the index that follows store 0, the cuts and batches kept open"""

    def __init__(self, kind, alg=pc.SHA256, n_generated=N_GENERATED, store=WalkStore):
        assert kind in KINDS
        self.kind, self.alg = kind, alg
        self.chunks, self.dig = population(n_generated), digests(alg, n_generated)
        self.dmg = damaged()
        self.stores = [store() for _ in range(2 if kind == "two_sets" else 1)]
        self.ref = {k: i for i, k in enumerate(self.dig)}
        self.ref.update({d[3]: len(self.dig) + j for j, d in enumerate(self.dmg)})
        self.index = set(self.ref)
        self.open_cuts, self.open_batches, self.cut_of = {}, {}, {}
        self.n_adds = 0                                # adds that succeeded
        self.codings = []                              # the coding of every add of them that a coder made (model or engine)

    def key(self, ref):
        if ref >= NEVER:
            return never_digest(ref - NEVER)
        return self.dig[ref] if ref < len(self.dig) else self.dmg[ref - len(self.dig)][3]

    def keys(self, refs):
        return [self.key(r) for r in refs]

    def held_refs(self, s):
        return sorted(self.ref[k] for k in self.stores[s].held)

    def is_damaged(self, ref):
        return len(self.dig) <= ref < NEVER


def build_add(ctx, rec):
    """an add_blob record -> (entries, blob), laid out by zpack_cases.build_zpack"""
    specs, keys = [], []
    for i, coding in rec["items"]:
        specs.append(zc._entry(form_of_chunk(ctx.chunks[i], coding), len(ctx.chunks[i])))
        keys.append(ctx.dig[i])
    for pos, j in rec["dmg"]:
        specs.insert(pos, dict(ctx.dmg[j][1]))
        keys.insert(pos, ctx.dmg[j][3])
    entries, blob = zc.build_zpack(specs, ctx.alg)
    if keys:
        entries["digest"] = _as_array(keys)
    return entries, blob


def build_engine_zpack(ctx, rec):
    """an add_engine_zpack record -> (the plain pack's entries and blob, the zpack the coder must make of it: the population's
    remembered forms, laid out in the pack's order with chunk_index = the pack's)"""
    entries, blob = zc.pack_of([ctx.chunks[i] for i in rec["chunks"]], ctx.alg)
    coding = rec["level"] + 2 * rec["entropy"]
    return entries, blob, build_add(ctx, {"items": [[i, coding] for i in rec["chunks"]], "dmg": []})


def _lengths_for(ctx, store, refs):
    out = []
    for r in refs:
        k = ctx.key(r)
        out.append(store.held[k][0] if k in store.held else len(ctx.chunks[r]) if r < len(ctx.chunks) else 77)
    return np.array(out, dtype=np.uint32)


def apply(ctx, rec):
    """one op on the model -> what the engine must answer: {"fails": None or (code, needles, first_bad or None), ...} with the
    op's inputs as the engine takes them and the model's answers.  An op that must fail changes nothing"""
    op, s = rec["op"], rec.get("set", 0)
    store = ctx.stores[s]
    out = {"fails": None}
    if op in ("add_blob", "add_engine_zpack", "add_cut_of_other", "add_open_cut"):
        if op == "add_blob":
            entries, blob = build_add(ctx, rec)
            bad = ze.first_refused(entries, blob) if rec["verify"] else None
            if bad is not None:
                out["fails"] = (-1, ["entry %d " % bad[0]], bad[0])
        elif op == "add_engine_zpack":
            out["plain"] = build_engine_zpack(ctx, rec)
            entries, blob = out["plain"][2]
        elif op == "add_cut_of_other":
            out["request"] = _as_array(ctx.keys(rec["request"]))
            entries, blob = ctx.stores[1 - s].cut(out["request"])
        else:
            entries, blob = ctx.open_cuts[rec["cut"]]
        out["zpack"] = (entries, blob)
        if out["fails"] is None:
            store.add(entries, blob)
            ctx.n_adds += 1
            if op == "add_blob" and rec["items"]:
                ctx.codings.append(rec["items"][0][1])
            elif op == "add_engine_zpack" and rec["chunks"]:
                ctx.codings.append(rec["level"] + 2 * rec["entropy"])
            if s == 0:
                ctx.index |= set(pr._keys(entries["digest"])) if len(entries) else set()
    elif op == "cut":
        out["request"] = _as_array(ctx.keys(rec["request"]))
        out["lengths"] = _lengths_for(ctx, store, rec["request"]) if rec["lengths"] else None
        entries, blob = store.cut(out["request"])
        out["zpack"] = (entries, blob)
        bad = [i for i, k in enumerate(pr._keys(entries["digest"])) if ctx.is_damaged(ctx.ref[k])] if rec["verify"] else []
        if bad:
            rule = store.rule(bytes(entries["digest"][bad[0]]))
            out["fails"] = (-5, ["row %d (entry %d)" % (int(entries["chunk_index"][bad[0]]), bad[0]),
                                 "does not decode" if rule and rule != ze.RULE_PAD else "do not hash to the requested digest"],
                            int(entries["chunk_index"][bad[0]]))
        elif rec["open"]:
            ctx.open_cuts[rec["id"]] = (entries, blob)
            ctx.cut_of[rec["id"]] = s
    elif op == "missing":
        out["request"] = _as_array(ctx.keys(rec["request"]))
        out["lengths"] = _lengths_for(ctx, store, rec["request"]) if rec["lengths"] else None
        out["answer"] = store.missing(out["request"], out["lengths"])
    elif op == "prune":
        refs = ctx.held_refs(1 - s) if rec.get("other") else rec["request"]
        out["request"] = _as_array(ctx.keys(refs))
        out["info"] = store.prune(out["request"], keep=rec["keep"], permille=rec["permille"])
        if s == 0:
            ctx.index &= set(store.held)
    elif op == "recode":
        bad = [k for k in store.held if ctx.is_damaged(ctx.ref[k])] if rec["verify"] else []
        if bad:
            out["fails"] = (-5, ["%d of %d entries" % (len(bad), len(store.held)), "unchanged"], None)
            out["bad"] = bad
        else:
            out["min_rounds"] = store.min_rounds(rec["scratch"]) if store.held else 0
            out["info"] = store.recode(rec["level"], verify=rec["verify"], scratch_bytes=rec["scratch"], entropy=rec["entropy"])
    elif op == "restore":
        out["recipes"] = [(_as_array(ctx.keys(f)), _lengths_for(ctx, store, f)) for f in rec["files"]]
        for fi, f in enumerate(rec["files"]):
            for row, r in enumerate(f):
                rule = store.rule(ctx.key(r))
                if rule and out["fails"] is None:
                    out["fails"] = (-1, ["file %d, row %d " % (fi, row), ctx.key(r).hex(), "does not decode: " + RULE_WORDS[rule]], None)
        if out["fails"] is None:
            out["files"] = [store.restore(d) for d, _ in out["recipes"]]
            if rec["open"]:
                ctx.open_batches[rec["id"]] = out["files"]
    else:
        raise ValueError(op)
    return out


# ---- drawing a walk ---------------------------------------------------------------------------------------------------------------------
# The first steps of a walk build the set: PREFIX adds of 350 to 500 chunks, so that the table has grown before anything else
# happens.  From then on THE ORDER IS DRAWN: every step's op comes from the walk's generator, by the kind's weights, among the ops
# that mean something in the model's state (nothing is cut from an empty set, no open cut is added where none is open); so do all
# of its parameters.  A set above 8 MB resident draws prunes four times as often
_A, _E = "add_blob", "add_engine_zpack"
PREFIX = 4
WEIGHTS = {"clean": {_A: 34, _E: 8, "cut": 8, "restore": 8, "missing": 4, "prune": 18, "recode": 20},
           "damaged": {_A: 36, _E: 4, "cut": 9, "restore": 9, "missing": 3, "prune": 18, "recode": 21},
           "two_sets": {_A: 30, _E: 6, "add_cut_of_other": 10, "add_open_cut": 6, "cut": 8, "restore": 8, "missing": 3, "prune": 16,
                        "recode": 18}}
MAX_OPEN = 3                                           # cuts, and batches, kept open at a time
BATCH_ROUTE_MAX = 2000                                 # a file of at most this many bytes is one chunk of a batch (the engine's min_size is 2 048)


def _some(rng, pool, n):
    n = min(n, len(pool))
    return [pool[int(i)] for i in rng.choice(len(pool), n, replace=False)] if n else []


def _pick(rng, values):
    return values[int(rng.integers(0, len(values)))]


def _choose(ctx, rng, step):
    """-> (op, set): the prefix's adds, then an op drawn by the kind's weights among those that mean something now"""
    n_sets = len(ctx.stores)
    if step < PREFIX:
        return (_E if step == 2 else _A), step % n_sets
    s = int(rng.integers(0, n_sets))
    good = any(not ctx.is_damaged(ctx.ref[k]) for k in ctx.stores[s].held)
    weights = dict(WEIGHTS[ctx.kind])
    if not good:
        for op in ("cut", "restore", "prune", "recode"):
            weights[op] = 0
    if n_sets == 2 and not ctx.stores[1 - s].held:
        weights["add_cut_of_other"] = 0
    if n_sets == 2 and not any(of == 1 - s for c, of in ctx.cut_of.items() if c in ctx.open_cuts):
        weights["add_open_cut"] = 0
    if ctx.stores[s].usage()["resident_bytes"] > 8 << 20:
        weights["prune"] *= 4
    ops = sorted(op for op, w in weights.items() if w)
    p = np.array([weights[op] for op in ops], dtype=float)
    return ops[int(rng.choice(len(ops), p=p / p.sum()))], s


def _draw(ctx, rng, step, seed):
    op, s = _choose(ctx, rng, step)
    store = ctx.stores[s]
    held = ctx.held_refs(s)
    good = [r for r in held if not ctx.is_damaged(r)]
    bad = [r for r in held if ctx.is_damaged(r)]
    rec = {"op": op, "set": s}
    flip = lambda: bool(rng.integers(0, 2))                                                # noqa: E731
    if op in (_A, _E):
        if step < PREFIX:
            size = int(rng.integers(350, 501))
        else:
            size = _pick(rng, [0, 1]) if op == _A and rng.integers(0, 12) == 0 else int(np.exp(rng.uniform(np.log(2), np.log(500))))
        n_held = int(size * (0.1 if step < PREFIX else _pick(rng, [0.1, 0.25, 0.5, 0.8])))
        used = [ctx.codings.count(c) for c in range(5)]
        coding = used.index(min(used)) if flip() else int(rng.integers(0, 5))              # half of the adds: the coding least added so far
        batch = op == _E and coding in (1, 2) and flip()                                   # the arena's coder: files of one chunk each
        fits = (lambda i: len(ctx.chunks[i]) <= BATCH_ROUTE_MAX) if batch else (lambda i: True)
        fresh = [i for i in range(len(ctx.chunks)) if ctx.dig[i] not in store.held and fits(i)]
        picks = _some(rng, [r for r in good if fits(r)], n_held)
        picks += _some(rng, fresh, size - len(picks))
        picks += _some(rng, [r for r in good if r not in set(picks) and fits(r)], size - len(picks))
        picks = [picks[int(i)] for i in rng.permutation(len(picks))]
        if op == _E:
            coding = coding or 1
            return dict(rec, chunks=picks, level=(coding - 1) % 2 + 1, entropy=coding >= 3, verify=flip(), route="batch" if batch else "pack")
        items = [[i, coding] for i in picks]
        if size >= 2 and rng.integers(0, 3) == 0:                                          # repeats inside the add (this file's head)
            for i in _some(rng, [i for i in picks if ctx.dig[i] in store.held], 5):
                items.insert(int(rng.integers(0, len(items) + 1)), [i, (coding + 1 + int(rng.integers(0, 4))) % 5])
            for i in _some(rng, [i for i in picks if ctx.dig[i] not in store.held], 5):
                items.insert(int(rng.integers(0, len(items) + 1)), [i, coding])
        dmg = []
        if ctx.kind == "damaged":
            for j in sorted(_some(rng, [j for j in range(len(ctx.dmg)) if ctx.dmg[j][3] not in store.held], _pick(rng, [0, 3, 8, 12, 12]))):
                dmg.append([int(rng.integers(0, len(items) + len(dmg) + 1)), j])
        return dict(rec, items=items, dmg=dmg, verify=bool(rng.integers(0, 4) == 0) if dmg else flip())
    if op == "add_cut_of_other":
        theirs = ctx.held_refs(1 - s)
        request = _some(rng, theirs, int(rng.integers(1, 300)))
        request += _some(rng, request, 5)
        return dict(rec, request=request, verify=flip())
    if op == "add_open_cut":
        return dict(rec, cut=_pick(rng, sorted(c for c, of in ctx.cut_of.items() if of == 1 - s and c in ctx.open_cuts)), verify=flip())
    if op in ("cut", "missing"):
        request = _some(rng, good, int(rng.integers(1, 200)))
        request += _some(rng, request, 7)
        if op == "missing":
            request += _some(rng, [i for i in range(len(ctx.chunks)) if ctx.dig[i] not in store.held], 20)
            request += [NEVER + int(x) for x in rng.integers(0, 50, 6)]
        request = [request[int(i)] for i in rng.permutation(len(request))]
        if op == "cut" and bad and rng.integers(0, 5) < 2:                                 # one damaged entry among them
            request.insert(int(rng.integers(0, len(request) + 1)), _pick(rng, bad))
        rec = dict(rec, request=request, lengths=flip())
        if op == "cut":
            rec.update(verify=flip(), open=len(ctx.open_cuts) < MAX_OPEN and flip(), id=step)
        return rec
    if op == "prune":
        other = len(ctx.stores) == 2 and ctx.stores[1 - s].held and rng.integers(0, 10) < 3
        permille = _pick(rng, [0, 300, 600, 1000])
        if other:                                                                          # keep = the other set's entries()
            return dict(rec, other=True, keep=True, permille=permille)
        if rng.integers(0, 12) == 0:                                                       # n = 0: DROP changes nothing, KEEP empties the set
            return dict(rec, request=[], keep=bool(rng.integers(0, 4) == 0), permille=permille)
        keep, part = flip(), _pick(rng, [0.25, 0.4, 0.5, 0.6, 0.75])
        spare = bool(bad) and rng.integers(0, 10) < 7                                      # the damaged entries stay, to be moved
        pool = good + ([] if spare else bad)
        request = _some(rng, pool, int(len(pool) * part))
        if spare and keep:
            request += bad
        request += _some(rng, request, 9) + [NEVER + int(x) for x in rng.integers(0, 50, 4)]
        return dict(rec, request=request, keep=keep, permille=permille)
    if op == "recode":
        return dict(rec, level=int(rng.integers(1, 3)), entropy=flip(), verify=bool(rng.integers(0, 4) == 0) if bad else flip(),
                    scratch=_pick(rng, [0, 100000]))
    if op == "restore":
        files = []
        for _ in range(int(rng.integers(1, 4))):
            f = _some(rng, good, int(rng.integers(1, 40)))
            files.append(f + _some(rng, f, 3))
        if bad and rng.integers(0, 5) < 2:                                                 # one damaged entry among them
            f = _pick(rng, files)
            f.insert(int(rng.integers(0, len(f) + 1)), _pick(rng, bad))
        return dict(rec, files=files, verify=flip(), open=len(ctx.open_batches) < MAX_OPEN and flip(), id=step)
    raise ValueError(op)


_KIND_ID = {"clean": 1, "damaged": 2, "two_sets": 3}


def walk(kind, seed, n_steps=STEPS, n_generated=N_GENERATED):
    """-> n_steps plain op records, op and parameters drawn from the seed and the model's state as it goes: walk(kind, seed, k) is
    the first k of walk(kind, seed, n) for any n >= k"""
    ctx = Ctx(kind, n_generated=n_generated)
    rng = np.random.default_rng([_KIND_ID[kind], seed])
    recs = []
    for step in range(n_steps):
        rec = _draw(ctx, rng, step, seed)
        apply(ctx, rec)
        recs.append(rec)
    return recs
