"""GPU tests of zpack level 2 (MI_ZPACK_LEVEL2, MI_MEMFS_ZPACK_LEVEL2): every blob and every entry array the device produces at
level 2 is compared byte for byte with the model of zpack2_cases.py -- planted chunks whose sequence lists are known by
construction, one per rule of the parse -- the zpack coded straight from the arena with the one compressed from the plain pack,
and the level-2 zpack goes through every reader of stored forms, none of which knows of levels.  The last test holds level 1's
bytes against level 1's model for the same chunks: without the flag nothing changes.  Bit for bit: there are no tolerances."""
import ctypes as C
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
import zbatch_cases as bc  # noqa: E402
import zpack2_cases as z2  # noqa: E402
import zpack_cases as zc  # noqa: E402
from commit_cases import commit_to_bytes, make_tree, write_file  # noqa: E402

pytestmark = pytest.mark.gpu
MTIME = 1_600_000_000
SUBSET = ("text 4095", "the 8-byte table's candidate is longer", "a later lane inside the first's match wins",
          "backwards to the anchor: literal run 0", "a source inside an earlier match", "match length 132, the cap is 68", "zeros")


@pytest.fixture(scope="module")
def cases():
    """the planted chunks, their plain pack and both models of it, computed once and left as they are"""
    got = z2.planted_chunks2()
    chunks = [c for _, c, _ in got]
    entries, blob = zc.pack_of(chunks)
    return {"cases": got, "chunks": chunks, "entries": entries, "blob": blob, "l1": zc.model_compress(entries, blob),
            "l2": z2.model_compress2(entries, blob)}


def _engine(alg):
    return M.Engine(flags=M.FLAG_CHUNK_BLAKE2S if alg == pc.BLAKE2S else 0)


def _pack_of(engine, entries, blob):
    """a plain pack laid out by hand -> a Pack that holds it (through a set: mi_packset_pack takes any length)"""
    with engine.packset() as s:
        s.add_blob(blob, entries, verify=True)
        p = s.pack(np.ascontiguousarray(entries["digest"]), verify=True)
    assert pc.same_entries(p.entries(), entries) and p.bytes() == blob
    return p


def _same(z, want, what):
    want_e, want_b = want
    got_e, got_b = z.entries().copy(), z.read()
    differ = [(k, int(got_e["stored"][k]), int(want_e["stored"][k])) for k in range(min(len(got_e), len(want_e)))
              if got_e["stored"][k] != want_e["stored"][k] or got_e["offset"][k] != want_e["offset"][k]][:10]
    assert bc.same_zentries(got_e, want_e), (what, differ)
    assert got_b == want_b, (what, next(i for i in range(max(len(want_b), len(got_b))) if i >= min(len(got_b), len(want_b)) or got_b[i] != want_b[i]))
    return got_e, got_b


# ---- 1. the planted chunks at level 2 ------------------------------------------------------------------------------------------------
def test_planted_chunks_code_to_the_level_2_models_bytes(cases):
    for name, chunk, want in cases["cases"]:
        if want is not None:
            assert z2.parse2(chunk) == want, name
    want_e, want_b = cases["l2"]
    assert (want_e["stored"] < cases["l1"][0]["stored"]).any() and want_b != cases["l1"][1]    # the two levels differ on these chunks
    with M.Engine() as e, _pack_of(e, cases["entries"], cases["blob"]) as p:
        for verify in (False, True):
            flags = M.ZPACK_LEVEL2 | (M.ZPACK_VERIFY if verify else 0)                          # the flag alone, and with VERIFY
            h = C.c_void_p()
            assert e._lib.mi_pack_compress(p._h, flags, C.byref(h)) == 0, e._lib.mi_last_error(e._h)
            with M.ZPack(e, h) as z:
                got_e, got_b = _same(z, cases["l2"], "verify=%r" % verify)
                info = z.info
                assert (info.n_entries, info.blob_bytes, info.stored_bytes, info.verified) == \
                    (len(want_e), len(want_b), int(want_e["stored"].sum()), int(verify))
                assert info.n_raw == int((want_e["stored"] == want_e["length"]).sum()) and info.ms_encode > 0
                assert M.zpack_check(got_b, got_e) is None
        assert p.bytes() == cases["blob"]                                                          # the input is unchanged
        with p.compress(verify=True, level=2) as z:                                                # the binding's keyword
            _same(z, cases["l2"], "level=2")


def test_a_subset_of_the_planted_chunks_under_blake2s(cases):
    chunks = [c for name, c, _ in cases["cases"] if name in SUBSET]
    assert len(chunks) == len(SUBSET)
    entries, blob = zc.pack_of(chunks, pc.BLAKE2S)
    want = z2.model_compress2(entries, blob)
    with _engine(pc.BLAKE2S) as e, _pack_of(e, entries, blob) as p, p.compress(verify=True, level=2) as z:
        got_e, got_b = _same(z, want, "blake2s")
        assert z.info.verified == 1 and z.info.alg == pc.BLAKE2S and M.zpack_check(got_b, got_e, alg=pc.BLAKE2S) is None


# ---- 2. straight from the arena ------------------------------------------------------------------------------------------------------
def _arena_against_pack(b, select=None, model=None):
    """b.zpack_at(2) against b.pack().compress(level=2) (and the model, if given); -> (entries, blob)"""
    with b.zpack_at(2, select, verify=True) as z, b.pack(select) as p, p.compress(level=2) as ref:
        got = _same(z, (ref.entries().copy(), ref.read()), "arena against pack + compress")
        assert z.info.verified == 1 and z.info.ms_encode > 0
        if model:
            _same(z, z2.model_compress2(p.entries().copy(), p.bytes()), "arena against the model")
    assert M.zpack_check(got[1], got[0]) is None
    return got


def test_the_arenas_zpack_is_the_packs_at_every_alignment():
    data = bc.mixed_file(seed=45, size=320 << 10) + zc.text_like(4099, 9)                         # an odd size
    odd = zc.text_like(1237, 4)
    with M.Engine(mask_bits=6, min_size=64, max_size=1024) as e, e.batch() as b:
        b.add_bytes(odd, 0)
        b.add_bytes(data, 1)
        b.run()
        rows = pc.rows_of(b.chunks())
        entries, blob = _arena_against_pack(b, model=True)
        coded = bc.kinds(entries)
        start = np.array([rows[int(k)][1] % 16 for k in entries["chunk_index"]])                 # files begin on 256-byte boundaries
        assert set(start[coded].tolist()) == set(range(16)) and coded.sum() > 100 and (~coded).sum() > 50
        with b.zpack(verify=True) as one:                                                          # level 1 of the same rows: other bytes
            assert one.info.stored_bytes != int(entries["stored"].sum())


def test_what_follows_a_chunk_in_the_arena_does_not_show(cases):
    """chunks of exactly 400 bytes under min_size = max_size = 400: the planted chunk whose match runs to n - 5 while its source
    goes on, followed once by the bytes its source goes on with and once by others.  The stored form is the model's both times"""
    chunk = dict((n, c) for n, c, _ in cases["cases"])["match to n - 5"]
    assert len(chunk) == 400 and chunk[-5:] == chunk[105:110]
    stored = z2.compress_chunk2(chunk)
    tails = [chunk[110:400] + chunk[:110], bytes(x ^ 0xFF for x in chunk[110:400]) + chunk[:110]]  # the source's next bytes; others
    assert len(tails[0]) == len(tails[1]) == 400 and tails[0][:8] != tails[1][:8]
    forms = []
    for tail in tails:
        with M.Engine(mask_bits=0, min_size=400, max_size=400) as e, e.batch() as b:
            b.add_bytes(chunk + tail, 0)
            b.run()
            assert [r[1:] for r in pc.rows_of(b.chunks())] == [(0, 400), (400, 400)]
            entries, blob = _arena_against_pack(b, model=True)
            forms.append(blob[:int(entries["stored"][0])])
    assert forms[0] == forms[1] == stored


def test_more_entries_than_the_encode_launch_has_waves_at_level_2():
    """32 768 + 300 chunks of 64 bytes: the first 300 workgroups go round again (mi_pack_compress's launch has a workgroup an
    entry, so the two sides differ in their grids)"""
    n = bc.ENCODE_GRID + 300
    rng = np.random.default_rng(46)
    pieces = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() if k % 3 else bytes((k + j % (1 + k % 7)) & 255 for j in range(64))
              for k in range(n)]
    with M.Engine(mask_bits=0, min_size=64, max_size=64) as e, e.batch() as b:
        b.add_bytes(b"".join(pieces), 0)
        b.run()
        assert len(b.chunks()) == n
        entries, blob = _arena_against_pack(b)
        coded = bc.kinds(entries)
        assert coded[bc.ENCODE_GRID:].any() and (~coded[bc.ENCODE_GRID:]).any()
        for k in (2, bc.ENCODE_GRID + 2, n - 1):                                                  # the model, on both trips
            at, stored = int(entries["offset"][k]), int(entries["stored"][k])
            assert blob[at:at + stored] == z2.compress_chunk2(pieces[k]), k


# ---- 3. every reader of stored forms ---------------------------------------------------------------------------------------------------
def test_the_level_2_zpack_goes_through_every_reader(cases):
    chunks, entries, blob = cases["chunks"], cases["entries"], cases["blob"]
    dig = np.ascontiguousarray(entries["digest"])
    lengths = entries["length"].astype(np.uint32)
    recipes = [(dig[k:k + 1], lengths[k:k + 1]) for k in range(len(chunks))]                     # every chunk a file of its own
    with M.Engine() as e, _pack_of(e, entries, blob) as p, p.compress(level=2) as z2pack, p.compress() as z1pack:
        e2, b2 = _same(z2pack, cases["l2"], "level 2")
        e1, b1 = _same(z1pack, cases["l1"], "level 1")
        with e.packset() as s:                                                                     # decoded into an ordinary set
            s.add_zpack(z2pack, verify=True)
            with s.pack(dig, lengths, verify=True) as back:
                assert back.bytes() == blob
        with e.zset() as zs, e.batch() as r:                                                       # resident as stored
            zs.add_zpack(z2pack, verify=True)
            assert zs.info.n_digests == len(chunks) and zs.info.stored_bytes == int(e2["stored"].sum())
            sub = np.ascontiguousarray(dig[::3])
            with zs.zpack(sub, verify=True) as cut:                                                # a cut MOVES the stored spans
                ce, cb = cut.entries().copy(), cut.read()
                for k, en in enumerate(ce):
                    src = int(e2["offset"][3 * k])
                    assert int(en["stored"]) == int(e2["stored"][3 * k])
                    assert cb[int(en["offset"]):int(en["offset"]) + int(en["stored"])] == b2[src:src + int(en["stored"])]
            st = r.add_zrecipes(zs, recipes, verify=True)
            assert st.n_files == len(chunks)
            r.run()
            assert [r.read_file(i, 0, len(c)) for i, c in enumerate(chunks)] == chunks
        # the same digest at two levels: the first form stays, in either order
        for first, second, kept_e, kept_b in ((z1pack, z2pack, e1, b1), (z2pack, z1pack, e2, b2)):
            with e.zset() as zs:
                zs.add_zpack(first, verify=True)
                zs.add_zpack(second, verify=True)
                assert zs.info.n_digests == len(chunks) and zs.info.stored_bytes == int(kept_e["stored"].sum())
                with zs.zpack(dig, verify=True) as cut:
                    assert cut.read() == kept_b and bc.same_zentries(cut.entries(), kept_e)


# ---- 4. the commit ---------------------------------------------------------------------------------------------------------------------
def test_the_commits_zpack_at_level_2_is_take_pack_then_compress_at_level_2(tmp_path):
    root = str(tmp_path / "root")
    files = make_tree(root, seed=24, n_dirs=3, files_per_dir=6, mtime=MTIME)
    files["text/notes.txt"] = open(os.path.join(ROOT, "DESIGN.md"), "rb").read()[:90000]         # (the tree's files are random: this one is coded)
    write_file(os.path.join(root, "text/notes.txt"), files["text/notes.txt"], mtime=MTIME)
    with M.Engine() as eng:
        got = {}
        for level in (2, 1):
            with M.MemFS(root) as fs, M.MemFS(root) as ref, M.ChunkIndex(eng) as ix, M.ChunkIndex(eng) as ix_ref:
                fs.set_index(ix)
                fs.set_options(chunk_zpack=True, zpack_level=level)
                ref.set_index(ix_ref)
                ref.set_options(chunk_pack=True)
                r, raw = commit_to_bytes(fs, tmp_path, "l%d.tar" % level, must_scan=True, engine=eng)
                r0, raw0 = commit_to_bytes(ref, tmp_path, "l%d_ref.tar" % level, must_scan=True, engine=eng)
                assert raw == raw0 and r["tar_digest"] == r0["tar_digest"]                          # the layer does not know of levels
                with fs.take_zpack() as z, ref.take_pack() as p, p.compress(level=level) as want:
                    assert z.info.verified == 1 and len(z) > 5
                    got[level] = _same(z, (want.entries().copy(), want.read()), "the commit at level %d" % level)
                    model = (z2.model_compress2 if level == 2 else zc.model_compress)(p.entries().copy(), p.bytes())
                    _same(z, model, "the commit against the model at level %d" % level)
                assert M.zpack_check(got[level][1], got[level][0]) is None
                fs.release_device()
                ref.release_device()
        assert int(got[2][0]["stored"].sum()) < int(got[1][0]["stored"].sum())                    # DESIGN.md is text: level 2 pays here
        assert np.array_equal(got[2][0]["digest"], got[1][0]["digest"])


# ---- 5. without the flag nothing changes ----------------------------------------------------------------------------------------------------
def test_without_the_flag_the_bytes_are_level_1s(cases):
    with M.Engine() as e, _pack_of(e, cases["entries"], cases["blob"]) as p:
        for flags in (0, M.ZPACK_VERIFY):
            h = C.c_void_p()
            assert e._lib.mi_pack_compress(p._h, flags, C.byref(h)) == 0, e._lib.mi_last_error(e._h)
            with M.ZPack(e, h) as z:
                _same(z, cases["l1"], "flags %d" % flags)
                assert z.info.verified == (1 if flags else 0)
