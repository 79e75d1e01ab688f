"""Inputs for the chunk store's tests beyond the plan's first round and the wave grids' first trip, and their plain models.  No
engine code is involved: the per-chunk models are zpack_cases.compress_chunk, zpack2_cases.compress_chunk2 and
zentropy_cases.compress_chunk_h, the digests are hashlib's, and every layout is restated here in numpy (row order, each span
rounded up to 16, zero pads) because the row-by-row models of the other case files take minutes at these sizes.

The constants, from the code:
  PLAN_TILE   csrc/mi_plan.h: kPlanTile = 256 threads * 8 rows a block of the plan's block sums and compaction;
  PLAN_ROUND  csrc/mi_plan.h, plan_block_offsets: ONE block of 256 threads scans 256 block sums a round and carries carry_a /
              carry_b into the next: a second round exists only above 256 * 2 048 = 524 288 rows (mi_zprune / mi_zrecode: slots);
  WAVE_GRID   csrc/mi_zpack.hip and mi_zrecode.hip, wave_grid(n) = min(n, 2^20): workgroup j goes on to row j + 2^20;
  N_ROWS      WAVE_GRID + 300 = 1 048 876 rows: 513 plan blocks = three rounds (256 + 256 + 1), 300 second trips.

MILLION ROWS (million_rows).  Row k is TINY unless planted: the 8 bytes of k * ODD mod 2^64 (a bijection of k) and k % 5 filler
bytes -- 8..12 bytes, distinct, under zpack_cases.MIN_CHUNK, so its stored form is itself at every level with and without the
entropy stage, and every 16 KiB gather tile holds exactly 1 024 entries.  PLANTED rows (planted_rows) are coded by the per-chunk
models; their kind is k % 8, their bytes are seeded by k.  Rows j and WAVE_GRID + j have the same kind (2^20 % 8 == 0).

A RUN BATCH (batch_files) for Engine(mask_bits=0, min_size=64, max_size=64): 526 413 chunks, 1 251 files with a tail chunk."""
import functools

import numpy as np

import pack_cases as pc
import zentropy_cases as ze
import zentropy_rows_cases as zr
import zpack_cases as zc
import zpack2_cases as z2

PLAN_TILE = 2048
PLAN_ROUND = 256 * PLAN_TILE
WAVE_GRID = 1 << 20
TRIP = 300
N_ROWS = WAVE_GRID + TRIP
EDGE_SIZES = (PLAN_ROUND, PLAN_ROUND + 1, PLAN_ROUND + PLAN_TILE + 77)
EVERY = 4099
ODD = 0x9E3779B97F4A7C15
GATHER_TILE = 16384
MODELS = ("l1", "l2", "l1h")                                       # level 1, level 2, level 1 with the entropy stage
assert PLAN_ROUND == 524288 and N_ROWS == 1048876 and (N_ROWS + PLAN_TILE - 1) // PLAN_TILE == 513


def round16(a):
    return (a + 15) // 16 * 16


# ---- numpy layouts -------------------------------------------------------------------------------------------------------------------
def layout(sizes):
    """sizes in row order -> (offsets, total): every span on the sum of the spans before it, each rounded up to 16"""
    spans = round16(np.asarray(sizes, dtype=np.uint64))
    ends = np.cumsum(spans)
    return ends - spans, int(ends[-1]) if len(ends) else 0


def layout_without_carry(sizes):
    """THE WRONG LAYOUT of a plan_block_offsets that drops its carry: every round of PLAN_ROUND rows begins again at 0"""
    off, _ = layout(sizes)
    start = (np.arange(len(off)) // PLAN_ROUND) * PLAN_ROUND
    return off - off[start]


def copy_spans(dst, dst_off, src, src_off, lens, slab=1 << 16):
    """dst[dst_off[i] : + lens[i]] = src[src_off[i] : + lens[i]] for every i (uint8 arrays; spans of any alignment)"""
    dst_off, src_off, lens = (np.asarray(x, dtype=np.int64) for x in (dst_off, src_off, lens))
    for a in range(0, len(lens), slab):
        n = lens[a:a + slab]
        ends = np.cumsum(n)
        within = np.arange(int(ends[-1]), dtype=np.int64) - np.repeat(ends - n, n)
        dst[np.repeat(dst_off[a:a + slab], n) + within] = src[np.repeat(src_off[a:a + slab], n) + within]


def gather(blob, offsets, sizes, rows):
    """spans `rows` of a blob on the 16-byte grid, in that order -> (their new offsets, the new blob as bytes): the plain model
    of every cut -- mi_packset_pack, mi_zset_zpack, a prune's compaction -- over sources whose pads are zero"""
    src = np.frombuffer(blob, dtype=np.uint8)
    off, total = layout(np.asarray(sizes)[rows])
    out = np.zeros(total, dtype=np.uint8)
    if len(rows):
        copy_spans(out, off, src, np.asarray(offsets)[rows], round16(np.asarray(sizes, dtype=np.int64)[rows]))
    return off, out.tobytes()


def first_occurrences(ids):
    """the request rows at which an id occurs for the first time, ascending (fetch_cases.model_subpack's rule in numpy)"""
    _, first = np.unique(np.asarray(ids), return_index=True)
    return np.sort(first)


def digests_of(blob, offsets, lengths, alg=pc.SHA256):
    h, view = pc.HASHES[alg], memoryview(blob)
    out = bytearray(32 * len(offsets))
    for i, (o, n) in enumerate(zip(offsets.tolist(), lengths.tolist())):
        out[32 * i:32 * i + 32] = h(view[o:o + n]).digest()
    return np.frombuffer(bytes(out), dtype=np.uint8).reshape(-1, 32)


def entries_of(dtype, digests, offsets, index, lengths, stored=None):
    e = np.zeros(len(offsets), dtype=dtype)
    e["digest"], e["offset"], e["chunk_index"], e["length"] = digests, offsets, index, lengths
    if stored is not None:
        e["stored"] = stored
    return e


# ---- the planted rows ---------------------------------------------------------------------------------------------------------------------
def planted_rows():
    s = set(range(TRIP)) | set(range(WAVE_GRID, WAVE_GRID + TRIP)) | set(range(PLAN_TILE - 2, PLAN_TILE + 2))
    for edge in (PLAN_ROUND, 2 * PLAN_ROUND):
        s |= set(range(edge - 2, edge + 2))
    s |= {N_ROWS - 1} | set(range(0, N_ROWS, EVERY))
    return np.array(sorted(s), dtype=np.int64)


BOUNDARY_ROWS = tuple(k for edge in (PLAN_TILE, PLAN_ROUND, 2 * PLAN_ROUND) for k in range(edge - 2, edge + 2))
KINDS = ("lz4", "h over lz4", "raw", "h over raw", "lz4", "level 2 only", "mix", "h over lz4")           # by k % 8


def planted_chunk(k):
    """zpack_cases.text_like: on the model 200..1 200 bytes give LZ4, 2 500..4 500 H over LZ4, 1 500..2 500 either; 64 random
    bytes code raw; zentropy_rows_cases' 16 symbols at random give H over the plain bytes.  "level 2 only" is zpack2_cases'
    "backwards to a differing byte": a filler without a 4-byte repeat in which [110, 140) copies [70, 100) -- both begin in one
    step, level 1 finds 12 bytes of the copy from the next step on and keeps the chunk raw, level 2 goes back to 110 and keeps
    its block (text_like is so regular that both levels give nearly every such chunk the same size: this kind is what the
    recode replaces).  Every chunk holds or is seeded by k"""
    kind = KINDS[k % 8]
    if kind == "lz4":
        return zc.text_like(200 + (k * 37) % 1001, k)
    if kind == "h over lz4":
        return zc.text_like(2500 + (k * 37) % 2001, k)
    if kind == "mix":
        return zc.text_like(1500 + (k * 37) % 1001, k)
    rng = np.random.default_rng(k)
    if kind == "raw":
        return rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    if kind == "level 2 only":
        return bytes(zc.plant(zc.filler(rng, 180 + (k * 37) % 61), 70, 110, 30))
    return zr._h_over_raw(rng, k)


CODERS = {"l1": zc.compress_chunk, "l2": z2.compress_chunk2, "l1h": lambda c: ze.compress_chunk_h(c, 1)}


@functools.lru_cache(maxsize=None)
def planted():
    """-> (rows, chunks, {model: the stored forms}): THE PER-CHUNK MODELS, once per process whatever the digest"""
    rows = planted_rows()
    chunks = [planted_chunk(int(k)) for k in rows]
    return rows, chunks, {m: [CODERS[m](c) for c in chunks] for m in MODELS}


# ---- the million rows ------------------------------------------------------------------------------------------------------------------------
class Model:
    """one compressed form of the rows: stored (sizes), offsets, zentries, zblob, forms (zentropy_cases.form_of per row), census"""


class Rows:
    """n rows as a plain pack (entries, blob; lengths, offsets, digests, lens32), the planted rows among them (planted: their
    numbers, ascending; planted_chunks) and the three compressed models (models[m] for m in MODELS)"""

    def chunk(self, k):
        o = int(self.offsets[k])
        return self.blob[o:o + int(self.lengths[k])]

    def plain_of(self, rows):
        """the chunks of `rows` joined, without pads"""
        n = self.lengths[rows].astype(np.int64)
        ends = np.cumsum(n)
        out = np.zeros(int(ends[-1]), dtype=np.uint8)
        copy_spans(out, ends - n, np.frombuffer(self.blob, dtype=np.uint8), self.offsets[rows], n)
        return out.tobytes()


@functools.lru_cache(maxsize=1)
def million_rows(alg=pc.SHA256):
    """(the cache holds ONE digest's rows, some 250 MB: a module's fixture keeps its own alive and calls clear_caches when it ends)"""
    rows, chunks, forms = planted()
    r = Rows()
    r.n, r.alg = N_ROWS, alg
    k = np.arange(N_ROWS, dtype=np.uint64)
    r.lengths = (8 + k % 5).astype(np.uint32)
    r.lengths[rows] = [len(c) for c in chunks]
    r.offsets, total = layout(r.lengths)
    blob = np.zeros(total, dtype=np.uint8)
    tiny = np.ones(N_ROWS, dtype=bool)
    tiny[rows] = False
    at = r.offsets[tiny].astype(np.int64)
    keys = (k[tiny] * np.uint64(ODD)).astype("<u8").view(np.uint8).reshape(-1, 8)            # (wraps mod 2^64: ODD is odd, a bijection)
    blob[at[:, None] + np.arange(8)] = keys
    extra = (k[tiny] % 5).astype(np.int64)
    for i in range(4):
        blob[at[extra > i] + 8 + i] = 0x51 + i                                                 # filler: never zero, a pad cannot pass for it
    for row, c in zip(rows.tolist(), chunks):
        o = int(r.offsets[row])
        blob[o:o + len(c)] = np.frombuffer(c, dtype=np.uint8)
    r.blob = blob.tobytes()
    r.digests = digests_of(r.blob, r.offsets, r.lengths, alg)
    r.lens32 = r.lengths.copy()
    r.entries = entries_of(pc.ENTRY_DTYPE, r.digests, r.offsets, np.arange(N_ROWS), r.lengths)
    r.planted, r.planted_chunks = rows, chunks
    r.is_planted = ~tiny
    r.models = {}
    units = blob.reshape(-1, 16)
    for m in MODELS:
        z = Model()
        z.stored = r.lengths.copy()                                  # THE RULE: a chunk under MIN_CHUNK bytes is kept as it is
        z.stored[rows] = [len(f) for f in forms[m]]
        z.offsets, ztotal = layout(z.stored)
        zblob = np.zeros(ztotal, dtype=np.uint8)
        zblob.reshape(-1, 16)[(z.offsets[tiny] // 16).astype(np.int64)] = units[at // 16]       # a tiny row is one 16-byte unit in both blobs
        for row, f in zip(rows.tolist(), forms[m]):
            o = int(z.offsets[row])
            zblob[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
        z.zblob = zblob.tobytes()
        z.zentries = entries_of(zc.ZENTRY_DTYPE, r.digests, z.offsets, np.arange(N_ROWS), r.lengths, z.stored)
        z.forms = np.zeros(N_ROWS, dtype=np.uint8)
        z.forms[rows] = [ze.form_of(f, len(c)) for f, c in zip(forms[m], chunks)]
        z.census = census(z.forms, z.stored)
        r.models[m] = z
    return r


def clear_caches():
    """drops the large cached inputs (the planted rows' per-chunk models, which are small and slow, stay)"""
    for f in (million_rows, batch_files, batch_digests, batch_stored):
        f.cache_clear()


def census(forms, stored):
    """[[n, stored bytes]] * 4 in zentropy_cases.form_of's order, as mi_zforms counts"""
    return [[int((forms == f).sum()), int(stored[forms == f].astype(np.uint64).sum())] for f in range(4)]


def sliced(r, n):
    """the same pack and models cut to their first n entries"""
    assert 0 < n <= r.n
    if n == r.n:
        return r
    s = Rows()
    s.n, s.alg = n, r.alg
    s.lengths, s.offsets, s.digests, s.lens32, s.entries = r.lengths[:n], r.offsets[:n], r.digests[:n], r.lens32[:n], r.entries[:n]
    s.blob = r.blob[:int(r.offsets[n])]
    keep = r.planted < n
    s.planted, s.planted_chunks = r.planted[keep], [c for c, k in zip(r.planted_chunks, keep) if k]
    s.is_planted = r.is_planted[:n]
    s.models = {}
    for m, z in r.models.items():
        c = Model()
        c.stored, c.offsets, c.zentries, c.forms = z.stored[:n], z.offsets[:n], z.zentries[:n], z.forms[:n]
        c.zblob = z.zblob[:int(z.offsets[n])]
        c.census = census(c.forms, c.stored)
        s.models[m] = c
    return s


def tile_population(offsets, total):
    """entries that BEGIN in every 16 KiB tile of a blob"""
    return np.bincount((np.asarray(offsets) // GATHER_TILE).astype(np.int64), minlength=(total + GATHER_TILE - 1) // GATHER_TILE)


def pseudo_random_half(n, seed=1601):
    """one flag per row, about half of them set, both kinds on each side of every threshold"""
    return np.random.default_rng(seed).integers(0, 2, n, dtype=np.uint8).astype(bool)


def permuted_request(r, seed=1602, repeats=1000, unknown=1000):
    """every row once in a seeded order, `repeats` rows a second time and `unknown` digests nobody holds, shuffled among them
    -> (ids: the row per request row, r.n + i for the i-th unknown digest; digests; lengths)"""
    rng = np.random.default_rng(seed)
    ids = np.concatenate([rng.permutation(r.n), rng.integers(0, r.n, repeats), r.n + np.arange(unknown)])
    ids = ids[rng.permutation(len(ids))]
    strangers = np.zeros((unknown, 32), dtype=np.uint8)
    strangers[:, :8] = np.arange(unknown, dtype="<u8").view(np.uint8).reshape(-1, 8)
    strangers[:, 8:] = 0xEE                                          # (checked against the digests in the host test)
    digests = np.ascontiguousarray(np.concatenate([r.digests, strangers])[ids])
    lengths = np.concatenate([r.lens32, np.full(unknown, 77, dtype=np.uint32)])[ids]
    return ids, digests, lengths


def crafted_digests(n):
    """n opaque digests for unverified sets, zprune_cases.crafted_digests in numpy: row k's first eight bytes are k + 1, little
    endian.  A slot table's home of a digest is those eight bytes & (cap - 1), so in a table of more than n + 1 slots row k is
    AT HOME in slot k + 1, nothing collides, and slot order -- the order of a recode's rows -- is row order"""
    dig = np.random.default_rng(1606).integers(0, 256, (n, 32), dtype=np.uint8)
    dig[:, :8] = np.arange(1, n + 1, dtype="<u8").view(np.uint8).reshape(n, 8)
    return dig


def zpack_of_rows(r, stored, sources, pick, rows=None):
    """a zpack of `rows` (every row if None) in that order, row k's form taken from sources[pick[k]] (models of r), its size
    stored[k] -> (zentries with chunk_index = the place in `rows`, zblob): what a set that holds these forms cuts"""
    rows = np.arange(r.n) if rows is None else np.asarray(rows)
    off, total = layout(stored[rows])
    out = np.zeros(total, dtype=np.uint8)
    for i, z in enumerate(sources):
        mine = pick[rows] == i
        if mine.any():
            assert (z.stored[rows[mine]] == stored[rows[mine]]).all()
            copy_spans(out, off[mine], np.frombuffer(z.zblob, dtype=np.uint8), z.offsets[rows[mine]], round16(stored[rows[mine]].astype(np.int64)))
    return entries_of(zc.ZENTRY_DTYPE, r.digests[rows], off, np.arange(len(rows)), r.lengths[rows], stored[rows]), out.tobytes()


def model_prune(stored, lengths, kept, n_rows, n_unknown, cap, blob_bytes, permille, table_bytes=None):
    """zprune_cases.Store.prune restated in numpy for a set of ONE blob whose held rows have these stored sizes and lengths:
    kept (one flag per held row) stay -> (mi_prune_info's counters, mi_zset_usage afterwards), both as dicts.  The host test
    holds it against zprune_cases.Store on a slice.  table_bytes: what the table takes now, if a prune has rebuilt it before
    (None: it is as the adds left it)"""
    import zprune_cases as pr
    spans = round16(stored.astype(np.int64))
    gone = ~kept
    info = dict.fromkeys(["n_rows", "n_unknown", "n_dropped", "dropped_stored_bytes", "dropped_chunk_bytes", "n_blobs_freed", "freed_bytes",
                          "n_blobs_compacted", "moved_bytes", "n_blobs_sparse_kept", "peak_extra_bytes"], 0)
    info.update(n_rows=n_rows, n_unknown=n_unknown, n_dropped=int(gone.sum()), dropped_stored_bytes=int(stored[gone].astype(np.int64).sum()),
                dropped_chunk_bytes=int(lengths[gone].astype(np.int64).sum()))
    extra = pr.alloc(n_rows * 32) + pr.alloc(cap) + pr.alloc(cap * 4) + 2 * pr.alloc(8) + pr.alloc(64)
    live, survive = int(spans[kept].sum()), int(kept.sum())
    usage = {"n_blobs": 1, "resident_bytes": pr.alloc(blob_bytes), "live_bytes": live, "table_slots": cap,
             "table_bytes": pr.grown(cap * 8) + pr.grown(cap * 48) if table_bytes is None else table_bytes}
    if not gone.any():
        info["peak_extra_bytes"] = extra
        return info, usage
    dead, sparse = live == 0, 0 < live * 1000 < permille * blob_bytes
    if sparse:
        nb = (cap + PLAN_TILE - 1) // PLAN_TILE
        extra += pr.alloc(1) + pr.alloc((2 * nb + 8) * 8) + pr.alloc(live) + pr.alloc(4 * survive * 8) + pr.alloc(cap * 8)
    new_cap = 1024
    while new_cap < 2 * survive:
        new_cap *= 2
    table = pr.alloc(new_cap * 8) + pr.alloc(new_cap * 48)
    extra += table + pr.alloc(survive * 48) + pr.alloc(survive + 16) + pr.alloc(survive * 8 + 16) + pr.alloc(64)
    info["peak_extra_bytes"] = extra
    if dead or sparse:
        info.update(n_blobs_freed=1, freed_bytes=pr.alloc(blob_bytes))
    if sparse:
        info.update(n_blobs_compacted=1, moved_bytes=live)
    usage.update(n_blobs=0 if dead else 1, resident_bytes=0 if dead else pr.alloc(live) if sparse else pr.alloc(blob_bytes), table_slots=new_cap,
                 table_bytes=table)
    return info, usage


# ---- the second trip on a table nobody cleared ---------------------------------------------------------------------------------------------
def second_trip_with_dirty_table(first, second):
    """THE WRONG FORM of a level-1 coder whose wave does not clear its match table between its rows: the chunk `second` parsed
    on the table the parse of `first` left behind -> the stored form (the keep rule as ever)"""
    table = np.zeros(zc.TABLE, dtype=np.int64)
    zc.parse(first, table)
    block = zc.encode(second, zc.parse(second, table))
    n = len(second)
    return block if len(block) < n - (n >> 4) else bytes(second)


# ---- a run batch of 526 413 chunks -----------------------------------------------------------------------------------------------------------
CHUNK = 64
BATCH_CHUNKS = PLAN_ROUND + PLAN_TILE + 77
BATCH_SIZES = (BATCH_CHUNKS, PLAN_ROUND, PLAN_ROUND + 1)
ONE_IN = 500


def file_plan(n_chunks):
    """-> [(full chunks, tail bytes)] per file: 1 000 files of 500 chunks and a tail, then files of 100 chunks and a tail, then
    one file of what is left, without a tail; tails of 1..63 bytes, file i's is 1 + i % 63"""
    files, left = [], n_chunks
    while len(files) < 1000 and left >= 501 + 20000:
        files.append((500, 1 + len(files) % 63))
        left -= 501
    while left >= 101 + 50:
        files.append((100, 1 + len(files) % 63))
        left -= 101
    if left:
        files.append((left, 0))
    assert sum(q + (t > 0) for q, t in files) == n_chunks
    return files


class BatchFiles:
    """files (bytes each), data (all of them joined, uint8), rows as a pure-Python cut at 64 gives them: file, offset (in the
    file), length, at (in data); compressible: the rows planted to code; tails: the rows shorter than 64"""


@functools.lru_cache(maxsize=1)
def batch_files(n_chunks=BATCH_CHUNKS):
    plan = file_plan(n_chunks)
    sizes = np.array([q * CHUNK + t for q, t in plan], dtype=np.int64)
    starts = np.cumsum(sizes) - sizes
    b = BatchFiles()
    b.data = np.random.default_rng(1700 + n_chunks % 1000).integers(0, 256, int(sizes.sum()), dtype=np.uint8)
    per_file = (sizes + CHUNK - 1) // CHUNK
    b.file = np.repeat(np.arange(len(plan)), per_file)
    first_row = np.cumsum(per_file) - per_file
    b.offset = (np.arange(n_chunks) - first_row[b.file]) * CHUNK
    b.length = np.minimum(CHUNK, sizes[b.file] - b.offset).astype(np.uint32)
    b.at = starts[b.file] + b.offset
    b.n = n_chunks
    b.tails = np.flatnonzero(b.length < CHUNK)
    b.compressible = np.array([k for k in range(ONE_IN // 2, n_chunks, ONE_IN) if b.length[k] == CHUNK], dtype=np.int64)
    for k in b.compressible.tolist():                                # zentropy_rows_cases' 64 bytes of a short period, the row's number in them
        b.data[int(b.at[k]):int(b.at[k]) + CHUNK] = np.frombuffer(zr._short_lz4(None, k), dtype=np.uint8)
    raw = b.data.tobytes()
    b.files = [raw[int(s):int(s + n)] for s, n in zip(starts, sizes)]
    return b


def python_cut(files):
    """the rows Engine(mask_bits=0, min_size=64, max_size=64) must give, in pure Python: every file cut at 64"""
    return [(f, at, min(CHUNK, len(x) - at)) for f, x in enumerate(files) for at in range(0, len(x), CHUNK)]


def no_quad_repeats(data, at):
    """per 64-byte chunk at data[at[i]:]: True where no 4-byte value occurs twice inside it.  Then the level-1 parse finds no
    match (a candidate counts only if its 4 bytes are equal), the block is all literals, 66 bytes, and the chunk is stored raw"""
    out = np.zeros(len(at), dtype=bool)
    for a in range(0, len(at), 1 << 16):
        c = data[np.asarray(at[a:a + (1 << 16)], dtype=np.int64)[:, None] + np.arange(CHUNK)].astype(np.uint32)
        quad = np.sort(c[:, :-3] | c[:, 1:-2] << 8 | c[:, 2:-1] << 16 | c[:, 3:] << 24, axis=1)
        out[a:a + len(c)] = (quad[:, 1:] != quad[:, :-1]).all(axis=1)
    return out


@functools.lru_cache(maxsize=1)
def batch_digests(n_chunks=BATCH_CHUNKS, alg=pc.SHA256):
    b = batch_files(n_chunks)
    return digests_of(b.data.tobytes(), b.at, b.length, alg)


def selections(n):
    """name -> one flag per row, or None for every row"""
    rows = np.arange(n)
    return {"all": None, "half": pseudo_random_half(n, 1603), "from the second round on": rows >= PLAN_ROUND, "the first round": rows < PLAN_ROUND}


def model_batch_pack(b, select=None, digests=None):
    """pack_cases.model_pack in numpy: the selected rows in row order -> (entries, blob)"""
    rows = np.arange(b.n) if select is None else np.flatnonzero(select)
    digests = batch_digests(b.n) if digests is None else digests
    off, total = layout(b.length[rows])
    blob = np.zeros(total, dtype=np.uint8)
    if len(rows):
        copy_spans(blob, off, b.data, b.at[rows], b.length[rows])
    return entries_of(pc.ENTRY_DTYPE, digests[rows], off, rows, b.length[rows]), blob.tobytes()


@functools.lru_cache(maxsize=2)
def batch_stored(n_chunks=BATCH_CHUNKS, level=1):
    """every row's stored form at `level` -> (stored sizes, {row: the coded form} for the rows that are not raw, how many random
    64-byte chunks needed the per-chunk model).  A random chunk that passes no_quad_repeats is PROVEN raw at both levels (level
    2's candidates, of either table, count only if their 4 bytes are equal too); every other row -- the planted compressible
    chunks, the tails of 13 bytes and more, a random chunk that fails the check -- goes through zpack_cases.compress_chunk or
    zpack2_cases.compress_chunk2"""
    coder = zc.compress_chunk if level == 1 else z2.compress_chunk2
    b = batch_files(n_chunks)
    proven = np.zeros(b.n, dtype=bool)
    full = b.length == CHUNK
    full[b.compressible] = False
    rows = np.flatnonzero(full)
    proven[rows] = no_quad_repeats(b.data, b.at[rows])
    proven[b.length < zc.MIN_CHUNK] = True                           # THE RULE for the short tails
    stored, coded = b.length.copy(), {}
    for k in np.flatnonzero(~proven).tolist():
        c = b.data[int(b.at[k]):int(b.at[k]) + int(b.length[k])].tobytes()
        f = coder(c)
        if len(f) < len(c):
            stored[k], coded[k] = len(f), f
    return stored, coded, int((full & ~proven).sum())


def model_batch_zpack(b, select=None, level=1):
    """zbatch_cases.model_zpack in numpy (level 2: over zpack2_cases' coder) -> (zentries, zblob)"""
    stored, coded, _ = batch_stored(b.n, level)
    rows = np.arange(b.n) if select is None else np.flatnonzero(select)
    off, total = layout(stored[rows])
    blob = np.zeros(total, dtype=np.uint8)
    raw = stored[rows] == b.length[rows]
    copy_spans(blob, off[raw], b.data, b.at[rows[raw]], b.length[rows[raw]])
    for o, k in zip(off[~raw].tolist(), rows[~raw].tolist()):
        blob[o:o + len(coded[k])] = np.frombuffer(coded[k], dtype=np.uint8)
    return entries_of(zc.ZENTRY_DTYPE, batch_digests(b.n)[rows], off, rows, b.length[rows], stored[rows]), blob.tobytes()
