// mi_index.hip -- a persistent, device-resident set of chunk digests: dedup ACROSS batches.
//
// The reference remembers what it has already built as content-addressed layers
// (CAS link + IsExist, lib/builder/step/common.go:88-91) and as cacheID -> "tarHex,gzipHex"
// entries behind keyvalue.Store (lib/cache/cache_manager.go:239-252,
// lib/cache/keyvalue/store.go:22-26).  The chunk-granular analogue: a set of
// chunk digests that outlives a batch -- "which chunks of this layer did an earlier layer
// already contain?" -- and that can be exported/imported as a flat byte blob so the shim can
// keep it behind the same keyvalue.Store next to the existing entries.
//
// Device side: open addressing, slot = {64-bit tag, 32-byte digest}; tag = the digest's first 8
// bytes (0 is stored as 1), 0 = empty.  mi_index_add_batch marks the batch's digests
// (mi_dedup_mark) and probes the UNIQUE rows only (dup_of == -1), in two kernels per round:
//   probe   walks from the row's slot comparing TAGS only -- the value atomicCAS returns, coherent
//           by itself: an empty slot is claimed (CAS 0 -> tag) and the digest stored, a slot with
//           an equal tag is remembered for the next kernel, anything else is walked past;
//   verify  (after the kernel boundary, when every digest stored by `probe` is visible) compares
//           all 32 bytes at the remembered slot: equal = "known"; different = a 64-bit tag
//           collision, the row goes on probing from the next slot in another round.
// No thread ever reads digest bytes another thread of the same launch may still be writing, and
// never trusts a slot's bytes without its tag, so recycled device memory cannot fake a match.
// Rounds: of k new digests that share their first 8 bytes one claims a slot per round, the others
// fail verify and move on, so the group takes k rounds.  Every round each probing row either
// finishes or moves forward at least one slot, and the table stays under half full, so no row can
// walk more than `cap` slots: `cap` rounds always suffice, and more is an error.  Every return
// after the first probe round adds the rows placed so far to `count`, which therefore always
// equals the occupied slots; export and growth copy out at most `count` digests and fail with
// MI_ERR_STATE when the table holds a different number.
// Duplicate rows inherit the flag of the row they point to.  The table is rebuilt at twice
// the size when it gets more than half full.
//
// QUERY, PRUNE, RETAIN ask and forget without adding.
//   lookup   one thread a request row: the tag first, then all 32 bytes, walking to the first empty slot -- IN ONE KERNEL.  The
//            insert needs its kernel boundary because a prober may meet a tag whose digest another thread of the same launch
//            is still storing; a lookup launch has NO WRITER of the table (the stream orders it behind every insert), so a
//            slot's bytes are as complete as its tag and the full compare may follow the tag at once.  held[i] per row; with a
//            mark array one byte at the slot found; found and unknown rows counted with one atomic a wave and value;
//   sweep    one thread an item -- a slot of the table, or a row of an exported record array (retain) -- which survives by its
//            mark and the mode.  The survivors' digests are appended to a record array under a cursor (one atomic a wave),
//            the cursor is held against the limit as index_export_kernel's is; run with limit 0 it only counts;
//   rebuild  the survivors go through index_insert (dup_of == nullptr: they are distinct) into a FRESH table sized for them --
//            a second mi_index on the stack whose buffers this call allocated -- and the tables are swapped.  Open addressing
//            with linear probing cannot delete in place: a hole in front of a survivor would end the walk that finds it.
//   retain   index_export_kernel into a device array, mi_zset.hip's lookup over it (mi_zset_lookup_enqueue), a small kernel
//            that turns its answer into one keep flag a row, then sweep and rebuild over the rows.
// The old table is never written; everything a launch needs is allocated before it (alloc_exact: the bytes rounded up to 256,
// plus 256), the row scratch is the call's own; the new table is complete and its count checked before the swap.
// BOUNDS.  lookup READS digests [0, 32 n), tags / slots [0, cap) (the walk is masked and ends after cap steps), WRITES held
// [0, n), mark [0, cap) at a slot of the walk, two totals.  sweep READS state, digests, mark at [0, n_items), WRITES out at
// [0, 32 limit) (the cursor is checked), two totals.  flags READS src [0, n), WRITES flags [0, n).
#include "mi_internal.h"
#include "mi_wave.h"

#include <string.h>

using namespace mi;

namespace {

// Row states while an insert is in progress.
enum : u8 { kRowDone = 0, kRowVerify = 1, kRowProbe = 2 };

// first round: rows with dup_of == -1 (or all rows when dup_of == nullptr) start probing
__global__ __launch_bounds__(256)
void index_begin_kernel(const u8* __restrict__ digests, const i64* __restrict__ dup_of, u64 n, u64 mask,
                        u8* __restrict__ row_state, u64* __restrict__ row_slot) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool probe = !(dup_of && dup_of[i] >= 0);
    row_state[i] = probe ? kRowProbe : kRowDone;
    row_slot[i] = tag_of(*(const u64*)(digests + 32 * i)) & mask;
}

// known[i] = 0 if the row's digest was inserted now (known may be nullptr)
__global__ __launch_bounds__(256)
void index_probe_kernel(const u8* __restrict__ digests, u64 n, u64* __restrict__ tags,
                        u8* __restrict__ slots, u64 mask, u8* __restrict__ row_state,
                        u64* __restrict__ row_slot, u8* __restrict__ known, u64* __restrict__ n_new) {
    __shared__ u32 wg_new;
    if (threadIdx.x == 0) wg_new = 0;
    __syncthreads();
    u32 mine_new = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        if (row_state[i] != kRowProbe) continue;
        const u8* d = digests + 32 * i;
        const u64 tag = tag_of(*(const u64*)d);
        u64 slot = row_slot[i];
        for (;;) {
            const u64 old = atomicCAS((unsigned long long*)&tags[slot], 0ull, (unsigned long long)tag);
            if (old == 0ull) {                               // empty: mine now
                ((u32x4*)(slots + 32 * slot))[0] = ((const u32x4*)d)[0];
                ((u32x4*)(slots + 32 * slot))[1] = ((const u32x4*)d)[1];
                if (known) known[i] = 0;
                row_state[i] = kRowDone;
                ++mine_new;
                break;
            }
            if (old == tag) {                                // full compare after the kernel boundary
                row_slot[i] = slot;
                row_state[i] = kRowVerify;
                break;
            }
            slot = (slot + 1) & mask;
        }
    }
    if (mine_new) atomicAdd(&wg_new, mine_new);
    __syncthreads();
    if (threadIdx.x == 0 && wg_new) atomicAdd((unsigned long long*)n_new, (unsigned long long)wg_new);
}

__global__ __launch_bounds__(256)
void index_verify_kernel(const u8* __restrict__ digests, u64 n, const u8* __restrict__ slots, u64 mask,
                         u8* __restrict__ row_state, u64* __restrict__ row_slot, u8* __restrict__ known,
                         u64* __restrict__ n_retry) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || row_state[i] != kRowVerify) return;
    const u64 slot = row_slot[i];
    if (digest_eq32(slots + 32 * slot, digests + 32 * i)) {
        if (known) known[i] = 1;
        row_state[i] = kRowDone;
    } else {                                                 // equal tags, different digests
        row_slot[i] = (slot + 1) & mask;
        row_state[i] = kRowProbe;
        atomicAdd((unsigned long long*)n_retry, 1ull);
    }
}

__global__ __launch_bounds__(256)
void index_inherit_kernel(const i64* __restrict__ dup_of, u64 n, u8* __restrict__ known) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const i64 d = dup_of[i];
    if (d >= 0) known[i] = known[d];                         // d < i and d is a unique row
}

// appends every occupied slot's digest to out[0, limit); the cursor counts them all, so the host
// sees a table that holds more than `limit` without a write past the buffer
__global__ __launch_bounds__(256)
void index_export_kernel(const u64* __restrict__ state, const u8* __restrict__ slots, u64 cap,
                         u8* __restrict__ out, u64 limit, u64* __restrict__ cursor) {
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap || state[s] == 0ull) return;
    const u64 at = atomicAdd((unsigned long long*)cursor, 1ull);
    if (at >= limit) return;
    ((u32x4*)(out + 32 * at))[0] = ((const u32x4*)(slots + 32 * s))[0];
    ((u32x4*)(out + 32 * at))[1] = ((const u32x4*)(slots + 32 * s))[1];
}

// ---- query / prune / retain ---------------------------------------------------------------------------------------------------
enum : int { kTotUnknown = 0, kTotFound = 1, kTotSurvive = 2, kTotDropped = 3, kTotCursor = 4, kTotExport = 5, kTotZsetBad = 6 };

// held[r] = 1 if the table holds row r's digest (held may be nullptr); mark[slot] = 1 at the slot that holds it (mark may be
// nullptr); totals[kTotFound] / [kTotUnknown] += the rows found / not found.  No thread writes the table during the launch.
__global__ __launch_bounds__(256)
void index_lookup_kernel(const u8* __restrict__ digests, u64 n, const u64* __restrict__ tags, const u8* __restrict__ slots,
                         u64 mask, u8* __restrict__ held, u8* __restrict__ mark, u64* __restrict__ totals) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < n;
    bool found = false;
    if (in) {
        const u8* d = digests + 32 * r;
        const u64 tag = tag_of(*(const u64*)d);
        u64 slot = tag & mask;
        for (u64 walked = 0; walked <= mask; ++walked) {     // (the table is at most half full: an empty slot ends every walk)
            const u64 t = tags[slot];
            if (t == 0ull) break;
            if (t == tag && digest_eq32(slots + 32 * slot, d)) {
                if (mark) mark[slot] = 1;                    // (rows that repeat a digest store the same byte)
                found = true;
                break;
            }
            slot = (slot + 1) & mask;
        }
        if (held) held[r] = found ? 1 : 0;
    }
    const u64 hits = (u64)__popcll(__ballot(found)), misses = (u64)__popcll(__ballot(in && !found));
    if ((threadIdx.x & 63) == 0) {
        if (hits) atomicAdd((unsigned long long*)&totals[kTotFound], (unsigned long long)hits);
        if (misses) atomicAdd((unsigned long long*)&totals[kTotUnknown], (unsigned long long)misses);
    }
}

// item s of [0, n) -- a slot of a table (state given: an empty slot is no item) or a row of a record array (state == nullptr) --
// survives when (mark[s] != 0) == (keep != 0).  The survivors' digests are appended to out[0, limit); *cursor counts them all,
// so the host sees more survivors than `limit` without a write past the buffer (limit 0: a count and nothing else);
// *dropped (may be nullptr) += the items that do not survive
__global__ __launch_bounds__(256)
void index_sweep_kernel(const u64* __restrict__ state, const u8* __restrict__ digests, u64 n, const u8* __restrict__ mark,
                        u32 keep, u8* __restrict__ out, u64 limit, u64* __restrict__ cursor, u64* __restrict__ dropped) {
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool item = s < n && (!state || state[s] != 0ull);
    const bool stays = item && ((mark[s] != 0) == (keep != 0));
    const u64 stay_lanes = __ballot(stays);
    const u64 goes = (u64)__popcll(__ballot(item && !stays));
    u64 base = 0;
    if (lane == 0) {
        if (stay_lanes) base = atomicAdd((unsigned long long*)cursor, (unsigned long long)__popcll(stay_lanes));
        if (goes && dropped) atomicAdd((unsigned long long*)dropped, (unsigned long long)goes);
    }
    const u32 lo = __shfl((u32)base, 0), hi = __shfl((u32)(base >> 32), 0);
    if (!stays) return;
    const u64 at = (((u64)hi << 32) | lo) + (u64)__popcll(stay_lanes & ((1ull << lane) - 1ull));
    if (at >= limit) return;
    ((u32x4*)(out + 32 * at))[0] = ((const u32x4*)(digests + 32 * s))[0];
    ((u32x4*)(out + 32 * at))[1] = ((const u32x4*)(digests + 32 * s))[1];
}

// retain: flags[r] = 1 if the set's lookup found row r (src[r]: where the set holds it, 0: it does not)
__global__ __launch_bounds__(256)
void index_held_flags_kernel(const u64* __restrict__ src, u64 n, u8* __restrict__ flags) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r < n) flags[r] = src[r] != 0ull ? 1 : 0;
}

}  // namespace

struct mi_index {
    mi_ctx* ctx;
    DevBuf state, slots, counter, scratch, dup, row_state, row_slot;
    u64 cap = 0;           // slots, power of two
    u64 count = 0;         // digests held
};

namespace {

int index_alloc(mi_index* x, u64 cap) {
    mi_ctx* c = x->ctx;
    HIPCHK(c, x->state.ensure(cap * 8));
    HIPCHK(c, x->slots.ensure(cap * 32));
    HIPCHK(c, x->counter.ensure(16));
    HIPCHK(c, hipMemsetAsync(x->state.p, 0, cap * 8, c->stream));
    x->cap = cap;
    return MI_OK;
}

// inserts n device-resident digests (rows filtered by dup_of when given); grows first if needed
int index_insert(mi_index* x, const u8* d_digests, const i64* d_dup_of, u64 n, u8* d_known, u64* n_new);

int index_grow(mi_index* x, u64 min_cap) {
    mi_ctx* c = x->ctx;
    u64 cap = x->cap ? x->cap : 1024;
    while (cap < min_cap) cap <<= 1;
    if (cap == x->cap) return MI_OK;
    // export the current content, reallocate, re-insert
    DevBuf old;
    const u64 have = x->count;
    if (have) {
        HIPCHK(c, old.ensure(have * 32));
        HIPCHK(c, hipMemsetAsync(x->counter.p, 0, 8, c->stream));
        hipLaunchKernelGGL(index_export_kernel, dim3((u32)((x->cap + 255) / 256)), dim3(256), 0, c->stream,
                           x->state.as<u64>(), x->slots.as<u8>(), x->cap, old.as<u8>(), have, x->counter.as<u64>());
        HIPCHK(c, hipMemcpyAsync(c->h_word.p, x->counter.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->h_word.as<u64>()[0] != have)                           // the table is left as it was
            return fail(c, MI_ERR_STATE, "chunk index holds %llu digests, counted %llu",
                        (unsigned long long)c->h_word.as<u64>()[0], (unsigned long long)have);
    }
    x->state.release();
    x->slots.release();
    int rc = index_alloc(x, cap);
    if (rc) { x->cap = 0; x->count = 0; return rc; }     // out of memory: an empty, still usable index
    x->count = 0;
    if (have) {
        u64 n_new = 0;
        rc = index_insert(x, old.as<u8>(), nullptr, have, nullptr, &n_new);
        if (rc) return rc;
        if (n_new != have) return fail(c, MI_ERR_HIP, "index rebuild lost entries (%llu of %llu)",
                                       (unsigned long long)n_new, (unsigned long long)have);
    }
    return MI_OK;
}

int index_insert(mi_index* x, const u8* d_digests, const i64* d_dup_of, u64 n, u8* d_known, u64* n_new) {
    mi_ctx* c = x->ctx;
    *n_new = 0;
    if (n == 0) return MI_OK;
    if ((x->count + n) * 2 > x->cap) {                      // keep the load factor under 1/2
        int rc = index_grow(x, (x->count + n) * 2);
        if (rc) return rc;
    }
    HIPCHK(c, x->row_state.ensure(n + 16));
    HIPCHK(c, x->row_slot.ensure(n * 8 + 16));
    HIPCHK(c, hipMemsetAsync(x->counter.p, 0, 16, c->stream));   // [0] inserted, [1] rows to re-probe
    const u32 per_row = (u32)((n + 255) / 256);
    const u32 grid = per_row < 2048u ? per_row : 2048u;
    u64* d_cnt = x->counter.as<u64>();
    hipLaunchKernelGGL(index_begin_kernel, dim3(per_row), dim3(256), 0, c->stream, d_digests, d_dup_of, n,
                       x->cap - 1, x->row_state.as<u8>(), x->row_slot.as<u64>());
    // from here on the table holds every row placed so far: each return adds them (counter[0] as
    // last read) to x->count
    u64 added = 0;
    int rc = MI_OK;
    hipError_t e = hipSuccess;
    for (u64 round = 0;; ++round) {
        hipLaunchKernelGGL(index_probe_kernel, dim3(grid), dim3(256), 0, c->stream, d_digests, n,
                           x->state.as<u64>(), x->slots.as<u8>(), x->cap - 1, x->row_state.as<u8>(),
                           x->row_slot.as<u64>(), d_known, d_cnt);
        hipLaunchKernelGGL(index_verify_kernel, dim3(per_row), dim3(256), 0, c->stream, d_digests, n,
                           x->slots.as<u8>(), x->cap - 1, x->row_state.as<u8>(), x->row_slot.as<u64>(),
                           d_known, d_cnt + 1);
        e = hipMemcpyAsync(c->h_word.p, x->counter.p, 16, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) break;
        added = c->h_word.as<u64>()[0];
        if (c->h_word.as<u64>()[1] == 0) break;                       // no 64-bit tag collisions (the normal case)
        if (round >= x->cap) { rc = fail(c, MI_ERR_HIP, "chunk index: probing does not converge"); break; }
        e = hipMemsetAsync(d_cnt + 1, 0, 8, c->stream);
        if (e != hipSuccess) break;
    }
    if (!rc && e == hipSuccess && d_dup_of && d_known) {
        hipLaunchKernelGGL(index_inherit_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, c->stream,
                           d_dup_of, n, d_known);
        e = hipStreamSynchronize(c->stream);
    }
    if (!rc && e == hipSuccess) e = hipGetLastError();
    if (!rc && e != hipSuccess)
        rc = fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "chunk index insert: %s", hipGetErrorString(e));
    x->count += added;
    *n_new = added;
    return rc;
}

// ---- query / prune / retain: the host side ------------------------------------------------------------------------------------
int does_not_fit(mi_ctx* c, const char* who, hipError_t e, const char* what, u64 bytes) {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: %s of %llu bytes does not fit: the device has %llu bytes free (%s)",
                who, what, (unsigned long long)bytes, (unsigned long long)free_b, hipGetErrorString(e));
}

#define INDEX_ALLOC(buf, want, what)                                                      \
    do {                                                                                  \
        const hipError_t e_ = (buf).alloc_exact((want), &extra);                        \
        if (e_ != hipSuccess) return does_not_fit(c, who, e_, (what), (want));            \
    } while (0)

// held[r] for n digests on the device, by the table alone; *n_held = the rows held.  ONE synchronisation; the index is read only
int index_lookup_rows(mi_index* x, const u8* d_digests, u64 n, u8* held_out, u64* n_held) {
    mi_ctx* c = x->ctx;
    if (n_held) *n_held = 0;
    if (n == 0) return MI_OK;
    if (x->cap == 0) {                                       // (an index that lost its table to an allocation failure holds nothing)
        if (held_out) memset(held_out, 0, n);
        return MI_OK;
    }
    DevBuf d_held, d_tot;
    StreamDrain drain{c->stream};
    if (held_out) HIPCHK(c, d_held.ensure(n));
    HIPCHK(c, d_tot.ensure(64));
    HIPCHK(c, hipMemsetAsync(d_tot.p, 0, 64, c->stream));
    hipLaunchKernelGGL(index_lookup_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, c->stream, d_digests, n, x->state.as<u64>(),
                       x->slots.as<u8>(), x->cap - 1, held_out ? d_held.as<u8>() : (u8*)nullptr, (u8*)nullptr, d_tot.as<u64>());
    HIPCHK(c, hipMemcpyAsync(c->h_word.p, d_tot.p, 16, hipMemcpyDeviceToHost, c->stream));
    if (held_out) HIPCHK(c, hipMemcpyAsync(held_out, d_held.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    const u64* h = c->h_word.as<u64>();
    if (h[kTotFound] + h[kTotUnknown] != n)
        return fail(c, MI_ERR_HIP, "chunk index query: %llu rows answered of %llu", (unsigned long long)(h[kTotFound] + h[kTotUnknown]),
                    (unsigned long long)n);
    if (n_held) *n_held = h[kTotFound];
    return MI_OK;
}

// The second half of a prune: sweep pass 1 counted n_survive survivors among the n_items items (state, digests, mark, keep: the
// sweep kernel's arguments) and something goes.  The survivors' records, a fresh table sized for them and the insert's scratch
// are allocated (*extra_io += their bytes, the call's peak), the records exported, the table built by index_insert in a second
// mi_index on the stack, its count and the export's cursor checked -- and only then the tables are swapped.  Whatever fails
// before, x is as it was.  Synchronisations: one a probing round of the insert (one round unless 64-bit tags collide; none for
// an empty survivor list, which takes one of its own)
int index_rebuild(mi_index* x, const char* who, const u64* state, const u8* digests, u64 n_items, const u8* mark, u32 keep,
                  u64 n_survive, u64* d_tot, u64* extra_io, mi_index_prune_info* pi) {
    mi_ctx* c = x->ctx;
    hipStream_t st = c->stream;
    u64 extra = *extra_io;
    u64 new_cap = 1024;
    while (new_cap < 2 * n_survive) new_cap <<= 1;
    mi_index fresh;
    fresh.ctx = c;
    DevBuf d_recs;
    Event ev[2];
    StreamDrain drain{st};
    for (auto& e : ev) HIPCHK(c, e.create());
    INDEX_ALLOC(fresh.state, new_cap * 8, "the new table's tags");
    INDEX_ALLOC(fresh.slots, new_cap * 32, "the new table's digests");
    INDEX_ALLOC(d_recs, n_survive * 32, "the survivors' records");
    INDEX_ALLOC(fresh.row_state, n_survive + 16, "the insert's row states");
    INDEX_ALLOC(fresh.row_slot, n_survive * 8 + 16, "the insert's row slots");
    INDEX_ALLOC(fresh.counter, 64, "the insert's counters");
    *extra_io = extra;
    u64* h = c->h_word.as<u64>();
    HIPCHK(c, hipEventRecord(ev[0], st));
    int rc = index_alloc(&fresh, new_cap);                    // (all three are large enough: only the tags' memset is enqueued)
    if (rc) return rc;
    if (n_survive) {
        hipLaunchKernelGGL(index_sweep_kernel, dim3((u32)((n_items + 255) / 256)), dim3(256), 0, st, state, digests, n_items, mark, keep,
                           d_recs.as<u8>(), n_survive, d_tot + kTotCursor, (u64*)nullptr);
        HIPCHK(c, hipMemcpyAsync(h + 2, d_tot + kTotCursor, 8, hipMemcpyDeviceToHost, st));   // (lands with the insert's first round)
        u64 n_new = 0;
        rc = index_insert(&fresh, d_recs.as<u8>(), nullptr, n_survive, nullptr, &n_new);
        if (rc) return rc;
        if (h[2] != n_survive || n_new != n_survive)
            return fail(c, MI_ERR_HIP, "%s: %llu records exported, %llu inserted, %llu survive", who, (unsigned long long)h[2],
                        (unsigned long long)n_new, (unsigned long long)n_survive);
    } else {
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(ev[1], st));
    HIPCHK(c, hipEventSynchronize(ev[1]));                    // (the stream is idle: this waits for the event alone)
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    pi->ms_rebuild = ms;
    // ---- the index changes: nothing below can fail; the old table goes with `fresh` ----------------------------------------------
    std::swap(x->state, fresh.state);
    std::swap(x->slots, fresh.slots);
    x->cap = new_cap;
    x->count = n_survive;
    pi->rebuilt = 1;
    pi->n_after = n_survive;
    pi->slots_after = new_cap;
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_index_create(mi_ctx* c, uint64_t capacity_hint, mi_index** out) {
    if (!c || !out) return MI_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    mi_index* x = new mi_index();
    x->ctx = c;
    ++c->live_children;                                 // mi_index_free undoes it
    u64 cap = 1024;
    while (cap < 2 * capacity_hint) cap <<= 1;
    int rc = index_alloc(x, cap);
    if (rc) { mi_index_free(x); return rc; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = x;
    return MI_OK;
}

void mi_index_free(mi_index* x) {
    if (!x) return;
    (void)hipSetDevice(x->ctx->device);
    (void)hipStreamSynchronize(x->ctx->stream);
    --x->ctx->live_children;
    delete x;
}

int mi_index_count(mi_index* x, uint64_t* n) {
    if (!x || !n) return MI_ERR_INVALID;
    *n = x->count;
    return MI_OK;
}

int mi_index_add_batch(mi_index* x, mi_batch* b, uint8_t* known_out, uint64_t cap, uint64_t* n_new,
                       uint64_t* n_known) {
    if (!x || !b || b->ctx != x->ctx) return MI_ERR_INVALID;
    mi_ctx* c = x->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if (!b->ran || b->in_flight) return fail(c, MI_ERR_STATE, "the batch must have run (and been waited for)");
    const u64 n = b->n_chunks;
    if (known_out && cap < n) return fail(c, MI_ERR_CAPACITY, "known buffer holds %llu rows, need %llu",
                                          (unsigned long long)cap, (unsigned long long)n);
    HIPCHK(c, x->scratch.ensure(n + 16));
    HIPCHK(c, x->dup.ensure(n * 8 + 16));
    // a fresh in-batch marking: the batch's own dup_of may be absent (MI_FLAG_NO_DEDUP) or hold
    // job-wide indices (mi_batch_set_global_dedup)
    u64 added = 0, uniq = 0;
    int rc = n ? mi_dedup_mark(c, b->digests.p, n, x->dup.p, &uniq) : MI_OK;
    if (rc) return rc;
    rc = index_insert(x, b->digests.as<u8>(), x->dup.as<i64>(), n, x->scratch.as<u8>(), &added);
    if (rc) return rc;
    std::vector<u8> known(n);
    if (n) HIPCHK(c, hipMemcpy(known.data(), x->scratch.p, n, hipMemcpyDeviceToHost));
    u64 nk = 0;
    for (u8 k : known) nk += k;
    if (known_out && n) memcpy(known_out, known.data(), n);
    if (n_new) *n_new = added;
    if (n_known) *n_known = nk;
    return MI_OK;
}

// mi_index_add_batch for digests that lie in HOST memory -- a batch that ran on another GPU than the index's (the commit over
// several ctxs feeds one index: 32 bytes per chunk cross the host, 0.4 % of the data).  known_out: n flags.  (hidden: mi_local.h)
int mi_index_add_digests(mi_index* x, const void* digests, uint64_t n, uint8_t* known_out, uint64_t* n_new, uint64_t* n_known) {
    if (!x || (!digests && n)) return MI_ERR_INVALID;
    mi_ctx* c = x->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if (n_new) *n_new = 0;
    if (n_known) *n_known = 0;
    if (n == 0) return MI_OK;
    DevBuf d;
    HIPCHK(c, d.ensure(n * 32));
    HIPCHK(c, x->scratch.ensure(n + 16));
    HIPCHK(c, x->dup.ensure(n * 8 + 16));
    HIPCHK(c, hipMemcpy(d.p, digests, n * 32, hipMemcpyHostToDevice));
    u64 added = 0, uniq = 0;
    int rc = mi_dedup_mark(c, d.p, n, x->dup.p, &uniq);
    if (!rc) rc = index_insert(x, d.as<u8>(), x->dup.as<i64>(), n, x->scratch.as<u8>(), &added);
    if (rc) return rc;
    std::vector<u8> known(n);
    HIPCHK(c, hipMemcpy(known.data(), x->scratch.p, n, hipMemcpyDeviceToHost));
    u64 nk = 0;
    for (u8 k : known) nk += k;
    if (known_out) memcpy(known_out, known.data(), n);
    if (n_new) *n_new = added;
    if (n_known) *n_known = nk;
    return MI_OK;
}

int mi_index_same_ctx(mi_index* x, mi_batch* b) { return x && b && b->ctx == x->ctx ? 1 : 0; }
mi_ctx* mi_index_ctx(mi_index* x) { return x ? x->ctx : nullptr; }

int mi_index_export(mi_index* x, void* out, uint64_t cap_digests) {
    if (!x || (!out && cap_digests)) return MI_ERR_INVALID;
    mi_ctx* c = x->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if (cap_digests < x->count) return fail(c, MI_ERR_CAPACITY, "export buffer holds %llu digests, need %llu",
                                            (unsigned long long)cap_digests, (unsigned long long)x->count);
    if (x->count == 0) return MI_OK;
    DevBuf tmp;
    HIPCHK(c, tmp.ensure(x->count * 32));
    HIPCHK(c, hipMemsetAsync(x->counter.p, 0, 8, c->stream));
    hipLaunchKernelGGL(index_export_kernel, dim3((u32)((x->cap + 255) / 256)), dim3(256), 0, c->stream,
                       x->state.as<u64>(), x->slots.as<u8>(), x->cap, tmp.as<u8>(), x->count, x->counter.as<u64>());
    hipError_t e = hipMemcpyAsync(c->h_word.p, x->counter.p, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp.p, x->count * 32, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, MI_ERR_HIP, "mi_index_export: %s", hipGetErrorString(e));
    if (c->h_word.as<u64>()[0] != x->count)
        return fail(c, MI_ERR_STATE, "mi_index_export: the index holds %llu digests, counted %llu",
                    (unsigned long long)c->h_word.as<u64>()[0], (unsigned long long)x->count);
    return MI_OK;
}

int mi_index_import(mi_index* x, const void* digests, uint64_t n, uint64_t* n_new) {
    if (!x || (!digests && n)) return MI_ERR_INVALID;
    mi_ctx* c = x->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if (n_new) *n_new = 0;
    if (n == 0) return MI_OK;
    // imported digests may repeat each other or the table's content: mark them first so only
    // unique rows probe (the kernel's no-equal-probers precondition)
    DevBuf d, dup;
    HIPCHK(c, d.ensure(n * 32));
    HIPCHK(c, dup.ensure(n * 8));
    HIPCHK(c, hipMemcpy(d.p, digests, n * 32, hipMemcpyHostToDevice));
    uint64_t uniq = 0;
    int rc = mi_dedup_mark(c, d.p, n, dup.p, &uniq);
    u64 added = 0;
    if (!rc) rc = index_insert(x, d.as<u8>(), dup.as<i64>(), n, nullptr, &added);
    if (!rc && n_new) *n_new = added;
    return rc;
}

// ---- asking without adding ----------------------------------------------------------------------------------------------------
int mi_index_query(mi_index* x, const uint8_t* digests, uint64_t n, uint8_t* held, uint64_t* n_held) {
    if (n_held) *n_held = 0;
    if (!x || (n && !digests)) return MI_ERR_INVALID;
    mi_ctx* c = x->ctx;
    if (n >> 32) return fail(c, MI_ERR_INVALID, "mi_index_query: %llu rows, a request holds fewer than 2^32", (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0) return MI_OK;
    DevBuf d;                                                // (index_lookup_rows leaves the stream idle)
    HIPCHK(c, d.ensure(n * 32));
    HIPCHK(c, hipMemcpyAsync(d.p, digests, n * 32, hipMemcpyHostToDevice, c->stream));
    return index_lookup_rows(x, d.as<u8>(), n, held, n_held);
}

int mi_index_query_batch(mi_index* x, mi_batch* b, uint8_t* held, uint64_t cap, uint64_t* n_held) {
    if (n_held) *n_held = 0;
    if (!x || !b || b->ctx != x->ctx) return MI_ERR_INVALID;
    mi_ctx* c = x->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if (!b->ran || b->in_flight) return fail(c, MI_ERR_STATE, "the batch must have run (and been waited for)");
    const u64 n = b->n_chunks;
    if (held && cap < n) return fail(c, MI_ERR_CAPACITY, "held buffer holds %llu rows, need %llu", (unsigned long long)cap,
                                     (unsigned long long)n);
    return index_lookup_rows(x, b->digests.as<u8>(), n, held, n_held);
}

// ---- forgetting ------------------------------------------------------------------------------------------------------------------
int mi_index_prune(mi_index* x, const uint8_t* digests, uint64_t n, uint32_t flags, mi_index_prune_info* info) {
    if (info) memset(info, 0, sizeof *info);
    if (!x || (n && !digests)) return MI_ERR_INVALID;
    static const char* who = "mi_index_prune";
    mi_ctx* c = x->ctx;
    if (flags != MI_INDEX_PRUNE_KEEP && flags != MI_INDEX_PRUNE_DROP)
        return fail(c, MI_ERR_INVALID, "%s: flags %#x: exactly one of MI_INDEX_PRUNE_KEEP and MI_INDEX_PRUNE_DROP", who, flags);
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu rows, a request holds fewer than 2^32", who, (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const u64 cap = x->cap;
    const u32 keep = flags == MI_INDEX_PRUNE_KEEP ? 1u : 0u;
    mi_index_prune_info pi = {};
    pi.n_rows = n;
    pi.n_before = pi.n_after = x->count;
    pi.slots_before = pi.slots_after = cap;
    if (cap == 0) {                                          // (no table, nothing held: every row is unknown, nothing goes)
        pi.n_unknown = n;
        if (info) *info = pi;
        return MI_OK;
    }
    u64 extra = 0;                                           // what this call allocates, from the sizes
    DevBuf d_dig, d_mark, d_tot;
    Event ev[2];
    StreamDrain drain{st};
    for (auto& e : ev) HIPCHK(c, e.create());
    // ---- mark, count; synchronisation 1 -------------------------------------------------------------------------------------
    INDEX_ALLOC(d_dig, n * 32, "the request");
    INDEX_ALLOC(d_mark, cap, "the mark array");
    INDEX_ALLOC(d_tot, 64, "the totals");
    u64* tot = d_tot.as<u64>();
    u64* h = c->h_word.as<u64>();
    HIPCHK(c, hipEventRecord(ev[0], st));
    if (n) HIPCHK(c, hipMemcpyAsync(d_dig.p, digests, n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_mark.p, 0, cap, st));
    HIPCHK(c, hipMemsetAsync(tot, 0, 64, st));
    if (n)
        hipLaunchKernelGGL(index_lookup_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_dig.as<u8>(), n, x->state.as<u64>(),
                           x->slots.as<u8>(), cap - 1, (u8*)nullptr, d_mark.as<u8>(), tot);
    hipLaunchKernelGGL(index_sweep_kernel, dim3((u32)((cap + 255) / 256)), dim3(256), 0, st, x->state.as<u64>(), x->slots.as<u8>(), cap,
                       d_mark.as<u8>(), keep, (u8*)nullptr, (u64)0, tot + kTotSurvive, tot + kTotDropped);
    HIPCHK(c, hipEventRecord(ev[1], st));
    HIPCHK(c, hipMemcpyAsync(h, tot, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    pi.ms_mark = ms;
    pi.n_unknown = h[kTotUnknown];
    const u64 n_survive = h[kTotSurvive];
    pi.n_dropped = h[kTotDropped];
    pi.peak_extra_bytes = extra;
    if (n_survive + pi.n_dropped != x->count || h[kTotFound] + h[kTotUnknown] != n)
        return fail(c, MI_ERR_STATE, "%s: the index holds %llu digests, the sweep counted %llu that stay and %llu that go", who,
                    (unsigned long long)x->count, (unsigned long long)n_survive, (unsigned long long)pi.n_dropped);
    if (pi.n_dropped == 0) {                                 // nothing to drop: the table is untouched
        if (info) *info = pi;
        return MI_OK;
    }
    const int rc = index_rebuild(x, who, x->state.as<u64>(), x->slots.as<u8>(), cap, d_mark.as<u8>(), keep, n_survive, tot, &extra, &pi);
    if (rc) return rc;
    pi.peak_extra_bytes = extra;
    if (info) *info = pi;
    return MI_OK;
}

int mi_index_retain_zset(mi_index* x, const mi_zset* set, mi_index_prune_info* info) {
    if (info) memset(info, 0, sizeof *info);
    if (!x || !set) return MI_ERR_INVALID;
    static const char* who = "mi_index_retain_zset";
    mi_ctx* c = x->ctx;
    mi_ctx* set_ctx = nullptr;
    int rc = mi_zset_ctx(set, who, &set_ctx);                // MI_ERR_STATE with the first message for a set in its failed state
    if (set_ctx != c) return fail(c, MI_ERR_INVALID, "%s: the index and the set belong to different contexts", who);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const u64 count = x->count;
    mi_index_prune_info pi = {};
    pi.n_before = pi.n_after = count;
    pi.slots_before = pi.slots_after = x->cap;
    if (count == 0) {                                        // nothing held, nothing to ask the set
        if (info) *info = pi;
        return MI_OK;
    }
    u64 extra = 0;
    DevBuf d_exp, d_src, d_word, d_len64, d_flags, d_tot;
    Event ev[2];
    StreamDrain drain{st};
    for (auto& e : ev) HIPCHK(c, e.create());
    // ---- export, the set's lookup, the flags, count; synchronisation 1 ----------------------------------------------------------
    INDEX_ALLOC(d_exp, count * 32, "the exported digests");
    INDEX_ALLOC(d_src, count * 8, "the lookup's addresses");
    INDEX_ALLOC(d_word, count * 8, "the lookup's words");
    INDEX_ALLOC(d_len64, count * 8, "the lookup's lengths");
    INDEX_ALLOC(d_flags, count, "the keep flags");
    INDEX_ALLOC(d_tot, 64, "the totals");
    u64* tot = d_tot.as<u64>();
    u64* h = c->h_word.as<u64>();
    const u32 row_blocks = (u32)((count + 255) / 256);
    HIPCHK(c, hipEventRecord(ev[0], st));
    HIPCHK(c, hipMemsetAsync(tot, 0, 64, st));
    hipLaunchKernelGGL(index_export_kernel, dim3((u32)((x->cap + 255) / 256)), dim3(256), 0, st, x->state.as<u64>(), x->slots.as<u8>(),
                       x->cap, d_exp.as<u8>(), count, tot + kTotExport);
    rc = mi_zset_lookup_enqueue(set, d_exp.as<u8>(), nullptr, count, d_src.as<u64>(), d_word.as<u64>(), d_len64.as<u64>(), tot + kTotZsetBad);
    if (rc) return fail(c, rc, "%s: the set's lookup was refused", who);
    hipLaunchKernelGGL(index_held_flags_kernel, dim3(row_blocks), dim3(256), 0, st, d_src.as<u64>(), count, d_flags.as<u8>());
    hipLaunchKernelGGL(index_sweep_kernel, dim3(row_blocks), dim3(256), 0, st, (const u64*)nullptr, d_exp.as<u8>(), count, d_flags.as<u8>(),
                       1u, (u8*)nullptr, (u64)0, tot + kTotSurvive, tot + kTotDropped);
    HIPCHK(c, hipEventRecord(ev[1], st));
    HIPCHK(c, hipMemcpyAsync(h, tot, 48, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    pi.ms_mark = ms;
    const u64 n_survive = h[kTotSurvive];
    pi.n_dropped = h[kTotDropped];
    pi.peak_extra_bytes = extra;
    if (h[kTotExport] != count || n_survive + pi.n_dropped != count)
        return fail(c, MI_ERR_STATE, "%s: the index holds %llu digests, the export counted %llu, the sweep %llu that stay and %llu that go",
                    who, (unsigned long long)count, (unsigned long long)h[kTotExport], (unsigned long long)n_survive,
                    (unsigned long long)pi.n_dropped);
    if (pi.n_dropped == 0) {
        if (info) *info = pi;
        return MI_OK;
    }
    rc = index_rebuild(x, who, nullptr, d_exp.as<u8>(), count, d_flags.as<u8>(), 1u, n_survive, tot, &extra, &pi);
    if (rc) return rc;
    pi.peak_extra_bytes = extra;
    if (info) *info = pi;
    return MI_OK;
}

}  // extern "C"
