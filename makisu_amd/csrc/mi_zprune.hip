// mi_zprune.hip -- a compressed pack set (mi_zset.hip) PRUNED IN PLACE: digests are dropped from the table, blobs that hold
// nothing live go back to the device, the survivors of mostly-dead blobs are moved together into one new blob, and nothing else
// is touched (mi_zset_prune); and what is resident (mi_zset_get_usage).  For the digests still held the set answers every call
// as before: the stored form, the length | stored word and which form is held never change, only a moved span's address.
//
//   mark      one thread a request row: slot_table_find's walk (the tag first, then all 32 bytes); the slot found gets a
//             byte in a per-slot mark array, misses are counted (one atomic a wave);
//   sweep     over the slots, grid-stride: survivor or victim by mark and mode.  A survivor's blob is found by binary search
//             of its span address in the sorted blob bases and remembered per slot; per-blob live bytes (round16(stored)) go
//             through per-workgroup bins in LDS (the first 256 blobs; beyond: global atomics) and the totals (survivors,
//             dropped digests, their stored and chunk bytes) through a workgroup sum -- one global atomic a workgroup and value.
//             Synchronisation 1: the per-blob sums.  The host classifies: dead (no live bytes), sparse (under the threshold);
//   plan      over the slots whose blob is sparse: mi_plan.h's three launches over round16(stored): where each span goes in the
//             new blob, and the list of (source address, bytes, destination, slot) in slot order.  Synchronisation 2: the
//             totals, before the blob is allocated;
//   move      zset_gather_kernel's form WITHOUT the masking: destination-driven, 16 KiB tiles, one wave searching the entries'
//             offsets, every lane's units loaded before the first is stored.  Whole units, the pad as it was;
//   repoint   the moved spans' new addresses into a per-slot array: THE OLD TABLE IS NEVER WRITTEN;
//   rebuild   the survivors' records, with the repointed addresses, exported into a record array and inserted into a fresh
//             table sized for them -- a SlotTable of this call's (mi_slot_table.h: one synchronisation a probing round: one, unless
//             64-bit tags collide).  Open addressing with linear probing cannot delete in place; a rebuild is the simple
//             correct form, and it shrinks the table.  Synchronisation 3 behind it; then the table is swapped, the dead and
//             the compacted blobs are freed and the new blob joins the set.
//
// Everything is allocated before anything changes, by DevBuf::alloc_exact (the bytes rounded up to 256, plus 256), and the old
// table and blobs go only when the new table is complete: whatever fails, the set is as it was.  Offsets and addresses are 64-bit.
// The host's side is mi::ZsetSweep (mi_zset_local.h): begin(), the caller's mark, finish() -- mi_zset_prune marks by a list,
// mi_zset_expire (mi_zage.hip) by age; an ageing set's stamps follow the survivors into the new table.
//
// BOUNDS.  mark READS digests [0, 32 n), tags / slots [0, cap) (the walk is masked), WRITES mark [0, cap).  sweep READS tags,
// slots, mark [0, cap) and bases [0, n_blobs), WRITES slot_blob [0, cap), live [0, n_blobs) -- the index comes from the search,
// which stays in [0, n_blobs) -- and five totals.  The plan READS slot_blob, slots [0, cap), cls at an index that sweep wrote
// (< n_blobs), WRITES block_cnt / block_bytes [0, n_blocks) and the lists at [0, n_move): the positions are the exclusive scan
// of the same predicate the totals counted.  The move READS aligned 16-byte units inside [src, src + round16(stored)) -- inside
// the source blob by the structural check of every add (offset + round16(stored) <= blob_bytes), to its last byte when the span
// ends on the blob's last unit -- and WRITES aligned units inside [0, moved_bytes) of the new blob.  repoint WRITES new_addr at
// slots the plan listed (< cap).  export READS slot_blob, slots, new_addr [0, cap), WRITES records [0, limit) (the cursor is checked).
#include "mi_plan.h"
#include "mi_zset_local.h"

using namespace mi;

namespace mi {

constexpr u64 kPNone = ~0ull;
constexpr u32 kPNoBlob = 0xFFFFFFFFu;                 // slot_blob: an empty slot, or a victim
enum : u8 { kPStay = 0, kPCompact = 1, kPDead = 2 };  // a blob's fate
enum : int { kPTotUnknown = 0, kPTotSurvive = 1, kPTotDropped = 2, kPTotDropStored = 3, kPTotDropChunk = 4, kPTotCursor = 6 };

constexpr int kPWG    = 256;                          // the workgroup of the sweep, the move and the usage kernel
constexpr int kPBins  = 256;                          // blobs with a bin in LDS

// ---- mark ---------------------------------------------------------------------------------------------------------------------
// mark[slot] = 1 for the slot that holds row r's digest; totals[kPTotUnknown] += rows whose digest the set does not hold
__global__ __launch_bounds__(256)
void zprune_mark_kernel(const u8* __restrict__ digests, u64 n, const u64* __restrict__ tags, const u64* __restrict__ slots, u64 mask,
                        u8* __restrict__ mark, u64* __restrict__ totals) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    bool miss = false;
    if (r < n) {
        const u64 slot = slot_table_find(tags, slots, mask, digests + 32 * r);
        miss = slot == kSlotNone;
        if (!miss) mark[slot] = 1;                             // (rows that repeat a digest store the same byte)
    }
    const u64 misses = (u64)__popcll(__ballot(miss));
    if ((threadIdx.x & 63) == 0 && misses) atomicAdd((unsigned long long*)&totals[kPTotUnknown], (unsigned long long)misses);
}

// ---- sweep --------------------------------------------------------------------------------------------------------------------
// slot_blob[s] = the blob (its place among the sorted bases) a SURVIVING slot points into, kPNoBlob for an empty slot and for a
// victim; live[b] += round16(stored) of the survivors; the totals: survivors, victims, the victims' stored and chunk bytes
__global__ __launch_bounds__(kPWG)
void zprune_sweep_kernel(const u64* __restrict__ tags, const u64* __restrict__ slots, u64 cap, const u8* __restrict__ mark, u32 keep,
                         const u64* __restrict__ bases, u32 n_blobs, u32* __restrict__ slot_blob, u64* __restrict__ live,
                         u64* __restrict__ totals) {
    __shared__ unsigned long long bins[kPBins];
    __shared__ u64 lds[4][kPWG / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < kPBins; i += kPWG) bins[i] = 0;
    __syncthreads();
    u64 v[4] = {0, 0, 0, 0};                          // survivors, victims, the victims' stored bytes, their chunk bytes
    for (u64 s = (u64)blockIdx.x * kPWG + threadIdx.x; s < cap; s += (u64)gridDim.x * kPWG) {
        u32 b = kPNoBlob;
        if (tags[s] != 0ull) {
            const u64 word = slots[kSlotWords * s + 5];
            const u64 len = word & 0xFFFFFFFFull, stored = word >> 32;
            const bool survives = (mark[s] != 0) == (keep != 0);
            if (survives && n_blobs) {
                const u64 addr = slots[kSlotWords * s + 4];
                u32 lo = 0, hi = n_blobs;             // the last base at or below the span's address
                while (hi - lo > 1) {
                    const u32 mid = lo + ((hi - lo) >> 1);
                    if (bases[mid] <= addr) lo = mid; else hi = mid;
                }
                b = lo;
                ++v[0];
                if (b < (u32)kPBins) atomicAdd(&bins[b], (unsigned long long)round16(stored));
                else atomicAdd((unsigned long long*)&live[b], (unsigned long long)round16(stored));
            } else {
                ++v[1];
                v[2] += stored;
                v[3] += len;
            }
        }
        slot_blob[s] = b;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q] = wave_sum(v[q]);
        if (lane == 0) lds[q][wave] = v[q];
    }
    __syncthreads();
    const u32 n_bins = n_blobs < (u32)kPBins ? n_blobs : (u32)kPBins;
    for (u32 i = threadIdx.x; i < n_bins; i += kPWG)
        if (bins[i]) atomicAdd((unsigned long long*)&live[i], bins[i]);
    if (threadIdx.x < 4) {
        u64 t = 0;
#pragma unroll
        for (int w = 0; w < kPWG / 64; ++w) t += lds[threadIdx.x][w];
        if (t) atomicAdd((unsigned long long*)&totals[kPTotSurvive + threadIdx.x], (unsigned long long)t);
    }
}

// ---- plan: mi_plan.h's over round16(stored) of the survivors of the blobs to be compacted, a slot a row ------------------------
static __device__ __forceinline__ bool zprune_moves(const u32* __restrict__ slot_blob, const u8* __restrict__ cls, u64 s, u64 cap) {
    if (s >= cap) return false;
    const u32 b = slot_blob[s];
    return b != kPNoBlob && cls[b] == kPCompact;
}

__global__ __launch_bounds__(kPlanBlock)
void zprune_block_sums_kernel(const u32* __restrict__ slot_blob, const u8* __restrict__ cls, const u64* __restrict__ slots, u64 cap,
                              u64* __restrict__ block_cnt, u64* __restrict__ block_bytes) {
    __shared__ u64 lds[2][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[2] = {0, 0};                                // spans, their rounded-up stored bytes
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (!zprune_moves(slot_blob, cls, base + k, cap)) continue;
        ++v[0];
        v[1] += round16(slots[kSlotWords * (base + k) + 5] >> 32);
    }
    plan_block_sum<2>(v, lds);
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = v[0];
        block_bytes[blockIdx.x] = v[1];
    }
}

// single block: exclusive scan of both block arrays in place; totals[0] = the spans, totals[1] = the new blob's bytes
__global__ __launch_bounds__(kPlanBlock)
void zprune_block_offsets_kernel(u64* __restrict__ block_cnt, u64* __restrict__ block_bytes, u64 n_blocks, u64* __restrict__ totals) {
    plan_block_offsets<true>(block_cnt, block_bytes, n_blocks, &totals[0], &totals[1]);
}

// the move list, in slot order: where the span lies, its bytes (round16(stored): whole units), where it goes, whose it is
__global__ __launch_bounds__(kPlanBlock)
void zprune_compact_kernel(const u32* __restrict__ slot_blob, const u8* __restrict__ cls, const u64* __restrict__ slots, u64 cap,
                           const u64* __restrict__ block_cnt, const u64* __restrict__ block_bytes, u64* __restrict__ e_src,
                           u64* __restrict__ e_len, u64* __restrict__ e_dst, u64* __restrict__ e_slot) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 len[kPlanPer];
    u32 sel = 0;
    u64 cnt = 0, bytes = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const bool m = zprune_moves(slot_blob, cls, base + k, cap);
        len[k] = m ? round16(slots[kSlotWords * (base + k) + 5] >> 32) : 0;
        if (m) { sel |= 1u << k; ++cnt; bytes += len[k]; }
    }
    u64 at = plan_first(cnt, block_cnt);
    u64 dst = plan_first(bytes, block_bytes);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (!(sel & (1u << k))) continue;
        e_src[at] = slots[kSlotWords * (base + k) + 4];
        e_len[at] = len[k];
        e_dst[at] = dst;
        e_slot[at] = base + k;
        ++at;
        dst += len[k];
    }
}

// ---- move: the gather of mi_gather.h WITHOUT the masking, the lengths clamped to the tile: a kernel of its own ----------------
constexpr u32 kPGatherTile = 16384;                   // bytes of the blob a workgroup writes
constexpr u32 kPUnits = kPGatherTile / 16;            // ... in 16-byte units: a span takes at least one, so at most as many spans
constexpr int kPUnitsPer = kPUnits / kPWG;            // units per lane

__global__ __launch_bounds__(kPWG)
void zprune_gather_kernel(const u64* __restrict__ e_src, const u64* __restrict__ e_len, const u64* __restrict__ e_dst, u64 n_entries,
                          u64 blob_bytes, u8* __restrict__ blob) {
    __shared__ u64 s_src[kPUnits];
    __shared__ u32 s_rel[kPUnits];                   // where the span begins in the tile
    __shared__ u32 s_len[kPUnits];
    __shared__ u64 s_k[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 tile0 = (u64)blockIdx.x * kPGatherTile;
    const u64 tile1 = tile0 + kPGatherTile < blob_bytes ? tile0 + kPGatherTile : blob_bytes;
    if (wave < 2) {
        const u64 k = wave_last_le(e_dst, n_entries, wave == 0 ? tile0 : tile1 - 16, lane);
        if (lane == 0) s_k[wave] = k;
    }
    __syncthreads();
    const u64 k0 = s_k[0];
    const u64 reach = s_k[1] - k0 + 1;
    const u32 cnt = reach < kPUnits ? (u32)reach : kPUnits;
    for (u32 i = threadIdx.x; i < cnt; i += kPWG) {
        u64 src = e_src[k0 + i], len = e_len[k0 + i];
        const u64 dst = e_dst[k0 + i];
        u32 rel = (u32)(dst - tile0);
        if (dst < tile0) {                           // the first span may begin in front of the tile: the tile sees what is left
            const u64 skip = tile0 - dst;            // of it -- skip is a multiple of 16 below its bytes
            src += skip;
            len -= skip;
            rel = 0;
        }
        s_src[i] = src;
        s_len[i] = (u32)(len < kPGatherTile ? len : kPGatherTile);   // (what lies beyond the tile is another workgroup's)
        s_rel[i] = rel;
    }
    __syncthreads();
    u64 src[kPUnitsPer];
    bool have[kPUnitsPer];
#pragma unroll
    for (int j = 0; j < kPUnitsPer; ++j) {
        const u32 r = ((u32)threadIdx.x + (u32)j * kPWG) * 16;
        src[j] = s_src[0];                            // a unit behind the blob's end (the last tile) loads the tile's first unit and
        have[j] = false;                              // drops it: a lane's four loads are in flight together
        if (tile0 + r >= tile1) continue;
        u32 lo = 0, hi = cnt;                         // the span this unit lies in: the last that begins at or before it
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (s_rel[mid] <= r) lo = mid; else hi = mid;
        }
        const u32 o = r - s_rel[lo];
        if (o < s_len[lo]) {                          // (always: the spans tile the blob)
            src[j] = s_src[lo] + o;                   // a multiple of 16 behind an aligned address
            have[j] = true;
        }
    }
    u32x4 v[kPUnitsPer];
#pragma unroll
    for (int j = 0; j < kPUnitsPer; ++j) v[j] = load16_global(src[j]);
#pragma unroll
    for (int j = 0; j < kPUnitsPer; ++j) {
        const u32 r = ((u32)threadIdx.x + (u32)j * kPWG) * 16;
        if (have[j]) *(u32x4*)(blob + tile0 + r) = v[j];      // the whole unit, the pad as it was
    }
}

// ---- repoint, export ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void zprune_repoint_kernel(const u64* __restrict__ e_slot, const u64* __restrict__ e_dst, u64 n, u64 new_base, u64* __restrict__ new_addr) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k < n) new_addr[e_slot[k]] = new_base + e_dst[k];
}

// every surviving slot's record to out[0, limit), a moved span with its new address (new_addr: NULL, nothing moved; 0, not
// this one); the cursor counts them all
__global__ __launch_bounds__(256)
void zprune_export_kernel(const u32* __restrict__ slot_blob, const u64* __restrict__ slots, u64 cap, const u64* __restrict__ new_addr,
                          u64* __restrict__ out, u64 limit, u64* __restrict__ cursor) {
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= cap || slot_blob[s] == kPNoBlob) return;
    const u64 at = atomicAdd((unsigned long long*)cursor, 1ull);
    if (at >= limit) return;
    const u64 moved = new_addr ? new_addr[s] : 0ull;
#pragma unroll
    for (int w = 0; w < kSlotWords; ++w) out[kSlotWords * at + w] = w == 4 && moved ? moved : slots[kSlotWords * s + w];
}

// ---- usage: the sum of round16(stored) over the occupied slots --------------------------------------------------------------------
__global__ __launch_bounds__(kPWG)
void zprune_live_kernel(const u64* __restrict__ tags, const u64* __restrict__ slots, u64 cap, u64* __restrict__ total) {
    __shared__ u64 lds[kPWG / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 v = 0;
    for (u64 s = (u64)blockIdx.x * kPWG + threadIdx.x; s < cap; s += (u64)gridDim.x * kPWG)
        if (tags[s] != 0ull) v += round16(slots[kSlotWords * s + 5] >> 32);
    v = wave_sum(v);
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
#pragma unroll
        for (int w = 0; w < kPWG / 64; ++w) t += lds[w];
        if (t) atomicAdd((unsigned long long*)total, (unsigned long long)t);
    }
}

}  // namespace mi

namespace {

int does_not_fit(mi_ctx* c, const char* who, hipError_t e, const char* what, u64 bytes) {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: %s of %llu bytes does not fit: the device has %llu bytes free (%s)",
                who, what, (unsigned long long)bytes, (unsigned long long)free_b, hipGetErrorString(e));
}

#define PRUNE_ALLOC(buf, want, what)                                                      \
    do {                                                                                  \
        const hipError_t e_ = (buf).alloc_exact((want), &extra);                        \
        if (e_ != hipSuccess) return does_not_fit(c, who, e_, (what), (want));            \
    } while (0)

}  // namespace

namespace mi {

// (hidden: mi_zset_local.h) what the sweep needs, allocated; where ms_mark begins; the memsets and the blob bases, ENQUEUED
int ZsetSweep::begin(mi_zset* s, const char* who) {
    mi_ctx* c = s->ctx;
    hipStream_t st = c->stream;
    const u64 cap = s->table.cap, n_blobs = s->blobs.size();
    HIPCHK(c, ev_begin.create());

    // the blobs by base address: what a span's address is searched in
    order.resize(n_blobs);
    for (u32 i = 0; i < n_blobs; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return (size_t)s->blobs[a].mem.p < (size_t)s->blobs[b].mem.p; });
    h_bases.resize(n_blobs);
    for (u64 i = 0; i < n_blobs; ++i) h_bases[i] = (u64)(size_t)s->blobs[order[i]].mem.p;

    PRUNE_ALLOC(mark, cap, "the mark array");
    PRUNE_ALLOC(slot_blob, cap * 4, "the per-slot blob array");
    PRUNE_ALLOC(bases, n_blobs * 8, "the blob bases");
    PRUNE_ALLOC(blob_live, n_blobs * 8, "the per-blob sums");
    PRUNE_ALLOC(totals, 64, "the totals");
    HIPCHK(c, hipEventRecord(ev_begin, st));
    if (n_blobs) HIPCHK(c, hipMemcpyAsync(bases.p, h_bases.data(), n_blobs * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(mark.p, 0, cap, st));
    if (n_blobs) HIPCHK(c, hipMemsetAsync(blob_live.p, 0, n_blobs * 8, st));
    HIPCHK(c, hipMemsetAsync(totals.p, 0, 64, st));
    return MI_OK;
}

// (hidden: mi_zset_local.h) everything of a prune behind the mark
int ZsetSweep::finish(mi_zset* s, const char* who, u64 n_rows, bool keep, u32 min_live_permille, mi_prune_info* info) {
    mi_ctx* c = s->ctx;
    hipStream_t st = c->stream;
    const u64 cap = s->table.cap, n_blobs = s->blobs.size();
    mi_prune_info pi = {};
    pi.n_rows = n_rows;
    int rc = MI_OK;

    DevBuf d_cls, d_scan, d_list, d_new_addr, d_recs, new_stamps;
    DevBuf new_blob;
    SlotTable fresh;                                           // the table the survivors go into: this call's, scratch and all
    fresh.sum_bytes = true;                                    // (as the set's own inserts run)
    Event ev[8];
    StreamDrain drain{st};   // (goes first: buffers and events after it)
    for (auto& e : ev) HIPCHK(c, e.create());
    std::vector<u64> live(n_blobs);

    // ---- sweep; synchronisation 1 -----------------------------------------------------------------------------------------------
    u64* tot = totals.as<u64>();
    u64* h = c->h_word.as<u64>();
    const u32 sweep_grid = (u32)std::min<u64>((cap + kPWG - 1) / kPWG, 2048);
    hipLaunchKernelGGL(zprune_sweep_kernel, dim3(sweep_grid), dim3(kPWG), 0, st, s->table.tags.as<u64>(), s->table.slots.as<u64>(), cap, mark.as<u8>(),
                       keep ? 1u : 0u, bases.as<u64>(), (u32)n_blobs, slot_blob.as<u32>(), blob_live.as<u64>(), tot);
    HIPCHK(c, hipEventRecord(ev[1], st));
    HIPCHK(c, hipMemcpyAsync(h, tot, 40, hipMemcpyDeviceToHost, st));
    if (n_blobs) HIPCHK(c, hipMemcpyAsync(live.data(), blob_live.p, n_blobs * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev_begin, ev[1]));
    pi.ms_mark = ms;
    pi.n_unknown = h[kPTotUnknown];
    const u64 n_survive = h[kPTotSurvive];
    pi.n_dropped = h[kPTotDropped];
    pi.dropped_stored_bytes = h[kPTotDropStored];
    pi.dropped_chunk_bytes = h[kPTotDropChunk];
    if (n_survive + pi.n_dropped != s->table.count || pi.dropped_stored_bytes > s->info.stored_bytes || pi.dropped_chunk_bytes > s->info.chunk_bytes)
        return fail(c, MI_ERR_STATE, "%s: the set holds %llu digests, the sweep counted %llu that stay and %llu that go", who,
                    (unsigned long long)s->table.count, (unsigned long long)n_survive, (unsigned long long)pi.n_dropped);
    if (pi.n_dropped == 0) {                                   // nothing to drop: the set is untouched
        pi.peak_extra_bytes = extra;
        if (info) *info = pi;
        return MI_OK;
    }

    // ---- the blobs' fates -----------------------------------------------------------------------------------------------------
    std::vector<u8> cls(n_blobs, kPStay);
    u64 n_sparse = 0;
    for (u64 i = 0; i < n_blobs; ++i) {
        const u64 given = s->blobs[order[i]].bytes;
        if (live[i] > given) return fail(c, MI_ERR_STATE, "%s: a blob of %llu bytes with %llu live bytes", who, (unsigned long long)given, (unsigned long long)live[i]);
        if (live[i] == 0) cls[i] = kPDead;
        else if (live[i] * 1000 < (u64)min_live_permille * given) { cls[i] = kPCompact; ++n_sparse; }
    }

    // ---- plan; synchronisation 2 ------------------------------------------------------------------------------------------------
    const u64 nb = (cap + kPlanTile - 1) / kPlanTile;
    u64 n_move = 0, moved_bytes = 0;
    u64* block_cnt = nullptr;
    u64* block_bytes = nullptr;
    float ms_plan = 0;
    if (n_sparse) {
        PRUNE_ALLOC(d_cls, n_blobs, "the blobs' fates");
        PRUNE_ALLOC(d_scan, (2 * nb + 8) * 8, "the scan");
        block_cnt = d_scan.as<u64>();
        block_bytes = block_cnt + nb;
        u64* totals = block_bytes + nb;
        HIPCHK(c, hipEventRecord(ev[2], st));
        HIPCHK(c, hipMemcpyAsync(d_cls.p, cls.data(), n_blobs, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(zprune_block_sums_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, st, slot_blob.as<u32>(), d_cls.as<u8>(), s->table.slots.as<u64>(),
                           cap, block_cnt, block_bytes);
        hipLaunchKernelGGL(zprune_block_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, st, block_cnt, block_bytes, nb, totals);
        HIPCHK(c, hipEventRecord(ev[3], st));
        HIPCHK(c, hipMemcpyAsync(h, totals, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventElapsedTime(&ms_plan, ev[2], ev[3]));
        n_move = h[0];
        moved_bytes = h[1];
        u64 want_bytes = 0;
        for (u64 i = 0; i < n_blobs; ++i) want_bytes += cls[i] == kPCompact ? live[i] : 0;
        if (n_move == 0 || n_move > n_survive || moved_bytes != want_bytes || moved_bytes < 16 * n_move)
            return fail(c, MI_ERR_HIP, "%s: the plan counted %llu spans of %llu bytes, the sweep %llu live bytes in %llu sparse blobs", who,
                        (unsigned long long)n_move, (unsigned long long)moved_bytes, (unsigned long long)want_bytes, (unsigned long long)n_sparse);
        if ((moved_bytes + kPGatherTile - 1) / kPGatherTile >> 31)
            return fail(c, MI_ERR_INVALID, "%s: a compaction blob of %llu bytes is more than one launch covers", who, (unsigned long long)moved_bytes);
        const hipError_t e = new_blob.alloc_exact(moved_bytes, &extra);
        if (e == hipErrorOutOfMemory) {                        // not an error: the dead blobs still go, the sparse ones stay
            (void)hipGetLastError();
            pi.n_blobs_sparse_kept = n_sparse;
            for (auto& f : cls) if (f == kPCompact) f = kPStay;
            n_sparse = n_move = moved_bytes = 0;
        } else if (e != hipSuccess) {
            return does_not_fit(c, who, e, "the compaction blob", moved_bytes);
        }
    }

    // ---- everything else that is needed, before anything is launched that the set will point at ----------------------------------
    u64 new_cap = 1024;
    while (new_cap < 2 * n_survive) new_cap <<= 1;
    if (n_move) {
        PRUNE_ALLOC(d_list, 4 * n_move * 8, "the move list");
        PRUNE_ALLOC(d_new_addr, cap * 8, "the per-slot address array");
    }
    PRUNE_ALLOC(fresh.tags, new_cap * 8, "the new table's tags");
    PRUNE_ALLOC(fresh.slots, new_cap * kSlotWords * 8, "the new table's slots");
    PRUNE_ALLOC(d_recs, n_survive * kSlotWords * 8, "the survivors' records");
    PRUNE_ALLOC(fresh.row_state, n_survive + 16, "the insert's row states");
    PRUNE_ALLOC(fresh.row_slot, n_survive * 8 + 16, "the insert's row slots");
    PRUNE_ALLOC(fresh.counter, 64, "the insert's counters");
    if (s->ageing) PRUNE_ALLOC(new_stamps, new_cap * 4, "the new table's stamps");
    pi.peak_extra_bytes = extra;

    // ---- move, repoint ----------------------------------------------------------------------------------------------------------
    float ms_move = 0;
    if (n_move) {
        u64* e_src = d_list.as<u64>();
        u64* e_len = e_src + n_move;
        u64* e_dst = e_len + n_move;
        u64* e_slot = e_dst + n_move;
        const u64 n_tiles = (moved_bytes + kPGatherTile - 1) / kPGatherTile;
        HIPCHK(c, hipEventRecord(ev[4], st));
        HIPCHK(c, hipMemsetAsync(d_new_addr.p, 0, cap * 8, st));
        hipLaunchKernelGGL(zprune_compact_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, st, slot_blob.as<u32>(), d_cls.as<u8>(), s->table.slots.as<u64>(), cap,
                           block_cnt, block_bytes, e_src, e_len, e_dst, e_slot);
        hipLaunchKernelGGL(zprune_gather_kernel, dim3((u32)n_tiles), dim3(kPWG), 0, st, e_src, e_len, e_dst, n_move, moved_bytes, new_blob.as<u8>());
        hipLaunchKernelGGL(zprune_repoint_kernel, dim3((u32)((n_move + 255) / 256)), dim3(256), 0, st, e_slot, e_dst, n_move,
                           (u64)(size_t)new_blob.p, d_new_addr.as<u64>());
        HIPCHK(c, hipEventRecord(ev[5], st));
    }

    // ---- rebuild: the new table is complete before the old one goes ----------------------------------------------------------------
    HIPCHK(c, hipEventRecord(ev[6], st));
    rc = fresh.alloc(c, new_cap);                              // (both are large enough: only the tags' memset is enqueued)
    if (rc) return rc;
    if (n_survive) {
        hipLaunchKernelGGL(zprune_export_kernel, dim3((u32)((cap + 255) / 256)), dim3(256), 0, st, slot_blob.as<u32>(), s->table.slots.as<u64>(), cap,
                           n_move ? d_new_addr.as<u64>() : (const u64*)nullptr, d_recs.as<u64>(), n_survive, tot + kPTotCursor);
        u64 sums[3], conflict = kPNone;
        rc = fresh.insert(c, d_recs.as<u64>(), n_survive, sums, &conflict, "compressed pack set");
        if (rc) return rc;
        if (sums[0] != n_survive || conflict != kPNone)
            return fail(c, MI_ERR_HIP, "%s: the rebuild took %llu of %llu records", who, (unsigned long long)sums[0], (unsigned long long)n_survive);
    }
    if (s->ageing) {                                           // the survivors' stamps follow them: the new table is complete
        rc = zage_carry_enqueue(c, s->table.tags.as<u64>(), s->table.slots.as<u64>(), cap, s->stamps.as<u32>(), fresh.tags.as<u64>(),
                                fresh.slots.as<u64>(), new_cap, new_stamps.as<u32>());
        if (rc) return rc;
    }
    HIPCHK(c, hipEventRecord(ev[7], st));
    HIPCHK(c, hipMemcpyAsync(h, tot + kPTotCursor, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));                       // synchronisation 3
    HIPCHK(c, hipGetLastError());
    if (h[0] != n_survive)
        return fail(c, MI_ERR_HIP, "%s: %llu records exported, %llu survive", who, (unsigned long long)h[0], (unsigned long long)n_survive);
    if (n_move) HIPCHK(c, hipEventElapsedTime(&ms_move, ev[4], ev[5]));
    pi.ms_move = (double)ms_plan + ms_move;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[6], ev[7]));
    pi.ms_rebuild = ms;

    // ---- the set changes: nothing below can fail -------------------------------------------------------------------------------
    std::swap(s->table.tags, fresh.tags);                      // (the old table goes with the locals, and the insert's scratch)
    std::swap(s->table.slots, fresh.slots);
    if (s->ageing) std::swap(s->stamps, new_stamps);
    s->table.cap = new_cap;
    s->table.count = n_survive;
    std::vector<u8> fate(n_blobs);
    for (u64 i = 0; i < n_blobs; ++i) fate[order[i]] = cls[i];
    std::vector<ZsetBlob> kept;
    kept.reserve(n_blobs + 1);
    for (u64 k = 0; k < n_blobs; ++k) {
        if (fate[k] == kPStay) { kept.push_back(std::move(s->blobs[k])); continue; }
        ++pi.n_blobs_freed;
        pi.freed_bytes += s->blobs[k].mem.bytes;
        s->blobs[k].mem.release();
    }
    if (n_move) kept.push_back(ZsetBlob{std::move(new_blob), moved_bytes});
    s->blobs = std::move(kept);
    pi.n_blobs_compacted = n_sparse;
    pi.moved_bytes = moved_bytes;
    s->info.n_digests = n_survive;
    s->info.stored_bytes -= pi.dropped_stored_bytes;
    s->info.chunk_bytes -= pi.dropped_chunk_bytes;
    if (info) *info = pi;
    return MI_OK;
}

}  // namespace mi

extern "C" {

int mi_zset_prune(mi_zset* s, const uint8_t* digests, uint64_t n, uint32_t flags, uint32_t min_live_permille, mi_prune_info* info) {
    if (info) memset(info, 0, sizeof *info);
    if (!s || (n && !digests)) return MI_ERR_INVALID;
    static const char* who = "mi_zset_prune";
    mi_ctx* c = nullptr;
    int rc = mi_zset_ctx(s, who, &c);                          // MI_ERR_STATE with the first message for a set in its failed state
    if (rc) return rc;
    if (flags != MI_ZSET_PRUNE_KEEP && flags != MI_ZSET_PRUNE_DROP)
        return fail(c, MI_ERR_INVALID, "%s: flags %#x: exactly one of MI_ZSET_PRUNE_KEEP and MI_ZSET_PRUNE_DROP", who, flags);
    if (min_live_permille > 1000) return fail(c, MI_ERR_INVALID, "%s: min_live_permille %u is more than 1000", who, min_live_permille);
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu rows, a request holds fewer than 2^32", who, (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf d_dig;
    ZsetSweep sweep;                                           // mark, sweep and everything behind them (mi_zset_local.h)
    u64& extra = sweep.extra;                                  // what this call allocates, from the sizes
    StreamDrain drain{st};   // (goes first: buffers and events after it)
    PRUNE_ALLOC(d_dig, n * 32, "the request");
    if ((rc = sweep.begin(s, who))) return rc;
    if (n) {
        HIPCHK(c, hipMemcpyAsync(d_dig.p, digests, n * 32, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(zprune_mark_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_dig.as<u8>(), n, s->table.tags.as<u64>(),
                           s->table.slots.as<u64>(), s->table.cap - 1, sweep.mark.as<u8>(), sweep.totals.as<u64>());
    }
    return sweep.finish(s, who, n, flags == MI_ZSET_PRUNE_KEEP, min_live_permille, info);
}

int mi_zset_get_usage(const mi_zset* s, mi_zset_usage* out) {
    if (!s || !out) return MI_ERR_INVALID;
    static const char* who = "mi_zset_get_usage";
    memset(out, 0, sizeof *out);
    mi_ctx* c = nullptr;
    const int rc = mi_zset_ctx(s, who, &c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf d_total;
    StreamDrain drain{st};   // (goes first: the buffer above after it)
    HIPCHK(c, d_total.ensure(8));
    HIPCHK(c, hipMemsetAsync(d_total.p, 0, 8, st));
    const u32 grid = (u32)std::min<u64>((s->table.cap + kPWG - 1) / kPWG, 2048);
    hipLaunchKernelGGL(zprune_live_kernel, dim3(grid), dim3(kPWG), 0, st, s->table.tags.as<u64>(), s->table.slots.as<u64>(), s->table.cap, d_total.as<u64>());
    HIPCHK(c, hipMemcpyAsync(c->h_word.p, d_total.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    out->n_blobs = s->blobs.size();
    for (const ZsetBlob& b : s->blobs) out->resident_bytes += b.mem.bytes;
    out->live_bytes = c->h_word.as<u64>()[0];
    out->table_slots = s->table.cap;
    out->table_bytes = s->table.tags.bytes + s->table.slots.bytes;
    return MI_OK;
}

}  // extern "C"
