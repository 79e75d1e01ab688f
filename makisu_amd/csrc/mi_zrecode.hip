// mi_zrecode.hip -- a compressed pack set (mi_zset.hip) RECODED IN PLACE: every chunk the set holds is decoded, coded again at the
// requested level, and its stored form is replaced where -- and only where -- the new one is strictly smaller (mi_zset_recode).
// A blob with a replaced entry is rewritten into ONE new blob of the call and freed; every other blob is not touched.
//
//   list      the occupied slots become ROWS, in slot order: mi_plan.h's three launches over the table (block sums of the count
//             and of the rows' scratch NEED, the scan, the compacting pass).  A row: the span's address, length | stored << 32, its
//             slot, its blob (binary search of the address in the sorted bases) and the exclusive scan of the need -- for a coded
//             row round16(length) of plain bytes + z_worst_span(length), for a raw row the worst-case span alone (the coder reads
//             it where it lies).  Synchronisation 1: the scan comes to the host, which cuts the rows into ROUNDS of at most
//             scratch_bytes (a row that needs more is a round of its own); the scratch is the largest round's;
//   decode    one wave a row of the round (the workgroup IS the wave): z_decode_block (mi_lz4_wave.h) into the row's plain bytes,
//             the pad behind the stored span read and held against zero; the rule that refuses a row is kept per row;
//   encode    another launch, z_encode_rows' shape: one wave a row that decoded, ZLevel1 (16 KiB of LDS) or ZLevel2 (32 KiB) into
//             the row's worst-case span; the candidate's size per row;
//   hash      MI_ZSET_RECODE_VERIFY: the ctx's hashing launcher over the round's plain bytes where they lie (a raw row's in its
//             blob: the launcher's base is 0 and the offsets are absolute device addresses);
//   choose    one thread a row: replaced = it decoded and the candidate is smaller than `stored`; the new size per row, a byte per
//             BLOB that has a replaced entry, the row's place in the round's STAGING piece and in the list of replaced rows (a
//             block scan and one atomic a workgroup for each), the totals through workgroup sums (one atomic a workgroup and
//             value), and with VERIFY the digests compared.  Synchronisation a round: the totals -- the staging piece is
//             allocated at exactly the round's sum of round16(new size);
//   stage     one wave a replaced row: the new form, in whole units, from the scratch into the staging piece -- the scratch is
//             the next round's.  The staging pieces live until the call returns: peak_extra_bytes counts them;
//   plan      over the rows whose blob is marked: mi_plan.h's three launches over round16(new size) or round16(stored).
//             Synchronisation: the totals, before the new blob is allocated;
//   gather    mi_gather.h's tile body over both kinds of source side by side, as zbatch_gather_kernel does it: a replaced row
//             from its staging piece with its new size (the pad ZERO), any other row of a rewritten blob from where it lies with
//             round16(stored) as its length: whole units, the pad as it was;
//   repoint   the new addresses into a per-row array, the records exported with the new address and the new length | stored
//             word, inserted into a fresh SlotTable (mi_slot_table.h).  THE OLD TABLE IS NEVER WRITTEN;
//   recheck   VERIFY: every replaced form decoded again FROM THE NEW BLOB into the scratch (round by round, the rows' own spans)
//             and hashed there, the digests compared.  The last synchronisation; then the table is swapped, the rewritten blobs
//             are freed and the new blob joins the set.
//
// Everything is allocated before anything changes, by DevBuf::alloc_exact; whatever fails, the set is as it was.
//
// BOUNDS.  list READS tags, slots [0, cap), bases [0, n_blobs), WRITES the row arrays at [0, n): the positions are the exclusive
// scan of the predicate the block sums counted, n = the table's count (checked against the scan's total before any row is used).
// decode READS [src, src + round16(stored)) -- z_decode_block compares every index with `stored` before the load, the pad check
// reads [stored, round16(stored)), inside the blob by the structural check of every add -- and WRITES [plain, plain + length) of
// the row's own span of the scratch (len <= length - op before every copy).  encode READS [plain, plain + length) (pos <= n - 12,
// match bytes below n - 5) of the scratch or, for a raw row, of the blob, and WRITES below z_worst_span(length) behind the row's
// plain bytes (checked per sequence).  The two are separate launches on one stream: the kernel boundary is what makes the
// decoder's stores visible to the coder's loads.  stage READS whole units below round16(new size) <= z_worst_span(length) of
// the row's span, WRITES the same units at the row's offset in a piece of exactly the sum of them.  gather READS aligned units
// inside [src, src + round16(len)) of a staging piece or a blob, WRITES aligned units inside [0, new_blob_bytes).  recheck's
// decoder WRITES [span, span + length) with length <= the span's bytes.  The hashing reads up to 67 bytes behind a string: a
// DevBuf's 256 bytes of slack, behind a blob as behind the scratch.
#include "mi_gather.h"
#include "mi_lz4_wave.h"
#include "mi_zrows.h"
#include "mi_zset_local.h"
#include "mi_zentropy.h"

using namespace mi;

namespace mi {

constexpr u64 kRNone = ~0ull;
constexpr int kRWG = 256;                                     // choose, repoint, export
constexpr u64 kRDefaultScratch = 256ull << 20;                // scratch_bytes = 0
enum : int { kRTotRows = 0, kRTotNeed = 1, kRTotLive = 2, kRTotRecoded = 3, kRTotRawRecoded = 4, kRTotUndecodable = 5, kRTotSavedStored = 6,
             kRTotSavedLive = 7, kRTotBad = 8, kRTotFirstBad = 9, kRTotStaged = 10, kRTotMove = 11, kRTotBlobBytes = 12, kRTotBad2 = 13,
             kRTotFirstBad2 = 14, kRTotWords = 16 };

typedef const u8 __attribute__((address_space(1))) * r_global_bytes;

// what a row takes in the scratch: the plain bytes of a coded row, and the coder's worst-case span
static __device__ __forceinline__ u64 zrecode_plain_bytes(u64 word) {
    const u64 len = word & 0xFFFFFFFFull, stored = word >> 32;
    return stored < len ? round16(len) : 0;
}
static __device__ __forceinline__ u64 zrecode_need(u64 word) { return zrecode_plain_bytes(word) + z_worst_span(word & 0xFFFFFFFFull); }

// ---- list: the occupied slots as rows, in slot order ------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlanBlock)
void zrecode_block_sums_kernel(const u64* __restrict__ tags, const u64* __restrict__ slots, u64 cap, u64* __restrict__ block_cnt,
                               u64* __restrict__ block_need, u64* __restrict__ totals) {
    __shared__ u64 lds[3][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[3] = {0, 0, 0};                             // rows, their need, their live bytes
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (base + k >= cap || tags[base + k] == 0ull) continue;
        const u64 word = slots[kSlotWords * (base + k) + 5];
        ++v[0];
        v[1] += zrecode_need(word);
        v[2] += round16(word >> 32);
    }
    plan_block_sum<3>(v, lds);
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = v[0];
        block_need[blockIdx.x] = v[1];
        if (v[2]) atomicAdd((unsigned long long*)&totals[kRTotLive], (unsigned long long)v[2]);
    }
}

__global__ __launch_bounds__(kPlanBlock)
void zrecode_block_offsets_kernel(u64* __restrict__ block_cnt, u64* __restrict__ block_need, u64 n_blocks, u64* __restrict__ totals) {
    plan_block_offsets<true>(block_cnt, block_need, n_blocks, &totals[kRTotRows], &totals[kRTotNeed]);
}

// rows at [0, limit): a row beyond it (the table's count and the scan disagree: the host refuses the call) is not written
__global__ __launch_bounds__(kPlanBlock)
void zrecode_list_kernel(const u64* __restrict__ tags, const u64* __restrict__ slots, u64 cap, const u64* __restrict__ block_cnt,
                         const u64* __restrict__ block_need, const u64* __restrict__ bases, u32 n_blobs, u64 limit, u64* __restrict__ r_src,
                         u64* __restrict__ r_word, u64* __restrict__ r_slot, u64* __restrict__ r_off, u32* __restrict__ r_blob) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 word[kPlanPer];
    u32 sel = 0;
    u64 cnt = 0, need = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const bool m = base + k < cap && tags[base + k] != 0ull;
        word[k] = m ? slots[kSlotWords * (base + k) + 5] : 0;
        if (m) { sel |= 1u << k; ++cnt; need += zrecode_need(word[k]); }
    }
    u64 at = plan_first(cnt, block_cnt);
    u64 off = plan_first(need, block_need);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (!(sel & (1u << k))) continue;
        if (at < limit) {
            const u64 addr = slots[kSlotWords * (base + k) + 4];
            u32 lo = 0, hi = n_blobs;                 // the last base at or below the span's address
            while (hi - lo > 1) {
                const u32 mid = lo + ((hi - lo) >> 1);
                if (bases[mid] <= addr) lo = mid; else hi = mid;
            }
            r_src[at] = addr;
            r_word[at] = word[k];
            r_slot[at] = base + k;
            r_off[at] = off;
            r_blob[at] = lo;
        }
        ++at;
        off += zrecode_need(word[k]);
    }
}

// ---- decode: one wave a row of the round [r0, r0 + n) -----------------------------------------------------------------------------
// r_rule[k] = 0 or the rule that refuses row k's stored form (a pad byte that is not zero among them); with h_off (VERIFY):
// where row k's plain bytes lie, as an absolute address, and their length, for the hashing launcher
__global__ __launch_bounds__(64)
void zrecode_decode_kernel(const u64* __restrict__ r_src, const u64* __restrict__ r_word, const u64* __restrict__ r_off, u64 r0, u64 n,
                           u64 base_off, u8* scratch, u32* __restrict__ r_rule, u64* __restrict__ h_off, u64* __restrict__ h_len) {
    const int lane = threadIdx.x;
    for (u64 i = blockIdx.x; i < n; i += gridDim.x) {
        const u64 k = r0 + i;
        const u8* src = (const u8*)(r_global_bytes)r_src[k];
        const u64 len = r_word[k] & 0xFFFFFFFFull, stored = r_word[k] >> 32;
        u8* plain = scratch + (r_off[k] - base_off);
        u32 rule = 0;
        if (stored < len) rule = z_decode_block(src, stored, plain, len, lane);
        const bool pad_set = stored + lane < round16(stored) && src[stored + lane] != 0;
        if (__ballot(pad_set) != 0 && rule == 0) rule = mi_host::kLz4PadNotZero;
        if (lane == 0) {
            r_rule[k] = rule;
            if (h_off) {
                h_off[k] = stored < len ? (u64)(size_t)plain : r_src[k];
                h_len[k] = len;
            }
        }
        __syncthreads();
    }
}

// ---- encode: z_encode_rows' shape over the rows that decoded; r_cand[k] = what the coder stores (length: raw) -----------------------
template <class Coder>
static __device__ __forceinline__ void zrecode_encode_rows(const u64* __restrict__ r_src, const u64* __restrict__ r_word, const u64* __restrict__ r_off,
                                                           const u32* __restrict__ r_rule, u64 r0, u64 n, u64 base_off, u8* scratch,
                                                           u32* __restrict__ r_cand, u32* tables) {
    const int lane = threadIdx.x;
    for (u64 i = blockIdx.x; i < n; i += gridDim.x) {
        const u64 k = r0 + i;
        const u32 len = (u32)r_word[k], stored = (u32)(r_word[k] >> 32);
        u8* span = scratch + (r_off[k] - base_off);
        u32 cand = len;                               // a row that does not decode has no candidate: never below `stored`
        if (r_rule[k] == 0) {
            const u8* plain = stored < len ? span : (const u8*)(r_global_bytes)r_src[k];
            cand = Coder::encode(plain, len, span + zrecode_plain_bytes(r_word[k]), z_worst_span(len), tables, lane);
        }
        if (lane == 0) r_cand[k] = cand;
    }
}

__global__ __launch_bounds__(64)
void zrecode_encode_l1_kernel(const u64* __restrict__ r_src, const u64* __restrict__ r_word, const u64* __restrict__ r_off,
                              const u32* __restrict__ r_rule, u64 r0, u64 n, u64 base_off, u8* scratch, u32* __restrict__ r_cand) {
    __shared__ u32 table[kZTable];
    zrecode_encode_rows<ZLevel1>(r_src, r_word, r_off, r_rule, r0, n, base_off, scratch, r_cand, table);
}

__global__ __launch_bounds__(64)
void zrecode_encode_l2_kernel(const u64* __restrict__ r_src, const u64* __restrict__ r_word, const u64* __restrict__ r_off,
                              const u32* __restrict__ r_rule, u64 r0, u64 n, u64 base_off, u8* scratch, u32* __restrict__ r_cand) {
    __shared__ u32 tables[2 * kZTable];                   // t4 | t8: 32 KiB a wave
    zrecode_encode_rows<ZLevel2>(r_src, r_word, r_off, r_rule, r0, n, base_off, scratch, r_cand, tables);
}

// ---- choose: one thread a row of the round ----------------------------------------------------------------------------------------
// r_new[k] = the new stored size of a replaced row, else 0; r_stage[k] = where its new form goes, counted from the call's first
// staged byte (totals[kRTotStaged] runs on from round to round); rep_rows: the replaced rows, a round's behind the round's before
// it (inside a round in no stated order: nothing depends on it); blob_mark[b] = 1 for a blob with a replaced row.  got (VERIFY):
// the round's digests, row k's at 32 k
__global__ __launch_bounds__(kRWG)
void zrecode_choose_kernel(const u64* __restrict__ r_word, const u32* __restrict__ r_rule, const u32* __restrict__ r_cand,
                           const u32* __restrict__ r_blob, const u64* __restrict__ r_slot, const u64* __restrict__ slots,
                           const u8* __restrict__ got, u64 r0, u64 n, u32* __restrict__ r_new, u64* __restrict__ r_stage,
                           u64* __restrict__ rep_rows, u8* __restrict__ blob_mark, u64* __restrict__ totals) {
    __shared__ u64 lds[5][kRWG / 64];
    __shared__ u64 s_first[2];
    const u64 i = (u64)blockIdx.x * kRWG + threadIdx.x;
    const u64 k = r0 + i;
    const bool in = i < n;
    u64 v[5] = {0, 0, 0, 0, 0};                       // replaced raw rows, undecodable rows, stored bytes saved, live bytes saved, bad rows
    u64 staged = 0;
    bool replaced = false;
    if (in) {
        const u64 len = r_word[k] & 0xFFFFFFFFull, stored = r_word[k] >> 32;
        const u32 rule = r_rule[k], cand = r_cand[k];
        replaced = rule == 0 && cand < stored;
        bool bad = false;
        if (got) {
            const u64* g = (const u64*)(got + 32 * k);
            const u64* w = slots + kSlotWords * r_slot[k];
            bad = rule != 0 || g[0] != w[0] || g[1] != w[1] || g[2] != w[2] || g[3] != w[3];
            if (bad) atomicMin((unsigned long long*)&totals[kRTotFirstBad], (unsigned long long)k);
        }
        v[1] = rule != 0 ? 1 : 0;
        v[4] = bad ? 1 : 0;
        if (replaced) {
            v[0] = stored == len ? 1 : 0;
            v[2] = stored - cand;
            v[3] = round16(stored) - round16(cand);
            staged = round16(cand);
            blob_mark[r_blob[k]] = 1;                 // (every writer stores the same byte)
        }
        r_new[k] = replaced ? cand : 0u;
    }
    u64 tot_cnt, tot_bytes;
    const u64 my_cnt = block_exclusive_scan_u64<kRWG>(replaced ? 1 : 0, &tot_cnt, plan_scan_lds());
    const u64 my_at = block_exclusive_scan_u64<kRWG>(staged, &tot_bytes, plan_scan_lds());
    if (threadIdx.x == 0) {                           // the workgroup's ranges: one atomic each
        s_first[0] = tot_cnt ? atomicAdd((unsigned long long*)&totals[kRTotRecoded], (unsigned long long)tot_cnt) : 0;
        s_first[1] = tot_bytes ? atomicAdd((unsigned long long*)&totals[kRTotStaged], (unsigned long long)tot_bytes) : 0;
    }
    __syncthreads();
    if (replaced) {
        rep_rows[s_first[0] + my_cnt] = k;
        r_stage[k] = s_first[1] + my_at;
    }
    plan_block_sum<5>(v, lds);                        // (the replaced rows and their staged bytes: the ranges' atomics above)
    if (threadIdx.x == 0) {
        if (v[0]) atomicAdd((unsigned long long*)&totals[kRTotRawRecoded], (unsigned long long)v[0]);
        if (v[1]) atomicAdd((unsigned long long*)&totals[kRTotUndecodable], (unsigned long long)v[1]);
        if (v[2]) atomicAdd((unsigned long long*)&totals[kRTotSavedStored], (unsigned long long)v[2]);
        if (v[3]) atomicAdd((unsigned long long*)&totals[kRTotSavedLive], (unsigned long long)v[3]);
        if (v[4]) atomicAdd((unsigned long long*)&totals[kRTotBad], (unsigned long long)v[4]);
    }
}

// ---- stage: one wave a replaced row of the round, rep[0, n): its new form out of the scratch, in whole units --------------------
// r_stage[k]: in, the place counted from the call's first staged byte (the round's piece begins at staged_before); out, the
// absolute address
__global__ __launch_bounds__(64)
void zrecode_stage_kernel(const u64* __restrict__ rep, u64 n, const u64* __restrict__ r_word, const u64* __restrict__ r_off,
                          const u32* __restrict__ r_new, u64 base_off, const u8* __restrict__ scratch, u64 staged_before,
                          u8* __restrict__ piece, u64* __restrict__ r_stage) {
    const int lane = threadIdx.x;
    for (u64 i = blockIdx.x; i < n; i += gridDim.x) {
        const u64 k = rep[i];
        const u8* src = scratch + (r_off[k] - base_off) + zrecode_plain_bytes(r_word[k]);
        u8* dst = piece + (r_stage[k] - staged_before);
        const u64 bytes = r_new[k];
        for (u64 u = (u64)lane * 16; u < bytes; u += 64 * 16) *(u32x4*)(dst + u) = *(const u32x4*)(src + u);
        __syncthreads();                              // every lane has read r_stage[k]
        if (lane == 0) r_stage[k] = (u64)(size_t)dst;
    }
}

// ---- plan: mi_plan.h's over the rows of the blobs to be rewritten --------------------------------------------------------------------
static __device__ __forceinline__ u64 zrecode_moved_bytes(const u64* __restrict__ r_word, const u32* __restrict__ r_new, u64 k) {
    const u32 now = r_new[k];
    return round16(now ? (u64)now : r_word[k] >> 32);
}

__global__ __launch_bounds__(kPlanBlock)
void zrecode_move_sums_kernel(const u32* __restrict__ r_blob, const u8* __restrict__ blob_mark, const u64* __restrict__ r_word,
                              const u32* __restrict__ r_new, u64 n, u64* __restrict__ block_cnt, u64* __restrict__ block_bytes) {
    __shared__ u64 lds[2][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (base + k >= n || !blob_mark[r_blob[base + k]]) continue;
        ++v[0];
        v[1] += zrecode_moved_bytes(r_word, r_new, base + k);
    }
    plan_block_sum<2>(v, lds);
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = v[0];
        block_bytes[blockIdx.x] = v[1];
    }
}

__global__ __launch_bounds__(kPlanBlock)
void zrecode_move_offsets_kernel(u64* __restrict__ block_cnt, u64* __restrict__ block_bytes, u64 n_blocks, u64* __restrict__ totals) {
    plan_block_offsets<true>(block_cnt, block_bytes, n_blocks, &totals[kRTotMove], &totals[kRTotBlobBytes]);
}

// the move list, in row order (= slot order): a replaced row from its staging piece with its new size, any other from where it
// lies with round16(stored) -- whole units, the pad as it was
__global__ __launch_bounds__(kPlanBlock)
void zrecode_compact_kernel(const u32* __restrict__ r_blob, const u8* __restrict__ blob_mark, const u64* __restrict__ r_src,
                            const u64* __restrict__ r_word, const u32* __restrict__ r_new, const u64* __restrict__ r_stage, u64 n,
                            const u64* __restrict__ block_cnt, const u64* __restrict__ block_bytes, u64* __restrict__ e_src,
                            u64* __restrict__ e_len, u64* __restrict__ e_dst, u64* __restrict__ e_row) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 len[kPlanPer];
    u32 sel = 0;
    u64 cnt = 0, bytes = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const bool m = base + k < n && blob_mark[r_blob[base + k]] != 0;
        len[k] = m ? zrecode_moved_bytes(r_word, r_new, base + k) : 0;
        if (m) { sel |= 1u << k; ++cnt; bytes += len[k]; }
    }
    u64 at = plan_first(cnt, block_cnt);
    u64 dst = plan_first(bytes, block_bytes);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (!(sel & (1u << k))) continue;
        const u32 now = r_new[base + k];
        e_src[at] = now ? r_stage[base + k] : r_src[base + k];
        e_len[at] = now ? (u64)now : len[k];
        e_dst[at] = dst;
        e_row[at] = base + k;
        ++at;
        dst += len[k];
    }
}

__global__ __launch_bounds__(kGatherWG)
void zrecode_gather_kernel(const u64* __restrict__ e_src, const u64* __restrict__ e_len, const u64* __restrict__ e_dst, u64 n_entries,
                           u64 blob_bytes, u8* __restrict__ blob) {
    gather_tile<true>(e_src, e_len, e_dst, n_entries, blob_bytes, blob);
}

// ---- repoint, export ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRWG)
void zrecode_repoint_kernel(const u64* __restrict__ e_row, const u64* __restrict__ e_dst, u64 n, u64 new_base, u64* __restrict__ r_addr) {
    const u64 k = (u64)blockIdx.x * kRWG + threadIdx.x;
    if (k < n) r_addr[e_row[k]] = new_base + e_dst[k];
}

// row k's record: the digest as the old table holds it, the new address of a moved span (r_addr: 0, not this one), the new
// length | stored word of a replaced one
__global__ __launch_bounds__(kRWG)
void zrecode_export_kernel(const u64* __restrict__ slots, const u64* __restrict__ r_slot, const u64* __restrict__ r_word,
                           const u32* __restrict__ r_new, const u64* __restrict__ r_addr, u64 n, u64* __restrict__ out) {
    const u64 k = (u64)blockIdx.x * kRWG + threadIdx.x;
    if (k >= n) return;
    const u64* w = slots + kSlotWords * r_slot[k];
    u64* o = out + kSlotWords * k;
    const u64 moved = r_addr[k];
    const u32 now = r_new[k];
    o[0] = w[0]; o[1] = w[1]; o[2] = w[2]; o[3] = w[3];
    o[4] = moved ? moved : w[4];
    o[5] = now ? ((r_word[k] & 0xFFFFFFFFull) | ((u64)now << 32)) : r_word[k];
}

// ---- recheck (VERIFY): the replaced forms decoded again from the new blob, one wave a row of rep[0, n) -----------------------------
// into the row's own span of the scratch (at least z_worst_span(length) bytes: more than its length); v_off / v_len: the
// hashing launcher's strings, entry i of the list at i
__global__ __launch_bounds__(64)
void zrecode_redecode_kernel(const u64* __restrict__ rep, u64 n, const u64* __restrict__ r_word, const u64* __restrict__ r_off,
                             const u32* __restrict__ r_new, const u64* __restrict__ r_addr, u64 base_off, u8* scratch,
                             u64* __restrict__ v_off, u64* __restrict__ v_len, u64* __restrict__ totals) {
    const int lane = threadIdx.x;
    for (u64 i = blockIdx.x; i < n; i += gridDim.x) {
        const u64 k = rep[i];
        const u8* src = (const u8*)(r_global_bytes)r_addr[k];
        const u64 len = r_word[k] & 0xFFFFFFFFull, stored = r_new[k];
        u8* dst = scratch + (r_off[k] - base_off);
        u32 rule = z_decode_block(src, stored, dst, len, lane);
        const bool pad_set = stored + lane < round16(stored) && src[stored + lane] != 0;
        if (__ballot(pad_set) != 0 && rule == 0) rule = mi_host::kLz4PadNotZero;
        if (lane == 0) {
            v_off[i] = (u64)(size_t)dst;
            v_len[i] = len;
            if (rule) {
                atomicAdd((unsigned long long*)&totals[kRTotBad2], 1ull);
                atomicMin((unsigned long long*)&totals[kRTotFirstBad2], (unsigned long long)k);
            }
        }
        __syncthreads();
    }
}

// entry i of the list of replaced rows: the digest of what its new form decodes to against the table's
__global__ __launch_bounds__(kRWG)
void zrecode_recheck_kernel(const u64* __restrict__ rep, u64 n, const u8* __restrict__ got, const u64* __restrict__ slots,
                            const u64* __restrict__ r_slot, u64* __restrict__ totals) {
    const u64 i = (u64)blockIdx.x * kRWG + threadIdx.x;
    if (i >= n) return;
    const u64 k = rep[i];
    const u64* g = (const u64*)(got + 32 * i);
    const u64* w = slots + kSlotWords * r_slot[k];
    if (g[0] != w[0] || g[1] != w[1] || g[2] != w[2] || g[3] != w[3]) {
        atomicAdd((unsigned long long*)&totals[kRTotBad2], 1ull);
        atomicMin((unsigned long long*)&totals[kRTotFirstBad2], (unsigned long long)k);
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

#define RECODE_ALLOC(buf, want, what)                                                     \
    do {                                                                                  \
        const hipError_t e_ = (buf).alloc_exact((want), &extra);                        \
        if (e_ != hipSuccess) return does_not_fit(c, who, e_, (what), (want));            \
    } while (0)

u32 wave_grid(u64 n) { return (u32)std::min<u64>(n, 1u << 20); }     // one wave a row; more rows: the waves go round

struct Round { u64 r0, r1, base_off, bytes, rep_before, n_rep, staged_before; };

}  // namespace

extern "C" {

int mi_zset_recode(mi_zset* s, uint32_t flags, uint64_t scratch_bytes, mi_recode_info* info) {
    if (info) memset(info, 0, sizeof *info);
    if (!s) return MI_ERR_INVALID;
    static const char* who = "mi_zset_recode";
    mi_ctx* c = nullptr;
    int rc = mi_zset_ctx(s, who, &c);                          // MI_ERR_STATE with the first message for a set in its failed state
    if (rc) return rc;
    if (flags & ~(uint32_t)(MI_ZSET_RECODE_VERIFY | MI_ZPACK_LEVEL2 | MI_ZPACK_ENTROPY)) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    const bool verify = (flags & MI_ZSET_RECODE_VERIFY) != 0, level2 = (flags & MI_ZPACK_LEVEL2) != 0, entropy = (flags & MI_ZPACK_ENTROPY) != 0;
    mi_recode_info ri = {};
    const u64 n = s->table.count, cap = s->table.cap, n_blobs = s->blobs.size();
    ri.n_digests = n;
    ri.stored_before = ri.stored_after = s->info.stored_bytes;
    if (n == 0) {                                              // a set of nothing
        if (info) *info = ri;
        return MI_OK;
    }
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu digests, a call recodes fewer than 2^32", who, (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const u64 budget = scratch_bytes ? scratch_bytes : kRDefaultScratch;
    u64 extra = 0;                                             // what this call allocates, from the sizes

    DevBuf d_bases, d_mark, d_tot, d_scan, d_rows, d_rule, d_cand, d_new, d_blob_of, d_rep, d_hash, d_got, d_scratch;
    DevBuf d_scan2, d_list, d_addr, d_recs, d_vstr, d_got2, new_blob, new_stamps;
    DevBuf d_urows, d_scratch2, d_vrows;                       // the entropy stage's (mi_zentropy.h): unwrapped rows, form H's scratch, the recheck's rows
    ZhUnwrap unwrap, unwrap2;                                  // ... the held forms' inner forms; the replaced forms', for the recheck
    std::vector<DevBuf> pieces;                                // the staging pieces, one a round that replaces something
    SlotTable fresh;                                           // the table the records go into: this call's, scratch and all
    fresh.sum_bytes = true;
    Event ev[6];
    StreamDrain drain{st};   // (goes first: buffers and events after it)
    for (auto& e : ev) HIPCHK(c, e.create());
    const u64* tags = s->table.tags.as<u64>();
    const u64* slots = s->table.slots.as<u64>();

    // the blobs by base address: what a span's address is searched in
    std::vector<u32> order(n_blobs);
    for (u32 i = 0; i < n_blobs; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return (size_t)s->blobs[a].mem.p < (size_t)s->blobs[b].mem.p; });
    std::vector<u64> bases(n_blobs);
    for (u64 i = 0; i < n_blobs; ++i) bases[i] = (u64)(size_t)s->blobs[order[i]].mem.p;
    if (n_blobs == 0) return fail(c, MI_ERR_STATE, "%s: the set holds %llu digests and no blob", who, (unsigned long long)n);

    // ---- list; synchronisation 1 ------------------------------------------------------------------------------------------------
    const u64 nb = (cap + kPlanTile - 1) / kPlanTile;
    RECODE_ALLOC(d_bases, n_blobs * 8, "the blob bases");
    RECODE_ALLOC(d_mark, n_blobs, "the blobs' marks");
    RECODE_ALLOC(d_tot, kRTotWords * 8, "the totals");
    RECODE_ALLOC(d_scan, 2 * nb * 8, "the scan");
    RECODE_ALLOC(d_rows, 5 * n * 8, "the rows");
    RECODE_ALLOC(d_rule, n * 4, "the rows' rules");
    RECODE_ALLOC(d_cand, n * 4, "the candidates' sizes");
    RECODE_ALLOC(d_new, n * 4, "the new sizes");
    RECODE_ALLOC(d_blob_of, n * 4, "the rows' blobs");
    RECODE_ALLOC(d_rep, n * 8, "the list of replaced rows");
    if (verify) {
        RECODE_ALLOC(d_hash, 2 * n * 8, "the hashing pass's strings");
        RECODE_ALLOC(d_got, n * 32, "the digests");
    }
    u64* tot = d_tot.as<u64>();
    u64* block_cnt = d_scan.as<u64>();
    u64* block_need = block_cnt + nb;
    u64* r_src = d_rows.as<u64>();
    u64* r_word = r_src + n;
    u64* r_slot = r_word + n;
    u64* r_off = r_slot + n;
    u64* r_stage = r_off + n;
    u32* r_rule = d_rule.as<u32>();
    u32* r_cand = d_cand.as<u32>();
    u32* r_new = d_new.as<u32>();
    u32* r_blob = d_blob_of.as<u32>();
    u64* rep_rows = d_rep.as<u64>();
    u64* h_off = verify ? d_hash.as<u64>() : nullptr;
    u64* h_len = verify ? h_off + n : nullptr;
    u64 h[kRTotWords];
    std::vector<u64> offs(n);
    HIPCHK(c, hipMemcpyAsync(d_bases.p, bases.data(), n_blobs * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_mark.p, 0, n_blobs, st));
    HIPCHK(c, hipMemsetAsync(tot, 0, kRTotWords * 8, st));
    HIPCHK(c, hipMemsetAsync(tot + kRTotFirstBad, 0xFF, 8, st));
    HIPCHK(c, hipMemsetAsync(tot + kRTotFirstBad2, 0xFF, 8, st));
    hipLaunchKernelGGL(zrecode_block_sums_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, st, tags, slots, cap, block_cnt, block_need, tot);
    hipLaunchKernelGGL(zrecode_block_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, st, block_cnt, block_need, nb, tot);
    hipLaunchKernelGGL(zrecode_list_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, st, tags, slots, cap, block_cnt, block_need, d_bases.as<u64>(),
                       (u32)n_blobs, n, r_src, r_word, r_slot, r_off, r_blob);
    HIPCHK(c, hipMemcpyAsync(h, tot, kRTotWords * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(offs.data(), r_off, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    const u64 total_need = h[kRTotNeed];
    if (h[kRTotRows] != n)
        return fail(c, MI_ERR_STATE, "%s: the set holds %llu digests, the scan counted %llu", who, (unsigned long long)n, (unsigned long long)h[kRTotRows]);
    ri.live_before = ri.live_after = h[kRTotLive];
    // the entropy forms the set holds (mi_zentropy.h) are unwrapped first, into a scratch of the call's: the decode, the coder and
    // the staging read a row through u_src / u_word, COPIES in which a form H row points at its inner form (kind 1: an LZ4 row,
    // kind 2: a raw row); everything that compares, counts or exports reads r_src / r_word, the set's own words.  A row's place in a
    // round's scratch comes from r_word: a kind 2 row has room for plain bytes that it does not use.  No form H: no copy
    mi_zforms forms;
    if ((rc = zh_count_forms(c, 0, r_src, 1u, r_word, 1u, n, nullptr, &forms))) return rc;
    const bool holds_h = forms.n[2] + forms.n[3] != 0;
    const u64* u_src = r_src;
    const u64* u_word = r_word;
    if (holds_h) {
        RECODE_ALLOC(d_urows, 2 * n * 8, "the unwrapped rows");
        HIPCHK(c, hipMemcpyAsync(d_urows.p, r_src, 2 * n * 8, hipMemcpyDeviceToDevice, st));      // (r_src and r_word lie side by side)
        if ((rc = unwrap.run(c, who, 0, d_urows.as<u64>(), 1u, d_urows.as<u64>() + n, 1u, n))) return rc;
        extra += unwrap.inner_bytes;
        u_src = d_urows.as<u64>();
        u_word = u_src + n;
    }

    // ---- the rounds: rows [r0, r1) whose need is at most the bound; a row that needs more is a round of its own -------------------
    std::vector<Round> rounds;
    u64 scratch_max = 0;
    for (u64 r0 = 0; r0 < n;) {
        u64 r1 = r0 + 1;
        auto end_of = [&](u64 r) { return r < n ? offs[r] : total_need; };
        while (r1 < n && end_of(r1 + 1) - offs[r0] <= budget) ++r1;
        rounds.push_back(Round{r0, r1, offs[r0], end_of(r1) - offs[r0], 0, 0, 0});
        scratch_max = std::max(scratch_max, rounds.back().bytes);
        r0 = r1;
    }
    ri.n_rounds = rounds.size();
    RECODE_ALLOC(d_scratch, scratch_max, "the scratch");
    if (entropy) RECODE_ALLOC(d_scratch2, scratch_max, "the entropy stage's scratch");
    u8* scratch = d_scratch.as<u8>();
    const auto hash_items = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? launch_blake2s_items : launch_sha256_items;

    u64 n_rep = 0, staged = 0;
    for (Round& r : rounds) {
        const u64 nr = r.r1 - r.r0;
        r.rep_before = n_rep;
        r.staged_before = staged;
        HIPCHK(c, hipEventRecord(ev[0], st));
        hipLaunchKernelGGL(zrecode_decode_kernel, dim3(wave_grid(nr)), dim3(64), 0, st, u_src, u_word, r_off, r.r0, nr, r.base_off, scratch, r_rule,
                           h_off, h_len);
        if (holds_h) zh_rules_merge_enqueue(c, unwrap.rules(), r_rule, r.r0, nr);
        HIPCHK(c, hipEventRecord(ev[1], st));
        if (level2)
            hipLaunchKernelGGL(zrecode_encode_l2_kernel, dim3(wave_grid(nr)), dim3(64), 0, st, u_src, u_word, r_off, r_rule, r.r0, nr, r.base_off,
                               scratch, r_cand);
        else
            hipLaunchKernelGGL(zrecode_encode_l1_kernel, dim3(wave_grid(nr)), dim3(64), 0, st, u_src, u_word, r_off, r_rule, r.r0, nr, r.base_off,
                               scratch, r_cand);
        if (entropy)                                           // form H over the candidates, where it is smaller by more than a sixteenth
            zh_recode_encode_enqueue(c, u_src, u_word, r_off, r_rule, r.r0, nr, r.base_off, scratch, d_scratch2.p, r_cand, wave_grid(nr));
        HIPCHK(c, hipEventRecord(ev[2], st));
        if (verify)                                            // base 0: the offsets are absolute device addresses
            hash_items(kShaBlobs, (const u8*)nullptr, h_off + r.r0, h_len + r.r0, nullptr, (u32)nr, nullptr, c->heads.as<u32>(), nullptr, true,
                       d_got.as<u8>() + 32 * r.r0, c->sha, c->prop.multiProcessorCount, r.bytes, st);
        HIPCHK(c, hipEventRecord(ev[3], st));
        hipLaunchKernelGGL(zrecode_choose_kernel, dim3((u32)((nr + kRWG - 1) / kRWG)), dim3(kRWG), 0, st, r_word, r_rule, r_cand, r_blob, r_slot, slots,
                           verify ? d_got.as<u8>() : (const u8*)nullptr, r.r0, nr, r_new, r_stage, rep_rows, d_mark.as<u8>(), tot);
        HIPCHK(c, hipEventRecord(ev[4], st));
        HIPCHK(c, hipMemcpyAsync(h, tot, kRTotWords * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));                   // the round's synchronisation
        HIPCHK(c, hipGetLastError());
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
        ri.ms_decode += ms;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[1], ev[2]));
        ri.ms_encode += ms;
        if (verify) {
            HIPCHK(c, hipEventElapsedTime(&ms, ev[2], ev[3]));
            ri.ms_verify += ms;
        }
        HIPCHK(c, hipEventElapsedTime(&ms, ev[3], ev[4]));
        ri.ms_move += ms;
        if (h[kRTotRecoded] < n_rep || h[kRTotRecoded] - n_rep > nr || h[kRTotStaged] < staged)
            return fail(c, MI_ERR_HIP, "%s: a round of %llu rows counted %llu replaced", who, (unsigned long long)nr,
                        (unsigned long long)(h[kRTotRecoded] - n_rep));
        r.n_rep = h[kRTotRecoded] - n_rep;
        const u64 piece_bytes = h[kRTotStaged] - staged;
        n_rep = h[kRTotRecoded];
        staged = h[kRTotStaged];
        if (r.n_rep && !(verify && h[kRTotBad])) {             // (a call that is going to fail stages nothing more)
            pieces.emplace_back();
            RECODE_ALLOC(pieces.back(), piece_bytes, "a staging piece");
            HIPCHK(c, hipEventRecord(ev[0], st));
            hipLaunchKernelGGL(zrecode_stage_kernel, dim3(wave_grid(r.n_rep)), dim3(64), 0, st, rep_rows + r.rep_before, r.n_rep, u_word, r_off, r_new,
                               r.base_off, scratch, r.staged_before, pieces.back().as<u8>(), r_stage);
            HIPCHK(c, hipEventRecord(ev[1], st));
            HIPCHK(c, hipStreamSynchronize(st));               // (the events are the next round's)
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
            ri.ms_move += ms;
        }
    }
    ri.n_undecodable = h[kRTotUndecodable];
    ri.peak_extra_bytes = extra;
    if (verify && h[kRTotBad]) {
        const u64 bad = h[kRTotFirstBad];
        u64 slot = 0;
        u8 dg[32] = {};
        u32 rule = 0;
        if (bad < n) {
            HIPCHK(c, hipMemcpy(&slot, r_slot + bad, 8, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(&rule, r_rule + bad, 4, hipMemcpyDeviceToHost));
            if (slot < cap) HIPCHK(c, hipMemcpy(dg, slots + kSlotWords * slot, 32, hipMemcpyDeviceToHost));
        }
        return fail(c, MI_ERR_IO, "%s: %llu of %llu entries do not decode to bytes that hash to their digest (%llu of them do not decode at all); "
                    "one of them: digest %s, %s%s -- the set was fed a damaged blob without MI_ZSET_VERIFY; the set is unchanged", who,
                    (unsigned long long)h[kRTotBad], (unsigned long long)n, (unsigned long long)ri.n_undecodable, hex32(dg).c_str(),
                    rule ? "the stored form does not decode: " : "the decoded bytes hash to another digest", rule ? mi_host::zrule_name(rule) : "");
    }
    ri.n_recoded = n_rep;
    ri.n_raw_recoded = h[kRTotRawRecoded];
    const u64 saved_stored = h[kRTotSavedStored], saved_live = h[kRTotSavedLive];
    if (n_rep > n || saved_stored > ri.stored_before || saved_live > ri.live_before || ri.n_raw_recoded > n_rep)
        return fail(c, MI_ERR_HIP, "%s: %llu of %llu forms replaced, %llu stored bytes saved of %llu", who, (unsigned long long)n_rep, (unsigned long long)n,
                    (unsigned long long)saved_stored, (unsigned long long)ri.stored_before);
    if (n_rep == 0) {                                          // nothing to replace: the set is untouched
        if (info) *info = ri;
        return MI_OK;
    }

    // ---- the blobs' fates; the plan over the rows of the marked ones; synchronisation --------------------------------------------
    std::vector<u8> mark(n_blobs);
    const u64 nb2 = (n + kPlanTile - 1) / kPlanTile;
    RECODE_ALLOC(d_scan2, 2 * nb2 * 8, "the move's scan");
    u64* move_cnt = d_scan2.as<u64>();
    u64* move_bytes = move_cnt + nb2;
    HIPCHK(c, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(zrecode_move_sums_kernel, dim3((u32)nb2), dim3(kPlanBlock), 0, st, r_blob, d_mark.as<u8>(), r_word, r_new, n, move_cnt, move_bytes);
    hipLaunchKernelGGL(zrecode_move_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, st, move_cnt, move_bytes, nb2, tot);
    HIPCHK(c, hipEventRecord(ev[1], st));
    HIPCHK(c, hipMemcpyAsync(h, tot, kRTotWords * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(mark.data(), d_mark.p, n_blobs, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    const u64 n_move = h[kRTotMove], blob_bytes = h[kRTotBlobBytes];
    u64 n_rewritten = 0;
    for (u64 i = 0; i < n_blobs; ++i) n_rewritten += mark[i] ? 1 : 0;
    if (n_move < n_rep || n_move > n || blob_bytes < 16 * n_move || n_rewritten == 0 || blob_bytes > ri.live_before)
        return fail(c, MI_ERR_HIP, "%s: the plan counted %llu spans of %llu bytes in %llu blobs for %llu replaced forms", who, (unsigned long long)n_move,
                    (unsigned long long)blob_bytes, (unsigned long long)n_rewritten, (unsigned long long)n_rep);
    const u64 n_tiles = (blob_bytes + kGatherTile - 1) / kGatherTile;
    if (n_tiles >> 31) return fail(c, MI_ERR_INVALID, "%s: a new blob of %llu bytes is more than one launch covers", who, (unsigned long long)blob_bytes);

    // ---- everything else that is needed, before anything is launched that the set will point at ----------------------------------
    u64 new_cap = 1024;
    while (new_cap < 2 * n) new_cap <<= 1;
    RECODE_ALLOC(new_blob, blob_bytes, "the new blob");
    RECODE_ALLOC(d_list, 4 * n_move * 8, "the move list");
    RECODE_ALLOC(d_addr, n * 8, "the per-row address array");
    RECODE_ALLOC(fresh.tags, new_cap * 8, "the new table's tags");
    RECODE_ALLOC(fresh.slots, new_cap * kSlotWords * 8, "the new table's slots");
    RECODE_ALLOC(d_recs, n * kSlotWords * 8, "the records");
    RECODE_ALLOC(fresh.row_state, n + 16, "the insert's row states");
    RECODE_ALLOC(fresh.row_slot, n * 8 + 16, "the insert's row slots");
    RECODE_ALLOC(fresh.counter, 64, "the insert's counters");
    if (verify) {
        RECODE_ALLOC(d_vstr, 2 * n_rep * 8, "the recheck's strings");
        RECODE_ALLOC(d_got2, n_rep * 32, "the recheck's digests");
        if (entropy) RECODE_ALLOC(d_vrows, 2 * n_rep * 8, "the recheck's rows");
    }
    if (s->ageing) RECODE_ALLOC(new_stamps, new_cap * 4, "the new table's stamps");
    ri.peak_extra_bytes = extra;

    // ---- move, repoint ----------------------------------------------------------------------------------------------------------
    u64* e_src = d_list.as<u64>();
    u64* e_len = e_src + n_move;
    u64* e_dst = e_len + n_move;
    u64* e_row = e_dst + n_move;
    u64* r_addr = d_addr.as<u64>();
    HIPCHK(c, hipEventRecord(ev[2], st));
    HIPCHK(c, hipMemsetAsync(r_addr, 0, n * 8, st));
    hipLaunchKernelGGL(zrecode_compact_kernel, dim3((u32)nb2), dim3(kPlanBlock), 0, st, r_blob, d_mark.as<u8>(), r_src, r_word, r_new, r_stage, n, move_cnt,
                       move_bytes, e_src, e_len, e_dst, e_row);
    hipLaunchKernelGGL(zrecode_gather_kernel, dim3((u32)n_tiles), dim3(kGatherWG), 0, st, e_src, e_len, e_dst, n_move, blob_bytes, new_blob.as<u8>());
    hipLaunchKernelGGL(zrecode_repoint_kernel, dim3((u32)((n_move + kRWG - 1) / kRWG)), dim3(kRWG), 0, st, e_row, e_dst, n_move, (u64)(size_t)new_blob.p,
                       r_addr);
    HIPCHK(c, hipEventRecord(ev[3], st));

    // ---- rebuild: the new table is complete before the old one goes ----------------------------------------------------------------
    rc = fresh.alloc(c, new_cap);                              // (both are large enough: only the tags' memset is enqueued)
    if (rc) return rc;
    hipLaunchKernelGGL(zrecode_export_kernel, dim3((u32)((n + kRWG - 1) / kRWG)), dim3(kRWG), 0, st, slots, r_slot, r_word, r_new, r_addr, n,
                       d_recs.as<u64>());
    u64 sums[3], conflict = kRNone;
    rc = fresh.insert(c, d_recs.as<u64>(), n, sums, &conflict, "compressed pack set");
    if (rc) return rc;
    if (sums[0] != n || conflict != kRNone || sums[1] != ri.stored_before - saved_stored)
        return fail(c, MI_ERR_HIP, "%s: the rebuild took %llu of %llu records with %llu stored bytes", who, (unsigned long long)sums[0], (unsigned long long)n,
                    (unsigned long long)sums[1]);
    if (s->ageing) {                                           // (mi_zage.hip) every digest's stamp follows it: the new table is complete
        rc = zage_carry_enqueue(c, tags, slots, cap, s->stamps.as<u32>(), fresh.tags.as<u64>(), fresh.slots.as<u64>(), new_cap, new_stamps.as<u32>());
        if (rc) return rc;
    }
    HIPCHK(c, hipEventRecord(ev[4], st));

    // ---- recheck (VERIFY): what the new blob holds, decoded and hashed round by round, before the swap -----------------------------
    if (verify) {
        u64* v_off = d_vstr.as<u64>();
        u64* v_len = v_off + n_rep;
        u64* v_src = entropy ? d_vrows.as<u64>() : nullptr;
        u64* v_word = entropy ? v_src + n_rep : nullptr;
        if (entropy) {                                         // the replaced forms may be form H: their rows, unwrapped from the new blob
            zh_rep_rows_enqueue(c, rep_rows, n_rep, r_word, r_new, r_addr, v_src, v_word);
            if ((rc = unwrap2.run(c, who, 0, v_src, 1u, v_word, 1u, n_rep))) return rc;
        }
        for (const Round& r : rounds) {
            if (!r.n_rep) continue;
            if (entropy)
                zh_redecode_enqueue(c, rep_rows + r.rep_before, r.n_rep, v_src + r.rep_before, v_word + r.rep_before, r_off, r.base_off, scratch,
                                    v_off + r.rep_before, v_len + r.rep_before, tot + kRTotBad2, tot + kRTotFirstBad2, wave_grid(r.n_rep));
            else
                hipLaunchKernelGGL(zrecode_redecode_kernel, dim3(wave_grid(r.n_rep)), dim3(64), 0, st, rep_rows + r.rep_before, r.n_rep, r_word, r_off, r_new,
                                   r_addr, r.base_off, scratch, v_off + r.rep_before, v_len + r.rep_before, tot);
            hash_items(kShaBlobs, (const u8*)nullptr, v_off + r.rep_before, v_len + r.rep_before, nullptr, (u32)r.n_rep, nullptr, c->heads.as<u32>(), nullptr,
                       true, d_got2.as<u8>() + 32 * r.rep_before, c->sha, c->prop.multiProcessorCount, r.bytes, st);
        }
        hipLaunchKernelGGL(zrecode_recheck_kernel, dim3((u32)((n_rep + kRWG - 1) / kRWG)), dim3(kRWG), 0, st, rep_rows, n_rep, d_got2.as<u8>(), slots, r_slot,
                           tot);
    }
    HIPCHK(c, hipEventRecord(ev[5], st));
    HIPCHK(c, hipMemcpyAsync(h, tot, kRTotWords * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));                       // the last synchronisation
    HIPCHK(c, hipGetLastError());
    float ms = 0, ms2 = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    HIPCHK(c, hipEventElapsedTime(&ms2, ev[2], ev[3]));
    ri.ms_move += (double)ms + ms2;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[3], ev[4]));
    ri.ms_rebuild = ms;
    if (verify) {
        HIPCHK(c, hipEventElapsedTime(&ms, ev[4], ev[5]));
        ri.ms_verify += ms;
        if (h[kRTotBad2]) {
            const u64 bad = h[kRTotFirstBad2];
            u64 slot = 0;
            u8 dg[32] = {};
            if (bad < n) {
                HIPCHK(c, hipMemcpy(&slot, r_slot + bad, 8, hipMemcpyDeviceToHost));
                if (slot < cap) HIPCHK(c, hipMemcpy(dg, slots + kSlotWords * slot, 32, hipMemcpyDeviceToHost));
            }
            return fail(c, MI_ERR_IO, "%s: %llu of %llu replaced forms, decoded again from the new blob, differ from their digest; one of them: digest %s "
                        "-- the set is unchanged", who, (unsigned long long)h[kRTotBad2], (unsigned long long)n_rep, hex32(dg).c_str());
        }
    }

    // ---- the set changes: nothing below can fail -------------------------------------------------------------------------------
    std::swap(s->table.tags, fresh.tags);                      // (the old table goes with the locals, and the insert's scratch)
    std::swap(s->table.slots, fresh.slots);
    if (s->ageing) std::swap(s->stamps, new_stamps);
    s->table.cap = new_cap;
    std::vector<u8> fate(n_blobs);
    for (u64 i = 0; i < n_blobs; ++i) fate[order[i]] = mark[i];
    std::vector<ZsetBlob> kept;
    kept.reserve(n_blobs + 1);
    for (u64 k = 0; k < n_blobs; ++k) {
        if (!fate[k]) { kept.push_back(std::move(s->blobs[k])); continue; }
        ++ri.n_blobs_freed;
        ri.freed_bytes += s->blobs[k].mem.bytes;
        s->blobs[k].mem.release();
    }
    kept.push_back(ZsetBlob{std::move(new_blob), blob_bytes});
    s->blobs = std::move(kept);
    ri.n_blobs_rewritten = n_rewritten;
    ri.new_blob_bytes = blob_bytes;
    ri.stored_after = ri.stored_before - saved_stored;
    ri.live_after = ri.live_before - saved_live;
    s->info.stored_bytes = ri.stored_after;
    if (info) *info = ri;
    return MI_OK;
}

}  // extern "C"
