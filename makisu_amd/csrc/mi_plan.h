// mi_plan.h -- THE PLAN of the chunk store's files, once: three launches that turn a selection over n rows into a
// compact list in row order.  Block sums: a block of kPlanBlock threads counts the selected rows among its kPlanTile rows (and
// sums their bytes); one block scans the block sums in place and leaves the totals; the compacting pass repeats the selection,
// ranks its rows inside the block and writes row k of the list at the block's offset + the rank.  What is selected, what is
// summed and what a list's row holds is each kernel's own; what is shared is here, with the 56-byte entry row, the digest
// compare of the verify passes and the want list's compaction.  Every function is forced inline (mi_wave.h's rule).
#pragma once

#include "../../include/makisu_mi.h"
#include "mi_wave.h"

namespace mi {

constexpr int kPlanBlock = 256;
constexpr int kPlanPer   = 8;                       // rows per thread
constexpr int kPlanTile  = kPlanBlock * kPlanPer;   // = 2048 rows per block

// the block's sums of Q values a thread: the four waves' results through LDS, in thread 0 (one barrier)
template <int Q>
static __device__ __forceinline__ void plan_block_sum(u64 (&v)[Q], u64 (*lds)[kPlanBlock / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        v[q] = wave_sum(v[q]);
        if (lane == 0) lds[q][wave] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            v[q] = 0;
#pragma unroll
            for (int w = 0; w < kPlanBlock / 64; ++w) v[q] += lds[q][w];
        }
    }
}

// the block scan's four words of LDS, one array for every caller below.  A kernel may scan twice through it (the count, then the
// bytes) ONLY because block_exclusive_scan_u64 ends with a barrier: nobody writes it while another wave still reads
static __device__ __forceinline__ u64* plan_scan_lds() {
    __shared__ u64 lds[kPlanBlock / 64];
    return lds;
}

// ONE block of kPlanBlock threads: the exclusive scan of block_a and, with kTwo, block_b in place (else block_b and total_b are
// not touched: NULL), kPlanBlock blocks a round with the carry between the rounds; *total_a, *total_b = their sums.  Both
// arrays are read before the first scan and written behind the second
template <bool kTwo>
static __device__ __forceinline__ void plan_block_offsets(u64* __restrict__ block_a, u64* __restrict__ block_b, u64 n_blocks,
                                                          u64* __restrict__ total_a, u64* __restrict__ total_b) {
    u64* lds = plan_scan_lds();
    u64 carry_a = 0, carry_b = 0;
    for (u64 b0 = 0; b0 < n_blocks; b0 += kPlanBlock) {
        const u64 i = b0 + threadIdx.x;
        const u64 va = i < n_blocks ? block_a[i] : 0, vb = kTwo && i < n_blocks ? block_b[i] : 0;
        u64 ta, tb = 0;
        const u64 ea = block_exclusive_scan_u64<kPlanBlock>(va, &ta, lds);
        const u64 eb = kTwo ? block_exclusive_scan_u64<kPlanBlock>(vb, &tb, lds) : 0;
        if (i < n_blocks) {
            block_a[i] = carry_a + ea;
            if (kTwo) block_b[i] = carry_b + eb;
        }
        carry_a += ta;
        carry_b += tb;
    }
    if (threadIdx.x == 0) {
        *total_a = carry_a;
        if (kTwo) *total_b = carry_b;
    }
}

// the head of a compacting kernel: where this thread's first row goes -- what the threads in front of it in the block hold
// (`mine` each) behind the block's own offset.  For the rows' count and, again, for their bytes
static __device__ __forceinline__ u64 plan_first(u64 mine, const u64* __restrict__ block_off) {
    u64 t;
    return block_exclusive_scan_u64<kPlanBlock>(mine, &t, plan_scan_lds()) + block_off[blockIdx.x];
}

// ---- the 56-byte row of a pack's and a zpack's entries: digest 4 | offset | chunk_index | length, reserved or stored ----------
constexpr int kEntryWords = sizeof(mi_pack_entry) / 8;
static_assert(sizeof(mi_pack_entry) == 56 && sizeof(mi_zpack_entry) == 56 && kEntryWords == 7,
              "mi_pack_entry and mi_zpack_entry are seven 8-byte words");

static __device__ __forceinline__ void put_entry_row(u64* __restrict__ r, const u8* __restrict__ digest32, u64 offset, u64 row, u64 length_word) {
    const u64* d = (const u64*)digest32;
    r[0] = d[0]; r[1] = d[1]; r[2] = d[2]; r[3] = d[3];
    r[4] = offset;
    r[5] = row;
    r[6] = length_word;
}

// a verify pass's compare: the digest the device computed for row k against the wanted one; the smallest row that differs
static __device__ __forceinline__ void digest_differs_mark(const u8* __restrict__ got, const u64* __restrict__ want4, u64 k,
                                                           u64* __restrict__ first_bad) {
    const u64* g = (const u64*)(got + 32 * k);
    if (g[0] != want4[0] || g[1] != want4[1] || g[2] != want4[2] || g[3] != want4[3])
        atomicMin((unsigned long long*)first_bad, (unsigned long long)k);
}

// the want list's compacting pass: the numbers of the rows selected(row) holds for, ascending
template <class Selected>
static __device__ __forceinline__ void want_rows_body(Selected selected, u64 n, const u64* __restrict__ block_cnt, u64* __restrict__ want_rows) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u32 sel = 0;
    u64 cnt = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
        if (base + k < n && selected(base + k)) { sel |= 1u << k; ++cnt; }
    u64 at = plan_first(cnt, block_cnt);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
        if (sel & (1u << k)) want_rows[at++] = base + k;
}

}  // namespace mi
