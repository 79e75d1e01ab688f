// mi_zrows.h -- what the two producers of a freshly coded zpack share around the coder (mi_zpack.hip: mi_pack_compress, from a
// plain pack's blob; mi_zbatch.hip: mi_batch_zpack_chunks, from a batch's arena; mi_zpack2.hip: the level-2 kernel of both): the
// encode loop over the rows, and the layout of the stored forms -- mi_plan.h's plan over round16(stored), and the placing pass
// that gives every entry its blob offset and its gather source.  The producers differ in the base the rows' offsets count
// from and in where their totals lie; each kernel keeps its own tables in LDS and its own launch bounds.
#pragma once

#include "mi_plan.h"
#include "mi_lz4_wave_enc.h"
#include "mi_lz4_wave_enc2.h"

namespace mi {

// the coder of a level over its tables in LDS: kZTable words (level 1), t4 | t8 of kZTable words each (level 2)
struct ZLevel1 {
    static __device__ __forceinline__ u32 encode(const u8* __restrict__ src, u32 len, u8* __restrict__ out, u64 cap, u32* tables, int lane) {
        return z_encode_block(src, len, out, cap, tables, lane);
    }
};
struct ZLevel2 {
    static __device__ __forceinline__ u32 encode(const u8* __restrict__ src, u32 len, u8* __restrict__ out, u64 cap, u32* tables, int lane) {
        return z_encode_block_l2(src, len, out, cap, tables, tables + kZTable, lane);
    }
};

// one wave an entry, the workgroup is the wave, grid-stride.  rows[k]: digest | the chunk's offset from `base` | chunk_index |
// length (the high half is written here: stored); the stored form goes to scratch + w_off[k], the entry's worst-case span
template <class Coder>
static __device__ __forceinline__ void z_encode_rows(const u8* __restrict__ base, u64* __restrict__ rows, const u64* __restrict__ w_off,
                                                     u8* __restrict__ scratch, u64 n, u32* tables) {
    const int lane = threadIdx.x;
    for (u64 k = blockIdx.x; k < n; k += gridDim.x) {
        const u64* r = rows + kEntryWords * k;
        const u32 len = (u32)r[6];
        const u32 stored = Coder::encode(base + r[4], len, scratch + w_off[k], z_worst_span(len), tables, lane);
        if (lane == 0) rows[kEntryWords * k + 6] = (u64)len | ((u64)stored << 32);
    }
}

// per block of kPlanTile entries: the rounded-up stored bytes; into the totals: stored bytes, raw entries and, with kChunk,
// chunk bytes
template <bool kChunk>
static __device__ __forceinline__ void z_layout_sums(const u64* __restrict__ rows, u64 n, u64* __restrict__ block_bytes, u64* __restrict__ totals,
                                                     int i_stored, int i_raw, int i_chunk) {
    constexpr int Q = kChunk ? 4 : 3;
    __shared__ u64 lds[Q][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[Q] = {};                                    // rounded-up stored bytes, stored bytes, raw entries, chunk bytes
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (base + k >= n) continue;
        const u64 w = rows[kEntryWords * (base + k) + 6];
        const u64 len = w & 0xFFFFFFFFull, stored = w >> 32;
        v[0] += round16(stored);
        v[1] += stored;
        v[2] += stored == len ? 1 : 0;
        if (kChunk) v[Q - 1] += len;
    }
    plan_block_sum<Q>(v, lds);
    if (threadIdx.x == 0) {
        block_bytes[blockIdx.x] = v[0];
        if (v[1]) atomicAdd((unsigned long long*)&totals[i_stored], (unsigned long long)v[1]);
        if (v[2]) atomicAdd((unsigned long long*)&totals[i_raw], (unsigned long long)v[2]);
        if (kChunk && v[Q - 1]) atomicAdd((unsigned long long*)&totals[i_chunk], (unsigned long long)v[Q - 1]);
    }
}

// every entry's place in the new blob, where its stored form lies now as an absolute device address (a raw chunk: at raw_base +
// the row's offset word, where the coder read it; a coded one: in its scratch span) and the row's offset word: from here on the
// rows are the zpack's entries
static __device__ __forceinline__ void z_place(u64* __restrict__ rows, const u64* __restrict__ w_off, u64 n, const u64* __restrict__ block_bytes,
                                               u64 raw_base, u64 scratch_base, u64* __restrict__ e_src, u64* __restrict__ e_len,
                                               u64* __restrict__ e_dst) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 stored[kPlanPer], len[kPlanPer];
    u64 bytes = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const u64 w = base + k < n ? rows[kEntryWords * (base + k) + 6] : 0;
        len[k] = w & 0xFFFFFFFFull;
        stored[k] = w >> 32;
        bytes += round16(stored[k]);
    }
    u64 dst = plan_first(bytes, block_bytes);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const u64 row = base + k;
        if (row >= n) continue;
        u64* r = rows + kEntryWords * row;
        e_src[row] = stored[k] == len[k] ? raw_base + r[4] : scratch_base + w_off[row];
        e_len[row] = stored[k];
        e_dst[row] = dst;
        r[4] = dst;
        dst += round16(stored[k]);
    }
}

}  // namespace mi
