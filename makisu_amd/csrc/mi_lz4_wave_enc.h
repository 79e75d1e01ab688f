// mi_lz4_wave_enc.h -- the coder of one standard LZ4 block by ONE WAVE: what zpack_encode_kernel (mi_zpack.hip: the
// chunks of a plain pack) and zbatch_encode_kernel (mi_zbatch.hip: the chunks where they lie in a batch's arena) both call.  The
// parse exists once, as the decoder does (mi_lz4_wave.h): a chunk's stored form is a pure function of its bytes, whoever codes it.
//
//   the parse   a hash table of 4 096 32-bit positions in LDS (16 KiB, cleared per chunk; the workgroup IS the wave).  The wave
//               advances in STEPS of 64 consecutive positions [p, p + 64), capped at n - 12: lane i reads its 4 bytes and the slot
//               (u32 * 2654435761) >> 20 AS THE TABLE WAS BEFORE THE STEP.  A candidate c counts if c < pos, pos - c <= 65535 and
//               the 4 bytes are equal (a table of zeros needs no "empty" mark).  No candidate: all 64 positions go into the table,
//               the bytes stay pending literals.  Otherwise the LOWEST lane with a candidate wins (one ballot), the match is
//               extended 64 bytes a round up to n - 5, the sequence is written (lane 0: token and offset; the wave: extension
//               bytes and literals), p becomes the match's end and the step's positions BELOW the new p go into the table.  Two
//               lanes of a step in one slot: the greater position wins (atomicMax: the order the hardware writes LDS in does not
//               show).  The block is kept if it is smaller than n - (n >> 4); chunks under 13 bytes are raw.
//
// BOUNDS.  READS: src[pos .. pos + 3] with pos <= n - 12 and match bytes below n - 5, literals below n: inside [src, src + n), at
// any byte alignment of src (unaligned dword and byte loads).  WRITES: below `cap`, checked per sequence -- a block that would
// pass it (none does with cap = z_worst_span(n)) is stored raw.
#pragma once

#include "mi_common.h"
#include "mi_lz4_wave.h"
#include "mi_wave.h"

namespace mi {

// what one chunk of n bytes takes in scratch: the LZ4 bound for a block of literals, on the 16-byte grid
__host__ __device__ static inline u64 z_worst_span(u64 n) { return round16(n + n / 255 + 16); }

typedef u32 u32_unaligned __attribute__((aligned(1)));

constexpr int kZHashBits = 12;
constexpr int kZTable = 1 << kZHashBits;                      // 32-bit positions: 16 KiB a wave
constexpr u32 kZMinChunk = 13;                                // below: raw
constexpr u32 kZMaxOffset = 65535;

// `count` extension bytes for the value e behind a nibble of 15 (count = e / 255 + 1), by the wave
static __device__ __forceinline__ void z_put_extension(u8* out, u32 e, int lane) {
    const u32 count = e / 255 + 1;
    for (u32 j = lane; j < count; j += 64) out[j] = j + 1 < count ? (u8)255 : (u8)(e % 255);
}

// one chunk src[0, len) -> the LZ4 block out[0, stored), by one wave with `table` (kZTable words of LDS) its own; returns
// `stored`: below len for a block that was kept, len for a chunk that stays raw (out then holds nothing of use)
static __device__ __forceinline__ u32 z_encode_block(const u8* __restrict__ src, u32 len, u8* __restrict__ out, u64 cap, u32* table, int lane) {
    u32 stored = len;
    if (len >= kZMinChunk) {
        for (int i = lane; i < kZTable; i += 64) table[i] = 0;
        __syncthreads();
        const u32 last = len - 12, limit = len - 5;      // a match starts at or before `last` and ends at or before `limit`
        u32 p = 0, anchor = 0;
        u64 op = 0;
        bool fits = true;
        while (p <= last) {
            const u32 cnt = last + 1 - p < 64u ? last + 1 - p : 64u;
            const u32 pos = p + lane;
            const bool active = (u32)lane < cnt;
            u32 v = 0, h = 0, c = 0;
            bool ok = false;
            if (active) {
                v = *(const u32_unaligned*)(src + pos);
                h = (v * 2654435761u) >> (32 - kZHashBits);
                c = table[h];
                ok = c < pos && pos - c <= kZMaxOffset && *(const u32_unaligned*)(src + c) == v;
            }
            const u64 m = __ballot(ok);
            __syncthreads();                              // every lane has read the table as it was before the step
            if (m == 0) {
                if (active) atomicMax(&table[h], pos);
                p += cnt;
                __syncthreads();
                continue;
            }
            const int f = z_first(m);
            const u32 mpos = p + f, mc = __shfl(c, f);
            u32 mlen = 4;
            for (;;) {                                    // 64 bytes a round; mpos + 4 < limit, so the first round has a lane inside
                const u32 i = mpos + mlen + lane;
                const bool differs = i >= limit || src[i] != src[mc + mlen + lane];
                const u64 d = __ballot(differs);
                if (d == 0) { mlen += 64; continue; }
                mlen += z_first(d);
                break;
            }
            const u32 lit = mpos - anchor, ml = mlen - 4;
            const u64 need = 1 + (lit >= 15 ? (lit - 15) / 255 + 1 : 0) + lit + 2 + (ml >= 15 ? (ml - 15) / 255 + 1 : 0);
            if (op + need > cap) { fits = false; break; }
            if (lane == 0) out[op] = (u8)(((lit < 15 ? lit : 15u) << 4) | (ml < 15 ? ml : 15u));
            op += 1;
            if (lit >= 15) { z_put_extension(out + op, lit - 15, lane); op += (lit - 15) / 255 + 1; }
            for (u32 j = lane; j < lit; j += 64) out[op + j] = src[anchor + j];
            op += lit;
            if (lane == 0) { out[op] = (u8)((mpos - mc) & 255); out[op + 1] = (u8)((mpos - mc) >> 8); }
            op += 2;
            if (ml >= 15) { z_put_extension(out + op, ml - 15, lane); op += (ml - 15) / 255 + 1; }
            const u32 next = mpos + mlen;
            if (active && pos < next) atomicMax(&table[h], pos);
            p = anchor = next;
            __syncthreads();
        }
        const u32 lit = len - anchor;                     // the last sequence: literals only (at least 5)
        const u64 need = 1 + (lit >= 15 ? (lit - 15) / 255 + 1 : 0) + lit;
        if (fits && op + need <= cap) {
            if (lane == 0) out[op] = (u8)((lit < 15 ? lit : 15u) << 4);
            op += 1;
            if (lit >= 15) { z_put_extension(out + op, lit - 15, lane); op += (lit - 15) / 255 + 1; }
            for (u32 j = lane; j < lit; j += 64) out[op + j] = src[anchor + j];
            op += lit;
            if (op < (u64)(len - (len >> 4))) stored = (u32)op;
        }
        __syncthreads();                                  // the next chunk clears the table
    }
    return stored;
}

}  // namespace mi
