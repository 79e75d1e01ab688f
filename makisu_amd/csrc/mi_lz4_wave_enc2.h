// mi_lz4_wave_enc2.h -- zpack LEVEL 2: the coder of one standard LZ4 block by ONE WAVE with a denser parse than
// mi_lz4_wave_enc.h's.  The stored form is the same block format: the decoder (mi_lz4_wave.h), the host check
// (host_lz4.h) and everything that moves stored spans know nothing of levels.  A chunk's stored form is a pure function of its
// bytes AND THE LEVEL; tests/zpack2_cases.py is the parse's model, which this file reproduces byte for byte.
//
//   the parse   level 1's frame: STEPS of 64 consecutive positions [p, p + 64) capped at n - 12, every lane reads the tables AS
//               THEY WERE BEFORE THE STEP, insertion by atomicMax (the greater position wins a slot: the order the hardware writes
//               LDS in does not show), a match starts at or before n - 12 and ends at or before n - 5, offsets 1..65535, the
//               block is kept if it is smaller than n - (n >> 4), chunks under 13 bytes are raw.  Inside it:
//          (a)  TWO tables of 4 096 32-bit positions in LDS (32 KiB, cleared per chunk; the workgroup IS the wave): t4 keyed by
//               (u32 at pos * 2654435761) >> 20, t8 by (u64 at pos * 0x9E3779B185EBCA87) >> 52.  A candidate c of either counts
//               if c < pos, pos - c <= 65535 and the 4 bytes at c and pos are equal;
//          (b)  every lane with a candidate measures each candidate's match length itself, capped at kZ2Cap = 4 + 64 and at
//               n - 5 - pos, keeps the longer and on a tie the greater source position;
//          (c)  f = the lowest lane with a candidate, L_f its length.  Among the lanes i in [f, f + L_f) with a candidate the one
//               with the greatest L_i - (i - f) wins, ties go to the lower lane (one max over a key that holds both).  A winner
//               at the cap is extended 64 bytes a ballot up to n - 5, as level 1 extends; then BACKWARDS, 64 bytes a ballot,
//               while the byte before the match equals the byte before the source, the match start is above `anchor` and the
//               source position above 0;
//          (d)  every position from p to the match's end (capped at n - 12) goes into both tables, 64 a round, the positions
//               inside the match included.
//               No candidate in a step: its positions go into both tables, the bytes stay pending literals.
//
// BOUNDS.  READS: src[pos .. pos + 7] with pos <= n - 12 (the two hashes); a lane's own length compares 8 bytes at a time only
// while l + 8 <= lmax with pos + lmax <= n - 5, and bytes from there on: below n - 5; the cooperative extension reads below
// n - 5, the backward one at and above `anchor` and source position 0; literals below n: all inside [src, src + n) at any byte
// alignment of src -- what follows the chunk in the arena is never read and cannot show.  The lanes' private length loops are
// bounded by the cap (8 rounds of 8 bytes for both candidates together, then at most 7 byte rounds each).  WRITES: below `cap`,
// checked per sequence -- a block that would pass it (none does with cap = z_worst_span(n), which bounds any parse with a
// minimum match of 4) is stored raw.
#pragma once

#include "mi_lz4_wave_enc.h"

namespace mi {

constexpr u32 kZ2Cap = 4 + 64;                                // a lane's own match length stops here; the wave takes over
constexpr u64 kZ2Mul8 = 0x9E3779B185EBCA87ull;

typedef u64 u64_unaligned __attribute__((aligned(1)));

// the match lengths of pos against its two candidates (each one's first 4 bytes are known to be equal; run4 / run8: measure it),
// at most lmax, pos + lmax <= n - 5.  8 bytes a round, BOTH candidates in one round (three loads in flight, the first differing
// byte from the xor's trailing zeros): eight rounds to the cap; then the bytes that are left below lmax, at most 7
static __device__ __forceinline__ void z2_lengths(const u8* __restrict__ src, u32 pos, u32 c4, u32 c8, bool run4, bool run8, u32 lmax,
                                                  u32* l4_out, u32* l8_out) {
    u32 l4 = 4, l8 = 4;
    for (u32 l = 4; l + 8 <= lmax && (run4 || run8); l += 8) {
        const u64 mine = *(const u64_unaligned*)(src + pos + l);
        if (run4) {
            const u64 x = mine ^ *(const u64_unaligned*)(src + c4 + l);
            l4 = l + (x ? (u32)(__ffsll((unsigned long long)x) - 1) >> 3 : 8u);
            run4 = x == 0;
        }
        if (run8) {
            const u64 x = mine ^ *(const u64_unaligned*)(src + c8 + l);
            l8 = l + (x ? (u32)(__ffsll((unsigned long long)x) - 1) >> 3 : 8u);
            run8 = x == 0;
        }
    }
    if (run4) while (l4 < lmax && src[pos + l4] == src[c4 + l4]) ++l4;
    if (run8) while (l8 < lmax && src[pos + l8] == src[c8 + l8]) ++l8;
    *l4_out = l4;
    *l8_out = l8;
}

// one sequence: lit literals from src + anchor, then (with a match) the offset and the match length's extension; false: it would
// pass cap
static __device__ __forceinline__ bool z2_put_sequence(const u8* __restrict__ src, u32 anchor, u32 lit, bool match, u32 offset, u32 ml,
                                                       u8* __restrict__ out, u64* op_io, u64 cap, int lane) {
    u64 op = *op_io;
    const u64 need = 1 + (lit >= 15 ? (lit - 15) / 255 + 1 : 0) + lit + (match ? 2 + (ml >= 15 ? (ml - 15) / 255 + 1 : 0) : 0);
    if (op + need > cap) return false;
    if (lane == 0) out[op] = (u8)(((lit < 15 ? lit : 15u) << 4) | (match ? (ml < 15 ? ml : 15u) : 0u));
    op += 1;
    if (lit >= 15) { z_put_extension(out + op, lit - 15, lane); op += (lit - 15) / 255 + 1; }
    for (u32 j = lane; j < lit; j += 64) out[op + j] = src[anchor + j];
    op += lit;
    if (match) {
        if (lane == 0) { out[op] = (u8)(offset & 255); out[op + 1] = (u8)(offset >> 8); }
        op += 2;
        if (ml >= 15) { z_put_extension(out + op, ml - 15, lane); op += (ml - 15) / 255 + 1; }
    }
    *op_io = op;
    return true;
}

// one chunk src[0, len) -> the LZ4 block out[0, stored), by one wave with `t4` and `t8` (kZTable words of LDS each) its own;
// returns `stored`: below len for a block that was kept, len for a chunk that stays raw (out then holds nothing of use)
static __device__ __forceinline__ u32 z_encode_block_l2(const u8* __restrict__ src, u32 len, u8* __restrict__ out, u64 cap, u32* t4, u32* t8,
                                                        int lane) {
    u32 stored = len;
    if (len >= kZMinChunk) {
        for (int i = lane; i < kZTable; i += 64) { t4[i] = 0; t8[i] = 0; }
        __syncthreads();
        const u32 last = len - 12, limit = len - 5;      // a match starts at or before `last` and ends at or before `limit`
        u32 p = 0, anchor = 0;
        u64 op = 0;
        bool fits = true;
        while (p <= last) {
            const u32 cnt = last + 1 - p < 64u ? last + 1 - p : 64u;
            const u32 pos = p + lane;
            const bool active = (u32)lane < cnt;
            u32 h4 = 0, h8 = 0, c4 = 0, c8 = 0;
            bool ok4 = false, ok8 = false;
            if (active) {
                const u32 v = *(const u32_unaligned*)(src + pos), v2 = *(const u32_unaligned*)(src + pos + 4);
                h4 = (v * 2654435761u) >> (32 - kZHashBits);
                h8 = (u32)(((((u64)v2 << 32) | v) * kZ2Mul8) >> (64 - kZHashBits));
                c4 = t4[h4];
                c8 = t8[h8];
                ok4 = c4 < pos && pos - c4 <= kZMaxOffset && *(const u32_unaligned*)(src + c4) == v;
                ok8 = c8 < pos && pos - c8 <= kZMaxOffset && *(const u32_unaligned*)(src + c8) == v;
            }
            const bool has = ok4 || ok8;
            const u64 m = __ballot(has);
            __syncthreads();                              // every lane has read the tables as they were before the step
            if (m == 0) {
                if (active) { atomicMax(&t4[h4], pos); atomicMax(&t8[h8], pos); }
                p += cnt;
                __syncthreads();
                continue;
            }
            u32 c = 0, lmine = 0;                         // this lane's candidate and its capped length
            if (has) {
                const u32 lmax = limit - pos < kZ2Cap ? limit - pos : kZ2Cap;
                const bool same = ok4 && ok8 && c8 == c4;
                u32 l4, l8;
                z2_lengths(src, pos, c4, c8, ok4, ok8 && !same, lmax, &l4, &l8);
                l4 = ok4 ? l4 : 0u;
                l8 = !ok8 ? 0u : same ? l4 : l8;
                const bool use8 = ok8 && (l8 > l4 || (l8 == l4 && c8 > c4));
                c = use8 ? c8 : c4;
                lmine = use8 ? l8 : l4;
            }
            const int f = z_first(m);
            const u32 lf = __shfl(lmine, f);
            // the greatest L_i - (i - f) among the lanes in [f, f + L_f) with a candidate, the lower lane on a tie: one max
            // over (score + 64) << 6 | 63 - lane (score >= 4 - 63)
            u32 key = 0;
            if (has && (u32)lane < (u32)f + lf) key = ((lmine + 64u - (u32)(lane - f)) << 6) | (u32)(63 - lane);
#pragma unroll
            for (int d = 32; d; d >>= 1) { const u32 o = __shfl_xor(key, d); key = o > key ? o : key; }
            const int w = 63 - (int)(key & 63u);
            u32 mpos = p + w, mc = __shfl(c, w), mlen = __shfl(lmine, w);
            if (mlen == kZ2Cap) {
                for (;;) {                                // 64 bytes a round, up to `limit`
                    const u32 i = mpos + mlen + lane;
                    const bool differs = i >= limit || src[i] != src[mc + mlen + lane];
                    const u64 d = __ballot(differs);
                    if (d == 0) { mlen += 64; continue; }
                    mlen += z_first(d);
                    break;
                }
            }
            for (;;) {                                    // backwards into the pending literals, 64 bytes a round
                const u32 k = lane + 1;
                const bool stops = mpos - anchor < k || mc < k || src[mpos - k] != src[mc - k];
                const u64 d = __ballot(stops);
                const u32 back = d == 0 ? 64u : (u32)z_first(d);
                mpos -= back;
                mc -= back;
                mlen += back;
                if (back < 64) break;
            }
            if (!z2_put_sequence(src, anchor, mpos - anchor, true, mpos - mc, mlen - 4, out, &op, cap, lane)) { fits = false; break; }
            const u32 next = mpos + mlen, end = next < last + 1 ? next : last + 1;
            if (active && pos < end) { atomicMax(&t4[h4], pos); atomicMax(&t8[h8], pos); }
            for (u32 q = pos + 64; q < end && q >= 64; q += 64) {   // the positions of the match beyond the step (q >= 64: no wrap)
                const u32 v = *(const u32_unaligned*)(src + q), v2 = *(const u32_unaligned*)(src + q + 4);
                atomicMax(&t4[(v * 2654435761u) >> (32 - kZHashBits)], q);
                atomicMax(&t8[(u32)(((((u64)v2 << 32) | v) * kZ2Mul8) >> (64 - kZHashBits))], q);
            }
            p = anchor = next;
            __syncthreads();
        }
        // the last sequence: literals only (at least 5)
        if (fits && z2_put_sequence(src, anchor, len - anchor, false, 0, 0, out, &op, cap, lane) && op < (u64)(len - (len >> 4))) stored = (u32)op;
        __syncthreads();                                  // the next chunk clears the tables
    }
    return stored;
}

}  // namespace mi
