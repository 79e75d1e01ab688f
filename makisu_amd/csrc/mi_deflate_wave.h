// mi_deflate_wave.h -- one PIECE of the layer writer's device deflate leg BY ONE WAVE (include/makisu_mi.h FORMAT "the
// device deflate leg"): the plan of a piece (df_plan_piece: parse, counts, the three codes, the header, THE SIZE) and its emit at
// the final offset (df_emit_piece).  The kernels are mi_deflate.hip's.  tests/deflate_cases.py states every rule and is the
// model the bytes are held against; the rules are restated where they are coded.
//
//   pieces      65 536 bytes of the input, the last one shorter; a piece knows nothing of its neighbours.  Stored form (D): one
//               dynamic-Huffman block (BFINAL 0) and an empty stored block (Z_SYNC_FLUSH's: 000, zero bits to the byte, 00 00 FF FF);
//               or (S): stored blocks of at most 65 535 bytes.  (D) is kept where it is SMALLER than (S), decided in the plan: a
//               (D) form that is not kept is never written.  No fixed-Huffman block, no BFINAL.
//   the parse   mi_lz4_wave_enc.h's step rule with a table of 4 096 32-bit positions in LDS (16 KiB, cleared per piece; the
//               positions would fit 16 bits, but atomicMax is a 32-bit LDS instruction): steps of 64 consecutive positions capped
//               at n - 4, the table read as it was before the step, a candidate c counts if c < pos, pos - c <= 32 768 and the 4
//               bytes are equal, the lowest lane with a candidate wins, the match is extended 64 bytes a round TO THE PIECE'S END
//               (LZ4's n - 12 and n - 5 restrictions are gone: deflate has none), positions go into the table by atomicMax.
//   the split   a match of L >= 4 bytes: (L - 3) / 258 matches of 258, the rest r = L - 258 * that (3 <= r <= 260) as one match,
//               or -- r = 259, 260 -- as r - 3 and 3.  No part is shorter than 3.
//   the items   the parse runs ONCE: every literal and every deflate match goes into the piece's scratch as one 32-bit ITEM
//               (literal: the byte; match: bit 31 | (length - 3) << 15 | (distance - 1)), counted in LDS as it is written.  An
//               item covers at least one byte: AT MOST n ITEMS, 4 n bytes of scratch a piece (256 KiB for a full one).  Chosen
//               over a second parse because the emit then is one uniform loop -- 64 items a round, no table, no match search --
//               and the parse's global loads are paid once.
//   the codes   df_code_lengths: a length-limited COMPLETE canonical code by lane 0 over the ranked leaves (limits 15, 15, 7);
//               the header's greedy run rule with 16, 17 and 18 (df_header).
//   the emit    a second kernel, at the piece's FINAL offset (mi_plan.h's scan over the sizes): the code lengths (320 bytes) and
//               the header's bits (at most 80 words) wait in scratch.  Per round every lane takes one item -- a literal's code, or
//               length code + extra + distance code + extra, at most 48 bits --, a wave scan of the bit counts places them, the
//               bits are OR-ed into a staging buffer in LDS and the whole words go to global memory.
//
// LDS.  df_plan_piece: kDfPlanLds = 23 088 bytes -- the table (16 384), 320 counts (1 280), 576 node weights (2 304), 576 16-bit
// parents (1 152), 288 ranked symbols (576), 320 code lengths (320), the code-length code's 20 counts (80) and 32 bytes for its
// lengths, 320 header symbols (640), 80 header words (320).  df_emit_piece: kDfEmitLds = 1 440 bytes -- 320 16-bit codes (640),
// 320 lengths (320), 16 next-code words (64), 104 staging words (416).
//
// BOUNDS.  plan READS src[pos .. pos + 3] with pos <= n - 4, match bytes below n, literals below n: inside [src, src + n) at any
// alignment (unaligned dword and byte loads).  It WRITES items[k] with k < the item count <= n <= 65 536 (the piece's own 65 536
// slots), and the piece's own meta, lengths and header rows.  LDS: table[h] with h < 4 096 (a 12-bit hash); count[] by a byte,
// by a length symbol <= 285 or by 288 + a distance symbol <= 29; the leaves and nodes of a code with at most 286 symbols below
// 576; header symbols at most 286 + 30 = 316 <= 320; header bits at most 17 + 57 + 316 * 7 = 2 286 <= 80 * 32.  emit READS the
// items below the count the plan stored and src as the plan did (form (S): dwords below the block's end, then bytes), and WRITES
// whole words only while they END at or below the piece's size and single bytes below it: inside the piece's own span
// [offset, offset + size) whatever the items hold.  Staging: a round adds at most 64 * 48 bits to at most 31 carried: 98 words.
#pragma once

#include "mi_common.h"
#include "mi_lz4_wave.h"
#include "mi_lz4_wave_enc.h"
#include "mi_huff_wave.h"
#include "mi_wave.h"

namespace mi {

constexpr u32 kDfPiece = 65536;
constexpr int kDfHashBits = 12;
constexpr int kDfTable = 1 << kDfHashBits;
constexpr u32 kDfMaxDist = 32768;
constexpr u32 kDfMaxLen = 258;
constexpr u32 kDfLitLen = 286, kDfDist = 30, kDfCl = 19, kDfEob = 256;
constexpr u32 kDfDistAt = 288;                                  // the distance symbols' place in the count and length rows
constexpr u32 kDfLens = 320;                                    // a piece's row of code lengths: 286 (+ 2) and 30 (+ 2)
constexpr u32 kDfHeaderWords = 80;
constexpr u32 kDfStage = 104;
constexpr u32 kDfItemMatch = 0x80000000u;

struct DfMeta { u32 size, n_items, header_bits, dynamic; };     // a piece's row of the plan

__host__ __device__ static inline u32 df_stored_size(u32 n) { return n + 5 * ((n + 65534) / 65535); }
// what dst must hold for any n bytes: every piece stored (two blocks for a full one)
__host__ __device__ static inline u64 df_bound(u64 n) { return n + 10 * ((n + kDfPiece - 1) / kDfPiece); }

struct DfPlanLds {
    u32 table[kDfTable];
    u32 count[kDfLens];
    u32 weight[576];                                  // the leaves in rank order, the merged nodes behind them; then the lengths
    u32 header[kDfHeaderWords];
    u32 clcount[20];
    u16 parent[576];
    u16 ranked[288];
    u16 hsym[kDfLens];                                // symbol | extra value << 8
    u8 len[kDfLens];
    u8 cllen[32];
};
constexpr u32 kDfPlanLds = 16384 + 1280 + 2304 + 320 + 80 + 1152 + 576 + 640 + 320 + 32;
static_assert(sizeof(DfPlanLds) == kDfPlanLds && kDfPlanLds == 23088, "what the file header states");

struct DfEmitLds {
    u32 stage[kDfStage];
    u32 next[16];
    u16 code[kDfLens];
    u8 len[kDfLens];
};
constexpr u32 kDfEmitLds = 416 + 64 + 640 + 320;
static_assert(sizeof(DfEmitLds) == kDfEmitLds, "what the file header states");

// ---- the codes ----------------------------------------------------------------------------------------------------------------------
// the symbols of count[0, nsym) that occur, ranked by (count, symbol): ranked[] and weight[]; returns how many.  nsym <= 320
static __device__ __forceinline__ u32 df_rank(const u32* count, u32 nsym, DfPlanLds* lds, int lane) {
    u32 mine = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const u32 s = lane + 64 * q;
        const u32 c = s < nsym ? count[s] : 0;
        if (!c) continue;
        u32 rank = 0;
        for (u32 t = 0; t < nsym; ++t) {
            const u32 ct = count[t];
            rank += ct && (ct < c || (ct == c && t < s)) ? 1 : 0;
        }
        lds->ranked[rank] = (u16)s;
        lds->weight[rank] = c;
        ++mine;
    }
    return (u32)wave_sum(mine);
}

// THE CODE LENGTHS (tests/deflate_cases.py code_lengths), by lane 0 over the n ranked leaves; weight[k] becomes leaf k's length:
//   1. one leaf: length 1;   2. the two-queue merge, the lighter front twice, the LEAF on a tie; a leaf's length is its depth;
//   3. lengths above the limit become the limit;   4. while the Kraft sum is above 2^limit: of the leaves shorter than the limit
//   the longest -- on a tie the first in rank order -- grows by one bit;   5. while it is below 2^limit by d: of the leaves whose
//   own term 2^(limit - length) is at most d the shortest -- on a tie the LAST in rank order -- shrinks by one bit.
static __device__ __forceinline__ void df_code_lengths(DfPlanLds* lds, u32 n, u32 limit) {
    if (n == 0) return;
    if (n == 1) { lds->weight[0] = 1; return; }
    u32 i = 0, j = n;
    for (u32 k = n; k < 2 * n - 1; ++k) {
        u32 w = 0;
        for (int t = 0; t < 2; ++t) {
            u32 take;
            if (i < n && (j >= k || lds->weight[i] <= lds->weight[j])) take = i++; else take = j++;
            w += lds->weight[take];
            lds->parent[take] = (u16)k;
        }
        lds->weight[k] = w;
    }
    lds->weight[2 * n - 2] = 0;                       // from here on: depths
    for (int k = (int)(2 * n - 3); k >= 0; --k) lds->weight[k] = lds->weight[lds->parent[k]] + 1;
    const u32 full = 1u << limit;
    u32 kraft = 0;
    for (u32 k = 0; k < n; ++k) {
        if (lds->weight[k] > limit) lds->weight[k] = limit;
        kraft += 1u << (limit - lds->weight[k]);
    }
    while (kraft > full) {
        u32 best = n;
        for (u32 k = 0; k < n; ++k)
            if (lds->weight[k] < limit && (best == n || lds->weight[k] > lds->weight[best])) best = k;
        if (best == n) break;                         // (n <= 2^limit leaves: there is one)
        lds->weight[best] += 1;
        kraft -= 1u << (limit - lds->weight[best]);
    }
    while (kraft < full) {
        const u32 d = full - kraft;
        u32 best = n;
        for (u32 k = 0; k < n; ++k)
            if ((1u << (limit - lds->weight[k])) <= d && (best == n || lds->weight[k] <= lds->weight[best])) best = k;
        if (best == n) break;                         // (a leaf of the greatest length qualifies: see the rule)
        kraft += 1u << (limit - lds->weight[best]);
        lds->weight[best] -= 1;
    }
}

// count[0, nsym) -> len[0, nsym), by the wave
static __device__ __forceinline__ void df_make_code(const u32* count, u32 nsym, u8* len, u32 limit, DfPlanLds* lds, int lane) {
    const u32 n = df_rank(count, nsym, lds, lane);
    for (u32 s = lane; s < nsym; s += 64) len[s] = 0;
    __syncthreads();
    if (lane == 0) df_code_lengths(lds, n, limit);
    __syncthreads();
    for (u32 k = lane; k < n; k += 64) len[lds->ranked[k]] = (u8)lds->weight[k];
    __syncthreads();
}

static __device__ __forceinline__ void df_put_serial(u32* words, u32* at, u32 value, u32 bits) {   // lane 0; bits <= 16
    const u32 w = *at >> 5, sh = *at & 31;
    words[w] |= value << sh;
    if (sh + bits > 32) words[w + 1] |= value >> (32 - sh);
    *at += bits;
}

// RFC 1951's order of the code-length code's lengths (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15), five bits each
static __device__ __forceinline__ u32 df_cl_order(u32 k) {
    return (u32)((k < 12 ? 0x22caa324e804a30ull >> (5 * k) : 0x3c2e1346cull >> (5 * (k - 12))) & 31);
}
static __device__ __forceinline__ u32 df_len_extra(u32 s) { return s >= 265 && s < 285 ? (s - 261) >> 2 : 0; }
static __device__ __forceinline__ u32 df_dist_extra(u32 s) { return s >= 4 ? (s >> 1) - 1 : 0; }

// THE HEADER (tests/deflate_cases.py header_symbols), by lane 0: len[] -> hsym[], the code-length code, header[]; returns its bits.
// At position i with value v and r equal values from i on:  v == 0, r >= 11: 18 for min(r, 138);  v == 0, r >= 3: 17 for r;
// v != 0, the value before i is v and r >= 3: 16 for min(r, 6);  else v itself.
static __device__ __forceinline__ u32 df_header(DfPlanLds* lds, int lane) {
    u32 hlit = 0, hdist = 0, nh = 0;
    if (lane < 20) lds->clcount[lane] = 0;
    for (u32 i = lane; i < kDfHeaderWords; i += 64) lds->header[i] = 0;
    __syncthreads();
    if (lane == 0) {
        hlit = kDfLitLen;
        while (hlit > 257 && lds->len[hlit - 1] == 0) --hlit;
        hdist = kDfDist;
        while (hdist > 1 && lds->len[kDfDistAt + hdist - 1] == 0) --hdist;
        const u32 total = hlit + hdist;
        u32 prev = 0xFFFFFFFFu;
        for (u32 i = 0; i < total;) {
            const u32 v = lds->len[i < hlit ? i : kDfDistAt + i - hlit];
            u32 r = 1;
            while (r < 138 && i + r < total && lds->len[i + r < hlit ? i + r : kDfDistAt + i + r - hlit] == v) ++r;
            u32 sym, ev, take;
            if (v == 0 && r >= 11)                 { sym = 18; take = r; ev = take - 11; }
            else if (v == 0 && r >= 3)             { sym = 17; take = r; ev = take - 3; }
            else if (v != 0 && prev == v && r >= 3) { sym = 16; take = r < 6 ? r : 6; ev = take - 3; }
            else                                   { sym = v; take = 1; ev = 0; }
            lds->hsym[nh++] = (u16)(sym | (ev << 8));
            lds->clcount[sym] += 1;
            prev = v;
            i += take;
        }
    }
    nh = __shfl(nh, 0);
    hlit = __shfl(hlit, 0);
    hdist = __shfl(hdist, 0);
    __syncthreads();
    df_make_code(lds->clcount, kDfCl, lds->cllen, 7, lds, lane);
    u32 bits = 0;
    if (lane == 0) {
        u32 hclen = 19;
        while (hclen > 4 && lds->cllen[df_cl_order(hclen - 1)] == 0) --hclen;
        df_put_serial(lds->header, &bits, 0, 1);
        df_put_serial(lds->header, &bits, 2, 2);
        df_put_serial(lds->header, &bits, hlit - 257, 5);
        df_put_serial(lds->header, &bits, hdist - 1, 5);
        df_put_serial(lds->header, &bits, hclen - 4, 4);
        for (u32 k = 0; k < hclen; ++k) df_put_serial(lds->header, &bits, lds->cllen[df_cl_order(k)], 3);
        // the canonical code-length codes by (length, symbol): clcount[s] becomes symbol s's code
        u32 code = 0;
        for (u32 l = 1; l <= 7; ++l) {
            for (u32 s = 0; s < kDfCl; ++s)
                if (lds->cllen[s] == l) lds->clcount[s] = zh_reverse(code++, l);
            code <<= 1;
        }
        for (u32 k = 0; k < nh; ++k) {
            const u32 sym = lds->hsym[k] & 255, ev = lds->hsym[k] >> 8;
            df_put_serial(lds->header, &bits, lds->clcount[sym], lds->cllen[sym]);
            if (sym >= 16) df_put_serial(lds->header, &bits, ev, sym == 16 ? 2 : sym == 17 ? 3 : 7);
        }
    }
    bits = __shfl(bits, 0);
    __syncthreads();
    return bits;
}

// ---- the plan of one piece ------------------------------------------------------------------------------------------------------------
// src[0, n), 0 < n <= 65 536 -> items[0, n_items), lens[0, 320), header[0, 80), *meta.  By one wave; the workgroup IS the wave
static __device__ __forceinline__ void df_plan_piece(const u8* __restrict__ src, u32 n, u32* __restrict__ items, u8* __restrict__ lens,
                                                     u32* __restrict__ header, DfMeta* __restrict__ meta, DfPlanLds* lds, int lane) {
    for (int i = lane; i < kDfTable; i += 64) lds->table[i] = 0;
    for (u32 i = lane; i < kDfLens; i += 64) lds->count[i] = 0;
    __syncthreads();
    u32 p = 0, anchor = 0, ni = 0;
    if (n >= 4) {
        const u32 last = n - 4;
        while (p <= last) {
            const u32 cnt = last + 1 - p < 64u ? last + 1 - p : 64u;
            const u32 pos = p + lane;
            const bool active = (u32)lane < cnt;
            u32 v = 0, h = 0, c = 0;
            bool ok = false;
            if (active) {
                v = *(const u32_unaligned*)(src + pos);
                h = (v * 2654435761u) >> (32 - kDfHashBits);
                c = lds->table[h];
                ok = c < pos && pos - c <= kDfMaxDist && *(const u32_unaligned*)(src + c) == v;
            }
            const u64 m = __ballot(ok);
            __syncthreads();                              // every lane has read the table as it was before the step
            if (m == 0) {
                if (active) atomicMax(&lds->table[h], pos);
                p += cnt;
                __syncthreads();
                continue;
            }
            const int f = z_first(m);
            const u32 mpos = p + f, mc = __shfl(c, f);
            u32 mlen = 4;
            for (;;) {                                    // 64 bytes a round, to the piece's end
                const u32 i = mpos + mlen + lane;
                const bool differs = i >= n || src[i] != src[mc + mlen + lane];
                const u64 d = __ballot(differs);
                if (d == 0) { mlen += 64; continue; }
                mlen += z_first(d);
                break;
            }
            const u32 lit = mpos - anchor;
            for (u32 j = lane; j < lit; j += 64) {
                const u32 b = src[anchor + j];
                items[ni + j] = b;
                atomicAdd(&lds->count[b], 1u);
            }
            ni += lit;
            // the split: `full` matches of 258, the rest as one match or as rest - 3 and 3
            const u32 full = (mlen - 3) / kDfMaxLen, rest = mlen - kDfMaxLen * full;
            const u32 parts = full + (rest > kDfMaxLen ? 2u : 1u);
            const u32 dist = mpos - mc;
            for (u32 j = lane; j < parts; j += 64) {
                const u32 l = j < full ? kDfMaxLen : j == full ? (rest > kDfMaxLen ? rest - 3 : rest) : 3u;
                items[ni + j] = kDfItemMatch | ((l - 3) << 15) | (dist - 1);
                const u32 q = l - 3;
                u32 sym;
                if (q == 255) sym = 285;
                else if (q < 8) sym = 257 + q;
                else { const u32 k = 31 - __clz(q); sym = 257 + 4 * (k - 1) + ((q >> (k - 2)) & 3); }
                atomicAdd(&lds->count[sym], 1u);
            }
            ni += parts;
            if (lane == 0) {
                const u32 d = dist - 1;
                u32 sym = d;
                if (d >= 4) { const u32 k = 31 - __clz(d); sym = 2 * k + ((d >> (k - 1)) & 1); }
                atomicAdd(&lds->count[kDfDistAt + sym], parts);
            }
            const u32 next = mpos + mlen;
            if (active && pos < next) atomicMax(&lds->table[h], pos);
            p = anchor = next;
            __syncthreads();
        }
    }
    const u32 lit = n - anchor;
    for (u32 j = lane; j < lit; j += 64) {
        const u32 b = src[anchor + j];
        items[ni + j] = b;
        atomicAdd(&lds->count[b], 1u);
    }
    ni += lit;
    if (lane == 0) lds->count[kDfEob] = 1;
    __syncthreads();
    df_make_code(lds->count, kDfLitLen, lds->len, 15, lds, lane);
    df_make_code(lds->count + kDfDistAt, kDfDist, lds->len + kDfDistAt, 15, lds, lane);
    if (lane < 2) { lds->len[kDfLitLen + lane] = 0; lds->len[kDfDistAt + kDfDist + lane] = 0; }
    __syncthreads();
    const u32 header_bits = df_header(lds, lane);
    u32 body = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const u32 s = lane + 64 * q;
        if (s < kDfLitLen) body += lds->count[s] * (lds->len[s] + df_len_extra(s));
        if (s < kDfDist) body += lds->count[kDfDistAt + s] * (lds->len[kDfDistAt + s] + df_dist_extra(s));
    }
    body = (u32)wave_sum(body);                        // (the end-of-block code is in it: its count is 1)
    const u32 d_size = (header_bits + body + 3 + 7) / 8 + 4, s_size = df_stored_size(n);
    const bool dynamic = d_size < s_size;
    for (u32 i = lane; i < kDfLens; i += 64) lens[i] = lds->len[i];
    for (u32 i = lane; i < kDfHeaderWords; i += 64) header[i] = lds->header[i];
    if (lane == 0) *meta = DfMeta{dynamic ? d_size : s_size, ni, header_bits, dynamic ? 1u : 0u};
    __syncthreads();
}

// ---- the emit of one piece ------------------------------------------------------------------------------------------------------------
struct DfOut { u8* out; u32 size; u32 bitpos; u32 flushed; };     // flushed: whole words already in global memory

// every lane's `bits` (<= 48) bits of `value`, in lane order, behind what the piece's stream holds
static __device__ __forceinline__ void df_put_wave(DfOut* o, u64 value, u32 bits, DfEmitLds* lds, int lane) {
    u32 total = 0;
    const u32 at = zh_wave_exclusive_u32(bits, lane, &total);
    if (bits) {
        const u32 rel = o->bitpos - 32 * o->flushed + at, w = rel >> 5, sh = rel & 31;
        const u64 a = (value & 0xFFFFFFFFull) << sh, b = (value >> 32) << sh;
        atomicOr(&lds->stage[w], (u32)a);
        const u32 w1 = (u32)(a >> 32) | (u32)b, w2 = (u32)(b >> 32);
        if (w1) atomicOr(&lds->stage[w + 1], w1);
        if (w2) atomicOr(&lds->stage[w + 2], w2);
    }
    o->bitpos += total;
    __syncthreads();
    const u32 nw = (o->bitpos >> 5) - o->flushed;      // whole words in the staging buffer
    const u32 carry = lds->stage[nw];
    for (u32 i = lane; i < nw; i += 64) {
        const u32 byte = 4 * (o->flushed + i);
        if (byte + 4 <= o->size) *(u32_unaligned*)(o->out + byte) = lds->stage[i];
    }
    __syncthreads();
    for (u32 i = lane; i <= nw; i += 64) lds->stage[i] = i == 0 ? carry : 0u;
    o->flushed += nw;
    __syncthreads();
}

// the piece src[0, n) with its plan -> out[0, meta.size).  By one wave
static __device__ __forceinline__ void df_emit_piece(const u8* __restrict__ src, u32 n, const u32* __restrict__ items, const u8* __restrict__ lens,
                                                     const u32* __restrict__ header, DfMeta meta, u8* __restrict__ out, DfEmitLds* lds, int lane) {
    if (!meta.dynamic) {                               // (S): as GzipSink::store writes it
        u32 at = 0;
        for (u32 done = 0; done < n;) {
            const u32 take = n - done < 65535u ? n - done : 65535u;
            if (lane < 5 && at + 5 <= meta.size)
                out[at + lane] = lane == 0 ? (u8)0 : lane == 1 ? (u8)take : lane == 2 ? (u8)(take >> 8) : lane == 3 ? (u8)~take : (u8)(~take >> 8);
            at += 5;
            const u32 whole = take & ~3u;
            for (u32 j = 4 * lane; j < whole; j += 256)
                if (at + j + 4 <= meta.size) *(u32_unaligned*)(out + at + j) = *(const u32_unaligned*)(src + done + j);
            if (whole + lane < take && at + whole + lane < meta.size) out[at + whole + lane] = src[done + whole + lane];
            at += take;
            done += take;
        }
        return;
    }
    for (u32 i = lane; i < kDfLens; i += 64) { lds->len[i] = lens[i]; lds->code[i] = 0; }
    for (u32 i = lane; i < kDfStage; i += 64) lds->stage[i] = 0;
    __syncthreads();
    if (lane == 0) {                                   // the canonical codes by (length, symbol), both alphabets
        for (u32 base = 0; base <= kDfDistAt; base += kDfDistAt) {
            const u32 nsym = base ? kDfDist : kDfLitLen;
            for (u32 l = 0; l < 16; ++l) lds->next[l] = 0;
            for (u32 s = 0; s < nsym; ++s) lds->next[lds->len[base + s] & 15] += 1;
            u32 code = 0, before = 0;
            for (u32 l = 1; l < 16; ++l) {
                code = (code + before) << 1;
                before = lds->next[l];
                lds->next[l] = code;
            }
            for (u32 s = 0; s < nsym; ++s) {
                const u32 l = lds->len[base + s] & 15;
                if (l) lds->code[base + s] = (u16)zh_reverse(lds->next[l]++, l);
            }
        }
    }
    __syncthreads();
    DfOut o{out, meta.size, 0, 0};
    const u32 hw = (meta.header_bits + 31) >> 5;
    for (u32 w0 = 0; w0 < hw && w0 < kDfHeaderWords; w0 += 64) {
        const u32 w = w0 + lane;
        const bool mine = w < hw && w < kDfHeaderWords;
        const u32 left = mine ? meta.header_bits - 32 * w : 0;
        df_put_wave(&o, mine ? header[w] : 0, left < 32 ? left : 32, lds, lane);
    }
    const u32 n_items = meta.n_items < kDfPiece ? meta.n_items : kDfPiece;
    for (u32 i0 = 0; i0 < n_items; i0 += 64) {
        u64 value = 0;
        u32 bits = 0;
        if (i0 + lane < n_items) {
            const u32 it = items[i0 + lane];
            if (it & kDfItemMatch) {
                const u32 q = (it >> 15) & 255, d = it & 32767;
                u32 ls, le = 0, ds = d, de = 0;
                if (q == 255) ls = 285;
                else if (q < 8) ls = 257 + q;
                else { const u32 k = 31 - __clz(q); le = k - 2; ls = 257 + 4 * (k - 1) + ((q >> (k - 2)) & 3); }
                if (d >= 4) { const u32 k = 31 - __clz(d); de = k - 1; ds = 2 * k + ((d >> (k - 1)) & 1); }
                const u32 ll = lds->len[ls], dl = lds->len[kDfDistAt + ds];
                value = (u64)lds->code[ls] | ((u64)(q & ((1u << le) - 1)) << ll) | ((u64)lds->code[kDfDistAt + ds] << (ll + le)) |
                        ((u64)(d & ((1u << de) - 1)) << (ll + le + dl));
                bits = ll + le + dl + de;
            } else {
                value = lds->code[it & 255];
                bits = lds->len[it & 255];
            }
        }
        df_put_wave(&o, value, bits, lds, lane);
    }
    // the end-of-block code and the empty stored block: 000, zero bits to the byte boundary, 00 00 FF FF
    df_put_wave(&o, lane == 0 ? lds->code[kDfEob] : 0, lane == 0 ? lds->len[kDfEob] + 3u : 0u, lds, lane);
    const u32 pad = (8 - (o.bitpos & 7)) & 7;
    df_put_wave(&o, 0, lane == 0 ? pad : 0u, lds, lane);
    df_put_wave(&o, lane == 0 ? 0xFFFF0000ull : 0ull, lane == 0 ? 32u : 0u, lds, lane);
    const u32 tail = (o.bitpos >> 3) - 4 * o.flushed;  // at most 3 bytes of a last word
    if ((u32)lane < tail && 4 * o.flushed + lane < o.size) out[4 * o.flushed + lane] = (u8)(lds->stage[0] >> (8 * lane));
    __syncthreads();
}

}  // namespace mi
