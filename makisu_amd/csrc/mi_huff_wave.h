// mi_huff_wave.h -- the zpack entropy stage BY ONE WAVE (include/makisu_mi.h FORMAT): form H coded from the form
// under it (zh_encode_row) and unwrapped into it again (zh_unwrap_row), under host_huff.h's rules and numbers.  The kernels are
// mi_zentropy.hip's; the LZ4 kernels (mi_lz4_wave.h and its callers) know nothing of this file and keep their resources.
//
//   encode   the 256 counts of the inner bytes in LDS; the symbols that occur ranked by (count, symbol) -- every lane ranks four
//            symbols against all 256; lane 0 runs the two-queue merge over the ranked leaves (at most 255 merges), clamps the
//            depths to 11 and repairs the Kraft sum (tests/zentropy_cases.py states the rule; it is restated at zh_code_lengths),
//            and assigns the canonical codes.  Lane s < 32 sums the bits of stream s (the symbols s, s + 32, ...), a wave scan gives
//            the streams' places: THE FORM'S SIZE IS KNOWN BEFORE A BYTE OF IT IS WRITTEN, and a form that is not smaller than the
//            form under it by more than a sixteenth is never written.  Else lane s packs stream s through a 64-bit accumulator;
//   unwrap   the header is read by every lane alike and checked (rule 8); every lane takes four code lengths, the counts per
//            length go through LDS (rule 9); lane 0 assigns the canonical codes, the lanes fill the 2 048-entry table of their
//            symbols (symbol | length << 8, 0 = nobody's code); the stream sizes are summed (rule 10) and scanned; lane s < S
//            decodes stream s through the table, refilling its accumulator byte by byte BELOW THE STREAM'S END; in each round the
//            wave stores S consecutive bytes.  Rule 11 is a ballot over the lanes.
//
// LDS.  zh_unwrap_row: kZhUnwrapLds = 4 928 bytes -- the table (2 048 16-bit entries, 4 KiB) and 832 bytes beside it: 256 code
// lengths (256 bytes), 256 16-bit codes (512 bytes), 16 counts per length (64 bytes).  zh_encode_row: kZhEncodeLds = 5 376 bytes --
// 256 counts (1 KiB), 511 node weights (2 KiB, the last word unused), 512 16-bit parents (1 KiB), 256 ranked symbols and 256 codes
// as 16-bit words (1 KiB), 256 code lengths (256 bytes).
//
// BOUNDS.  encode READS inner[0, m) (m = the size of the form under it: the LZ4 block in its scratch span or the chunk in the
// pack) and WRITES out[0, h) with h = 136 + 64 + the streams' bytes < m - (m >> 4), computed before the first store; lane s
// writes [at_s, at_s + bytes_s), the exclusive scan of the sizes it counted with the lengths it packs with.  unwrap READS the
// header only after stored >= 8, the table and the sizes only after stored >= 136 + 2 S, stream s inside [at_s, at_s + size_s)
// where the sizes sum to EXACTLY stored - 136 - 2 S (checked first: rule 10) -- every byte load is guarded by ip < size; the pad
// check reads [stored, round16(stored)), inside the blob by the structural check of every add.  It WRITES inner[i] for
// i < inner length and zeroes up to round16(inner length), where inner length <= length <= 65 536 (rule 8) and the caller
// has checked that round16(inner length) bytes at `inner` are the row's own.
#pragma once

#include "host_huff.h"
#include "mi_common.h"
#include "mi_lz4_wave.h"
#include "mi_wave.h"

namespace mi {

typedef uint16_t u16;

constexpr u32 kZhMaxBits = mi_host::kHuffMaxBits;
constexpr u32 kZhTable = mi_host::kHuffTable;
constexpr u32 kZhStreams = mi_host::kHuffStreams;
constexpr u32 kZhHead = mi_host::kHuffHead;
constexpr u32 kZhMaxChunk = mi_host::kHuffMaxChunk;

// ---- the forms --------------------------------------------------------------------------------------------------------------------
enum : u32 { kZhRaw = 0, kZhLz4 = 1, kZhOverLz4 = 2, kZhOverRaw = 3 };

// a stored span's form, from its word (length | stored << 32) and its first bytes
static __device__ __forceinline__ u32 zh_form(const u8* src, u64 word) {
    const u64 len = word & 0xFFFFFFFFull, stored = word >> 32;
    if (stored >= len) return kZhRaw;
    if (src[0] != 0) return kZhLz4;
    // (a bad kind: rule 8 says so at the unwrap.  The census, makisu_mi.h "the census of a zpack's ... stored forms": a span that begins
    // like form H counts by its kind byte alone, 1 under [2], any other value -- or no kind byte at all, stored == 1 -- under [3])
    return stored >= 2 && src[1] == mi_host::kHuffKindLz4 ? kZhOverLz4 : kZhOverRaw;
}

// what a form H row takes in the unwrap's scratch: round16(inner length) if the header's length obeys rule 8, else 0 (the row is
// refused without a byte of scratch)
static __device__ __forceinline__ u64 zh_inner_need(const u8* src, u64 word) {
    const u64 len = word & 0xFFFFFFFFull, stored = word >> 32;
    if (stored < 8 || len > kZhMaxChunk) return 0;
    const u64 n = (u64)src[4] | ((u64)src[5] << 8) | ((u64)src[6] << 16) | ((u64)src[7] << 24);
    const bool fits = src[1] == mi_host::kHuffKindLz4 ? (n > 0 && n < len) : (src[1] == mi_host::kHuffKindRaw && n == len);
    return fits ? round16(n) : 0;
}

static __device__ __forceinline__ u32 zh_reverse(u32 v, u32 bits) { return __brev(v) >> (32 - bits); }

static __device__ __forceinline__ u32 zh_wave_exclusive_u32(u32 v, int lane, u32* total) {
    u32 x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    *total = __shfl(x, 63);
    return x - v;
}

// ---- unwrap -------------------------------------------------------------------------------------------------------------------------
constexpr u32 kZhUnwrapLds = 2 * kZhTable + 256 + 2 * 256 + 4 * 16;
struct ZhUnwrapLds {
    u16 table[kZhTable];
    u16 code[256];
    u32 count[16];
    u8 len[256];
};
static_assert(sizeof(ZhUnwrapLds) == kZhUnwrapLds, "what the file header states");

// one form H src[0, stored) of a chunk of `length` bytes -> inner[0, *n_out) with zeroes up to round16(*n_out), *kind_out; 0 or
// the rule (8..11).  `room`: the bytes at `inner` that are this row's
static __device__ __forceinline__ u32 zh_unwrap_row(const u8* __restrict__ src, u64 stored, u64 length, u8* __restrict__ inner, u64 room,
                                                    u32* n_out, u32* kind_out, ZhUnwrapLds* lds, int lane) {
    if (stored < 8 || length > kZhMaxChunk) return mi_host::kHuffHeader;
    const u32 kind = src[1], s_minus = src[2];
    const u64 n = (u64)src[4] | ((u64)src[5] << 8) | ((u64)src[6] << 16) | ((u64)src[7] << 24);
    if (src[0] != 0 || (kind != mi_host::kHuffKindLz4 && kind != mi_host::kHuffKindRaw) || s_minus >= mi_host::kHuffMaxStreams || src[3] != 0)
        return mi_host::kHuffHeader;
    if (kind == mi_host::kHuffKindLz4 ? (n == 0 || n >= length) : n != length) return mi_host::kHuffHeader;
    const u32 streams = s_minus + 1;
    const u64 body = kZhHead + 2 * streams;
    if (stored < body || round16(n) > room) return mi_host::kHuffHeader;
    // the code: four lengths a lane
    if (lane < 16) lds->count[lane] = 0;
    for (int i = lane; i < (int)kZhTable / 2; i += 64) ((u32*)lds->table)[i] = 0;
    __syncthreads();
    const u32 b0 = src[8 + 2 * lane], b1 = src[8 + 2 * lane + 1];
    const u32 l4[4] = {b0 & 15, b0 >> 4, b1 & 15, b1 >> 4};
    bool over = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        over = over || l4[q] > kZhMaxBits;
        lds->len[4 * lane + q] = (u8)l4[q];
        if (l4[q]) atomicAdd(&lds->count[l4[q]], 1u);
    }
    __syncthreads();
    u32 kraft = 0;
    for (u32 l = 1; l <= kZhMaxBits; ++l) kraft += lds->count[l] << (kZhMaxBits - l);
    const bool bad_code = __ballot(over) != 0 || kraft == 0 || kraft > kZhTable;
    __syncthreads();                                  // every lane has read the counts: lane 0 reuses them below
    if (bad_code) return mi_host::kHuffCode;
    if (lane == 0) {                                  // canonical codes by (length, symbol): count[l] becomes the next code of length l
        u32 code = 0, before = 0;
        for (u32 l = 1; l <= kZhMaxBits; ++l) {
            code = (code + before) << 1;
            before = lds->count[l];
            lds->count[l] = code;
        }
        for (u32 s = 0; s < 256; ++s) {
            const u32 l = lds->len[s];
            if (l) lds->code[s] = (u16)zh_reverse(lds->count[l]++, l);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u32 l = l4[q], s = 4 * lane + q;
        if (!l) continue;
        for (u32 i = lds->code[s]; i < kZhTable; i += 1u << l) lds->table[i] = (u16)(s | (l << 8));
    }
    // the streams' sizes and places
    const u32 size = (u32)lane < streams ? (u32)src[kZhHead + 2 * lane] | ((u32)src[kZhHead + 2 * lane + 1] << 8) : 0u;
    u32 sum = 0;
    const u32 at = zh_wave_exclusive_u32(size, lane, &sum);
    __syncthreads();                                  // the table is whole
    if ((u64)sum != stored - body) return mi_host::kHuffSizes;
    bool bad = false;
    if ((u32)lane < streams) {
        const u8* p = src + body + at;                // [p, p + size): inside the span, the sizes sum to its rest
        u64 acc = 0;
        u32 have = 0, ip = 0;
        for (u64 i = lane; i < n; i += streams) {
            while (have <= 56 && ip < size) { acc |= (u64)p[ip++] << have; have += 8; }
            const u32 e = lds->table[(u32)acc & (kZhTable - 1)], l = e >> 8;
            if (l == 0 || l > have) { bad = true; break; }
            inner[i] = (u8)e;
            acc >>= l;
            have -= l;
        }
        bad = bad || ip != size || have >= 8 || acc != 0;
    }
    if (__ballot(bad) != 0) return mi_host::kHuffBits;
    if (n + lane < round16(n)) inner[n + lane] = 0;
    *n_out = (u32)n;
    *kind_out = kind;
    return 0;
}

// ---- encode -------------------------------------------------------------------------------------------------------------------------
struct ZhEncodeLds {
    u32 count[256];
    u32 weight[512];                                  // the leaves in rank order, the merged nodes behind them; then the depths
    u16 parent[512];
    u16 ranked[256];                                  // the symbols that occur, by (count, symbol)
    u16 code[256];
    u8 len[256];
};
constexpr u32 kZhEncodeLds = 1024 + 2048 + 1024 + 512 + 512 + 256;
static_assert(sizeof(ZhEncodeLds) == kZhEncodeLds, "what the file header states");

// THE CODE LENGTHS (tests/zentropy_cases.py code_lengths), by lane 0 over the ranked leaves:
//   1. one leaf: length 1;   2. the two-queue merge, the lighter front twice, the LEAF on a tie; a leaf's length is its depth;
//   3. lengths above 11 become 11;   4. while the Kraft sum is above 2^11: of the leaves shorter than 11 bits the longest -- on a
//   tie the first in rank order -- grows by one bit.
static __device__ __forceinline__ void zh_code_lengths(ZhEncodeLds* lds, u32 n) {
    for (u32 s = 0; s < 256; ++s) lds->len[s] = 0;
    if (n == 1) { lds->len[lds->ranked[0]] = 1; return; }
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
    u32 kraft = 0;
    for (u32 k = 0; k < n; ++k) {
        if (lds->weight[k] > kZhMaxBits) lds->weight[k] = kZhMaxBits;
        kraft += 1u << (kZhMaxBits - lds->weight[k]);
    }
    while (kraft > kZhTable) {
        u32 best = n;
        for (u32 k = 0; k < n; ++k)
            if (lds->weight[k] < kZhMaxBits && (best == n || lds->weight[k] > lds->weight[best])) best = k;
        lds->weight[best] += 1;
        kraft -= 1u << (kZhMaxBits - lds->weight[best]);
    }
    for (u32 k = 0; k < n; ++k) lds->len[lds->ranked[k]] = (u8)lds->weight[k];
}

// the form under it inner[0, m) -> form H at out[0, h) if h < m - (m >> 4); returns h, or 0 for a form that is not kept (out is
// then not written)
static __device__ __forceinline__ u32 zh_encode_row(const u8* __restrict__ inner, u32 m, u32 kind, u8* __restrict__ out, ZhEncodeLds* lds, int lane) {
    const u32 bound = m - (m >> 4);
    if (bound <= kZhHead + 2 * kZhStreams) return 0;  // (header, table and sizes alone are no smaller)
#pragma unroll
    for (int q = 0; q < 4; ++q) lds->count[lane + 64 * q] = 0;
    __syncthreads();
    for (u32 i = lane; i < m; i += 64) atomicAdd(&lds->count[inner[i]], 1u);
    __syncthreads();
    u32 mine = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {                     // the rank of symbol s among those that occur, by (count, symbol)
        const u32 s = lane + 64 * q, c = lds->count[s];
        if (!c) continue;
        u32 rank = 0;
        for (u32 t = 0; t < 256; ++t) {
            const u32 ct = lds->count[t];
            rank += ct && (ct < c || (ct == c && t < s)) ? 1 : 0;
        }
        lds->ranked[rank] = (u16)s;
        lds->weight[rank] = c;
        ++mine;
    }
    const u32 n_sym = (u32)wave_sum(mine);
    __syncthreads();
    if (lane == 0) {
        zh_code_lengths(lds, n_sym);
        u32 per[kZhMaxBits + 2] = {};
        for (u32 s = 0; s < 256; ++s) ++per[lds->len[s]];
        u32 code = 0, before = 0;
        for (u32 l = 1; l <= kZhMaxBits; ++l) {       // per[l] becomes the next code of length l
            code = (code + before) << 1;
            before = per[l];
            per[l] = code;
        }
        for (u32 s = 0; s < 256; ++s) {
            const u32 l = lds->len[s];
            lds->code[s] = l ? (u16)zh_reverse(per[l]++, l) : (u16)0;
        }
    }
    __syncthreads();
    u32 bits = 0;
    if ((u32)lane < kZhStreams)
        for (u32 i = lane; i < m; i += kZhStreams) bits += lds->len[inner[i]];
    const u32 bytes = (bits + 7) >> 3;
    u32 sum = 0;
    const u32 at = zh_wave_exclusive_u32(bytes, lane, &sum);
    const u32 body = kZhHead + 2 * kZhStreams, h = body + sum;
    if (h >= bound) { __syncthreads(); return 0; }
    if (lane == 0) {
        out[0] = 0; out[1] = (u8)kind; out[2] = (u8)(kZhStreams - 1); out[3] = 0;
        out[4] = (u8)m; out[5] = (u8)(m >> 8); out[6] = (u8)(m >> 16); out[7] = (u8)(m >> 24);
    }
    out[8 + 2 * lane] = (u8)(lds->len[4 * lane] | (lds->len[4 * lane + 1] << 4));
    out[8 + 2 * lane + 1] = (u8)(lds->len[4 * lane + 2] | (lds->len[4 * lane + 3] << 4));
    if ((u32)lane < kZhStreams) {
        out[kZhHead + 2 * lane] = (u8)bytes;
        out[kZhHead + 2 * lane + 1] = (u8)(bytes >> 8);
        u8* p = out + body + at;                      // [p, p + bytes): this lane's
        u64 acc = 0;
        u32 have = 0, op = 0;
        for (u32 i = lane; i < m; i += kZhStreams) {
            const u32 s = inner[i];
            acc |= (u64)lds->code[s] << have;         // have <= 7 here: 11 more bits fit
            have += lds->len[s];
            while (have >= 8) { p[op++] = (u8)acc; acc >>= 8; have -= 8; }
        }
        if (have) p[op++] = (u8)acc;                  // the pad bits are zero: nothing was shifted in above them
    }
    __syncthreads();                                  // the next row clears the counts
    return h;
}

}  // namespace mi
