// mi_lz4_wave.h -- the decoder of one standard LZ4 block by ONE WAVE, under host_lz4.h's rules: what zpack_decode_kernel
// (mi_zpack.hip: a zpack into the plain layout of a pack) and zset_restore_kernel (mi_zset.hip: a recipe row straight to its
// place in the arena) both call.  A decoder that parses bytes from elsewhere exists once.
//
// BOUNDS.  WRITES: a literal run or a match is copied only after len <= n - op was checked: nothing outside [dst, dst + n), at
// any byte alignment of dst (byte stores).  READS of the stored form: every index is compared with `stored` before the load
// (token, extension bytes, the two offset bytes, the literal run as a whole).  READS of the output: op - offset + (i mod offset)
// with 0 < offset <= op: inside [dst, dst + op).  The workgroup IS the wave: the barrier in front of a match that reads what the
// wave has just written is what makes the wave's earlier stores visible to every lane's loads.
#pragma once

#include "mi_common.h"
#include "host_lz4.h"

namespace mi {

static __device__ __forceinline__ int z_first(u64 mask) { return __ffsll((unsigned long long)mask) - 1; }

// the extension bytes behind a nibble of 15, 64 at a time; false: the span ended first (host_lz4.h lz4_extension)
static __device__ __forceinline__ bool z_get_extension(const u8* __restrict__ src, u64 stored, u64* ip, u64* len, int lane) {
    for (;;) {
        const u64 idx = *ip + lane;
        const bool in = idx < stored;
        const u32 b = in ? src[idx] : 0u;
        const u64 m = __ballot(!in || b != 255u);
        if (m == 0) { *len += 255ull * 64; *ip += 64; continue; }
        const int f = z_first(m);
        if (*ip + f >= stored) { *len += 255ull * f; *ip += f; return false; }
        *len += 255ull * f + __shfl(b, f);
        *ip += f + 1;
        return true;
    }
}

// one LZ4 block src[0, stored) -> dst[0, n), by one wave, under host_lz4.h's rules: 0 or the rule that refuses it
static __device__ __forceinline__ u32 z_decode_block(const u8* __restrict__ src, u64 stored, u8* dst, u64 n, int lane) {
    u64 ip = 0, op = 0, seen = 0;                     // seen: the output below it is visible to every lane's loads
    for (;;) {
        if (ip >= stored) return mi_host::kLz4OutputShort;
        const u32 token = src[ip++];
        u64 lit = token >> 4;
        if (lit == 15 && !z_get_extension(src, stored, &ip, &lit, lane)) return mi_host::kLz4ExtensionCut;
        if (lit > stored - ip) return mi_host::kLz4LiteralsLeave;
        if (lit > n - op) return mi_host::kLz4OutputPasses;
        for (u64 i = lane; i < lit; i += 64) dst[op + i] = src[ip + i];
        ip += lit;
        op += lit;
        if (ip == stored) return op == n ? mi_host::kLz4Ok : mi_host::kLz4OutputShort;
        if (stored - ip < 2) return mi_host::kLz4ExtensionCut;
        const u64 off = (u64)src[ip] | ((u64)src[ip + 1] << 8);
        ip += 2;
        if (off == 0) return mi_host::kLz4OffsetZero;
        if (off > op) return mi_host::kLz4OffsetBeyond;
        u64 len = token & 15u;
        if (len == 15 && !z_get_extension(src, stored, &ip, &len, lane)) return mi_host::kLz4ExtensionCut;
        len += 4;
        if (len > n - op) return mi_host::kLz4OutputPasses;
        // the match repeats the `off` bytes in front of op: every byte comes from [op - off, op), written before this match
        if (op - off + (len < off ? len : off) > seen) {
            __syncthreads();                          // the wave's earlier stores have landed
            seen = op;
        }
        const u8* from = dst + (op - off);
        for (u64 i = lane; i < len; i += 64) dst[op + i] = from[i < off ? i : (u32)i % (u32)off];
        op += len;
    }
}

}  // namespace mi
