// mi_wave.h -- the device primitives the chunk store's files share (mi_pack, mi_fetch, mi_restore, mi_zpack, mi_zset, mi_zbatch,
// mi_zprune, mi_index): the block scan and the wave's sum of 64-bit values, the wave's search over an ascending array, the
// digest compare and the table's tag, 16-byte loads from an absolute device address, and the masking of an entry's last unit.
// Every one is forced inline: a kernel compiles as it did with the function in its own file.  Its siblings: mi_plan.h (the
// plan's three launches over these primitives), mi_zrows.h (a coded zpack's rows), mi_gather.h (the tile gather).  tables.hip
// keeps its own scan (another LDS contract), the two hashing kernels share mi_item_loads.h, whose load types these functions use.
#pragma once

#include "mi_common.h"
#include "mi_item_loads.h"

namespace mi {

__host__ __device__ static inline u64 round16(u64 v) { return (v + 15) & ~15ull; }

// the block scan of tables.hip: inclusive scan per wave with shuffles, then across the kBlock / 64 waves through LDS
template <int kBlock = 256>
static __device__ __forceinline__ u64 block_exclusive_scan_u64(u64 v, u64* total, u64* lds /*>= kBlock / 64*/) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 lo = __shfl_up((u32)x, d), hi = __shfl_up((u32)(x >> 32), d);
        const u64 y = ((u64)hi << 32) | lo;
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    u64 wave_off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        const u64 s = lds[w];
        if (w < wave) wave_off += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return wave_off + x - v;
}

// a wave's sum, in every lane
static __device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const u32 lo = __shfl_xor((u32)v, d), hi = __shfl_xor((u32)(v >> 32), d);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}

// the largest k in [0, n) with a[k] <= x (a ascending, a[0] <= x), by one wave: 64 probes a round
static __device__ __forceinline__ u64 wave_last_le(const u64* __restrict__ a, u64 n, u64 x, int lane) {
    u64 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u64 step = (hi - lo + 63) >> 6;
        const u64 p = lo + (u64)lane * step;
        const bool ok = p < hi && a[p] <= x;
        const u64 c = (u64)__popcll(__ballot(ok));   // the probes that hold are a prefix of the lanes; lane 0 probes lo: c >= 1
        hi = lo + c * step < hi ? lo + c * step : hi;
        lo = lo + (c - 1) * step;
    }
    return lo;
}

// two digests of 32 bytes, each on a 16-byte boundary
static __device__ __forceinline__ bool digest_eq32(const u8* a, const u8* b) {
    const u32x4 a0 = ((const u32x4*)a)[0], a1 = ((const u32x4*)a)[1];
    const u32x4 b0 = ((const u32x4*)b)[0], b1 = ((const u32x4*)b)[1];
    const u32x4 d0 = a0 ^ b0, d1 = a1 ^ b1;
    return (d0.x | d0.y | d0.z | d0.w | d1.x | d1.y | d1.z | d1.w) == 0;
}

// a table's tag: the digest's first 8 bytes, 0 stored as 1 (0 = an empty slot)
static __device__ __forceinline__ u64 tag_of(u64 first8) { return first8 ? first8 : 1ull; }

// an ALIGNED 16-byte load from an absolute device address (the address space is said here: a generic pointer would make it flat)
static __device__ __forceinline__ u32x4 load16_global(u64 addr) {
    typedef const u32x4 __attribute__((address_space(1))) * global_ptr;
    return *(global_ptr)addr;
}

// a 16-byte load at any alignment from an ABSOLUTE device address: the table hands out addresses, not offsets from a kernel
// argument, so the address space is said here (a generic pointer would make it a flat load)
static __device__ __forceinline__ u32x4 load16_global_unaligned(u64 addr) {
    typedef const u32x4_unaligned __attribute__((address_space(1))) * global_ptr;
    return *(global_ptr)addr;
}

// the first `valid` (< 16) bytes of a unit, the rest zero
static __device__ __forceinline__ u32x4 keep_first_bytes(u32x4 v, u32 valid) {
    u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u32 have = valid > 4u * q ? valid - 4u * q : 0u;
        w[q] = have >= 4 ? w[q] : have ? (w[q] & ((1u << (8 * have)) - 1u)) : 0u;
    }
    return u32x4{w[0], w[1], w[2], w[3]};
}

}  // namespace mi
