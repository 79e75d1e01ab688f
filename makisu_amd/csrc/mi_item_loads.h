// mi_item_loads.h -- what the two one-lane-per-string hashing kernels (sha256.hip, blake2s.hip) share on the way in:
// the 16-byte load types and the quad-cooperative fetch.  Everything behind the loaded block -- byte order, tail, the
// compression, the digest -- is each file's own.
#pragma once

#include "mi_common.h"

namespace mi {

typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));

template <int kM>
__device__ __forceinline__ u32 quad_bcast(u32 v) {            // value of lane (lane & ~3) + kM
    return (u32)__builtin_amdgcn_update_dpp(0, (int)v, kM * 0x55, 0xF, 0xF, true);
}
constexpr int kXRow = 20;                                      // LDS row: 64 B of block + 16 B pad (dwords)

// every quad fetches the next blocks of its owners that want one (kAll: all four do), owner m's 64
// bytes with ONE instruction; piece `sub` of owner qbase + m lands in g_m
template <bool kAll>
__device__ __forceinline__ void coop_fetch(u32x4& g0, u32x4& g1, u32x4& g2, u32x4& g3, const u8* ptr, bool want, int sub) {
    const u32 wf = want ? 1u : 0u;
    const u32 plo = (u32)(size_t)ptr, phi = (u32)((size_t)ptr >> 32);
    const u32 l0 = quad_bcast<0>(plo), l1 = quad_bcast<1>(plo), l2 = quad_bcast<2>(plo), l3 = quad_bcast<3>(plo);
    const u32 h0 = quad_bcast<0>(phi), h1 = quad_bcast<1>(phi), h2 = quad_bcast<2>(phi), h3 = quad_bcast<3>(phi);
    const u64 mine = 16u * (u32)sub;                 // my 16-byte piece of every owner's block
    if (kAll || quad_bcast<0>(wf)) g0 = *(const u32x4_a4*)(size_t)((((u64)h0 << 32) | l0) + mine);
    if (kAll || quad_bcast<1>(wf)) g1 = *(const u32x4_a4*)(size_t)((((u64)h1 << 32) | l1) + mine);
    if (kAll || quad_bcast<2>(wf)) g2 = *(const u32x4_a4*)(size_t)((((u64)h2 << 32) | l2) + mine);
    if (kAll || quad_bcast<3>(wf)) g3 = *(const u32x4_a4*)(size_t)((((u64)h3 << 32) | l3) + mine);
}

// a lane asks for its next string when fewer than kLook blocks of the current one are left (the
// four-stage next-string pipeline of both kernels)
constexpr u32 kLook = 5;

}  // namespace mi
