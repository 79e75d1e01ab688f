// mi_gather.h -- the destination-driven gather of the chunk store, once: a blob is cut into tiles of 16 KiB, a workgroup of 256
// writes a tile from the entries (e_src: an ABSOLUTE device address, e_len: the entry's bytes, e_dst: its blob offset, ascending,
// on the 16-byte grid) that reach into it, so the length distribution of the entries cannot unbalance the launch.  What
// fetch_gather_kernel (mi_fetch.hip), zpack_gather_kernel (mi_zpack.hip), zset_gather_kernel (mi_zset.hip) and
// zbatch_gather_kernel (mi_zbatch.hip) are: they differ in how a unit is loaded only.  pack_gather_kernel (offsets into the
// arena, a signed offset in the tile) and zprune_gather_kernel (no masking, clamped lengths) are kernels of their own.
#pragma once

#include "mi_wave.h"

namespace mi {

constexpr int kGatherWG = 256;
constexpr u32 kGatherTile = 16384;                    // bytes of the blob a workgroup writes
constexpr u32 kGatherUnits = kGatherTile / 16;        // ... in 16-byte units: an entry takes at least one, so at most as many entries
constexpr int kGatherUnitsPer = kGatherUnits / kGatherWG;   // units per lane

// kAligned: every source is 16-byte aligned (a unit is one ALIGNED global_load_dwordx4); else a unit is loaded at whatever
// alignment its source has.  The bytes at and beyond an entry's length are zeroed in registers: the source's pad is never
// trusted.  READS [src, src + round16(len)) of an entry, WRITES aligned units inside [0, blob_bytes).  16 400 bytes of LDS
template <bool kAligned>
static __device__ __forceinline__ void gather_tile(const u64* __restrict__ e_src, const u64* __restrict__ e_len, const u64* __restrict__ e_dst,
                                                   u64 n_entries, u64 blob_bytes, u8* __restrict__ blob) {
    __shared__ u64 s_src[kGatherUnits];
    __shared__ u32 s_rel[kGatherUnits];              // where the entry begins in the tile
    __shared__ u32 s_len[kGatherUnits];
    __shared__ u64 s_k[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 tile0 = (u64)blockIdx.x * kGatherTile;
    const u64 tile1 = tile0 + kGatherTile < blob_bytes ? tile0 + kGatherTile : blob_bytes;
    // the first and the last entry that reach into the tile: the last one that begins at or before the tile's first / last unit
    if (wave < 2) {
        const u64 k = wave_last_le(e_dst, n_entries, wave == 0 ? tile0 : tile1 - 16, lane);
        if (lane == 0) s_k[wave] = k;
    }
    __syncthreads();
    const u64 k0 = s_k[0];
    const u64 reach = s_k[1] - k0 + 1;
    const u32 cnt = reach < kGatherUnits ? (u32)reach : kGatherUnits;
    for (u32 i = threadIdx.x; i < cnt; i += kGatherWG) {
        u64 src = e_src[k0 + i], len = e_len[k0 + i];
        const u64 dst = e_dst[k0 + i];
        u32 rel = (u32)(dst - tile0);
        if (dst < tile0) {                           // the first entry may begin in front of the tile (by up to 4 GiB): the tile sees
            const u64 skip = tile0 - dst;            // what is left of it -- skip is a multiple of 16 below its length
            src += skip;
            len -= skip;
            rel = 0;
        }
        s_src[i] = src;
        s_len[i] = (u32)len;
        s_rel[i] = rel;
    }
    __syncthreads();
    u64 src[kGatherUnitsPer];                        // device addresses of the units' 16 bytes
    u32 valid[kGatherUnitsPer];
#pragma unroll
    for (int j = 0; j < kGatherUnitsPer; ++j) {
        const u32 r = ((u32)threadIdx.x + (u32)j * kGatherWG) * 16;
        src[j] = s_src[0];                            // a unit behind the blob's end (the last tile) loads the tile's first unit and
        valid[j] = 0;                                 // drops it: an unconditional load, so that a lane's four are in flight together
        if (tile0 + r >= tile1) continue;
        u32 lo = 0, hi = cnt;                         // the entry this unit lies in: the last that begins at or before it
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (s_rel[mid] <= r) lo = mid; else hi = mid;
        }
        const u32 o = r - s_rel[lo], len = s_len[lo];
        if (o < len) {                                // (always, for entries of at least one byte)
            src[j] = s_src[lo] + o;                   // a multiple of 16 behind the entry's first byte
            valid[j] = len - o;
        }
    }
    u32x4 v[kGatherUnitsPer];
#pragma unroll
    for (int j = 0; j < kGatherUnitsPer; ++j) v[j] = kAligned ? load16_global(src[j]) : load16_global_unaligned(src[j]);
#pragma unroll
    for (int j = 0; j < kGatherUnitsPer; ++j) {
        const u32 r = ((u32)threadIdx.x + (u32)j * kGatherWG) * 16;
        if (tile0 + r >= tile1) continue;
        if (valid[j] < 16) v[j] = keep_first_bytes(v[j], valid[j]);   // the entry's last unit: zero at and beyond its bytes
        *(u32x4*)(blob + tile0 + r) = v[j];
    }
}

}  // namespace mi
