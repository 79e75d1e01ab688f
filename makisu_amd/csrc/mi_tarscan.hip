// mi_tarscan.hip -- the HEADER CANDIDATES of a tar that lies on the device.  A tar's headers are a serial chain --
// each says where the next one is -- and the host needs nothing else of the archive to list it.  The device cannot follow the chain,
// but it can say of every 512-byte block whether it COULD be a header, and the host follows the live chain through the marked ones.
//
// THE RULE.  Block j is the tar's bytes [512 j, 512 j + 512), j < floor(T / 512); a trailing piece of 1..511 bytes is never loaded
// and never marked.  Block j is a HEADER candidate iff mi_tar.hip's checksum_ok holds for it:
//   * the checksum field (bytes 148..155) is read as number() reads it: base-256 if its first byte has the top bit set (big-endian,
//     the flag bit dropped, complemented if bit 6 is set -- eight bytes never overflow); otherwise octal text, spaces and NULs trimmed
//     on both sides and cut at the first NUL; an empty field is 0; any other character fails;
//   * the value equals the unsigned or the signed sum of the 512 bytes with the field counted as eight spaces.
// Bit for bit the host's rule: a block the device does not mark is a block the parser would refuse.  A data block that passes is a
// DEAD candidate the chain never visits.  A header candidate of typeflag (byte 156) x, g, L or K also marks the next kTarMetaInline
// = 2 blocks, where they exist, as BODY: a pax record block or a GNU long name of up to 1 024 bytes travels with its header.
//
//   tar_mark_kernel      one wave a block, waves striding over the blocks: a lane loads 8 bytes (one coalesced 512-byte load a wave),
//                        the byte sum and the count of bytes >= 0x80 go through one wave_sum, the field and the typeflag reach lane 0
//                        by readlane, lane 0 decides: mark[j] = 0 | 1 (header) | 3 (header of a meta typeflag)
//   tar_count_kernel     mi_plan.h: a tile of kPlanTile blocks, how many are marked -- block j's kind is its own header bit and the
//   tar_scan_kernel      meta bit of the two blocks in front of it, so nobody writes another block's mark
//   tar_scatter_kernel   the marked blocks' numbers and kinds, ascending
//   tar_gather_kernel    one wave a marked block: its 512 bytes into the dense buffer, in the same order
// No scratch, no spills; LDS only for the scan.  The count comes down (8 bytes) to size the lists; numbers, kinds and the dense
// buffer then come down in one synchronisation.
#include "mi_internal.h"
#include "mi_plan.h"
#include "mi_tarscan.h"
#include "host_tarcache.h"

#include <algorithm>

namespace mi {

constexpr int kTarScanUnroll = 4;                       // blocks a wave has in flight

// the sum of a word's four bytes, and of a u64's eight
static __device__ __forceinline__ u32 tar_bytes_sum(u64 v) {
    const u64 pairs = (v & 0x00FF00FF00FF00FFull) + ((v >> 8) & 0x00FF00FF00FF00FFull);
    const u64 quads = (pairs & 0x0000FFFF0000FFFFull) + ((pairs >> 16) & 0x0000FFFF0000FFFFull);
    return (u32)quads + (u32)(quads >> 32);
}

// number() of mi_tar.hip over the eight bytes f (byte i = bits 8i..8i+7)
static __device__ __forceinline__ bool tar_field8(u64 f, i64* out) {
    if (f & 0x80) {
        const u32 inv = (f & 0x40) ? 0xFFu : 0u;
        u64 x = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            u32 c = ((u32)(f >> (8 * i)) & 0xFFu) ^ inv;
            if (i == 0) c &= 0x7Fu;
            x = (x << 8) | c;                           // 7 + 56 bits: nothing is lost
        }
        *out = inv ? (i64)~x : (i64)x;
        return true;
    }
    int a = 0, b = 8;
    while (a < b && (((f >> (8 * a)) & 0xFF) == ' ' || ((f >> (8 * a)) & 0xFF) == 0)) ++a;
    while (b > a && (((f >> (8 * (b - 1))) & 0xFF) == ' ' || ((f >> (8 * (b - 1))) & 0xFF) == 0)) --b;
    for (int i = a; i < b; ++i) if (((f >> (8 * i)) & 0xFF) == 0) { b = i; break; }
    u64 v = 0;
    for (int i = a; i < b; ++i) {
        const u32 c = (u32)(f >> (8 * i)) & 0xFFu;
        if (c < '0' || c > '7') return false;
        v = (v << 3) | (u64)(c - '0');                  // eight digits: 24 bits
    }
    *out = (i64)v;
    return true;
}

__global__ __launch_bounds__(256)
void tar_mark_kernel(const u64* __restrict__ tar, u64 n_blocks, u8* __restrict__ mark) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6), n_waves = (u64)gridDim.x * (blockDim.x / 64);
    for (u64 j0 = wave; j0 < n_blocks; j0 += kTarScanUnroll * n_waves) {
        u64 v[kTarScanUnroll];
#pragma unroll
        for (int q = 0; q < kTarScanUnroll; ++q) {
            const u64 j = j0 + (u64)q * n_waves;
            v[q] = j < n_blocks ? tar[j * 64 + lane] : 0;
        }
#pragma unroll
        for (int q = 0; q < kTarScanUnroll; ++q) {
            const u64 j = j0 + (u64)q * n_waves;
            if (j >= n_blocks) break;                   // (uniform over the wave)
            // bytes 148..155: the upper half of lane 18's word and the lower half of lane 19's, summed as spaces
            u64 w = v[q];
            if (lane == 18) w = (w & 0x00000000FFFFFFFFull) | 0x2020202000000000ull;
            if (lane == 19) w = (w & 0xFFFFFFFF00000000ull) | 0x0000000020202020ull;
            const u64 both = wave_sum((u64)tar_bytes_sum(w) | (u64)__popcll(w & 0x8080808080808080ull) << 32);
            const u32 f_lo = (u32)__builtin_amdgcn_readlane((int)(u32)(v[q] >> 32), 18);
            const u32 f_hi = (u32)__builtin_amdgcn_readlane((int)(u32)v[q], 19);
            const u32 type = (u32)__builtin_amdgcn_readlane((int)(u32)(v[q] >> 32), 19) & 0xFFu;
            if (lane == 0) {
                const i64 u = (i64)(both & 0xFFFFFFFFull), s = u - 256 * (i64)(both >> 32);
                i64 want = 0;
                const bool ok = tar_field8((u64)f_lo | (u64)f_hi << 32, &want) && (want == u || want == s);
                const bool meta = type == 'x' || type == 'g' || type == 'L' || type == 'K';
                mark[j] = ok ? (meta ? 3 : 1) : 0;
            }
        }
    }
}

// block j's kind from the marks: its own header bit, and BODY if one of the kTarMetaInline blocks in front of it is a meta header
static __device__ __forceinline__ u32 tar_kind(const u8* __restrict__ mark, u64 j) {
    u32 kind = mark[j] & 1u ? mi_host::kTarHeader : 0u;
#pragma unroll
    for (int d = 1; d <= mi_host::kTarMetaInline; ++d)
        if (j >= (u64)d && (mark[j - d] & 2u)) kind |= mi_host::kTarBody;
    return kind;
}

__global__ __launch_bounds__(kPlanBlock)
void tar_count_kernel(const u8* __restrict__ mark, u64 n_blocks, u64* __restrict__ block_cnt) {
    __shared__ u64 lds[1][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[1] = {0};
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
        if (base + k < n_blocks && tar_kind(mark, base + k)) ++v[0];
    plan_block_sum<1>(v, lds);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = v[0];
}

__global__ __launch_bounds__(kPlanBlock)
void tar_scan_kernel(u64* __restrict__ block_cnt, u64 n_tiles, u64* __restrict__ total) {
    plan_block_offsets<false>(block_cnt, nullptr, n_tiles, total, nullptr);
}

__global__ __launch_bounds__(kPlanBlock)
void tar_scatter_kernel(const u8* __restrict__ mark, u64 n_blocks, const u64* __restrict__ block_cnt, u64 n_marked, u64* __restrict__ blocks,
                        u8* __restrict__ kinds) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u32 kind[kPlanPer];
    u64 cnt = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        kind[k] = base + k < n_blocks ? tar_kind(mark, base + k) : 0u;
        if (kind[k]) ++cnt;
    }
    u64 at = plan_first(cnt, block_cnt);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
        if (kind[k] && at < n_marked) { blocks[at] = base + k; kinds[at] = (u8)kind[k]; ++at; }
}

__global__ __launch_bounds__(256)
void tar_gather_kernel(const u64* __restrict__ tar, u64 n_blocks, const u64* __restrict__ blocks, u64 n_marked, u64* __restrict__ dense) {
    const int lane = threadIdx.x & 63;
    const u64 n_waves = (u64)gridDim.x * (blockDim.x / 64);
    for (u64 k = (u64)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); k < n_marked; k += n_waves) {
        const u64 j = blocks[k];
        if (j < n_blocks) dense[k * 64 + lane] = tar[j * 64 + lane];
    }
}

#define TSCHK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

hipError_t tar_scan(const u8* d_tar, u64 tar_bytes, hipStream_t s, TarScan* out) {
    out->blocks.clear();
    out->kinds.clear();
    out->dense.clear();
    out->ms_device = 0;
    const u64 n_blocks = tar_bytes / mi_host::kTarBlock;
    if (n_blocks == 0) return hipSuccess;
    if ((uintptr_t)d_tar % 8) return hipErrorInvalidValue;
    const u64 n_tiles = (n_blocks + kPlanTile - 1) / kPlanTile;
    if (n_tiles >> 31) return hipErrorInvalidValue;
    DevBuf d_mark, d_cnt, d_tot, d_blocks, d_kinds, d_dense;
    Event ev[4];
    StreamDrain drain{s};                               // (goes first: buffers and events after it)
    for (auto& e : ev) TSCHK(e.create());
    TSCHK(d_mark.alloc_exact(n_blocks));
    TSCHK(d_cnt.alloc_exact(n_tiles * 8));
    TSCHK(d_tot.alloc_exact(8));
    const u64 most_waves = 32768;                       // waves that stride: four rounds of what 256 CUs hold at eight waves a SIMD
    const u32 mark_grid = (u32)((std::min(n_blocks, most_waves) + 3) / 4);
    TSCHK(hipEventRecord(ev[0], s));
    hipLaunchKernelGGL(tar_mark_kernel, dim3(mark_grid), dim3(256), 0, s, (const u64*)d_tar, n_blocks, d_mark.as<u8>());
    hipLaunchKernelGGL(tar_count_kernel, dim3((u32)n_tiles), dim3(kPlanBlock), 0, s, d_mark.as<u8>(), n_blocks, d_cnt.as<u64>());
    hipLaunchKernelGGL(tar_scan_kernel, dim3(1), dim3(kPlanBlock), 0, s, d_cnt.as<u64>(), n_tiles, d_tot.as<u64>());
    TSCHK(hipGetLastError());
    TSCHK(hipEventRecord(ev[1], s));
    u64 n_marked = 0;
    TSCHK(hipMemcpyAsync(&n_marked, d_tot.p, 8, hipMemcpyDeviceToHost, s));
    TSCHK(hipStreamSynchronize(s));
    float ms = 0;
    TSCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    out->ms_device = ms;
    if (n_marked > n_blocks) return hipErrorUnknown;
    if (n_marked == 0) return hipSuccess;
    TSCHK(d_blocks.alloc_exact(n_marked * 8));
    TSCHK(d_kinds.alloc_exact(n_marked));
    TSCHK(d_dense.alloc_exact(n_marked * mi_host::kTarBlock));
    out->blocks.resize(n_marked);
    out->kinds.resize(n_marked);
    out->dense.resize(n_marked * mi_host::kTarBlock);
    const u32 gather_grid = (u32)((std::min(n_marked, most_waves) + 3) / 4);
    TSCHK(hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(tar_scatter_kernel, dim3((u32)n_tiles), dim3(kPlanBlock), 0, s, d_mark.as<u8>(), n_blocks, d_cnt.as<u64>(), n_marked,
                       d_blocks.as<u64>(), d_kinds.as<u8>());
    hipLaunchKernelGGL(tar_gather_kernel, dim3(gather_grid), dim3(256), 0, s, (const u64*)d_tar, n_blocks, d_blocks.as<u64>(), n_marked,
                       d_dense.as<u64>());
    TSCHK(hipGetLastError());
    TSCHK(hipEventRecord(ev[3], s));
    TSCHK(hipMemcpyAsync(out->blocks.data(), d_blocks.p, n_marked * 8, hipMemcpyDeviceToHost, s));
    TSCHK(hipMemcpyAsync(out->kinds.data(), d_kinds.p, n_marked, hipMemcpyDeviceToHost, s));
    TSCHK(hipMemcpyAsync(out->dense.data(), d_dense.p, n_marked * mi_host::kTarBlock, hipMemcpyDeviceToHost, s));
    TSCHK(hipStreamSynchronize(s));
    TSCHK(hipEventElapsedTime(&ms, ev[2], ev[3]));
    out->ms_device += ms;
    return hipSuccess;
}

}  // namespace mi
