// mi_item_launch.h -- what the launchers and the roof measurements of the two one-lane-per-string hashing kernels
// (sha256.hip, blake2s.hip) share on the host.
#pragma once

#include "mi_common.h"

#include <initializer_list>

namespace mi {

// ---- host: what launch_sha256_items and launch_blake2s_items do in front of their kernels ---------------------------
// false: nothing to launch.  Takes d_roles away when ShaTune.roles is off, clears the queue heads and role counters on
// request, works out the geometry (max_pinned, static_lds: sha_items_geometry) and the kernels' long_shift word
// (ShaTune.long_shift | 0x100 = no s_setprio) and, for a pinned launch, raises the dynamic-LDS limit of `pinned_kernels`
// once per device (attr_dev: the caller's thread-local record of the device that has been done).
static inline bool prepare_items_launch(ShaGeometry& geo, u32& shift_flags, u32*& d_roles, ShaPass pass, u32 n, u32* d_heads,
                                        bool zero_heads, const ShaTune& tune, int n_cu, u64 footprint_bytes, int max_pinned,
                                        size_t static_lds, std::initializer_list<const void*> pinned_kernels, int& attr_dev,
                                        hipStream_t s) {
    if (n == 0) return false;
    if (!tune.roles) d_roles = nullptr;
    if (zero_heads) {
        (void)hipMemsetAsync(d_heads, 0, sizeof(u32) * kShaHeadWords, s);
        if (d_roles) (void)hipMemsetAsync(d_roles, 0, sizeof(u32) * kShaRoleWords, s);
    }
    geo = sha_items_geometry(pass, n, tune, n_cu, footprint_bytes, max_pinned, static_lds);
    shift_flags = (u32)tune.long_shift | (tune.prio ? 0u : 0x100u);
    if (geo.pinned) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (attr_dev != dev) {
            for (const void* k : pinned_kernels) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
            attr_dev = dev;
        }
    }
    return true;
}

// ---- host: the VALU roof of a compression, measured on the device it runs on: bytes "hashed" per second by
// n_cu * waves_per_simd workgroups running `blocks` compressions per lane in `roof_kernel`
static inline double measure_valu_roof(void (*roof_kernel)(u32*, u32), int n_cu, int waves_per_simd, u32 blocks, u32* d_scratch,
                                       hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const u32 grid = (u32)(n_cu * waves_per_simd);                 // a workgroup = one wave on each of the CU's 4 SIMDs
    hipLaunchKernelGGL(roof_kernel, dim3(grid), dim3(kShaWG), 0, s, d_scratch, blocks / 8 + 1);   // clocks up
    double best = 0;
    for (int rep = 0; rep < 3; ++rep) {
        (void)hipEventRecord(e0, s);
        hipLaunchKernelGGL(roof_kernel, dim3(grid), dim3(kShaWG), 0, s, d_scratch, blocks);
        (void)hipEventRecord(e1, s);
        if (hipStreamSynchronize(s) != hipSuccess) return 0;
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        const double rate = ms > 0 ? (double)grid * kShaWG * blocks * 64.0 / (ms * 1e-3) : 0;
        best = rate > best ? rate : best;
    }
    return best;
}

}  // namespace mi
