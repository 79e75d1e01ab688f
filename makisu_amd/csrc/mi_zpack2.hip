// mi_zpack2.hip -- zpack LEVEL 2's encode kernel (MI_ZPACK_LEVEL2): z_encode_block_l2 (csrc/mi_lz4_wave_enc2.h) in
// mi_zrows.h's loop over the rows.  ONE kernel serves both producers, because their encode launches differ in nothing but the
// base pointer: mi_pack_compress (mi_zpack.hip) hands it a plain pack's blob, mi_batch_zpack_chunks (mi_zbatch.hip) a batch's
// arena.  Everything around the coder is the same at either level.  The kernel lives in a file of its own because the resource
// tests of those two files list their kernels by name.
//
// BOUNDS.  The coder's: mi_lz4_wave_enc2.h.  rows[k] and w_off[k] are read for k < n; the row's last word is written by lane 0.
#include "mi_internal.h"
#include "mi_zrows.h"

using namespace mi;

namespace mi {

// rows[k]: digest | the chunk's offset from `base` | chunk_index | length (the high half is written here: stored)
__global__ __launch_bounds__(64)
void zencode_l2_kernel(const u8* __restrict__ base, u64* __restrict__ rows, const u64* __restrict__ w_off, u8* __restrict__ scratch, u64 n) {
    __shared__ u32 tables[2 * kZTable];                   // t4 | t8: 32 KiB a wave
    z_encode_rows<ZLevel2>(base, rows, w_off, scratch, n, tables);
}

}  // namespace mi

extern "C" {

// (hidden: mi_local.h) the level-2 encode ENQUEUED on the ctx stream in place of the caller's level-1 kernel, same arguments
int mi_zencode_l2_enqueue(mi_ctx* c, const void* d_base, uint64_t* d_rows, const uint64_t* d_woff, void* d_scratch, uint64_t n, uint32_t waves) {
    if (!c || !d_base || !d_rows || !d_woff || !d_scratch || !n || !waves) return MI_ERR_INVALID;
    hipLaunchKernelGGL(zencode_l2_kernel, dim3(waves), dim3(64), 0, c->stream, (const u8*)d_base, d_rows, d_woff, (u8*)d_scratch, n);
    return MI_OK;
}

}  // extern "C"
