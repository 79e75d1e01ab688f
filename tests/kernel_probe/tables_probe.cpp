// tables_probe.cpp -- test infrastructure: the table launchers of csrc/tables.hip behind a C calling convention, so that
// tests/test_gpu_table_kernels.py can drive each of them alone on arrays made for the purpose.  Host code only: every
// wrapper hands its arguments to the library's own launcher on the null stream, waits for the device and returns the HIP
// status (0 = hipSuccess).  No kernels here, nothing the product loads; links against makisu_amd/libmakisu_mi.so.
#include "../../makisu_amd/csrc/mi_common.h"

using mi::u8;
using mi::u32;
using mi::u64;

static int finish() {
    const hipError_t launch = hipGetLastError();
    const hipError_t run = hipDeviceSynchronize();
    return (int)(launch != hipSuccess ? launch : run);
}

extern "C" {

u64 probe_scan_scratch_elems(u64 n) { return mi::scan_scratch_elems(n); }

u64 probe_group_rec_bytes() { return (u64)mi::gear_group_rec_bytes(); }

int probe_scan_counts(const u32* d_counts, u64* d_first, u64* d_total, u64 n, u64* d_scratch) {
    mi::launch_scan_counts(d_counts, d_first, d_total, n, d_scratch, nullptr);
    return finish();
}

int probe_compact_chunks(const u64* d_file_off, const u64* d_file_seg0, const u32* d_seg_file, const u64* d_seg_slot,
                         const u32* d_ends32, const u64* d_seg_first, const u32* d_seg_group, const void* d_group_recs,
                         u32 region, u64 n_files, u64 n_segs, u64 n_max, const u64* d_n, u64* d_chunk_off,
                         u64* d_chunk_len, u32* d_chunk_file, u64* d_chunk_start, u64* d_first, u32* d_n_chunks,
                         u32* d_hist, u32 n_bins, u32 bin_shift, const u8* d_digests, u64* d_item_off,
                         u64* d_item_len) {
    mi::launch_compact_chunks(d_file_off, d_file_seg0, d_seg_file, d_seg_slot, d_ends32, d_seg_first, d_seg_group,
                              d_group_recs, region, n_files, n_segs, n_max, d_n, d_chunk_off, d_chunk_len, d_chunk_file,
                              d_chunk_start, d_first, d_n_chunks, d_hist, n_bins, bin_shift, d_digests, d_item_off,
                              d_item_len, nullptr);
    return finish();
}

int probe_bin_order(const u64* d_off, const u64* d_len, u32 n, const u64* d_n, u32* d_hist, u32* d_cursor, u32 n_bins,
                    u32 bin_shift, u64* d_s_off, u64* d_s_len, u32* d_s_id) {
    mi::launch_bin_order(d_off, d_len, n, d_n, d_hist, d_cursor, n_bins, bin_shift, d_s_off, d_s_len, d_s_id, nullptr);
    return finish();
}

int probe_root_init(const u8* d_digests, const u64* d_first, const u32* d_n_chunks, u64 n_files, u64* d_cur_addr,
                    u32* d_cur_cnt) {
    mi::launch_root_init(d_digests, d_first, d_n_chunks, n_files, d_cur_addr, d_cur_cnt, nullptr);
    return finish();
}

int probe_root_level(u64 n_files, u64 n_nodes_ub, const u64* d_cur_addr, const u32* d_cur_cnt, u64* d_next_addr,
                     u32* d_next_cnt, u32* d_seg_cnt, u64* d_seg_first, u64* d_seg_total, u64* d_scratch,
                     u8* d_level_out, u64* d_item_off, u64* d_item_len) {
    mi::launch_root_level(n_files, n_nodes_ub, d_cur_addr, d_cur_cnt, d_next_addr, d_next_cnt, d_seg_cnt, d_seg_first,
                          d_seg_total, d_scratch, d_level_out, d_item_off, d_item_len, nullptr);
    return finish();
}

int probe_root_final_items(const u64* d_cur_addr, const u32* d_cur_cnt, u64 n_files, u64* d_off, u64* d_len) {
    mi::launch_root_final_items(d_cur_addr, d_cur_cnt, n_files, d_off, d_len, nullptr);
    return finish();
}

}  // extern "C"
