// tar_probe.cpp -- test infrastructure: the tar header pass (csrc/mi_tarscan.hip: mark, compaction, gather) behind a C calling
// convention, so that tests/test_gpu_layer_blob.py can drive it alone on buffers made for the purpose.  Host code only: the wrapper
// hands its arguments to the library's own launcher on the null stream and returns the HIP status (0 = hipSuccess), the number of
// marked blocks in *n_marked and, where they fit cap, their numbers, kinds and 512 bytes each.  No kernels here, nothing the product
// loads; links against makisu_amd/libmakisu_mi.so.
#include "../../makisu_amd/csrc/mi_tarscan.h"

#include <string.h>

extern "C" int probe_tar_scan(const mi::u8* d_tar, mi::u64 tar_bytes, mi::u64* n_marked, mi::u64* blocks, mi::u8* kinds, mi::u8* dense, mi::u64 cap) {
    mi::TarScan scan;
    const hipError_t e = mi::tar_scan(d_tar, tar_bytes, nullptr, &scan);
    if (e != hipSuccess) return (int)e;
    *n_marked = scan.blocks.size();
    if (scan.blocks.size() <= cap && !scan.blocks.empty()) {
        memcpy(blocks, scan.blocks.data(), scan.blocks.size() * 8);
        memcpy(kinds, scan.kinds.data(), scan.kinds.size());
        memcpy(dense, scan.dense.data(), scan.dense.size());
    }
    return 0;
}

// ... and the pass's device time alone (tools/layer_ingest_bench.py): the launcher's own events around the kernels
extern "C" int probe_tar_scan_ms(const mi::u8* d_tar, mi::u64 tar_bytes, mi::u64* n_marked, float* ms_device) {
    mi::TarScan scan;
    const hipError_t e = mi::tar_scan(d_tar, tar_bytes, nullptr, &scan);
    if (e != hipSuccess) return (int)e;
    *n_marked = scan.blocks.size();
    *ms_device = scan.ms_device;
    return 0;
}
