// mi_tarscan.h -- the launcher of mi_tarscan.hip: the header candidates of a tar that lies on the device.  For
// mi_layerblob.hip and tests/kernel_probe/tar_probe.cpp.
#pragma once

#include "mi_common.h"

#include <vector>

namespace mi {

struct TarScan {
    std::vector<u64> blocks;     // the marked blocks' numbers, ascending
    std::vector<u8>  kinds;      // mi_host::kTarHeader | kTarBody of each
    std::vector<u8>  dense;      // their 512 bytes each, in the same order
    float ms_device = 0;         // the kernels' time (mark, count, scan | scatter, gather), without the wait in between
};

// d_tar[0, tar_bytes) on the device (8-byte aligned): mark, compaction and gather on `s`, the result on the host when the call
// returns.  Only whole blocks are read: nothing at or behind 512 * floor(tar_bytes / 512)
hipError_t tar_scan(const u8* d_tar, u64 tar_bytes, hipStream_t s, TarScan* out);

}  // namespace mi
