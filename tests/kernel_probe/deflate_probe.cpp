// deflate_probe.cpp -- test infrastructure: the device deflate leg's length-limiting rule (csrc/mi_deflate_wave.h df_code_lengths)
// behind a C calling convention, so that tests/test_gpu_deflate.py can drive it alone on counts made for the purpose.  Host code
// only: the wrapper hands its arguments to the library's own launcher on the null stream, waits for the device and returns the
// HIP status (0 = hipSuccess).  No kernels here, nothing the product loads; links against makisu_amd/libmakisu_mi.so.
#include "../../makisu_amd/csrc/mi_common.h"

extern "C" int probe_deflate_code_lengths(const mi::u32* d_counts, mi::u32 nsym, mi::u32 limit, mi::u8* d_lens) {
    mi::launch_deflate_code_lengths(d_counts, nsym, limit, d_lens, nullptr);
    const hipError_t launch = hipGetLastError();
    const hipError_t run = hipDeviceSynchronize();
    return (int)(launch != hipSuccess ? launch : run);
}
