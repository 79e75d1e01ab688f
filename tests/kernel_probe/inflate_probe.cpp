// inflate_probe.cpp -- test infrastructure: the device inflate's table builder (csrc/mi_inflate_wave.h inf_build, and inf_symbol over
// what it built) behind a C calling convention, so that tests/test_gpu_inflate.py can drive it alone on code lengths made for the
// purpose.  Host code only: the wrapper hands its arguments to the library's own launcher on the null stream, waits for the device
// and returns the HIP status (0 = hipSuccess).  No kernels here, nothing the product loads; links against makisu_amd/libmakisu_mi.so.
#include "../../makisu_amd/csrc/mi_common.h"

extern "C" int probe_inflate_table(const mi::u8* d_lens, mi::u32 nsym, mi::u32 tab_bits, const mi::u8* d_bits, mi::u32 n_bits, mi::u32* d_verdict,
                                   mi::u32* d_out, mi::u32 max_out) {
    mi::launch_inflate_table(d_lens, nsym, tab_bits, d_bits, n_bits, d_verdict, d_out, max_out, nullptr);
    const hipError_t launch = hipGetLastError();
    const hipError_t run = hipDeviceSynchronize();
    return (int)(launch != hipSuccess ? launch : run);
}
