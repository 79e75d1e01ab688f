// inflate_index_probe.cpp -- test infrastructure: the span decoder of the indexed device inflate alone (csrc/mi_inflate_index.hip
// inflate_span_kernel over a given span table) behind a C calling convention, so that tests/test_gpu_inflate_index.py can hold every
// span's bytes and end against the model's.  Host code only: the wrapper hands its arguments to the library's own launcher on the
// null stream, waits for the device and returns the HIP status (0 = hipSuccess).  No kernels here, nothing the product loads; links
// against makisu_amd/libmakisu_mi.so.
#include "../../makisu_amd/csrc/mi_common.h"

// d_span: six words a span (in_bit, end_bit or 0, its offset in d_out, its bytes, its window's offset in d_hist, the window's bytes);
// d_out holds round_bytes, d_hist hist_total; *d_bad is ~0 before; d_verdict: 16 bytes a span (u32 span, u32 rule, u64 bit)
extern "C" int probe_inflate_spans(const mi::u8* d_gz, mi::u64 n, const mi::u64* d_span, mi::u64 n_span, mi::u64 round_bytes, mi::u8* d_out,
                                   const mi::u8* d_hist, mi::u64 hist_total, mi::u64* d_bad, void* d_verdict) {
    mi::launch_inflate_spans(d_gz, n, d_span, n_span, round_bytes, d_out, d_hist, hist_total, d_bad, d_verdict, nullptr);
    const hipError_t launch = hipGetLastError();
    const hipError_t run = hipDeviceSynchronize();
    return (int)(launch != hipSuccess ? launch : run);
}
