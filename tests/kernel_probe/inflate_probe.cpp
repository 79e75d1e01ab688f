// inflate_probe.cpp -- test infrastructure: the device inflate's table builder (csrc/mi_inflate_wave.h inf_build, and inf_symbol over
// what it built) and its two passes alone (inflate_size_kernel over given starts: the rows; inflate_write_kernel over a given segment
// table: the written bytes) behind a C calling convention, so that tests/test_gpu_inflate.py and tests/test_gpu_inflate_planted.py
// can drive them on inputs made for the purpose.  Host code only: a wrapper hands its arguments to the library's own launcher on the
// null stream, waits for the device and returns the HIP status (0 = hipSuccess).  No kernels here, nothing the product loads; links
// against makisu_amd/libmakisu_mi.so.
#include "../../makisu_amd/csrc/mi_common.h"

static int probe_wait() {
    const hipError_t launch = hipGetLastError();
    const hipError_t run = hipDeviceSynchronize();
    return (int)(launch != hipSuccess ? launch : run);
}

extern "C" int probe_inflate_table(const mi::u8* d_lens, mi::u32 nsym, mi::u32 tab_bits, const mi::u8* d_bits, mi::u32 n_bits, mi::u32* d_verdict,
                                   mi::u32* d_out, mi::u32 max_out) {
    mi::launch_inflate_table(d_lens, nsym, tab_bits, d_bits, n_bits, d_verdict, d_out, max_out, nullptr);
    return probe_wait();
}

// d_rows: n_starts rows of 32 bytes (end, out_bytes, status, rule, bit), one a start, in the starts' order
extern "C" int probe_inflate_rows(const mi::u8* d_gz, mi::u64 n, const mi::u64* d_starts, mi::u64 n_starts, mi::u64 window, void* d_rows) {
    mi::launch_inflate_rows(d_gz, n, d_starts, n_starts, window, d_rows, nullptr);
    return probe_wait();
}

// d_seg: three words a segment (its start in the member, its offset in d_out, its bytes); d_out holds round_bytes; *d_bad is ~0 before
extern "C" int probe_inflate_write(const mi::u8* d_gz, mi::u64 n, const mi::u64* d_seg, mi::u64 n_seg, mi::u64 round_bytes, mi::u8* d_out,
                                   mi::u64* d_bad) {
    mi::launch_inflate_write(d_gz, n, d_seg, n_seg, round_bytes, d_out, d_bad, nullptr);
    return probe_wait();
}
