// inflate_spec_probe.cpp -- test infrastructure: the three kernels of the speculative device inflate (csrc/mi_inflate_spec.hip: the
// finder, the speculative pass, the window pass), each alone behind a C calling convention, so that tests/test_gpu_inflate_spec.py can
// hold the candidate table, every candidate's row and ring and the window area against the model's.  Host code only: a wrapper hands
// its arguments to the library's own launcher on the null stream, waits for the device and returns the HIP status (0 = hipSuccess).
// No kernels here, nothing the product loads; links against makisu_amd/libmakisu_mi.so.
#include "../../makisu_amd/csrc/mi_common.h"

static int probe_done() {
    const hipError_t launch = hipGetLastError();
    const hipError_t run = hipDeviceSynchronize();
    return (int)(launch != hipSuccess ? launch : run);
}

// d_cand: one u64 a piece
extern "C" int probe_inflate_find(const mi::u8* d_gz, mi::u64 n, mi::u64 hdr, mi::u64 piece, mi::u64 n_pieces, mi::u64* d_cand) {
    mi::launch_inflate_find(d_gz, n, hdr, piece, n_pieces, d_cand, nullptr);
    return probe_done();
}

// d_rings: 32 768 u16 a piece; d_rows: 32 bytes a piece (end bit, output bytes, status, rule, bit), written for a candidate that got a wave
extern "C" int probe_inflate_speculate(const mi::u8* d_gz, mi::u64 n, mi::u64 hdr, mi::u64 piece, mi::u64 n_pieces, const mi::u64* d_cand,
                                       mi::u64 window, mi::u64 cap, uint16_t* d_rings, void* d_rows) {
    mi::launch_inflate_speculate(d_gz, n, hdr, piece, n_pieces, d_cand, window, cap, d_rings, d_rows, nullptr);
    return probe_done();
}

// d_live: five words a live span (out_at, out_bytes, win_at, win_bytes, the piece whose ring holds its output); *d_bad is ~0 before
extern "C" int probe_inflate_spec_windows(const uint16_t* d_rings, mi::u64 n_rings, const mi::u64* d_live, mi::u64 n_live, mi::u8* d_hist,
                                          mi::u64 hist_total, mi::u64* d_bad) {
    mi::launch_inflate_spec_windows(d_rings, n_rings, d_live, n_live, d_hist, hist_total, d_bad, nullptr);
    return probe_done();
}
