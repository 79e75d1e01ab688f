// mi_inflate_local.h -- the inflater object (mi_local.h: mi_inflater_*) as mi_inflate.hip and mi_inflate_index.hip share it: the
// member on the device, the two slots a round goes through, the plan.  mi_inflate.hip owns the streams, the upload, the rounds and
// their CRC; mi_inflate_index.hip plans from an index of checkpoints instead of a size pass and decodes a round's
// SPANS with a kernel of its own -- everything around that one launch is the same code.
#pragma once

#include "mi_internal.h"
#include "host_inflate.h"

#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <vector>

namespace mi {

struct InfSlot {
    PinBuf h_out, h_seg, h_small;                       // h_small: [0..2] the CRC pass's file row, [4] the CRC, [5] the bad segment
    DevBuf d_out, d_seg, d_row, d_tile_file, d_tile_raw, d_crc, d_bad;
    DevBuf d_verdict;                                   // (spans) 16 bytes a span of the round: span, rule, bit -- written by a refused span only
    Event done, down, t0, t1;
    u64 bytes = 0, n_seg = 0;
    bool pending = false;
};

//  what a call that plans speculatively asks for: the piece, and where the plan's figures and its index go (each may be NULL)
struct InfSpecAsk { u64 piece_bytes; mi_inflate_spec_info* spec_info; void** index; u64* index_bytes; };

constexpr int kInflateRefused = 1;                      // (spans) inflate_run_rounds: a span broke a rule or the trailer does not hold; d->info says which

}  // namespace mi

struct mi_inflater {
    mi_ctx* ctx = nullptr;
    mi::u64 window = 0;
    mi::Stream code, copy;
    mi::PinBuf h_stage[2];
    mi::Event staged[2], t0, t1;
    mi::DevBuf d_gz, d_cand, d_rows, d_blk, d_tot;
    mi::InfSlot slot[2];
    std::string err;
    mi_inflate_info info = {};
    // the plan
    mi::u64 n = 0, header = 0;
    mi::u32 want_crc = 0, want_isize = 0;
    std::vector<mi::u64> cand, round_first;
    std::vector<mi_host::InflateRow> rows;
    mi_host::InflateChain chain;
    // the plan from an index: chain.segs holds the spans (in_at = in_bit / 8), spans six words each -- in_bit, end_bit (0: the last
    // span), out_at in the member's output, out_bytes, the window's offset in d_hist, its bytes
    bool indexed = false;
    std::vector<mi::u64> spans;
    mi::DevBuf d_hist;
    mi::u64 hist_bytes = 0;
    // the plan from speculative spans (mi_inflate_spec.hip): an indexed plan whose table and windows were made on the device
    bool spec_plan = false;
    mi_inflate_spec_info spec = {};
    ~mi_inflater() {                                    // nothing is under way when the buffers and events go
        if (code) (void)hipStreamSynchronize(code);
        if (copy) (void)hipStreamSynchronize(copy);
    }
    int fail(int code_, const char* fmt, ...) {
        char buf[400];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code_;
    }
};

#define IFCHK(d, call)                                                                                                   \
    do {                                                                                                                 \
        const hipError_t e_ = (call);                                                                                    \
        if (e_ != hipSuccess)                                                                                            \
            return (d)->fail(e_ == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "device inflate: %s failed: %s", #call, \
                             hipGetErrorString(e_));                                                                     \
    } while (0)

namespace mi {

// mi_inflate.hip.  upload: the member goes up through the two pinned buffers; `seen` (may be NULL) is told every piece, in order.
// run_rounds: the rounds of a plan that said DONE, two in flight, through emit (d_dst NULL) or to d_dst (emit NULL); with an indexed
// plan it may return kInflateRefused (d->info.verdict is then MI_INFLATE_INDEX_REFUSED or MI_INFLATE_NOT_PARALLEL)
MI_LOCAL int inflate_upload(mi_inflater* d, const u8* gz, u64 n, mi_inflate_seen_fn seen, void* arg);
MI_LOCAL int inflate_run_rounds(mi_inflater* d, mi_inflate_emit_fn emit, void* arg, u8* d_dst);
// mi_inflate_index.hip.  span_submit: the table of the round's spans [a, b) goes up and inflate_span_kernel decodes them to
// out[0, bytes) (base: the round's first output offset in the member's output) on d->code; span_refused: the verdict of the
// round's bad span `k` comes down and becomes d->info -- kInflateRefused
MI_LOCAL int inflate_span_submit(mi_inflater* d, InfSlot* s, u64 a, u64 b, u64 base, u64 bytes, u8* out);
MI_LOCAL int inflate_span_refused(mi_inflater* d, InfSlot* s, u64 round_first, u64 k);
// mi_inflate_spec.hip.  spec_index: a speculative plan that was run to DONE as a MIGZIX01 index (malloc'ed), the windows brought down
MI_LOCAL int inflate_spec_index(mi_inflater* d, void** index, u64* index_bytes);
// mi_inflate.hip.  mi_tar_inflate_ctx's body -- index (may be NULL): mi_tar_inflate_ctx_indexed's; spec (may be NULL): mi_tar_inflate_ctx_spec's
MI_LOCAL int tar_inflate_ctx_route(mi_ctx* c, const char* blob_path, const u8* index, u64 index_bytes, const InfSpecAsk* spec, const char* tar_path_out,
                                   uint64_t* tar_bytes, uint8_t* tar_sha256, uint8_t* blob_sha256, mi_inflate_info* info, char* err, uint64_t err_cap);

}  // namespace mi
