// mi_inflate_index.hip -- ANY gzip member inflated on the device from an INDEX OF CHECKPOINTS (host_inflate_index.h: the
// format, the builder, the checker).  The index is built once, by zlib, when a blob is pulled for the first time, and kept beside it;
// with it every span between two checkpoints is independent -- its output size is known (no size pass), it needs no marker (any
// encoder's output), and a match that reaches before it reads the checkpoint's window.  Here: inflate_span_kernel (one wave a span,
// mi_inflate_wave.h's one body in its span mode, straight to the span's final offset), the plan from an index over mi_inflate.hip's
// inflater (its streams, slots, upload, rounds and CRC), and the calls: mi_inflate_index_build / _free / _check,
// mi_inflate_buffer_indexed and mi_tar_inflate_ctx_indexed.  (mi_batch_add_layer_blob_indexed is mi_layerblob.hip's.)
//
// The index is only ever A HINT: it is checked on the host before anything goes up, a span that does not end where the index says
// (or breaks any other rule) is a verdict, and the member's CRC-32 and ISIZE decide at the end -- a stale index cannot be told from
// a corrupt blob, so neither is ever MI_ERR_INVALID here: the verdict is MI_INFLATE_INDEX_REFUSED and zlib decides.
#include "mi_internal.h"
#include "mi_inflate_local.h"
#include "mi_inflate_wave.h"
#include "host_inflate_index.h"
#include "host_sha256.h"

#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

namespace mi {

struct InfSpanVerdict { u32 span, rule; u64 bit; };
static_assert(sizeof(InfSpanVerdict) == 16, "a span's verdict is 16 bytes");
constexpr u32 kInfSpanEndsEarly = 0x100;                // (device to host only) the last span's BFINAL block ends before n - 8

// span: six words a span -- in_bit, end_bit (0: the last span), where its bytes go in `out`, how many they are, its window's offset in
// hist[0, hist_total), the window's bytes.  Nothing of the table is trusted: a span whose words point outside the member, the round
// or the window area is refused before a byte is decoded.  *bad: the smallest refused span (~0: none); verdict[k]: why
__global__ __launch_bounds__(64)
void inflate_span_kernel(const u8* __restrict__ gz, u64 n, const u64* __restrict__ span, u64 n_span, u64 round_bytes, u8* __restrict__ out,
                         const u8* __restrict__ hist, u64 hist_total, u64* __restrict__ bad, InfSpanVerdict* __restrict__ verdict) {
    __shared__ InfLds lds;
    const u64 k = blockIdx.x;
    if (k >= n_span) return;
    const u64 in_bit = span[6 * k], end_bit = span[6 * k + 1], at = span[6 * k + 2], bytes = span[6 * k + 3], win_at = span[6 * k + 4],
              win_bytes = span[6 * k + 5];
    u32 rule = 0;
    u64 bit = in_bit;
    if (n < 8 || in_bit / 8 >= n || (end_bit && end_bit <= in_bit) || at > round_bytes || bytes > round_bytes - at || win_bytes > 32768 ||
        win_at > hist_total || win_bytes > hist_total - win_at) {
        rule = mi_host::kInfIndex;
    } else {
        const InfSpan sp = {end_bit, hist + win_at, (u32)win_bytes};
        const InfEnd e = inf_segment<true, true>(gz, n, in_bit, out + at, bytes, &lds, (int)threadIdx.x, &sp);
        bit = e.bit;
        if (e.status > mi_host::kInfSegFinal) rule = e.rule;
        else if (e.out_bytes != bytes) rule = mi_host::kInfIndex;
        else if (!end_bit && e.end != n - 8) rule = e.end < n - 8 ? kInfSpanEndsEarly : (u32)mi_host::kInfIndex;
    }
    if (rule && threadIdx.x == 0) {
        verdict[k] = InfSpanVerdict{(u32)k, rule, bit};
        atomicMin((unsigned long long*)bad, (unsigned long long)k);
    }
}

void launch_inflate_spans(const u8* d_gz, u64 n, const u64* d_span, u64 n_span, u64 round_bytes, u8* d_out, const u8* d_hist, u64 hist_total,
                          u64* d_bad, void* d_verdict, hipStream_t s) {
    if (n_span == 0 || n_span > 0x7FFFFFFFull) return;
    hipLaunchKernelGGL(inflate_span_kernel, dim3((u32)n_span), dim3(64), 0, s, d_gz, n, d_span, n_span, round_bytes, d_out, d_hist, hist_total, d_bad,
                       (InfSpanVerdict*)d_verdict);
}

int inflate_span_submit(mi_inflater* d, InfSlot* s, u64 a, u64 b, u64 base, u64 bytes, u8* out) {
    u64* t = s->h_seg.as<u64>();
    for (u64 k = a; k < b; ++k) {
        memcpy(t + 6 * (k - a), d->spans.data() + 6 * k, 48);
        t[6 * (k - a) + 2] -= base;
    }
    IFCHK(d, hipMemcpyAsync(s->d_seg.p, t, 48 * (b - a), hipMemcpyHostToDevice, d->code));
    launch_inflate_spans(d->d_gz.as<u8>(), d->n, s->d_seg.as<u64>(), b - a, bytes, out, d->d_hist.as<u8>(), d->hist_bytes, s->d_bad.as<u64>(),
                         s->d_verdict.p, d->code);
    return MI_OK;
}

int inflate_span_refused(mi_inflater* d, InfSlot* s, u64 round_first, u64 k) {
    InfSpanVerdict v = {};
    if (k >= s->n_seg) return d->fail(MI_ERR_HIP, "device inflate: the bad word names span %llu of a round of %llu", (unsigned long long)k,
                                      (unsigned long long)s->n_seg);
    IFCHK(d, hipStreamSynchronize(d->code));
    IFCHK(d, hipMemcpy(&v, s->d_verdict.as<InfSpanVerdict>() + k, sizeof v, hipMemcpyDeviceToHost));
    const u64 span = round_first + k;
    d->info.at_in = d->spans[6 * span] / 8;
    d->info.at_out = d->spans[6 * span + 2];
    if (v.rule == kInfSpanEndsEarly) {
        d->info.verdict = MI_INFLATE_NOT_PARALLEL;
        d->info.rule = 0;
        d->fail(kInflateRefused, "the deflate stream ends at bit %llu, before the trailer: more members or trailing bytes", (unsigned long long)v.bit);
    } else {
        d->info.verdict = MI_INFLATE_INDEX_REFUSED;
        d->info.rule = v.rule;
        d->fail(kInflateRefused, "span %llu at input bit %llu (output offset %llu) breaks rule %u at bit %llu: %s", (unsigned long long)span,
                (unsigned long long)d->spans[6 * span], (unsigned long long)d->info.at_out, v.rule, (unsigned long long)v.bit,
                mi_host::inflate_rule_name(v.rule));
    }
    return kInflateRefused;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_inflater_plan_indexed(mi_inflater* d, const uint8_t* gz, uint64_t n, const uint8_t* index, uint64_t index_bytes, mi_inflate_seen_fn seen,
                             void* arg) {
    if (!d || !gz || !index) return MI_ERR_INVALID;
    IFCHK(d, hipSetDevice(d->ctx->device));
    d->info = mi_inflate_info();
    d->info.in_bytes = n;
    d->n = n;
    d->indexed = true;
    const int refusal = mi_host::index_check(index, index_bytes, gz, n);
    if (refusal) {
        d->info.verdict = MI_INFLATE_INDEX_REFUSED;
        d->info.reserved = (u32)refusal;
        d->fail(MI_OK, "the index is refused (%d): %s", refusal, mi_host::index_refusal_text(refusal));
        return MI_OK;
    }
    mi_host::IndexHead h;
    mi_host::index_head(index, &h);
    d->header = h.header;
    d->want_crc = mi_host::inflate_le32(gz + n - 8);
    d->want_isize = mi_host::inflate_le32(gz + n - 4);
    d->chain = mi_host::InflateChain();
    d->spans.resize(6 * h.n_points);
    for (u64 k = 0; k < h.n_points; ++k) {
        const mi_host::IndexPoint p = mi_host::index_point(index, k);
        const u64 next_out = k + 1 < h.n_points ? mi_host::index_point(index, k + 1).out_at : h.out_bytes;
        const u64 end_bit = k + 1 < h.n_points ? mi_host::index_point(index, k + 1).in_bit : 0;
        const u64 row[6] = {p.in_bit, end_bit, p.out_at, next_out - p.out_at, p.win_at, p.win_bytes};
        memcpy(d->spans.data() + 6 * k, row, sizeof row);
        d->chain.segs.push_back(mi_host::InflateSeg{p.in_bit / 8, p.out_at, next_out - p.out_at, k});
        if (next_out - p.out_at > d->window) {             // no span is split: zlib takes the member
            d->info.verdict = MI_INFLATE_NOT_PARALLEL;
            d->info.rule = mi_host::kInfWindow;
            d->info.at_in = p.in_bit / 8;
            d->info.at_out = p.out_at;
            return MI_OK;
        }
    }
    d->chain.end = mi_host::kInfChainDone;
    d->chain.total = h.out_bytes;
    d->chain.at_in = d->chain.segs.back().in_at;
    d->chain.at_out = d->chain.segs.back().out_at;
    int rc = inflate_upload(d, gz, n, seen, arg);
    if (rc) return rc;
    const u8* windows = index + mi_host::kIndexHeader + mi_host::kIndexRow * h.n_points;
    d->hist_bytes = h.windows_bytes;
    d->d_hist.release();
    if (h.windows_bytes) {
        if (guard_alloc()) {                                // exactly the area: its last byte is the allocation's last
            void* p = nullptr;
            IFCHK(d, dev_alloc(&p, (size_t)h.windows_bytes));
            d->d_hist.p = p;
            d->d_hist.bytes = (size_t)h.windows_bytes;
        } else {
            IFCHK(d, d->d_hist.alloc_exact(h.windows_bytes));
        }
        IFCHK(d, hipMemcpyAsync(d->d_hist.p, windows, h.windows_bytes, hipMemcpyHostToDevice, d->copy));
        IFCHK(d, hipStreamSynchronize(d->copy));
    }
    d->info.n_candidates = h.n_points;
    d->info.n_segments = h.n_points;
    d->info.at_in = d->chain.at_in;
    d->info.at_out = d->chain.at_out;
    d->info.verdict = MI_INFLATE_DONE;
    d->info.out_bytes = h.out_bytes;
    mi_host::inflate_rounds(d->chain.segs, d->window, &d->round_first);
    d->info.n_rounds = d->round_first.size() - 1;
    return MI_OK;
}

// ---- the index itself: host only ---------------------------------------------------------------------------------------------------
int mi_inflate_index_build(const void* gz, uint64_t n, uint64_t spacing, void** index, uint64_t* index_bytes, mi_inflate_index_info* info,
                           uint8_t* tar_sha256, char* err, uint64_t err_cap) {
    if (index) *index = nullptr;
    if (index_bytes) *index_bytes = 0;
    if (info) memset(info, 0, sizeof *info);
    if (err && err_cap) err[0] = 0;
    if (!gz || !index || !index_bytes) return MI_ERR_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<u8> ix;
    mi_host::IndexBuilt built;
    mi_host::Sha256 sha;
    std::string why;
    if (!mi_host::index_build((const u8*)gz, n, spacing, &ix, &built, tar_sha256 ? &sha : nullptr, &why)) {
        if (err && err_cap) snprintf(err, (size_t)err_cap, "mi_inflate_index_build: %s", why.c_str());
        return MI_ERR_INVALID;
    }
    void* p = malloc(ix.size());
    if (!p) return MI_ERR_NOMEM;
    memcpy(p, ix.data(), ix.size());
    *index = p;
    *index_bytes = ix.size();
    if (tar_sha256) sha.final(tar_sha256);
    if (info) {
        info->n_points = built.n_points;
        info->n_blocks = built.n_blocks;
        info->out_bytes = built.out_bytes;
        info->windows_bytes = built.windows_bytes;
        info->spacing = built.spacing;
        info->ms_build = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return MI_OK;
}

void mi_inflate_index_free(void* index) { free(index); }

int mi_inflate_index_check(const void* index, uint64_t index_bytes, const void* gz, uint64_t n) {
    return mi_host::index_check((const u8*)index, index_bytes, (const u8*)gz, n);
}

const char* mi_inflate_index_refusal(int refusal) { return mi_host::index_refusal_text(refusal); }

// ---- the calls -------------------------------------------------------------------------------------------------------------------
namespace {
struct IndexedSink { u8* dst; u64 at; };
int indexed_buffer_emit(void* arg, const uint8_t* bytes, uint64_t n) {
    IndexedSink* b = (IndexedSink*)arg;
    memcpy(b->dst + b->at, bytes, n);                   // (cap >= the index's total: checked before anything went up)
    b->at += n;
    return MI_OK;
}
}  // namespace

int mi_inflate_buffer_indexed(mi_ctx* c, const void* gz, uint64_t n, const void* index, uint64_t index_bytes, void* dst, uint64_t cap,
                              uint64_t* out_bytes, mi_inflate_info* info) {
    if (!c || !gz || !index || !out_bytes || (!dst && cap)) return MI_ERR_INVALID;
    *out_bytes = 0;
    if (info) memset(info, 0, sizeof *info);
    if (mi_host::index_check((const u8*)index, index_bytes, (const u8*)gz, n) == 0) {
        mi_host::IndexHead h;
        mi_host::index_head((const u8*)index, &h);
        if (h.out_bytes > cap) {                            // known from the index: before any device work
            *out_bytes = h.out_bytes;
            if (info) { info->in_bytes = n; info->out_bytes = h.out_bytes; info->n_candidates = info->n_segments = h.n_points; }
            return fail(c, MI_ERR_CAPACITY, "mi_inflate_buffer_indexed: the member inflates to %llu bytes, dst holds %llu",
                        (unsigned long long)h.out_bytes, (unsigned long long)cap);
        }
    }
    mi_inflater* d = nullptr;
    int rc = mi_inflater_create(c, &d);
    if (rc) return rc;
    rc = mi_inflater_plan_indexed(d, (const u8*)gz, n, (const u8*)index, index_bytes, nullptr, nullptr);
    if (rc == MI_OK && d->info.verdict == MI_INFLATE_DONE) {
        IndexedSink sink{(u8*)dst, 0};
        rc = mi_inflater_run(d, indexed_buffer_emit, &sink);
        if (rc == MI_OK) *out_bytes = sink.at;
        if (rc == kInflateRefused) rc = MI_OK;              // a verdict, not an error: nothing is delivered
    }
    if (rc) fail(c, rc, "mi_inflate_buffer_indexed: %s", d->err.c_str());
    if (info) *info = d->info;
    mi_inflater_free(d);
    return rc;
}

int mi_tar_inflate_ctx_indexed(mi_ctx* c, const char* blob_path, const void* index, uint64_t index_bytes, const char* tar_path_out, uint64_t* tar_bytes,
                               uint8_t* tar_sha256, uint8_t* blob_sha256, mi_inflate_info* info, char* err, uint64_t err_cap) {
    if (!c || !blob_path || !index) return MI_ERR_INVALID;
    return mi_tar_inflate_ctx_with(c, blob_path, (const u8*)index, index_bytes, tar_path_out, tar_bytes, tar_sha256, blob_sha256, info, err, err_cap);
}

}  // extern "C"
