// mi_inflate.hip -- the DEVICE INFLATE of a pulled layer's gzip blob: the kernels over mi_inflate_wave.h's one
// body, the object that moves a member through them (mi_inflater_*, hidden), and the two calls on top of it: mi_inflate_buffer
// (a member in host memory in, its inflation out) and mi_tar_inflate_ctx (mi_tar_inflate's contract on the device).
//
// The member goes up whole (it is the smaller side) and through
//   inflate_mark_count_kernel    a tile of positions: how many are candidates (00 00 FF FF in front, or the header's end)
//   inflate_mark_scan_kernel     mi_plan.h's one-block scan over the tiles' counts
//   inflate_mark_scatter_kernel  the candidates, ascending
//   inflate_size_kernel          one wave a candidate: its row, no byte written
// then the rows come down, the host walks the live chain (host_inflate.h), gives every live segment its output offset and cuts
// the segments into rounds whose output fits the window.  A round is
//   inflate_write_kernel         one wave a live segment: the decode again, to its final offset in the round's output
//   crc32.hip's tiles and fold over the round's output as ONE file: the rounds' CRCs are combined on the host
// and comes down through a pinned window.  TWO ROUNDS are in flight, on streams of the object's own (never the ctx's scan stream):
// round k comes down on the copy stream while round k + 1 is decoded on the code stream.  With a DEVICE DESTINATION
// (mi_inflater_run_device, DESIGN 4.21: a layer inflated into a batch's arena) a round is decoded where it belongs in the caller's
// memory, its CRC taken there, and only the CRC and the bad word come down.
#include "mi_internal.h"
#include "mi_inflate_local.h"
#include "mi_inflate_wave.h"
#include "mi_plan.h"
#include "host_sha256.h"

#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

namespace mi {

// the positions [base, base + kPlanPer) that are candidates, as a mask: p == header, or 4 <= p <= n - 8 with 00 00 FF FF in front.
// n_pos = n - 7 positions exist (0 .. n - 8); a thread sees the bytes [base - 4, base + kPlanPer - 1), each index below n
static __device__ __forceinline__ u32 inflate_mark_mask(const u8* __restrict__ gz, u64 n_pos, u64 header, u64 base) {
    u32 sel = 0, w = 0;                                 // w: the four bytes in front of p, the nearest one highest
    for (int k = 4; k >= 2; --k) w = w >> 8 | (base >= (u64)k && base - k < n_pos + 7 ? (u32)gz[base - k] << 24 : 0u);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const u64 p = base + k;
        if (p >= n_pos) break;
        if (p >= 1) w = w >> 8 | (u32)gz[p - 1] << 24;  // p - 1 <= n - 9
        if ((p >= 4 && w == 0xFFFF0000u) || p == header) sel |= 1u << k;
    }
    return sel;
}

__global__ __launch_bounds__(kPlanBlock)
void inflate_mark_count_kernel(const u8* __restrict__ gz, u64 n_pos, u64 header, u64* __restrict__ block_cnt) {
    __shared__ u64 lds[1][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[1] = {(u64)__popc(inflate_mark_mask(gz, n_pos, header, base))};
    plan_block_sum<1>(v, lds);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = v[0];
}

__global__ __launch_bounds__(kPlanBlock)
void inflate_mark_scan_kernel(u64* __restrict__ block_cnt, u64 n_blocks, u64* __restrict__ total) {
    plan_block_offsets<false>(block_cnt, nullptr, n_blocks, total, nullptr);
}

__global__ __launch_bounds__(kPlanBlock)
void inflate_mark_scatter_kernel(const u8* __restrict__ gz, u64 n_pos, u64 header, const u64* __restrict__ block_cnt, u64 n_cand,
                                 u64* __restrict__ cand) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    const u32 sel = inflate_mark_mask(gz, n_pos, header, base);
    u64 at = plan_first((u64)__popc(sel), block_cnt);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
        if ((sel & (1u << k)) && at < n_cand) cand[at++] = base + k;
}

__global__ __launch_bounds__(64)
void inflate_size_kernel(const u8* __restrict__ gz, u64 n, const u64* __restrict__ cand, u64 n_cand, u64 window,
                         mi_host::InflateRow* __restrict__ rows) {
    __shared__ InfLds lds;
    const u64 k = blockIdx.x;
    if (k >= n_cand) return;
    const u64 start = cand[k];
    if (start >= n) return;
    const InfEnd e = inf_segment<false>(gz, n, start, nullptr, window, &lds, (int)threadIdx.x);
    if (threadIdx.x == 0) rows[k] = mi_host::InflateRow{e.end, e.out_bytes, e.status, e.rule, e.bit};
}

// seg: three words a live segment of the round -- where it starts in the member, where its bytes go in `out`, how many they are.
// *bad: the smallest segment whose second decode did not end as its row said (~0: none)
__global__ __launch_bounds__(64)
void inflate_write_kernel(const u8* __restrict__ gz, u64 n, const u64* __restrict__ seg, u64 n_seg, u64 round_bytes, u8* __restrict__ out,
                          u64* __restrict__ bad) {
    __shared__ InfLds lds;
    const u64 k = blockIdx.x;
    if (k >= n_seg) return;
    const u64 start = seg[3 * k], at = seg[3 * k + 1], bytes = seg[3 * k + 2];
    if (start >= n || at > round_bytes || bytes > round_bytes - at) return;
    const InfEnd e = inf_segment<true>(gz, n, start, out + at, bytes, &lds, (int)threadIdx.x);
    if (threadIdx.x == 0 && (e.status > mi_host::kInfSegFinal || e.out_bytes != bytes)) atomicMin((unsigned long long*)bad, (unsigned long long)k);
}

// (hidden: the kernel probe's) the table builder alone: lens[0, nsym) -> what inf_build says of them, and the symbols the bit
// string bits[0, n_bits) decodes to under the primary table of `tab_bits` bits (at most max_out; kInfNoSymbol ends the list)
__global__ __launch_bounds__(64)
void inflate_table_kernel(const u8* __restrict__ lens, u32 nsym, u32 tab_bits, const u8* __restrict__ bits, u32 n_bits, u32* __restrict__ verdict,
                          u32* __restrict__ out, u32 max_out) {
    __shared__ InfLds lds;
    const int lane = (int)threadIdx.x;
    for (u32 i = lane; i < kInfMaxLit; i += 64) lds.lens[i] = i < nsym ? lens[i] & 15u : 0u;
    const InfBuilt t = inf_build(lds.lens, nsym, lds.lit_tab, tab_bits, lds.lit_sym, &lds.lit, lds.cnt, lane);
    if (lane == 0) { verdict[0] = t.over ? 1u : 0u; verdict[1] = t.over ? 0u : (u32)t.left; verdict[2] = t.total; verdict[3] = t.max_len; }
    u32 made = 0;
    if (!t.over) {
        InfBits b;
        b.gz = bits;
        b.n = (n_bits + 7) / 8;
        inf_seek(&b, 0, lane);
        while (made < max_out && inf_bit(&b) < n_bits) {
            inf_need(&b, lane);
            const u32 s = inf_symbol(&b, lds.lit_tab, tab_bits, lds.lit_sym, &lds.lit);
            if (lane == 0) out[made] = s;
            ++made;
            if (s == kInfNoSymbol) break;
        }
    }
    if (lane == 0) verdict[4] = made;
}

void launch_inflate_table(const u8* d_lens, u32 nsym, u32 tab_bits, const u8* d_bits, u32 n_bits, u32* d_verdict, u32* d_out, u32 max_out,
                          hipStream_t s) {
    if (nsym == 0 || nsym > kInfMaxLit || tab_bits < 1 || tab_bits > kInfLitBits) return;
    hipLaunchKernelGGL(inflate_table_kernel, dim3(1), dim3(64), 0, s, d_lens, nsym, tab_bits, d_bits, n_bits, d_verdict, d_out, max_out);
}

// (hidden: the kernel probe's) the size pass over given starts, and the write pass over a given segment table
void launch_inflate_rows(const u8* d_gz, u64 n, const u64* d_starts, u64 n_starts, u64 window, void* d_rows, hipStream_t s) {
    if (n_starts == 0 || n_starts > 0x7FFFFFFFull) return;
    hipLaunchKernelGGL(inflate_size_kernel, dim3((u32)n_starts), dim3(64), 0, s, d_gz, n, d_starts, n_starts, window, (mi_host::InflateRow*)d_rows);
}

void launch_inflate_write(const u8* d_gz, u64 n, const u64* d_seg, u64 n_seg, u64 round_bytes, u8* d_out, u64* d_bad, hipStream_t s) {
    if (n_seg == 0 || n_seg > 0x7FFFFFFFull) return;
    hipLaunchKernelGGL(inflate_write_kernel, dim3((u32)n_seg), dim3(64), 0, s, d_gz, n, d_seg, n_seg, round_bytes, d_out, d_bad);
}

}  // namespace mi

using namespace mi;
using mi_host::InflateRow;

namespace {

constexpr u64 kMiB = 1ull << 20;
constexpr u64 kStage = 4 * kMiB;                        // the member goes up in pieces of this, through two pinned buffers
typedef InfSlot Slot;

u64 inflate_window() {
    u64 mb = 64;
    if (const char* e = getenv("MI_INFLATE_WINDOW_MB")) { const long v = atol(e); if (v >= 1 && v <= 1024) mb = (u64)v; }
    return mb * kMiB;
}

}  // namespace

// the member goes up through the two pinned buffers; `seen` (may be NULL) is told every piece, in order, while it is under way
int mi::inflate_upload(mi_inflater* d, const u8* gz, u64 n, mi_inflate_seen_fn seen, void* arg) {
    if (guard_alloc()) {                                // exactly n bytes: the member's last byte is the allocation's last
        d->d_gz.release();
        void* p = nullptr;
        IFCHK(d, dev_alloc(&p, (size_t)n));
        d->d_gz.p = p;
        d->d_gz.bytes = (size_t)n;
    } else {
        IFCHK(d, d->d_gz.alloc_exact(n));
    }
    const u64 piece = n < kStage ? n : kStage;
    for (int k = 0; k < 2; ++k) {
        if (k == 1 && n <= kStage) break;
        IFCHK(d, d->h_stage[k].ensure(piece));
        IFCHK(d, d->staged[k].create(hipEventDisableTiming));
    }
    int k = 0;
    for (u64 at = 0; at < n; at += kStage, k ^= 1) {
        const u64 take = n - at < kStage ? n - at : kStage;
        if (at >= 2 * kStage) IFCHK(d, hipEventSynchronize(d->staged[k]));
        memcpy(d->h_stage[k].p, gz + at, take);
        IFCHK(d, hipMemcpyAsync(d->d_gz.as<u8>() + at, d->h_stage[k].p, take, hipMemcpyHostToDevice, d->copy));
        IFCHK(d, hipEventRecord(d->staged[k], d->copy));
        if (seen) seen(arg, gz + at, take);
    }
    IFCHK(d, hipStreamSynchronize(d->copy));
    return MI_OK;
}

namespace {

// windows: the round's output lies in the slot's own d_out and comes down through h_out (false: the caller's device destination)
int slot_prepare(mi_inflater* d, Slot* s, u64 out_bytes, u64 n_seg, bool windows) {
    const u64 nt = (out_bytes + kGearTile - 1) / kGearTile;
    if (!s->h_small.p) {
        IFCHK(d, s->h_small.ensure(64));
        IFCHK(d, s->d_row.alloc_exact(24));
        IFCHK(d, s->d_crc.alloc_exact(4));
        IFCHK(d, s->d_bad.alloc_exact(8));
        IFCHK(d, s->done.create(hipEventDisableTiming));
        IFCHK(d, s->down.create(hipEventDisableTiming));
        IFCHK(d, s->t0.create());
        IFCHK(d, s->t1.create());
    }
    if (windows ? out_bytes > s->h_out.bytes || !s->d_out.p : nt * 4 + 256 > s->d_tile_file.bytes) {
        if (windows) {
            IFCHK(d, s->h_out.ensure(out_bytes ? out_bytes : 1));
            IFCHK(d, s->d_out.alloc_exact(out_bytes));
        }
        IFCHK(d, s->d_tile_file.alloc_exact(nt * 4));
        IFCHK(d, s->d_tile_raw.alloc_exact(nt * 4));
        if (nt) IFCHK(d, hipMemsetAsync(s->d_tile_file.p, 0, nt * 4, d->code));     // every tile is file 0's
    }
    const u64 row = d->indexed ? 48 : 24;               // a span's six words, a segment's three
    if (row * n_seg > s->h_seg.bytes) {
        IFCHK(d, s->h_seg.ensure(row * n_seg));
        IFCHK(d, s->d_seg.alloc_exact(row * n_seg));
    }
    if (d->indexed && 16 * n_seg > s->d_verdict.bytes) IFCHK(d, s->d_verdict.alloc_exact(16 * n_seg));
    return MI_OK;
}

// round r of the plan: its segments' table goes up, the decode, the CRC, the bytes on their way down; s->down is its end.
// d_dst (may be NULL: the slot's window): the member's inflation lies at d_dst[0, total) -- the round is written where it
// belongs there and no byte comes down
int slot_submit(mi_inflater* d, Slot* s, u64 r, u8* d_dst) {
    const u64 a = d->round_first[r], b = d->round_first[r + 1];
    const mi_host::InflateSeg* segs = d->chain.segs.data();
    const u64 base = segs[a].out_at;
    u64* t = s->h_seg.as<u64>();
    u64 bytes = 0;
    for (u64 k = a; k < b; ++k) {
        if (!d->indexed) {
            t[3 * (k - a)] = segs[k].in_at;
            t[3 * (k - a) + 1] = segs[k].out_at - base;
            t[3 * (k - a) + 2] = segs[k].out_bytes;
        }
        bytes += segs[k].out_bytes;
    }
    s->bytes = bytes;
    s->n_seg = b - a;
    u64* row = s->h_small.as<u64>();
    row[0] = 0; row[1] = bytes; row[2] = 0; row[4] = 0; row[5] = ~0ull;
    u8* out = d_dst ? d_dst + base : s->d_out.as<u8>();
    if (!d->indexed) IFCHK(d, hipMemcpyAsync(s->d_seg.p, t, 24 * s->n_seg, hipMemcpyHostToDevice, d->code));
    IFCHK(d, hipMemcpyAsync(s->d_row.p, row, 24, hipMemcpyHostToDevice, d->code));
    IFCHK(d, hipMemcpyAsync(s->d_bad.p, row + 5, 8, hipMemcpyHostToDevice, d->code));
    IFCHK(d, hipEventRecord(s->t0, d->code));
    if (d->indexed) {
        const int rc = inflate_span_submit(d, s, a, b, base, bytes, out);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(inflate_write_kernel, dim3((u32)s->n_seg), dim3(64), 0, d->code, d->d_gz.as<u8>(), d->n, s->d_seg.as<u64>(), s->n_seg, bytes,
                           out, s->d_bad.as<u64>());
    }
    IFCHK(d, hipEventRecord(s->t1, d->code));
    if (bytes) {
        const u64* rw = s->d_row.as<u64>();
        launch_crc32_files(out, rw, rw + 1, s->d_tile_file.as<u32>(), rw + 2, (bytes + kGearTile - 1) / kGearTile, 1,
                           d->ctx->crc_consts.as<u32>(), s->d_tile_raw.as<u32>(), s->d_crc.as<u32>(), d->code);
        IFCHK(d, hipMemcpyAsync(row + 4, s->d_crc.p, 4, hipMemcpyDeviceToHost, d->code));
    }
    IFCHK(d, hipGetLastError());
    IFCHK(d, hipMemcpyAsync(row + 5, s->d_bad.p, 8, hipMemcpyDeviceToHost, d->code));
    IFCHK(d, hipEventRecord(s->done, d->code));
    IFCHK(d, hipStreamWaitEvent(d->copy, s->done, 0));
    if (bytes && !d_dst) IFCHK(d, hipMemcpyAsync(s->h_out.p, s->d_out.p, bytes, hipMemcpyDeviceToHost, d->copy));
    IFCHK(d, hipEventRecord(s->down, d->copy));
    s->pending = true;
    return MI_OK;
}

struct RunState { u32 crc = 0; u64 bytes = 0; };

// waits for the round, folds its CRC into the member's and hands its bytes on (emit NULL: they stay where they are)
int slot_finish(mi_inflater* d, Slot* s, u64 r, RunState* st, mi_inflate_emit_fn emit, void* arg) {
    if (!s->pending) return MI_OK;
    s->pending = false;
    IFCHK(d, hipEventSynchronize(s->down));
    const u64* row = s->h_small.as<u64>();
    if (row[5] != ~0ull && d->indexed) return inflate_span_refused(d, s, d->round_first[r], row[5]);
    if (row[5] != ~0ull)
        return d->fail(MI_ERR_HIP, "device inflate: segment %llu of a round did not decode a second time as it did the first", (unsigned long long)row[5]);
    float ms = 0;
    IFCHK(d, hipEventElapsedTime(&ms, s->t0, s->t1));
    d->info.ms_write += ms;
    if (s->bytes) {
        st->crc = st->bytes ? crc32_host_combine(st->crc, (u32)row[4], s->bytes) : (u32)row[4];
        st->bytes += s->bytes;
    }
    return s->bytes && emit ? emit(arg, s->h_out.as<u8>(), s->bytes) : MI_OK;
}

}  // namespace

extern "C" {

int mi_inflater_create(mi_ctx* c, mi_inflater** out) {
    if (!c || !out) return MI_ERR_INVALID;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    mi_inflater* d = new mi_inflater();
    d->ctx = c;
    d->window = inflate_window();
    if (d->code.create() != hipSuccess || d->copy.create() != hipSuccess || d->t0.create() != hipSuccess || d->t1.create() != hipSuccess) {
        delete d;
        return fail(c, MI_ERR_HIP, "mi_inflater_create: no stream");
    }
    *out = d;
    return MI_OK;
}

const char* mi_inflater_error(const mi_inflater* d) { return d ? d->err.c_str() : "null inflater"; }
void mi_inflater_info(const mi_inflater* d, mi_inflate_info* out) { if (d && out) *out = d->info; }

int mi_inflater_plan(mi_inflater* d, const uint8_t* gz, uint64_t n, mi_inflate_seen_fn seen, void* arg) {
    if (!d || !gz) return MI_ERR_INVALID;
    IFCHK(d, hipSetDevice(d->ctx->device));
    d->info = mi_inflate_info();
    d->info.in_bytes = n;
    d->n = n;
    if (!mi_host::gzip_header(gz, n, &d->header))
        return d->fail(MI_ERR_INVALID, "device inflate: no gzip header (magic, method 8, no reserved flag, complete) in a member of %llu bytes",
                       (unsigned long long)n);
    if (n < d->header + 8 + 1)
        return d->fail(MI_ERR_INVALID, "device inflate: a member of %llu bytes ends behind its %llu header bytes: no stream, no trailer",
                       (unsigned long long)n, (unsigned long long)d->header);
    d->want_crc = mi_host::inflate_le32(gz + n - 8);
    d->want_isize = mi_host::inflate_le32(gz + n - 4);
    int rc = inflate_upload(d, gz, n, seen, arg);
    if (rc) return rc;
    const u64 n_pos = n - 7, nb = (n_pos + kPlanTile - 1) / kPlanTile;
    IFCHK(d, d->d_blk.alloc_exact(nb * 8));
    IFCHK(d, d->d_tot.alloc_exact(8));
    IFCHK(d, hipEventRecord(d->t0, d->code));
    hipLaunchKernelGGL(inflate_mark_count_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, d->code, d->d_gz.as<u8>(), n_pos, d->header, d->d_blk.as<u64>());
    hipLaunchKernelGGL(inflate_mark_scan_kernel, dim3(1), dim3(kPlanBlock), 0, d->code, d->d_blk.as<u64>(), nb, d->d_tot.as<u64>());
    IFCHK(d, hipGetLastError());
    u64 n_cand = 0;
    IFCHK(d, hipMemcpyAsync(&n_cand, d->d_tot.p, 8, hipMemcpyDeviceToHost, d->code));
    IFCHK(d, hipStreamSynchronize(d->code));
    if (n_cand == 0 || n_cand > n_pos) return d->fail(MI_ERR_HIP, "device inflate: %llu candidates among %llu positions", (unsigned long long)n_cand,
                                                      (unsigned long long)n_pos);
    IFCHK(d, d->d_cand.alloc_exact(n_cand * 8));
    IFCHK(d, d->d_rows.alloc_exact(n_cand * sizeof(InflateRow)));
    IFCHK(d, hipMemsetAsync(d->d_rows.p, 0xFF, n_cand * sizeof(InflateRow), d->code));   // a row nobody wrote is no status at all
    hipLaunchKernelGGL(inflate_mark_scatter_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, d->code, d->d_gz.as<u8>(), n_pos, d->header, d->d_blk.as<u64>(),
                       n_cand, d->d_cand.as<u64>());
    hipLaunchKernelGGL(inflate_size_kernel, dim3((u32)n_cand), dim3(64), 0, d->code, d->d_gz.as<u8>(), n, d->d_cand.as<u64>(), n_cand, d->window,
                       d->d_rows.as<InflateRow>());
    IFCHK(d, hipGetLastError());
    IFCHK(d, hipEventRecord(d->t1, d->code));
    d->cand.resize(n_cand);
    d->rows.resize(n_cand);
    IFCHK(d, hipMemcpyAsync(d->cand.data(), d->d_cand.p, n_cand * 8, hipMemcpyDeviceToHost, d->code));
    IFCHK(d, hipMemcpyAsync(d->rows.data(), d->d_rows.p, n_cand * sizeof(InflateRow), hipMemcpyDeviceToHost, d->code));
    IFCHK(d, hipStreamSynchronize(d->code));
    float ms = 0;
    IFCHK(d, hipEventElapsedTime(&ms, d->t0, d->t1));
    d->info.ms_size = ms;
    d->info.n_candidates = n_cand;
    mi_host::inflate_chain(d->cand.data(), d->rows.data(), n_cand, d->header, n, &d->chain);
    const mi_host::InflateChain& ch = d->chain;
    d->info.n_segments = ch.segs.size();
    d->info.at_in = ch.at_in;
    d->info.at_out = ch.at_out;
    d->info.rule = ch.rule;
    switch (ch.end) {
    case mi_host::kInfChainDone:
        d->info.verdict = MI_INFLATE_DONE;
        d->info.out_bytes = ch.total;
        mi_host::inflate_rounds(ch.segs, d->window, &d->round_first);
        d->info.n_rounds = d->round_first.size() - 1;
        return MI_OK;
    case mi_host::kInfChainNotParallel:
        d->info.verdict = MI_INFLATE_NOT_PARALLEL;
        return MI_OK;
    case mi_host::kInfChainCorrupt:
        return d->fail(MI_ERR_INVALID, "corrupt gzip stream: the segment at input offset %llu (output offset %llu) breaks rule %u at bit %llu: %s",
                       (unsigned long long)ch.at_in, (unsigned long long)ch.at_out, ch.rule, (unsigned long long)ch.bit,
                       mi_host::inflate_rule_name(ch.rule));
    default:
        return d->fail(MI_ERR_HIP, "device inflate: the rows contradict the candidates at input offset %llu (%llu candidates)",
                       (unsigned long long)ch.at_in, (unsigned long long)n_cand);
    }
}

}  // extern "C"

// the rounds of a plan that said DONE, two in flight: through emit (d_dst NULL) or to d_dst (emit NULL)
int mi::inflate_run_rounds(mi_inflater* d, mi_inflate_emit_fn emit, void* arg, u8* d_dst) {
    if (d->info.verdict != MI_INFLATE_DONE || d->round_first.empty()) return d->fail(MI_ERR_STATE, "device inflate: run without a plan");
    IFCHK(d, hipSetDevice(d->ctx->device));
    const u64 n_rounds = d->round_first.size() - 1;
    u64 most_bytes = 0, most_seg = 0;
    for (u64 r = 0; r < n_rounds; ++r) {
        const u64 a = d->round_first[r], b = d->round_first[r + 1];
        const u64 bytes = (b < d->chain.segs.size() ? d->chain.segs[b].out_at : d->chain.total) - d->chain.segs[a].out_at;
        if (bytes > most_bytes) most_bytes = bytes;
        if (b - a > most_seg) most_seg = b - a;
    }
    RunState st;
    int rc = MI_OK;
    for (u64 r = 0; r < n_rounds && rc == MI_OK; ++r) {
        Slot* s = &d->slot[r & 1];
        rc = slot_finish(d, s, r - 2, &st, emit, arg);      // round r - 2, while r - 1 is under way (nothing is pending before round 2)
        if (rc == MI_OK) rc = slot_prepare(d, s, most_bytes, most_seg, d_dst == nullptr);
        if (rc == MI_OK) rc = slot_submit(d, s, r, d_dst);
    }
    for (u64 r = n_rounds; r < n_rounds + 2 && rc == MI_OK; ++r) rc = slot_finish(d, &d->slot[r & 1], r - 2, &st, emit, arg);
    if (rc != MI_OK) {
        (void)hipStreamSynchronize(d->code);
        (void)hipStreamSynchronize(d->copy);
        d->slot[0].pending = d->slot[1].pending = false;
        return rc;
    }
    if (st.bytes != d->chain.total) return d->fail(MI_ERR_HIP, "device inflate: the rounds gave %llu bytes, the plan %llu", (unsigned long long)st.bytes,
                                                   (unsigned long long)d->chain.total);
    if (d->indexed && (st.crc != d->want_crc || (u32)st.bytes != d->want_isize)) {     // a stale index cannot be told from a corrupt blob: zlib decides
        d->info.verdict = MI_INFLATE_INDEX_REFUSED;
        d->info.rule = 0;
        d->fail(kInflateRefused, "the spans gave %llu bytes with CRC-32 %08x, the trailer states %u (mod 2^32) and %08x", (unsigned long long)st.bytes, st.crc,
                d->want_isize, d->want_crc);
        return kInflateRefused;
    }
    if (st.crc != d->want_crc || (u32)st.bytes != d->want_isize)
        return d->fail(MI_ERR_INVALID, "corrupt gzip stream: %llu bytes with CRC-32 %08x, the trailer states %u (mod 2^32) and %08x; the last segment "
                       "lies at input offset %llu (output offset %llu)", (unsigned long long)st.bytes, st.crc, d->want_isize, d->want_crc,
                       (unsigned long long)d->chain.at_in, (unsigned long long)d->chain.at_out);
    return MI_OK;
}

extern "C" {

int mi_inflater_run(mi_inflater* d, mi_inflate_emit_fn emit, void* arg) {
    if (!d || !emit) return MI_ERR_INVALID;
    return inflate_run_rounds(d, emit, arg, nullptr);
}

// what lies at d_dst was put there on wait_for (may be NULL: nothing to wait for) -- the rounds begin behind it
int mi_inflater_run_device(mi_inflater* d, uint8_t* d_dst, hipStream_t wait_for) {
    if (!d || !d_dst) return MI_ERR_INVALID;
    if (wait_for) IFCHK(d, hipStreamSynchronize(wait_for));
    return inflate_run_rounds(d, nullptr, nullptr, d_dst);
}

void mi_inflater_free(mi_inflater* d) {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    delete d;
}

namespace {
struct BufferSink { u8* dst; u64 at; };
int inflate_buffer_emit(void* arg, const uint8_t* bytes, uint64_t n) {
    BufferSink* b = (BufferSink*)arg;
    memcpy(b->dst + b->at, bytes, n);                   // (cap >= the plan's total: checked before the first round)
    b->at += n;
    return MI_OK;
}
}  // namespace

int mi_inflate_buffer(mi_ctx* c, const void* gz, uint64_t n, void* dst, uint64_t cap, uint64_t* out_bytes, mi_inflate_info* info) {
    if (!c || !gz || !out_bytes || (!dst && cap)) return MI_ERR_INVALID;
    *out_bytes = 0;
    if (info) memset(info, 0, sizeof *info);
    mi_inflater* d = nullptr;
    int rc = mi_inflater_create(c, &d);
    if (rc) return rc;
    rc = mi_inflater_plan(d, (const u8*)gz, n, nullptr, nullptr);
    if (rc == MI_OK && d->info.verdict == MI_INFLATE_DONE) {
        if (d->info.out_bytes > cap) {
            *out_bytes = d->info.out_bytes;
            if (info) *info = d->info;
            mi_inflater_free(d);
            return fail(c, MI_ERR_CAPACITY, "mi_inflate_buffer: the member inflates to %llu bytes, dst holds %llu", (unsigned long long)*out_bytes,
                        (unsigned long long)cap);
        }
        BufferSink sink{(u8*)dst, 0};
        rc = mi_inflater_run(d, inflate_buffer_emit, &sink);
        if (rc == MI_OK) *out_bytes = sink.at;
    }
    if (rc) fail(c, rc, "mi_inflate_buffer: %s", d->err.c_str());
    if (info) *info = d->info;
    mi_inflater_free(d);
    return rc;
}

namespace {
void inflate_put_err(char* err, uint64_t cap, const std::string& msg) {
    if (err && cap) snprintf(err, (size_t)cap, "%s", msg.c_str());
}
void inflate_sha_seen(void* arg, const uint8_t* bytes, uint64_t n) { ((mi_host::Sha256*)arg)->update(bytes, (size_t)n); }
struct TarSink { int fd; mi_host::Sha256 sha; u64 bytes; int io_errno; };
int inflate_tar_emit(void* arg, const uint8_t* bytes, uint64_t n) {
    TarSink* t = (TarSink*)arg;
    t->sha.update(bytes, (size_t)n);
    t->bytes += n;
    u64 w = 0;
    while (t->fd >= 0 && w < n) {
        const ssize_t r = write(t->fd, bytes + w, (size_t)(n - w));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) { t->io_errno = errno ? errno : EIO; return MI_ERR_IO; }
        w += (u64)r;
    }
    return MI_OK;
}
}  // namespace

int mi_tar_inflate_ctx(mi_ctx* c, const char* blob_path, const char* tar_path_out, uint64_t* tar_bytes, uint8_t* tar_sha256, uint8_t* blob_sha256,
                       mi_inflate_info* info, char* err, uint64_t err_cap) {
    return mi_tar_inflate_ctx_with(c, blob_path, nullptr, 0, tar_path_out, tar_bytes, tar_sha256, blob_sha256, info, err, err_cap);
}

int mi_tar_inflate_ctx_with(mi_ctx* c, const char* blob_path, const uint8_t* index, uint64_t index_bytes, const char* tar_path_out, uint64_t* tar_bytes,
                            uint8_t* tar_sha256, uint8_t* blob_sha256, mi_inflate_info* info, char* err, uint64_t err_cap) {
    return tar_inflate_ctx_route(c, blob_path, index, index_bytes, nullptr, tar_path_out, tar_bytes, tar_sha256, blob_sha256, info, err, err_cap);
}

}  // extern "C"

// index (may be NULL): the blob's index of checkpoints -- a hint: whatever it does not carry through goes the unindexed
// host way, fell_back 2 when it was refused.  spec (may be NULL; no index then): the plan from speculative spans, a hint
// in the same way
int mi::tar_inflate_ctx_route(mi_ctx* c, const char* blob_path, const u8* index, u64 index_bytes, const InfSpecAsk* spec, const char* tar_path_out,
                              uint64_t* tar_bytes, uint8_t* tar_sha256, uint8_t* blob_sha256, mi_inflate_info* info, char* err, uint64_t err_cap) {
    if (!c || !blob_path) return MI_ERR_INVALID;
    if (info) memset(info, 0, sizeof *info);
    const int fd = open(blob_path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) { inflate_put_err(err, err_cap, std::string("open ") + blob_path + ": " + strerror(errno)); return MI_ERR_IO; }
    struct stat st;
    if (fstat(fd, &st) != 0) { inflate_put_err(err, err_cap, std::string("stat: ") + strerror(errno)); close(fd); return MI_ERR_IO; }
    const u64 n = (u64)st.st_size;
    unsigned char magic[2] = {0, 0};
    const bool gz = n >= 2 && pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    void* map = gz ? mmap(nullptr, (size_t)n, PROT_READ, MAP_PRIVATE, fd, 0) : MAP_FAILED;
    close(fd);
    if (!gz) return mi_tar_inflate(blob_path, tar_path_out, tar_bytes, tar_sha256, blob_sha256, err, err_cap);   // a plain tar is copied
    if (map == MAP_FAILED) { inflate_put_err(err, err_cap, std::string("mmap ") + blob_path + ": " + strerror(errno)); return MI_ERR_IO; }
    mi_inflater* d = nullptr;
    int rc = mi_inflater_create(c, &d);
    if (rc) { munmap(map, (size_t)n); inflate_put_err(err, err_cap, "mi_tar_inflate_ctx: no stream"); return rc; }
    mi_host::Sha256 sha_blob;
    rc = spec  ? mi_inflater_plan_spec(d, (const u8*)map, n, spec->piece_bytes, inflate_sha_seen, &sha_blob)
       : index ? mi_inflater_plan_indexed(d, (const u8*)map, n, index, index_bytes, inflate_sha_seen, &sha_blob)
               : mi_inflater_plan(d, (const u8*)map, n, inflate_sha_seen, &sha_blob);
    if (info) *info = d->info;
    if (spec && spec->spec_info) *spec->spec_info = d->spec;
    if (rc == MI_OK && d->info.verdict != MI_INFLATE_DONE) {             // zlib decides; nothing has been written yet
        const u32 fb = d->info.verdict == MI_INFLATE_INDEX_REFUSED ? 2 : 1;
        mi_inflater_free(d);
        munmap(map, (size_t)n);
        if (info) info->fell_back = fb;
        return mi_tar_inflate(blob_path, tar_path_out, tar_bytes, tar_sha256, blob_sha256, err, err_cap);
    }
    TarSink sink{-1, mi_host::Sha256(), 0, 0};
    if (rc == MI_OK && tar_path_out) {
        sink.fd = open(tar_path_out, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
        if (sink.fd < 0) { inflate_put_err(err, err_cap, std::string("create ") + tar_path_out + ": " + strerror(errno)); rc = MI_ERR_IO; }
        else {
            rc = mi_inflater_run(d, inflate_tar_emit, &sink);
            close(sink.fd);
            if (rc) unlink(tar_path_out);
        }
    } else if (rc == MI_OK) {
        rc = mi_inflater_run(d, inflate_tar_emit, &sink);
    }
    if (rc == kInflateRefused) {                                         // (an index only) the spans did not carry through: the partial output
        const u32 fb = d->info.verdict == MI_INFLATE_INDEX_REFUSED ? 2 : 1;   // is gone, and zlib decides whether the blob is corrupt
        if (info) { *info = d->info; info->fell_back = fb; }
        mi_inflater_free(d);
        munmap(map, (size_t)n);
        return mi_tar_inflate(blob_path, tar_path_out, tar_bytes, tar_sha256, blob_sha256, err, err_cap);
    }
    if (rc == MI_ERR_IO && sink.io_errno) inflate_put_err(err, err_cap, std::string("write ") + tar_path_out + ": " + strerror(sink.io_errno));
    else if (rc && rc != MI_ERR_IO) {
        inflate_put_err(err, err_cap, std::string(blob_path) + ": " + d->err);
        fail(c, rc, "mi_tar_inflate_ctx: %s: %s", blob_path, d->err.c_str());
    }
    if (rc == MI_OK && spec && spec->index) {                            // the first pull leaves its index behind
        rc = inflate_spec_index(d, spec->index, spec->index_bytes);
        if (rc) { inflate_put_err(err, err_cap, std::string(blob_path) + ": " + d->err); if (tar_path_out) unlink(tar_path_out); }
    }
    if (info) { const u32 fb = info->fell_back; *info = d->info; info->fell_back = fb; }
    mi_inflater_free(d);
    munmap(map, (size_t)n);
    if (rc) return rc;
    if (tar_bytes) *tar_bytes = sink.bytes;
    if (tar_sha256) sink.sha.final(tar_sha256);
    if (blob_sha256) sha_blob.final(blob_sha256);
    return MI_OK;
}
