// mi_deflate.hip -- the layer writer's DEVICE DEFLATE LEG: the kernels over mi_deflate_wave.h's two bodies, the
// coder that moves windows of the stream through them (mi_deflater_*: what mi_layer.hip's device sink drives, hidden), and the
// building block mi_deflate_buffer (host bytes in, host bytes out).
//
// A window of the input (whole pieces, but for the stream's last) goes through five launches and one CRC pass:
//   deflate_plan_kernel      one wave a piece: parse, items, counts, codes, header, THE SIZE (mi_deflate_wave.h df_plan_piece)
//   deflate_sums_kernel      mi_plan.h's block sums over the sizes (and the (D) pieces' count)
//   deflate_scan_kernel      ... its one-block scan: the window's bytes and its (D) count
//   deflate_offsets_kernel   ... and every piece's offset: the pieces lie end to end, byte-aligned, no grid, no pads
//   deflate_emit_kernel      one wave a piece: the stored form at its final offset (df_emit_piece)
//   crc32.hip's tiles and fold over the window as ONE file: the sink combines the windows' CRCs as it combines the host leg's.
// What crosses PCIe downwards is the compressed bytes, sixteen bytes of totals and the CRC.
//
// TWO WINDOWS are in flight: each has its pinned input and output, its device buffers, two streams' worth of events.  The copies
// run on a stream of their own beside the coding stream (neither is the ctx's scan stream): window k + 1 goes up while window k
// is coded, window k comes down while k + 1 is coded.  The pieces do not depend on the window: the blob is a pure function of
// the stream.
//
// SCRATCH a window of W bytes: the items 4 W, the plan rows (16 + 320 + 320 bytes a piece), the output df_bound(W).
#include "mi_internal.h"
#include "mi_deflate_wave.h"
#include "mi_plan.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

namespace mi {

__global__ __launch_bounds__(64)
void deflate_plan_kernel(const u8* __restrict__ src, u64 n, u32* __restrict__ items, u8* __restrict__ lens, u32* __restrict__ header,
                         DfMeta* __restrict__ meta) {
    __shared__ DfPlanLds lds;
    const u64 piece = blockIdx.x, at = piece * kDfPiece;
    if (at >= n) return;
    const u32 len = n - at < kDfPiece ? (u32)(n - at) : kDfPiece;
    df_plan_piece(src + at, len, items + piece * kDfPiece, lens + piece * kDfLens, header + piece * kDfHeaderWords, meta + piece, &lds, (int)threadIdx.x);
}

// the plan's selection: every piece; what is summed: its size, and whether it is (D)
__global__ __launch_bounds__(kPlanBlock)
void deflate_sums_kernel(const DfMeta* __restrict__ meta, u64 n_pieces, u64* __restrict__ block_bytes, u64* __restrict__ block_dyn) {
    __shared__ u64 lds[2][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
        if (base + k < n_pieces) { v[0] += meta[base + k].size; v[1] += meta[base + k].dynamic; }
    plan_block_sum<2>(v, lds);
    if (threadIdx.x == 0) { block_bytes[blockIdx.x] = v[0]; block_dyn[blockIdx.x] = v[1]; }
}

__global__ __launch_bounds__(kPlanBlock)
void deflate_scan_kernel(u64* __restrict__ block_bytes, u64* __restrict__ block_dyn, u64 n_blocks, u64* __restrict__ totals) {
    plan_block_offsets<true>(block_bytes, block_dyn, n_blocks, totals, totals + 1);
}

__global__ __launch_bounds__(kPlanBlock)
void deflate_offsets_kernel(const DfMeta* __restrict__ meta, u64 n_pieces, const u64* __restrict__ block_bytes, u64* __restrict__ offset) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 mine = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
        if (base + k < n_pieces) mine += meta[base + k].size;
    u64 at = plan_first(mine, block_bytes);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
        if (base + k < n_pieces) { offset[base + k] = at; at += meta[base + k].size; }
}

__global__ __launch_bounds__(64)
void deflate_emit_kernel(const u8* __restrict__ src, u64 n, const u32* __restrict__ items, const u8* __restrict__ lens,
                         const u32* __restrict__ header, const DfMeta* __restrict__ meta, const u64* __restrict__ offset, u8* __restrict__ out) {
    __shared__ DfEmitLds lds;
    const u64 piece = blockIdx.x, at = piece * kDfPiece;
    if (at >= n) return;
    const u32 len = n - at < kDfPiece ? (u32)(n - at) : kDfPiece;
    df_emit_piece(src + at, len, items + piece * kDfPiece, lens + piece * kDfLens, header + piece * kDfHeaderWords, meta[piece], out + offset[piece], &lds,
                  (int)threadIdx.x);
}

// (hidden: the kernel probe's) df_code_lengths alone: counts[0, nsym) -> lens[0, nsym) under `limit`
__global__ __launch_bounds__(64)
void deflate_code_lengths_kernel(const u32* __restrict__ counts, u32 nsym, u32 limit, u8* __restrict__ lens) {
    __shared__ DfPlanLds lds;
    const int lane = (int)threadIdx.x;
    for (u32 i = lane; i < kDfLens; i += 64) lds.count[i] = i < nsym ? counts[i] : 0;
    __syncthreads();
    df_make_code(lds.count, nsym, lds.len, limit, &lds, lane);
    for (u32 i = lane; i < nsym; i += 64) lens[i] = lds.len[i];
}

void launch_deflate_code_lengths(const u32* d_counts, u32 nsym, u32 limit, u8* d_lens, hipStream_t s) {
    if (nsym == 0 || nsym > kDfLitLen || limit == 0 || limit > 15) return;
    hipLaunchKernelGGL(deflate_code_lengths_kernel, dim3(1), dim3(64), 0, s, d_counts, nsym, limit, d_lens);
}

}  // namespace mi

using namespace mi;

namespace {

constexpr u64 kMiB = 1ull << 20;

struct Slot {
    PinBuf h_in, h_out, h_small;                       // h_small: [0..2] the CRC pass's file row, [4] bytes, [5] (D) pieces, [6] the CRC
    DevBuf d_in, d_items, d_meta, d_lens, d_head, d_off, d_blk_a, d_blk_b, d_tot, d_out;
    DevBuf d_row, d_tile_file, d_tile_raw, d_crc;
    Event up, t0, t1;
    u64 n = 0;
    bool pending = false;
};

}  // namespace

struct mi_deflater {
    mi_ctx* ctx = nullptr;
    u64 window = 0;
    Stream code, copy;
    Slot slot[2];
    int cur = 0;
    std::string err;
    mi_deflate_info info = {};
    ~mi_deflater() {                                   // nothing is under way when the windows and events go
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

#define DFCHK(d, call)                                                                                                   \
    do {                                                                                                                 \
        const hipError_t e_ = (call);                                                                                    \
        if (e_ != hipSuccess)                                                                                            \
            return (d)->fail(e_ == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "device deflate: %s failed: %s", #call, \
                             hipGetErrorString(e_));                                                                     \
    } while (0)

namespace {

int slot_prepare(mi_deflater* d, Slot* s) {
    if (s->h_in.p) return MI_OK;
    const u64 w = d->window, np = (w + kDfPiece - 1) / kDfPiece, nb = (np + kPlanTile - 1) / kPlanTile;
    DFCHK(d, s->h_in.ensure(w));
    DFCHK(d, s->h_out.ensure(df_bound(w)));
    DFCHK(d, s->h_small.ensure(64));
    DFCHK(d, s->d_items.alloc_exact(4 * np * (u64)kDfPiece));
    DFCHK(d, s->d_meta.alloc_exact(np * sizeof(DfMeta)));
    DFCHK(d, s->d_lens.alloc_exact(np * kDfLens));
    DFCHK(d, s->d_head.alloc_exact(np * kDfHeaderWords * 4));
    DFCHK(d, s->d_off.alloc_exact(np * 8));
    DFCHK(d, s->d_blk_a.alloc_exact(nb * 8));
    DFCHK(d, s->d_blk_b.alloc_exact(nb * 8));
    DFCHK(d, s->d_tot.alloc_exact(16));
    DFCHK(d, s->d_out.alloc_exact(df_bound(w)));
    DFCHK(d, s->d_row.alloc_exact(24));
    DFCHK(d, s->d_tile_file.alloc_exact(np * 4));
    DFCHK(d, s->d_tile_raw.alloc_exact(np * 4));
    DFCHK(d, s->d_crc.alloc_exact(4));
    DFCHK(d, hipMemsetAsync(s->d_tile_file.p, 0, np * 4, d->code));     // every tile is file 0's
    DFCHK(d, s->up.create(hipEventDisableTiming));
    DFCHK(d, s->t0.create());
    DFCHK(d, s->t1.create());
    return MI_OK;
}

// the window in s->h_in[0, n) goes up and through the launches; s->t1 is its end
int slot_submit(mi_deflater* d, Slot* s, u64 n) {
    s->n = n;
    // the input: exactly n bytes under MI_GUARD_ALLOC (the last piece then ends on the allocation's last byte), else the window
    if (guard_alloc()) {
        s->d_in.release();
        void* p = nullptr;
        DFCHK(d, dev_alloc(&p, (size_t)n));
        s->d_in.p = p;
        s->d_in.bytes = (size_t)n;
    } else if (!s->d_in.p) {
        DFCHK(d, s->d_in.alloc_exact(d->window));
    }
    const u64 np = (n + kDfPiece - 1) / kDfPiece, nb = (np + kPlanTile - 1) / kPlanTile;
    u64* row = s->h_small.as<u64>();
    row[0] = 0; row[1] = n; row[2] = 0;
    DFCHK(d, hipMemcpyAsync(s->d_in.p, s->h_in.p, n, hipMemcpyHostToDevice, d->copy));
    DFCHK(d, hipMemcpyAsync(s->d_row.p, row, 24, hipMemcpyHostToDevice, d->copy));
    DFCHK(d, hipEventRecord(s->up, d->copy));
    DFCHK(d, hipStreamWaitEvent(d->code, s->up, 0));
    DFCHK(d, hipEventRecord(s->t0, d->code));
    hipLaunchKernelGGL(deflate_plan_kernel, dim3((u32)np), dim3(64), 0, d->code, s->d_in.as<u8>(), n, s->d_items.as<u32>(), s->d_lens.as<u8>(),
                       s->d_head.as<u32>(), s->d_meta.as<DfMeta>());
    hipLaunchKernelGGL(deflate_sums_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, d->code, s->d_meta.as<DfMeta>(), np, s->d_blk_a.as<u64>(), s->d_blk_b.as<u64>());
    hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(kPlanBlock), 0, d->code, s->d_blk_a.as<u64>(), s->d_blk_b.as<u64>(), nb, s->d_tot.as<u64>());
    hipLaunchKernelGGL(deflate_offsets_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, d->code, s->d_meta.as<DfMeta>(), np, s->d_blk_a.as<u64>(), s->d_off.as<u64>());
    hipLaunchKernelGGL(deflate_emit_kernel, dim3((u32)np), dim3(64), 0, d->code, s->d_in.as<u8>(), n, s->d_items.as<u32>(), s->d_lens.as<u8>(),
                       s->d_head.as<u32>(), s->d_meta.as<DfMeta>(), s->d_off.as<u64>(), s->d_out.as<u8>());
    const u64* r = s->d_row.as<u64>();
    launch_crc32_files(s->d_in.as<u8>(), r, r + 1, s->d_tile_file.as<u32>(), r + 2, np, 1, d->ctx->crc_consts.as<u32>(), s->d_tile_raw.as<u32>(),
                       s->d_crc.as<u32>(), d->code);
    DFCHK(d, hipGetLastError());
    DFCHK(d, hipMemcpyAsync(row + 4, s->d_tot.p, 16, hipMemcpyDeviceToHost, d->code));
    DFCHK(d, hipMemcpyAsync(row + 6, s->d_crc.p, 4, hipMemcpyDeviceToHost, d->code));
    DFCHK(d, hipEventRecord(s->t1, d->code));
    s->pending = true;
    return MI_OK;
}

// waits for the window, brings its bytes down and hands them on
int slot_finish(mi_deflater* d, Slot* s, mi_deflate_emit_fn emit, void* arg) {
    if (!s->pending) return MI_OK;
    s->pending = false;
    DFCHK(d, hipEventSynchronize(s->t1));
    const u64* row = s->h_small.as<u64>();
    const u64 bytes = row[4], n_dyn = row[5], np = (s->n + kDfPiece - 1) / kDfPiece;
    const u32 crc = (u32)row[6];
    if (bytes > df_bound(s->n) || n_dyn > np)
        return d->fail(MI_ERR_HIP, "device deflate: a window of %llu bytes came back as %llu bytes in %llu dynamic pieces", (unsigned long long)s->n,
                       (unsigned long long)bytes, (unsigned long long)n_dyn);
    float ms = 0;
    DFCHK(d, hipEventElapsedTime(&ms, s->t0, s->t1));
    DFCHK(d, hipMemcpyAsync(s->h_out.p, s->d_out.p, bytes, hipMemcpyDeviceToHost, d->copy));
    DFCHK(d, hipStreamSynchronize(d->copy));
    d->info.n_pieces += np;
    d->info.n_dynamic += n_dyn;
    d->info.n_stored += np - n_dyn;
    d->info.in_bytes += s->n;
    d->info.out_bytes += bytes;
    d->info.ms_device += ms;
    return emit(arg, s->h_out.as<u8>(), bytes, crc, s->n);
}

}  // namespace

extern "C" {

int mi_deflater_create(mi_ctx* c, uint64_t window_bytes, mi_deflater** out) {
    if (!c || !out || window_bytes == 0 || window_bytes % kDfPiece || window_bytes >> 32) return MI_ERR_INVALID;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    mi_deflater* d = new mi_deflater();
    d->ctx = c;
    d->window = window_bytes;
    if (d->code.create() != hipSuccess || d->copy.create() != hipSuccess) {
        delete d;
        return fail(c, MI_ERR_HIP, "mi_deflater_create: no stream");
    }
    *out = d;
    return MI_OK;
}

uint64_t mi_deflater_window(const mi_deflater* d) { return d ? d->window : 0; }
const char* mi_deflater_error(const mi_deflater* d) { return d ? d->err.c_str() : "null deflater"; }
void mi_deflater_info(const mi_deflater* d, mi_deflate_info* out) { if (d && out) *out = d->info; }

uint8_t* mi_deflater_room(mi_deflater* d) {
    if (!d || hipSetDevice(d->ctx->device) != hipSuccess) return nullptr;
    Slot* s = &d->slot[d->cur];
    if (s->pending || slot_prepare(d, s) != MI_OK) return nullptr;
    return s->h_in.as<u8>();
}

int mi_deflater_push(mi_deflater* d, uint64_t n, mi_deflate_emit_fn emit, void* arg) {
    if (!d || !emit || n == 0 || n > d->window) return MI_ERR_INVALID;
    DFCHK(d, hipSetDevice(d->ctx->device));
    Slot* s = &d->slot[d->cur];
    if (s->pending || !s->h_in.p) return d->fail(MI_ERR_STATE, "device deflate: push without room");
    int rc = slot_submit(d, s, n);
    if (rc) return rc;
    d->cur ^= 1;
    return slot_finish(d, &d->slot[d->cur], emit, arg);     // the older window, while this one is coded
}

int mi_deflater_flush(mi_deflater* d, mi_deflate_emit_fn emit, void* arg) {
    if (!d || !emit) return MI_ERR_INVALID;
    DFCHK(d, hipSetDevice(d->ctx->device));
    int rc = slot_finish(d, &d->slot[d->cur], emit, arg);
    if (rc == MI_OK) rc = slot_finish(d, &d->slot[d->cur ^ 1], emit, arg);
    return rc;
}

void mi_deflater_free(mi_deflater* d) {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    delete d;
}

uint64_t mi_deflate_bound(uint64_t n) { return df_bound(n); }

namespace {
struct BufferSink { u8* dst; u64 at; u32 crc; u64 in; };
int buffer_emit(void* arg, const uint8_t* bytes, uint64_t n_out, uint32_t crc, uint64_t n_in) {
    BufferSink* b = (BufferSink*)arg;
    memcpy(b->dst + b->at, bytes, n_out);               // (cap >= the bound of the whole input: checked before the first window)
    b->at += n_out;
    b->crc = b->in ? crc32_host_combine(b->crc, crc, n_in) : crc;
    b->in += n_in;
    return MI_OK;
}
}  // namespace

uint64_t mi_deflate_device_window(void) {
    u64 mb = 32;
    if (const char* e = getenv("MI_GZIP_DEVICE_WINDOW_MB")) { const long v = atol(e); if (v >= 1 && v <= 1024) mb = (u64)v; }
    return mb * kMiB;
}

int mi_deflate_buffer(mi_ctx* c, const void* src, uint64_t n, void* dst, uint64_t cap, uint64_t* out_bytes, uint32_t* crc32, mi_deflate_info* info) {
    if (!c || (!src && n) || !dst || !out_bytes) return MI_ERR_INVALID;
    *out_bytes = 0;
    if (crc32) *crc32 = 0;
    if (info) memset(info, 0, sizeof *info);
    if (cap < df_bound(n)) return fail(c, MI_ERR_CAPACITY, "mi_deflate_buffer: %llu bytes need room for %llu, dst holds %llu", (unsigned long long)n,
                                       (unsigned long long)df_bound(n), (unsigned long long)cap);
    if (n == 0) return MI_OK;
    u64 window = mi_deflate_device_window();
    if (window > n) window = (n + kDfPiece - 1) / kDfPiece * kDfPiece;
    mi_deflater* d = nullptr;
    int rc = mi_deflater_create(c, window, &d);
    if (rc) return rc;
    BufferSink sink{(u8*)dst, 0, 0, 0};
    for (u64 at = 0; at < n && rc == MI_OK; at += window) {
        const u64 take = n - at < window ? n - at : window;
        u8* room = mi_deflater_room(d);
        if (!room) { rc = d->err.empty() ? MI_ERR_NOMEM : MI_ERR_HIP; break; }
        memcpy(room, (const u8*)src + at, take);
        rc = mi_deflater_push(d, take, buffer_emit, &sink);
    }
    if (rc == MI_OK) rc = mi_deflater_flush(d, buffer_emit, &sink);
    if (rc) fail(c, rc, "mi_deflate_buffer: %s", d->err.empty() ? "no memory for a window" : d->err.c_str());
    else {
        *out_bytes = sink.at;
        if (crc32) *crc32 = sink.crc;
        if (info) *info = d->info;
    }
    mi_deflater_free(d);
    return rc;
}

}  // extern "C"
