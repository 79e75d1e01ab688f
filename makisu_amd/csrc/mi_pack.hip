// mi_pack.hip -- chunk packs: the selected rows of a batch's chunk table gathered into ONE contiguous blob on the device
// (mi_batch_pack_chunks and the mi_pack_* calls of include/makisu_mi.h).  What a chunk-addressed store takes in for a layer:
// the bytes of the chunks no earlier layer held, every chunk on a 16-byte offset, the pad behind it zero, addressed by digest.
//
//   plan      mi_plan.h's three launches over the selection flags and the ROUNDED-UP lengths of the selected rows; per entry:
//             source arena offset, length, blob offset, and the mi_pack_entry row;
//   gather    destination-driven: the blob is cut into tiles of kPackTile bytes, a workgroup takes a tile, so the length
//             distribution of the chunks cannot unbalance the launch (one 64 KiB chunk and 1 024 chunks of 16 bytes are the
//             same work).  The entries that reach into a tile are found by a search over the entries' blob offsets, 64 probes
//             a round by one wave (four rounds for 16 M entries); their offsets lie in LDS.  Every lane owns 16-byte units of
//             the destination: it finds its entry in LDS, loads 16 bytes from arena + chunk_off + (unit - entry offset) at
//             whatever alignment that has, zeroes the bytes at and beyond the chunk's length and stores one aligned dwordx4;
//   verify    MI_PACK_VERIFY: the blob's entries through the ctx's own hashing launcher (pass kShaBlobs), the digests held
//             against the rows' on the device -- bytes that crossed a hop are held against what was computed where they were read.
//
// OVER-READ BOUND.  A unit's load begins at chunk_off + o with o a multiple of 16 below the chunk's length, so it begins inside
// the chunk and never in front of it; the chunk's last unit reads up to chunk_off + round16(len) - 1: at most 15 bytes behind the
// chunk (len = 1 mod 16), inside the arena's 4 KiB slack.  The hashing of the verify pass reads up to 67 bytes behind the blob's
// last entry: the blob is allocated with the 256 bytes every DevBuf has behind it.
#include "mi_internal.h"
#include "mi_plan.h"
#include "host_blake2s.h"
#include "host_sha256.h"

#include <string.h>

#include <algorithm>
#include <vector>

using namespace mi;

namespace mi {

constexpr u64 kNoRow = ~0ull;
// ---- plan ------------------------------------------------------------------------------------------------------------
// per block of kPlanTile rows: how many are selected, and their rounded-up bytes; totals[2] += their bytes as they are
__global__ __launch_bounds__(kPlanBlock)
void pack_block_sums_kernel(const u8* __restrict__ select, const u64* __restrict__ chunk_len, u64 n,
                            u64* __restrict__ block_cnt, u64* __restrict__ block_bytes, u64* __restrict__ totals) {
    __shared__ u64 lds[3][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[3] = {0, 0, 0};                             // entries, their rounded-up bytes, their bytes
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
        if (base + k < n && (!select || select[base + k])) {
            const u64 len = chunk_len[base + k];
            ++v[0];
            v[1] += round16(len);
            v[2] += len;
        }
    plan_block_sum<3>(v, lds);
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = v[0];
        block_bytes[blockIdx.x] = v[1];
        if (v[2]) atomicAdd((unsigned long long*)&totals[2], (unsigned long long)v[2]);
    }
}

// single block: exclusive scan of both block arrays in place; totals[0] = entries, totals[1] = blob bytes
__global__ __launch_bounds__(kPlanBlock)
void pack_block_offsets_kernel(u64* __restrict__ block_cnt, u64* __restrict__ block_bytes, u64 n_blocks,
                               u64* __restrict__ totals) {
    plan_block_offsets<true>(block_cnt, block_bytes, n_blocks, &totals[0], &totals[1]);
}

// the selected rows, in row order, as entries: where the chunk lies in the arena, its length, where it goes in the blob, and
// the mi_pack_entry row (digest | offset | chunk_index | length, reserved = 0)
__global__ __launch_bounds__(kPlanBlock)
void pack_compact_kernel(const u8* __restrict__ select, const u64* __restrict__ chunk_off, const u64* __restrict__ chunk_len,
                         const u8* __restrict__ digests, u64 n, const u64* __restrict__ block_cnt,
                         const u64* __restrict__ block_bytes, u64* __restrict__ e_src, u64* __restrict__ e_len,
                         u64* __restrict__ e_dst, u64* __restrict__ rows) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 len[kPlanPer];
    u64 cnt = 0, bytes = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const bool sel = base + k < n && (!select || select[base + k]);
        len[k] = sel ? chunk_len[base + k] : kNoRow;
        if (sel) { ++cnt; bytes += round16(len[k]); }
    }
    u64 at = plan_first(cnt, block_cnt);
    u64 dst = plan_first(bytes, block_bytes);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (len[k] == kNoRow) continue;
        const u64 row = base + k;
        e_src[at] = chunk_off[row];
        e_len[at] = len[k];
        e_dst[at] = dst;
        put_entry_row(rows + kEntryWords * at, digests + 32 * row, dst, row, len[k] & 0xFFFFFFFFull);   // length | reserved = 0
        ++at;
        dst += round16(len[k]);
    }
}

// ---- gather ----------------------------------------------------------------------------------------------------------
constexpr int kPackWG = 256;
constexpr u32 kPackTile = 16384;                     // bytes of the blob a workgroup writes
constexpr u32 kPackUnits = kPackTile / 16;           // ... in 16-byte units: an entry takes at least one, so at most as many entries
constexpr int kPackPer = kPackUnits / kPackWG;       // units per lane

__global__ __launch_bounds__(kPackWG)
void pack_gather_kernel(const u8* __restrict__ arena, const u64* __restrict__ e_src, const u64* __restrict__ e_len,
                        const u64* __restrict__ e_dst, u64 n_entries, u64 blob_bytes, u8* __restrict__ blob) {
    __shared__ u64 s_src[kPackUnits];
    __shared__ int s_rel[kPackUnits];                // the entry's blob offset relative to the tile (the first may begin in front of it)
    __shared__ u32 s_len[kPackUnits];
    __shared__ u64 s_k[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 tile0 = (u64)blockIdx.x * kPackTile;
    const u64 tile1 = tile0 + kPackTile < blob_bytes ? tile0 + kPackTile : blob_bytes;
    // the first and the last entry that reach into the tile: the last one that begins at or before the tile's first / last unit
    if (wave < 2) {
        const u64 k = wave_last_le(e_dst, n_entries, wave == 0 ? tile0 : tile1 - 16, lane);
        if (lane == 0) s_k[wave] = k;
    }
    __syncthreads();
    const u64 k0 = s_k[0];
    const u64 reach = s_k[1] - k0 + 1;
    const u32 cnt = reach < kPackUnits ? (u32)reach : kPackUnits;
    for (u32 i = threadIdx.x; i < cnt; i += kPackWG) {
        s_src[i] = e_src[k0 + i];
        s_len[i] = (u32)e_len[k0 + i];
        s_rel[i] = (int)(long long)(e_dst[k0 + i] - tile0);
    }
    __syncthreads();
    u64 src[kPackPer];                               // arena offsets of the units' 16 bytes
    u32 valid[kPackPer];
#pragma unroll
    for (int j = 0; j < kPackPer; ++j) {
        const u32 r = ((u32)threadIdx.x + (u32)j * kPackWG) * 16;
        src[j] = 0;
        valid[j] = 0;
        if (tile0 + r >= tile1) continue;
        u32 lo = 0, hi = cnt;                         // the entry this unit lies in: the last that begins at or before it
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (s_rel[mid] <= (int)r) lo = mid; else hi = mid;
        }
        const u32 o = (u32)((int)r - s_rel[lo]), len = s_len[lo];
        if (o < len) {                                // (always, for entries of at least one byte)
            src[j] = s_src[lo] + o;
            valid[j] = len - o;
        }
    }
    u32x4 v[kPackPer];
#pragma unroll
    for (int j = 0; j < kPackPer; ++j) {
        v[j] = u32x4{0, 0, 0, 0};
        if (valid[j]) v[j] = *(const u32x4_unaligned*)(arena + src[j]);
    }
#pragma unroll
    for (int j = 0; j < kPackPer; ++j) {
        const u32 r = ((u32)threadIdx.x + (u32)j * kPackWG) * 16;
        if (tile0 + r >= tile1) continue;
        if (valid[j] < 16) v[j] = keep_first_bytes(v[j], valid[j]);   // the chunk's last unit: zero at and beyond its length
        *(u32x4*)(blob + tile0 + r) = v[j];
    }
}

// ---- verify: the digests of the blob's entries against the rows' -----------------------------------------------------
__global__ __launch_bounds__(256)
void pack_compare_kernel(const u8* __restrict__ got, const u64* __restrict__ rows, u64 n, u64* __restrict__ first_bad) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    digest_differs_mark(got, rows + kEntryWords * k, k, first_bad);
}

// ---- mi_pack_read: the blob through two pinned windows, the copy of one overlapping the consumption of the other (the
// scheme of mi::ReadBack for the arena, for a device range that does not change) ---------------------------------------------
constexpr u64 kPackWinBytes = 8ull << 20;
struct MI_LOCAL PackReader {
    Stream stream;
    struct Win { PinBuf buf; u64 start = 0, len = 0; bool pending = false; Event ev; };
    Win win[2];
    int cur = 0;
    PackReader() = default;
    PackReader(PackReader&&) = default;
    PackReader& operator=(PackReader&&) = default;
    ~PackReader() { if (stream) (void)hipStreamSynchronize(stream); }     // no copy into a window is under way when the windows go
    int prepare(mi_ctx* c) {
        if (win[0].buf.p) return MI_OK;
        PackReader r;                                 // whole or not at all
        HIPCHK(c, r.stream.create());
        for (auto& w : r.win) {
            HIPCHK(c, w.buf.ensure(kPackWinBytes));
            HIPCHK(c, w.ev.create(hipEventDisableTiming));
        }
        *this = std::move(r);
        return MI_OK;
    }
    int read(mi_ctx* c, const u8* base, u64 total, u64 at, void* dst, u64 len) {
        if (!len) return MI_OK;
        const int rc = prepare(c);
        if (rc) return rc;
        auto prefetch = [&](Win& w, u64 from) -> int {
            w.len = 0;
            if (from >= total) return MI_OK;
            const u64 want = std::min(kPackWinBytes, total - from);
            HIPCHK(c, hipMemcpyAsync(w.buf.p, base + from, want, hipMemcpyDeviceToHost, stream));
            HIPCHK(c, hipEventRecord(w.ev, stream));
            w.start = from;
            w.len = want;
            w.pending = true;
            return MI_OK;
        };
        u8* d = (u8*)dst;
        while (len) {
            Win* w = &win[cur];
            if (!(w->len && at >= w->start && at < w->start + w->len)) {
                Win* nx = &win[cur ^ 1];
                const bool follows = w->len && at == w->start + w->len;          // the reader streams
                if (nx->len && at >= nx->start && at < nx->start + nx->len) {
                    if (nx->pending) { HIPCHK(c, hipEventSynchronize(nx->ev)); nx->pending = false; }
                    cur ^= 1;
                    const int prc = prefetch(*w, nx->start + nx->len);           // the window just left takes what follows the new one
                    if (prc) return prc;
                    continue;
                }
                if (nx->pending) { HIPCHK(c, hipEventSynchronize(nx->ev)); nx->pending = false; }
                nx->len = 0;
                const u64 want = std::min(kPackWinBytes, total - at);
                w->len = 0;
                HIPCHK(c, hipMemcpyAsync(w->buf.p, base + at, want, hipMemcpyDeviceToHost, stream));
                HIPCHK(c, hipStreamSynchronize(stream));
                w->start = at;
                w->len = want;
                w->pending = false;
                if (follows || want < len) {
                    const int prc = prefetch(*nx, at + want);
                    if (prc) return prc;
                }
            }
            const u64 take = std::min(len, w->start + w->len - at);
            memcpy(d, (const u8*)w->buf.p + (at - w->start), take);
            d += take;
            at += take;
            len -= take;
        }
        return MI_OK;
    }
};

}  // namespace mi

struct mi_pack {
    mi_ctx* ctx = nullptr;
    mi_pack_info info = {};
    DevBuf blob;                                 // info.blob_bytes + the slack the hashing kernels are promised
    std::vector<mi_pack_entry> h_rows;           // n_entries rows as the plan wrote them, on the host before mi_batch_pack_chunks
                                                 // returns and never written again
    PackReader reader;
};

namespace {

void pack_delete(mi_pack* p) {
    mi_ctx* c = p->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    --c->live_children;
    delete p;
}

}  // namespace

extern "C" {

int mi_batch_pack_chunks(mi_batch* b, const uint8_t* select, uint64_t n_select, uint32_t flags, mi_pack** out) {
    if (!b || !out) return MI_ERR_INVALID;
    mi_ctx* c = b->ctx;
    *out = nullptr;
    if (b->group) return fail(c, MI_ERR_INVALID, "mi_batch_pack_chunks: a batch group has one arena per GPU; pack its members");
    if (flags & ~(uint32_t)MI_PACK_VERIFY) return fail(c, MI_ERR_INVALID, "mi_batch_pack_chunks: unknown flags %#x", flags);
    if (!b->ran || b->in_flight) return fail(c, MI_ERR_STATE, "mi_batch_pack_chunks: the batch must have run (and been waited for)");
    const u64 n = b->n_chunks;
    if (select && n_select != n)
        return fail(c, MI_ERR_INVALID, "mi_batch_pack_chunks: %llu selection flags for a batch of %llu chunks", (unsigned long long)n_select,
                    (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    u64 n_sel = n;
    if (select) n_sel = n - (u64)std::count(select, select + n, (uint8_t)0);
    if (n_sel >> 32) return fail(c, MI_ERR_INVALID, "mi_batch_pack_chunks: %llu entries, a pack holds fewer than 2^32", (unsigned long long)n_sel);
    const u32 alg = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? MI_DIGEST_BLAKE2S : MI_DIGEST_SHA256;
    mi_pack* p = new mi_pack();
    p->ctx = c;
    ++c->live_children;                                    // mi_pack_free undoes it (error paths: pack_delete)
    p->info.alg = alg;
    if (n_sel == 0) {                                      // a valid pack of nothing
        p->info.verified = (flags & MI_PACK_VERIFY) ? 1 : 0;
        *out = p;
        return MI_OK;
    }
    hipStream_t s = c->stream;
    const u64 nb = (n + kPlanTile - 1) / kPlanTile;
    DevBuf d_sel, d_scan, e_src, e_len, e_dst, d_rows, d_got;
    Event ev_t[3];                                         // the call's own: before the gather, behind it, behind the verification
    hipError_t e = hipSuccess;
    int rc = MI_OK;
    auto hip_failed = [&](const char* what) {
        rc = fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "mi_batch_pack_chunks: %s: %s", what, hipGetErrorString(e));
        pack_delete(p);
        return rc;
    };
    // plan, first half: the totals
    if ((e = d_scan.ensure((2 * nb + 4) * 8)) != hipSuccess || (select && (e = d_sel.ensure(n)) != hipSuccess) ||
        (e = ev_t[0].create()) != hipSuccess || (e = ev_t[1].create()) != hipSuccess || (e = ev_t[2].create()) != hipSuccess)
        return hip_failed("plan buffers");
    u64* block_cnt = d_scan.as<u64>();
    u64* block_bytes = block_cnt + nb;
    u64* totals = block_bytes + nb;                        // entries, blob bytes, chunk bytes, first differing entry
    if (select) e = hipMemcpyAsync(d_sel.p, select, n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(totals, 0, 3 * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(totals + 3, 0xFF, 8, s);
    if (e != hipSuccess) return hip_failed("plan upload");
    hipLaunchKernelGGL(pack_block_sums_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, s, d_sel.as<u8>(), b->chunk_len.as<u64>(), n,
                       block_cnt, block_bytes, totals);
    hipLaunchKernelGGL(pack_block_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, s, block_cnt, block_bytes, nb, totals);
    u64* h = c->h_word.as<u64>();
    e = hipMemcpyAsync(h, totals, 3 * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return hip_failed("plan");
    if (h[0] != n_sel) {
        rc = fail(c, MI_ERR_HIP, "mi_batch_pack_chunks: the plan counted %llu entries, the selection holds %llu", (unsigned long long)h[0],
                  (unsigned long long)n_sel);
        pack_delete(p);
        return rc;
    }
    p->info.n_entries = n_sel;
    p->info.blob_bytes = h[1];
    p->info.chunk_bytes = h[2];
    const u64 blob_bytes = h[1];
    // the blob: device memory of its own.  Does not fit: MI_ERR_NOMEM, nothing else has changed
    if ((e = p->blob.alloc_exact(blob_bytes)) != hipSuccess) {
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        (void)hipGetLastError();
        rc = fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP,
                  "mi_batch_pack_chunks: a blob of %llu bytes (%llu chunks) does not fit: the device has %llu bytes free (%s); pack in several calls "
                  "with partial selections", (unsigned long long)blob_bytes, (unsigned long long)n_sel, (unsigned long long)free_b, hipGetErrorString(e));
        pack_delete(p);
        return rc;
    }
    if ((e = d_rows.alloc_exact(n_sel * sizeof(mi_pack_entry))) != hipSuccess || (e = e_src.ensure(n_sel * 8)) != hipSuccess ||
        (e = e_len.ensure(n_sel * 8)) != hipSuccess || (e = e_dst.ensure(n_sel * 8)) != hipSuccess ||
        ((flags & MI_PACK_VERIFY) && (e = d_got.ensure(n_sel * 32)) != hipSuccess))
        return hip_failed("entry arrays");
    // plan, second half; the gather; the verification
    hipLaunchKernelGGL(pack_compact_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, s, d_sel.as<u8>(), b->chunk_off.as<u64>(),
                       b->chunk_len.as<u64>(), b->digests.as<u8>(), n, block_cnt, block_bytes, e_src.as<u64>(), e_len.as<u64>(),
                       e_dst.as<u64>(), d_rows.as<u64>());
    const u64 n_tiles = (blob_bytes + kPackTile - 1) / kPackTile;
    if (n_tiles >> 31) {
        rc = fail(c, MI_ERR_INVALID, "mi_batch_pack_chunks: a blob of %llu bytes is more than one launch covers", (unsigned long long)blob_bytes);
        pack_delete(p);
        return rc;
    }
    e = hipEventRecord(ev_t[0], s);
    if (n_tiles)
        hipLaunchKernelGGL(pack_gather_kernel, dim3((u32)n_tiles), dim3(kPackWG), 0, s, b->arena.as<u8>(), e_src.as<u64>(), e_len.as<u64>(),
                           e_dst.as<u64>(), n_sel, blob_bytes, p->blob.as<u8>());
    if (e == hipSuccess) e = hipEventRecord(ev_t[1], s);
    if (flags & MI_PACK_VERIFY) {
        const auto hash_items = alg == MI_DIGEST_BLAKE2S ? launch_blake2s_items : launch_sha256_items;
        hash_items(kShaBlobs, p->blob.as<u8>(), e_dst.as<u64>(), e_len.as<u64>(), nullptr, (u32)n_sel, nullptr, c->heads.as<u32>(), nullptr,
                   true, d_got.as<u8>(), c->sha, c->prop.multiProcessorCount, blob_bytes, s);     // entries in row order: flat sharing
        hipLaunchKernelGGL(pack_compare_kernel, dim3((u32)((n_sel + 255) / 256)), dim3(256), 0, s, d_got.as<u8>(), d_rows.as<u64>(), n_sel,
                           totals + 3);
        if (e == hipSuccess) e = hipMemcpyAsync(h, totals + 3, 8, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipEventRecord(ev_t[2], s);
    // the entries to the host with the same synchronisation: 56 bytes each, and mi_pack_entries only reads from then on
    p->h_rows.resize(n_sel);
    if (e == hipSuccess) e = hipMemcpyAsync(p->h_rows.data(), d_rows.p, n_sel * sizeof(mi_pack_entry), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return hip_failed("gather");
    float ms = 0;
    if ((e = hipEventElapsedTime(&ms, ev_t[0], ev_t[1])) != hipSuccess) return hip_failed("gather time");
    p->info.ms_gather = ms;
    if (flags & MI_PACK_VERIFY) {
        if ((e = hipEventElapsedTime(&ms, ev_t[1], ev_t[2])) != hipSuccess) return hip_failed("verify time");
        p->info.ms_verify = ms;
        const u64 bad = h[0];
        if (bad != ~0ull) {
            u64 src_off = 0;
            const mi_pack_entry row = bad < n_sel ? p->h_rows[bad] : mi_pack_entry{};
            (void)hipMemcpy(&src_off, e_src.as<u64>() + bad, 8, hipMemcpyDeviceToHost);
            rc = fail(c, MI_ERR_IO, "mi_batch_pack_chunks: entry %llu -- chunk row %llu, %u bytes, arena offset %llu, blob offset %llu -- hashes to "
                      "another digest in the blob than the batch computed from the arena", (unsigned long long)bad,
                      (unsigned long long)row.chunk_index, row.length, (unsigned long long)src_off, (unsigned long long)row.offset);
            pack_delete(p);
            return rc;
        }
        p->info.verified = 1;
    }
    *out = p;
    return MI_OK;
}

int mi_pack_empty(mi_ctx* c, mi_pack** out) {           // (hidden: mi_local.h)
    if (!c || !out) return MI_ERR_INVALID;
    mi_pack* p = new mi_pack();
    p->ctx = c;
    ++c->live_children;
    p->info.alg = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? MI_DIGEST_BLAKE2S : MI_DIGEST_SHA256;
    p->info.verified = 1;
    *out = p;
    return MI_OK;
}

mi_ctx* mi_pack_ctx(const mi_pack* p) { return p ? p->ctx : nullptr; }     // (hidden: mi_local.h)

// (hidden: mi_local.h) a pack whose blob and rows mi_fetch.hip writes: mi_packset_pack
int mi_pack_alloc(mi_ctx* c, const char* who, uint64_t n_entries, uint64_t blob_bytes, uint64_t chunk_bytes, mi_pack** out, void** d_blob,
                  mi_pack_entry** h_rows) {
    if (!c || !out || !d_blob || !h_rows || !n_entries) return MI_ERR_INVALID;
    *out = nullptr;
    mi_pack* p = new mi_pack();
    p->ctx = c;
    ++c->live_children;                                    // mi_pack_free undoes it
    p->info.alg = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? MI_DIGEST_BLAKE2S : MI_DIGEST_SHA256;
    p->info.n_entries = n_entries;
    p->info.blob_bytes = blob_bytes;
    p->info.chunk_bytes = chunk_bytes;
    const hipError_t e = p->blob.alloc_exact(blob_bytes);
    if (e != hipSuccess) {
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        (void)hipGetLastError();
        const int rc = fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: a blob of %llu bytes (%llu chunks) does not fit: the "
                            "device has %llu bytes free (%s); split the request", who, (unsigned long long)blob_bytes,
                            (unsigned long long)n_entries, (unsigned long long)free_b, hipGetErrorString(e));
        pack_delete(p);
        return rc;
    }
    p->h_rows.resize(n_entries);
    *d_blob = p->blob.p;
    *h_rows = p->h_rows.data();
    *out = p;
    return MI_OK;
}

void mi_pack_set_result(mi_pack* p, uint32_t verified, double ms_gather, double ms_verify) {
    p->info.verified = verified;
    p->info.ms_gather = ms_gather;
    p->info.ms_verify = ms_verify;
}

int mi_pack_get_info(const mi_pack* p, mi_pack_info* out) {
    if (!p || !out) return MI_ERR_INVALID;
    *out = p->info;
    return MI_OK;
}

int mi_pack_entries(const mi_pack* p, mi_pack_entry* out, uint64_t cap) {
    if (!p || (!out && cap)) return MI_ERR_INVALID;
    mi_ctx* c = p->ctx;
    const u64 n = p->info.n_entries;
    if (cap < n) return fail(c, MI_ERR_CAPACITY, "pack entry buffer holds %llu rows, need %llu", (unsigned long long)cap, (unsigned long long)n);
    if (n) memcpy(out, p->h_rows.data(), n * sizeof(mi_pack_entry));
    return MI_OK;
}

int mi_pack_read(mi_pack* p, uint64_t offset, void* dst, uint64_t len) {
    if (!p || (!dst && len)) return MI_ERR_INVALID;
    mi_ctx* c = p->ctx;
    if (offset > p->info.blob_bytes || len > p->info.blob_bytes - offset)
        return fail(c, MI_ERR_INVALID, "mi_pack_read: [%llu, +%llu) is outside the blob of %llu bytes", (unsigned long long)offset,
                    (unsigned long long)len, (unsigned long long)p->info.blob_bytes);
    if (!len) return MI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return p->reader.read(c, p->blob.as<u8>(), p->info.blob_bytes, offset, dst, len);
}

int mi_pack_device(const mi_pack* p, const void** d_blob, uint64_t* blob_bytes) {
    if (!p || !d_blob || !blob_bytes) return MI_ERR_INVALID;
    *d_blob = p->info.blob_bytes ? p->blob.p : nullptr;
    *blob_bytes = p->info.blob_bytes;
    return MI_OK;
}

void mi_pack_free(mi_pack* p) {
    if (p) pack_delete(p);
}

// Host logic: what the pulling side runs before it trusts a pack.  No ctx, no GPU.
int mi_pack_check(const void* blob, uint64_t blob_bytes, const mi_pack_entry* entries, uint64_t n, uint32_t alg, uint64_t* first_bad) {
    if (first_bad) *first_bad = 0;
    if ((!blob && blob_bytes) || (!entries && n)) return MI_ERR_INVALID;
    if (alg != MI_DIGEST_SHA256 && alg != MI_DIGEST_BLAKE2S) return MI_ERR_INVALID;
    const u8* base = (const u8*)blob;
    u64 end = 0;                                      // where the previous entry's unit(s) end
    for (u64 k = 0; k < n; ++k) {
        const mi_pack_entry& en = entries[k];
        const u64 span = round16(en.length);
        bool ok = en.offset % 16 == 0 && en.offset >= end && en.offset <= blob_bytes && span <= blob_bytes - en.offset;
        if (ok)
            for (u64 i = en.offset + en.length; i < en.offset + span; ++i) ok = ok && base[i] == 0;
        if (ok) {
            u8 got[32];
            if (alg == MI_DIGEST_BLAKE2S) {
                mi_host::Blake2s hsh;
                hsh.update(base + en.offset, en.length);
                hsh.final(got);
            } else {
                mi_host::Sha256 hsh;
                hsh.update(base + en.offset, en.length);
                hsh.final(got);
            }
            ok = memcmp(got, en.digest, 32) == 0;
        }
        if (!ok) {
            if (first_bad) *first_bad = k;
            return MI_ERR_INVALID;
        }
        end = en.offset + span;
    }
    return MI_OK;
}

}  // extern "C"
