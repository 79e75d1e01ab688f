// mi_zbatch.hip -- a compressed chunk pack coded STRAIGHT FROM A BATCH'S ARENA (mi_batch_zpack_chunks: what the commit hands over
// under MI_MEMFS_CHUNK_ZPACK), and a compressed pack set asked which digests of a request it lacks (mi_zset_missing).  With both
// the compressed line needs no plain pack anywhere: the commit produces a zpack, the store serves cuts (mi_zset_zpack), the
// puller asks its zset and restores from it (mi_batch_add_zrecipes).  A chunk's stored form is a pure function of its bytes
// (mi_lz4_wave_enc.h), so the zpack is byte for byte what mi_batch_pack_chunks + mi_pack_compress gives for the same selection --
// without the plain blob, its gather and its hashing pass.
//
//   plan      the selection flags go up; mi_plan.h's three launches over the WORST-CASE spans z_worst_span(length) of the
//             selected rows: per entry the 56-byte row (digest | the chunk's ARENA OFFSET | the batch row | length), its scratch
//             offset, its arena offset and its length;
//   encode    mi_zrows.h's loop with the arena as its base: the coder reads the chunk where it lies, at whatever byte
//             alignment it has;
//   layout    mi_zrows.h's, with the totals (stored bytes, raw entries): a coded entry's gather source is its scratch span
//             (16-byte aligned), a raw entry's its chunk in the arena (ANY alignment);
//   gather    destination-driven, 16 KiB tiles, one wave searching the entries' offsets (mi_pack.hip's scheme).  Sources of
//             either kind lie side by side in a tile: every lane's 16-byte unit is ONE global_load_dwordx4 at whatever alignment
//             its source has, the bytes at and beyond `stored` are zeroed in registers, one aligned 16-byte store writes the
//             unit -- the pads are zero whatever lay behind the chunk in the arena;
//   verify    MI_ZPACK_VERIFY: the new blob decoded by mi_zpack.hip's decode kernel into the scratch spans (the gather has read
//             them: same stream), hashed there by the ctx's launcher (pass kShaBlobs), held against THE BATCH'S OWN digest table at
//             chunk_index: one decode and one hashing pass vouch for both hops, arena -> stored form -> plain again;
//   missing   mi_fetch.hip's want list over zset_lookup_kernel's answer: held flags and the rows that state another length than
//             the set's, first occurrences by the engine's dedup marking, the plan, want_list_finish.
//
// BOUNDS.  The encoder READS inside the chunk only: positions <= length - 12 read 4 bytes, match bytes lie below length - 5,
// literals below length; it WRITES below the entry's worst-case span (checked per sequence).  The gather READS 16 bytes at
// src + o, o a multiple of 16 below `stored`: a coded entry's unit lies inside its scratch span; a RAW entry's last unit reads at
// most 15 bytes behind the chunk (length = 1 mod 16), inside the arena's 4 KiB slack -- mi_pack.hip's bound.  It WRITES aligned
// units inside the new blob.  The decoder's bounds are mi_zpack.hip's: it writes [w_off, w_off + round16(length)) of the
// scratch, inside the entry's worst-case span.  The hashing of the verify pass reads up to 67 bytes behind the last scratch
// span: the 256 bytes it is allocated with.  The want list's kernels index [0, n) of arrays of n elements.
#include "mi_internal.h"
#include "mi_gather.h"
#include "mi_lz4_wave.h"
#include "mi_zrows.h"

#include <string.h>

#include <algorithm>
#include <string>

using namespace mi;

namespace mi {

constexpr u64 kBNone = ~0ull;
// the totals of mi_batch_zpack_chunks ...
enum : int { kBTotEntries = 0, kBTotSpan = 1, kBTotChunk = 2, kBTotBlob = 3, kBTotStored = 4, kBTotRaw = 5, kBTotBad = 6, kBTotDiffer = 7 };
// ... and of mi_zset_missing (kMTotLookup: where zset_lookup_kernel notes the rows the set lacks -- not read)
enum : int { kMTotWant = 0, kMTotWantBytes = 2, kMTotFirst = 3, kMTotHeld = 4, kMTotHeldBytes = 5, kMTotBad = 6, kMTotLookup = 7 };

// ---- plan: mi_plan.h's over the worst-case spans of the selected rows -------------------------------------------------------------
// per block of kPlanTile rows: how many are selected and their worst-case spans; totals[kBTotChunk] += their bytes as they are
__global__ __launch_bounds__(kPlanBlock)
void zbatch_plan_sums_kernel(const u8* __restrict__ select, const u64* __restrict__ chunk_len, u64 n, u64* __restrict__ block_cnt,
                             u64* __restrict__ block_span, u64* __restrict__ totals) {
    __shared__ u64 lds[3][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[3] = {0, 0, 0};                             // entries, worst-case spans, chunk bytes
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
        if (base + k < n && (!select || select[base + k])) {
            const u64 len = chunk_len[base + k];
            ++v[0];
            v[1] += z_worst_span(len);
            v[2] += len;
        }
    plan_block_sum<3>(v, lds);
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = v[0];
        block_span[blockIdx.x] = v[1];
        if (v[2]) atomicAdd((unsigned long long*)&totals[kBTotChunk], (unsigned long long)v[2]);
    }
}

// single block: exclusive scan of one or two block arrays in place (block_b may be NULL); totals[ia], totals[ib] = their sums
__global__ __launch_bounds__(kPlanBlock)
void zbatch_block_offsets_kernel(u64* __restrict__ block_a, u64* __restrict__ block_b, u64 n_blocks, u64* __restrict__ totals, int ia, int ib) {
    if (block_b) plan_block_offsets<true>(block_a, block_b, n_blocks, &totals[ia], &totals[ib]);
    else plan_block_offsets<false>(block_a, nullptr, n_blocks, &totals[ia], nullptr);      // (ib is not read: callers pass ia again)
}

// the selected rows, in row order, as entries: the row (digest | the chunk's ARENA OFFSET | the batch row | length; the layout
// turns the offset word into the blob's), where its worst-case span begins in the scratch, and -- for the error message and the
// hashing launcher, which outlive the offset word -- the arena offset and the length once more
__global__ __launch_bounds__(kPlanBlock)
void zbatch_compact_kernel(const u8* __restrict__ select, const u64* __restrict__ chunk_off, const u64* __restrict__ chunk_len,
                           const u8* __restrict__ digests, u64 n, const u64* __restrict__ block_cnt, const u64* __restrict__ block_span,
                           u64* __restrict__ rows, u64* __restrict__ w_off, u64* __restrict__ a_off, u64* __restrict__ p_len) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 len[kPlanPer];
    u64 cnt = 0, span = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const bool sel = base + k < n && (!select || select[base + k]);
        len[k] = sel ? chunk_len[base + k] : kBNone;
        if (sel) { ++cnt; span += z_worst_span(len[k]); }
    }
    u64 at = plan_first(cnt, block_cnt);
    u64 w = plan_first(span, block_span);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (len[k] == kBNone) continue;
        const u64 row = base + k;
        const u64 off = chunk_off[row];
        put_entry_row(rows + kEntryWords * at, digests + 32 * row, off, row, len[k] & 0xFFFFFFFFull);   // length | stored: the coder's
        w_off[at] = w;
        a_off[at] = off;
        p_len[at] = len[k];
        ++at;
        w += z_worst_span(len[k]);
    }
}

// ---- encode: zpack_encode_kernel with the arena as its input --------------------------------------------------------------------
__global__ __launch_bounds__(64)
void zbatch_encode_kernel(const u8* __restrict__ arena, u64* __restrict__ rows, const u64* __restrict__ w_off, u8* __restrict__ scratch, u64 n) {
    __shared__ u32 table[kZTable];
    z_encode_rows<ZLevel1>(arena, rows, w_off, scratch, n, table);
}

// ---- layout: mi_zrows.h's, over round16(stored) ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlanBlock)
void zbatch_layout_sums_kernel(const u64* __restrict__ rows, u64 n, u64* __restrict__ block_bytes, u64* __restrict__ totals) {
    z_layout_sums<false>(rows, n, block_bytes, totals, kBTotStored, kBTotRaw, 0);
}

// a raw chunk lies in the arena, at any alignment
__global__ __launch_bounds__(kPlanBlock)
void zbatch_place_kernel(u64* __restrict__ rows, const u64* __restrict__ w_off, u64 n, const u64* __restrict__ block_bytes, u64 arena_base,
                         u64 scratch_base, u64* __restrict__ e_src, u64* __restrict__ e_len, u64* __restrict__ e_dst) {
    z_place(rows, w_off, n, block_bytes, arena_base, scratch_base, e_src, e_len, e_dst);
}

// ---- gather: mi_gather.h's tile body, sources of either kind at any alignment ------------------------------------------------------

__global__ __launch_bounds__(kGatherWG)
void zbatch_gather_kernel(const u64* __restrict__ e_src, const u64* __restrict__ e_len, const u64* __restrict__ e_dst, u64 n_entries,
                          u64 blob_bytes, u8* __restrict__ blob) {
    gather_tile<false>(e_src, e_len, e_dst, n_entries, blob_bytes, blob);
}

// ---- MI_ZPACK_VERIFY: the digests of the decoded chunks against the batch's own table at chunk_index ------------------------------
__global__ __launch_bounds__(256)
void zbatch_compare_kernel(const u8* __restrict__ got, const u64* __restrict__ rows, const u8* __restrict__ digests, u64 n,
                           u64* __restrict__ first_bad) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    digest_differs_mark(got, (const u64*)(digests + 32 * rows[kEntryWords * k + 5]), k, first_bad);
}

// ---- mi_zset_missing: mi_fetch.hip's want list over zset_lookup_kernel's answer -------------------------------------------------
// held[r]: whether the set holds row r's digest (src[r] != 0).  A bad row, with stated lengths: a length of 0; a held digest whose
// length is not the stated one
__global__ __launch_bounds__(256)
void zbatch_held_kernel(const u64* __restrict__ src, const u64* __restrict__ word, const u32* __restrict__ stated, u64 n,
                        u8* __restrict__ held, u64* __restrict__ first_bad) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const bool found = src[r] != 0;
    held[r] = found ? 1 : 0;
    if (stated) {
        const u32 len = stated[r];
        if (len == 0 || (found && (u32)word[r] != len)) atomicMin((unsigned long long*)first_bad, (unsigned long long)r);
    }
}

// per block of kPlanTile rows: the first occurrences the set lacks; into the totals: their STATED bytes (the set knows nothing of a
// chunk it lacks), the first occurrences, those of them the set holds, and their PLAIN bytes as the set states them
__global__ __launch_bounds__(kPlanBlock)
void zbatch_want_sums_kernel(const i64* __restrict__ dup_of, const u8* __restrict__ held, const u64* __restrict__ len64,
                             const u32* __restrict__ stated, u64 n, u64* __restrict__ block_cnt, u64* __restrict__ totals) {
    __shared__ u64 lds[5][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[5] = {0, 0, 0, 0, 0};                       // wanted, their stated bytes, firsts, held firsts, their bytes
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const u64 row = base + k;
        if (row >= n || dup_of[row] >= 0) continue;
        ++v[2];
        if (held[row]) { ++v[3]; v[4] += len64[row]; }
        else { ++v[0]; v[1] += stated ? (u64)stated[row] : 0ull; }
    }
    plan_block_sum<5>(v, lds);
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = v[0];
        if (v[1]) atomicAdd((unsigned long long*)&totals[kMTotWantBytes], (unsigned long long)v[1]);
        if (v[2]) atomicAdd((unsigned long long*)&totals[kMTotFirst], (unsigned long long)v[2]);
        if (v[3]) atomicAdd((unsigned long long*)&totals[kMTotHeld], (unsigned long long)v[3]);
        if (v[4]) atomicAdd((unsigned long long*)&totals[kMTotHeldBytes], (unsigned long long)v[4]);
    }
}

// the want list: the numbers of the rows at which a digest the set lacks occurs for the first time, ascending
__global__ __launch_bounds__(kPlanBlock)
void zbatch_want_rows_kernel(const i64* __restrict__ dup_of, const u8* __restrict__ held, u64 n, const u64* __restrict__ block_cnt,
                             u64* __restrict__ want_rows) {
    want_rows_body([=](u64 row) { return dup_of[row] < 0 && !held[row]; }, n, block_cnt, want_rows);
}

}  // namespace mi

namespace {

constexpr u32 kEncodeWaves = 1u << 15;                // one wave an entry; more entries: the waves go round

}  // namespace

extern "C" {

int mi_batch_zpack_chunks(mi_batch* b, const uint8_t* select, uint64_t n_select, uint32_t flags, mi_zpack** out) {
    if (!b || !out) return MI_ERR_INVALID;
    static const char* who = "mi_batch_zpack_chunks";
    mi_ctx* c = b->ctx;
    *out = nullptr;
    if (b->group) return fail(c, MI_ERR_INVALID, "%s: a batch group has one arena per GPU; pack its members", who);
    if (flags & ~(uint32_t)(MI_ZPACK_VERIFY | MI_ZPACK_LEVEL2)) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    if (!b->ran || b->in_flight) return fail(c, MI_ERR_STATE, "%s: the batch must have run (and been waited for)", who);
    const u64 n = b->n_chunks;
    if (select && n_select != n)
        return fail(c, MI_ERR_INVALID, "%s: %llu selection flags for a batch of %llu chunks", who, (unsigned long long)n_select, (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    u64 n_sel = n;
    if (select) n_sel = n - (u64)std::count(select, select + n, (uint8_t)0);
    if (n_sel >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu entries, a pack holds fewer than 2^32", who, (unsigned long long)n_sel);
    const bool verify = (flags & MI_ZPACK_VERIFY) != 0;
    struct Owned { mi_zpack* z = nullptr; ~Owned() { if (z) mi_zpack_free(z); } } mine;   // (drains the ctx stream before the blob goes)
    void* d_blob = nullptr;
    mi_zpack_entry* h_rows = nullptr;
    int rc;
    if (n_sel == 0) {                                      // a valid zpack of nothing
        if ((rc = mi_zpack_alloc(c, who, 0, 0, &mine.z, &d_blob, &h_rows))) return rc;
        mi_zpack_set_result(mine.z, 0, 0, 0, verify ? 1u : 0u, 0, 0, 0);
        *out = mine.z;
        mine.z = nullptr;
        return MI_OK;
    }
    hipStream_t s = c->stream;
    const u64 nb = (n + kPlanTile - 1) / kPlanTile, nb_sel = (n_sel + kPlanTile - 1) / kPlanTile;
    DevBuf d_sel, d_scan, d_rows, d_woff, d_aoff, d_plen, d_scratch, e_src, e_len, e_dst, d_rule, d_got;
    Event ev[10];
    StreamDrain drain{s};   // (goes first: buffers and events after it)
    for (auto& e : ev) HIPCHK(c, e.create());
    // plan, first half: the entries and what their worst-case spans take
    HIPCHK(c, d_scan.ensure((2 * nb + 8) * 8));
    if (select) HIPCHK(c, d_sel.ensure(n));
    u64* block_cnt = d_scan.as<u64>();
    u64* block_span = block_cnt + nb;                      // (the layout's block array later: the plan is done with it by then)
    u64* totals = block_span + nb;                         // kBTot*
    if (select) HIPCHK(c, hipMemcpyAsync(d_sel.p, select, n, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(totals, 0, 6 * 8, s));
    HIPCHK(c, hipMemsetAsync(totals + kBTotBad, 0xFF, 2 * 8, s));
    HIPCHK(c, hipEventRecord(ev[0], s));
    hipLaunchKernelGGL(zbatch_plan_sums_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, s, d_sel.as<u8>(), b->chunk_len.as<u64>(), n, block_cnt, block_span,
                       totals);
    hipLaunchKernelGGL(zbatch_block_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, s, block_cnt, block_span, nb, totals, (int)kBTotEntries,
                       (int)kBTotSpan);
    HIPCHK(c, hipEventRecord(ev[1], s));
    u64* h = c->h_word.as<u64>();
    HIPCHK(c, hipMemcpyAsync(h, totals, 3 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    const u64 scratch_bytes = h[kBTotSpan], chunk_bytes = h[kBTotChunk];
    if (h[kBTotEntries] != n_sel || scratch_bytes < 32 * n_sel || scratch_bytes < chunk_bytes)
        return fail(c, MI_ERR_HIP, "%s: the plan counted %llu entries with %llu chunk bytes in %llu bytes of scratch, the selection holds %llu", who,
                    (unsigned long long)h[kBTotEntries], (unsigned long long)chunk_bytes, (unsigned long long)scratch_bytes, (unsigned long long)n_sel);
    // the scratch.  Does not fit: MI_ERR_NOMEM, nothing has changed
    hipError_t e = d_scratch.alloc_exact(scratch_bytes);
    if (e != hipSuccess) {
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        (void)hipGetLastError();
        return fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: the coder's scratch of %llu bytes (%llu entries) does not fit: the "
                    "device has %llu bytes free (%s); pack in several calls with partial selections", who, (unsigned long long)scratch_bytes,
                    (unsigned long long)n_sel, (unsigned long long)free_b, hipGetErrorString(e));
    }
    HIPCHK(c, d_rows.ensure(n_sel * sizeof(mi_zpack_entry)));
    HIPCHK(c, d_woff.ensure(n_sel * 8));
    HIPCHK(c, d_aoff.ensure(n_sel * 8));
    HIPCHK(c, d_plen.ensure(n_sel * 8));
    // plan, second half; the coder; the layout's totals
    HIPCHK(c, hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(zbatch_compact_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, s, d_sel.as<u8>(), b->chunk_off.as<u64>(), b->chunk_len.as<u64>(),
                       b->digests.as<u8>(), n, block_cnt, block_span, d_rows.as<u64>(), d_woff.as<u64>(), d_aoff.as<u64>(), d_plen.as<u64>());
    HIPCHK(c, hipEventRecord(ev[3], s));
    if (flags & MI_ZPACK_LEVEL2) {                         // the denser parse (mi_zpack2.hip): the same rows, spans and scratch
        if ((rc = mi_zencode_l2_enqueue(c, b->arena.p, d_rows.as<u64>(), d_woff.as<u64>(), d_scratch.p, n_sel,
                                        (u32)std::min<u64>(n_sel, kEncodeWaves))))
            return fail(c, rc, "%s: the level-2 coder was refused", who);
    } else {
        hipLaunchKernelGGL(zbatch_encode_kernel, dim3((u32)std::min<u64>(n_sel, kEncodeWaves)), dim3(64), 0, s, b->arena.as<u8>(), d_rows.as<u64>(),
                           d_woff.as<u64>(), d_scratch.as<u8>(), n_sel);
    }
    HIPCHK(c, hipEventRecord(ev[4], s));
    u64* block_bytes = block_span;
    hipLaunchKernelGGL(zbatch_layout_sums_kernel, dim3((u32)nb_sel), dim3(kPlanBlock), 0, s, d_rows.as<u64>(), n_sel, block_bytes, totals);
    hipLaunchKernelGGL(zbatch_block_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, s, block_bytes, (u64*)nullptr, nb_sel, totals, (int)kBTotBlob,
                       (int)kBTotBlob);
    HIPCHK(c, hipEventRecord(ev[5], s));
    HIPCHK(c, hipMemcpyAsync(h, totals, 6 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    const u64 blob_bytes = h[kBTotBlob], stored_bytes = h[kBTotStored], n_raw = h[kBTotRaw];
    if (blob_bytes < 16 * n_sel || stored_bytes > chunk_bytes || stored_bytes > blob_bytes || n_raw > n_sel)
        return fail(c, MI_ERR_HIP, "%s: the layout counted %llu stored bytes (%llu raw entries) in a blob of %llu for %llu chunk bytes", who,
                    (unsigned long long)stored_bytes, (unsigned long long)n_raw, (unsigned long long)blob_bytes, (unsigned long long)chunk_bytes);
    const u64 n_tiles = (blob_bytes + kGatherTile - 1) / kGatherTile;
    if (n_tiles >> 31) return fail(c, MI_ERR_INVALID, "%s: a blob of %llu bytes is more than one launch covers", who, (unsigned long long)blob_bytes);
    // the blob: device memory of its own.  Does not fit: MI_ERR_NOMEM naming both sizes, nothing has changed
    if ((rc = mi_zpack_alloc(c, who, n_sel, blob_bytes, &mine.z, &d_blob, &h_rows))) return rc;
    HIPCHK(c, e_src.ensure(n_sel * 8));
    HIPCHK(c, e_len.ensure(n_sel * 8));
    HIPCHK(c, e_dst.ensure(n_sel * 8));
    if (verify) {
        HIPCHK(c, d_rule.ensure(n_sel * 4));
        HIPCHK(c, d_got.ensure(n_sel * 32));
    }
    HIPCHK(c, hipEventRecord(ev[6], s));
    hipLaunchKernelGGL(zbatch_place_kernel, dim3((u32)nb_sel), dim3(kPlanBlock), 0, s, d_rows.as<u64>(), d_woff.as<u64>(), n_sel, block_bytes,
                       (u64)(size_t)b->arena.p, (u64)(size_t)d_scratch.p, e_src.as<u64>(), e_len.as<u64>(), e_dst.as<u64>());
    hipLaunchKernelGGL(zbatch_gather_kernel, dim3((u32)n_tiles), dim3(kGatherWG), 0, s, e_src.as<u64>(), e_len.as<u64>(), e_dst.as<u64>(), n_sel, blob_bytes,
                       (u8*)d_blob);
    HIPCHK(c, hipEventRecord(ev[7], s));
    if (verify) {
        // the new blob decoded into the scratch spans (the gather has read them: same stream), hashed there, held against the
        // digests the batch computed from the arena
        if ((rc = mi_zpack_decode_enqueue(c, d_blob, d_rows.as<u64>(), d_woff.as<u64>(), n_sel, d_scratch.p, d_rule.as<u32>(), totals + kBTotBad)))
            return fail(c, rc, "%s: the decode was refused", who);
        HIPCHK(c, hipEventRecord(ev[8], s));
        const auto hash_items = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? launch_blake2s_items : launch_sha256_items;
        hash_items(kShaBlobs, d_scratch.as<u8>(), d_woff.as<u64>(), d_plen.as<u64>(), nullptr, (u32)n_sel, nullptr, c->heads.as<u32>(), nullptr, true,
                   d_got.as<u8>(), c->sha, c->prop.multiProcessorCount, scratch_bytes, s);
        hipLaunchKernelGGL(zbatch_compare_kernel, dim3((u32)((n_sel + 255) / 256)), dim3(256), 0, s, d_got.as<u8>(), d_rows.as<u64>(),
                           b->digests.as<u8>(), n_sel, totals + kBTotDiffer);
        HIPCHK(c, hipMemcpyAsync(h, totals + kBTotBad, 2 * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipEventRecord(ev[9], s));
    // the entries to the host with the same synchronisation: mi_zpack_entries only reads from then on
    HIPCHK(c, hipMemcpyAsync(h_rows, d_rows.p, n_sel * sizeof(mi_zpack_entry), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    float ms_plan = 0, ms_rows = 0, ms_enc = 0, ms_layout = 0, ms_gather = 0, ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms_plan, ev[0], ev[1]));
    HIPCHK(c, hipEventElapsedTime(&ms_rows, ev[2], ev[3]));
    HIPCHK(c, hipEventElapsedTime(&ms_enc, ev[3], ev[4]));
    HIPCHK(c, hipEventElapsedTime(&ms_layout, ev[4], ev[5]));
    HIPCHK(c, hipEventElapsedTime(&ms_gather, ev[6], ev[7]));
    double ms_verify = 0, ms_decode = 0;
    if (verify) {
        HIPCHK(c, hipEventElapsedTime(&ms, ev[7], ev[9]));
        ms_verify = ms;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[7], ev[8]));
        ms_decode = ms;
        const u64 undecodable = h[0], differs = h[1];
        const u64 bad = std::min(undecodable, differs);
        if (bad != kBNone) {
            const mi_zpack_entry row = bad < n_sel ? h_rows[bad] : mi_zpack_entry{};
            u64 arena_off = 0;
            u32 rule = 0;
            if (bad < n_sel) {
                HIPCHK(c, hipMemcpy(&arena_off, d_aoff.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
                HIPCHK(c, hipMemcpy(&rule, d_rule.as<u32>() + bad, 4, hipMemcpyDeviceToHost));
            }
            return fail(c, MI_ERR_IO, "%s: entry %llu -- chunk row %llu, %u bytes at arena offset %llu, %u bytes stored at blob offset %llu, digest %s "
                        "-- %s%s", who, (unsigned long long)bad, (unsigned long long)row.chunk_index, row.length, (unsigned long long)arena_off,
                        row.stored, (unsigned long long)row.offset, hex32(row.digest).c_str(),
                        rule ? "does not decode on the device: " : "decodes on the device to bytes that hash to another digest than the batch computed "
                        "from the arena", rule ? mi_host::lz4_rule_name(rule) : "");
        }
    }
    mi_zpack_set_result(mine.z, stored_bytes, n_raw, chunk_bytes, verify ? 1u : 0u, (double)ms_plan + ms_rows + ms_layout + ms_gather, ms_verify,
                        ms_decode);
    mi_zpack_set_encode_ms(mine.z, ms_enc);
    *out = mine.z;
    mine.z = nullptr;
    return MI_OK;
}

int mi_zset_missing(const mi_zset* set, const uint8_t* digests, const uint32_t* lengths, uint64_t n, uint8_t* held, uint64_t* want_rows,
                    uint64_t cap, mi_want_info* info) {
    if (info) memset(info, 0, sizeof *info);
    if (!set || (n && !digests) || (cap && !want_rows)) return MI_ERR_INVALID;
    static const char* who = "mi_zset_missing";
    mi_ctx* c = nullptr;
    int rc = mi_zset_ctx(set, who, &c);                    // (a set in its sticky failed state: MI_ERR_STATE)
    if (rc) return rc;
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu rows, a request holds fewer than 2^32", who, (unsigned long long)n);
    if (n == 0) return MI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevBuf d_dig, d_len32, d_src, d_word, d_len64, d_held, d_dup, d_scan, d_want;
    Event ev[2];
    StreamDrain drain{s};   // (goes first: buffers and events after it)
    for (auto& e : ev) HIPCHK(c, e.create());
    const u64 nb = (n + kPlanTile - 1) / kPlanTile;
    u64 dd_cap = 1024;
    while (dd_cap < 2 * n) dd_cap <<= 1;
    HIPCHK(c, d_dig.ensure(n * 32));
    if (lengths) HIPCHK(c, d_len32.ensure(n * 4));
    HIPCHK(c, d_src.ensure(n * 8));
    HIPCHK(c, d_word.ensure(n * 8));
    HIPCHK(c, d_len64.ensure(n * 8));
    HIPCHK(c, d_held.ensure(n));
    HIPCHK(c, d_dup.ensure(n * 8));
    HIPCHK(c, d_scan.ensure((nb + 8) * 8));
    HIPCHK(c, d_want.ensure(n * 8));
    HIPCHK(c, c->dd_table.ensure(dd_cap * 8));
    HIPCHK(c, c->dd_slot.ensure(n * 4 + 16));
    HIPCHK(c, c->dd_nuniq.ensure(8));
    u64* block_cnt = d_scan.as<u64>();
    u64* totals = block_cnt + nb;                          // kMTot*
    const u32* stated = lengths ? d_len32.as<u32>() : (const u32*)nullptr;
    // lookup, held flags, first occurrences, the scan, the want rows; one synchronisation: the totals
    HIPCHK(c, hipEventRecord(ev[0], s));
    HIPCHK(c, hipMemcpyAsync(d_dig.p, digests, n * 32, hipMemcpyHostToDevice, s));
    if (lengths) HIPCHK(c, hipMemcpyAsync(d_len32.p, lengths, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(totals, 0, 6 * 8, s));
    HIPCHK(c, hipMemsetAsync(totals + kMTotBad, 0xFF, 2 * 8, s));
    if ((rc = mi_zset_lookup_enqueue(set, d_dig.as<u8>(), nullptr, n, d_src.as<u64>(), d_word.as<u64>(), d_len64.as<u64>(), totals + kMTotLookup)))
        return fail(c, rc, "%s: the lookup was refused", who);
    hipLaunchKernelGGL(zbatch_held_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, s, d_src.as<u64>(), d_word.as<u64>(), stated, n,
                       d_held.as<u8>(), totals + kMTotBad);
    launch_dedup_mark(d_dig.as<u8>(), n, nullptr, c->dd_table.as<u32>(), c->dd_slot.as<u32>(), dd_cap, d_dup.as<i64>(), c->dd_nuniq.as<u64>(),
                      true, s);
    hipLaunchKernelGGL(zbatch_want_sums_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, s, d_dup.as<i64>(), d_held.as<u8>(), d_len64.as<u64>(), stated, n,
                       block_cnt, totals);
    hipLaunchKernelGGL(zbatch_block_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, s, block_cnt, (u64*)nullptr, nb, totals, (int)kMTotWant, (int)kMTotWant);
    hipLaunchKernelGGL(zbatch_want_rows_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, s, d_dup.as<i64>(), d_held.as<u8>(), n, block_cnt, d_want.as<u64>());
    HIPCHK(c, hipEventRecord(ev[1], s));
    u64* h = c->h_word.as<u64>();
    HIPCHK(c, hipMemcpyAsync(h, totals, 8 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (h[kMTotBad] != kBNone) {                           // the smallest bad row, in mi_packset_missing's words
        const u64 bad = h[kMTotBad];
        u64 w = 0;
        if (lengths && lengths[bad] == 0) return fail(c, MI_ERR_INVALID, "%s: row %llu has length 0", who, (unsigned long long)bad);
        HIPCHK(c, hipMemcpy(&w, d_word.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
        return fail(c, MI_ERR_INVALID, "%s: row %llu: the compressed pack set holds digest %s with %u bytes, the request states %u", who,
                    (unsigned long long)bad, hex32(digests + 32 * bad).c_str(), (u32)w, lengths ? lengths[bad] : 0u);
    }
    return want_list_finish(c, who, n, h[kMTotFirst], h[kMTotHeld], h[kMTotWant], h[kMTotHeldBytes], h[kMTotWantBytes], ev[0], ev[1], d_held.p,
                            d_want.p, held, want_rows, cap, info);
}

}  // extern "C"
