// mi_fetch.hip -- what connects the two halves of the chunk store at chunk granularity: a set of resident packs (mi_restore.hip)
// asked WHICH digests of a request it lacks (mi_packset_missing), and a set CUT BY DIGEST into a new pack of exactly the
// requested chunks, from whatever packs hold them (mi_packset_pack) -- a digest-addressed lookup plus a gather.  The puller
// turns a layer's recipes into a want list, the server turns a want list into one pack, a store compacts itself by packing
// its live digests.  Everything runs on the ctx stream.
//
//   resolve   36 (or 32) bytes a request row go up; one thread per row walks the set's table -- tag first, then all 32 bytes:
//             slot_table_find (mi_slot_table.h), the length compared only when lengths were given -- and writes the chunk's device
//             address, the SET'S length and the held flag; the smallest bad row by atomicMin;
//   firsts    a row counts only if no smaller row carries its digest: the engine's marking over the uploaded digests
//             (launch_dedup_mark, what mi_dedup_mark runs: whole digests, dup_of < 0 = a first occurrence);
//   plan      mi_plan.h's three launches with the lengths the resolve found.  missing: first occurrence and not held -> the
//             row numbers (the want list, finished by want_list_finish for mi_zset_missing too), the byte sums;
//             pack: first occurrence -> source address, length, blob offset and the 56-byte mi_pack_entry row per entry;
//   gather    destination-driven like pack_gather_kernel: 16 KiB tiles, a 256-thread workgroup a tile, the tile's entries (at
//             most 1 024) in LDS, every lane four 16-byte units 4 KiB apart, all its loads before its first store.  The
//             sources are ABSOLUTE device addresses in several allocations, every one 16-byte aligned (a blob's base is the
//             allocator's, an entry's offset a checked multiple of 16): a unit is one ALIGNED global_load_dwordx4, the bytes
//             at and beyond the chunk's length are zeroed in registers -- the source's own pad is never trusted -- and one
//             aligned global_store_dwordx4;
//   verify    MI_SUBPACK_VERIFY: the new blob's entries through the ctx's own hashing launcher (pass kShaBlobs), held against
//             the REQUESTED digests on the device.
//
// READ BOUND.  A unit's load begins at src + o, src the device address of an entry of a resident blob, o a multiple of 16 with
// 0 <= o < len, and is 16 bytes long: it lies inside [src, src + round16(len)), which the structural check of the add
// (offset + round16(length) <= blob_bytes, always, on the host) keeps inside the source blob.  Nothing in front of an entry and
// nothing behind its padded span is read -- not even the blob's slack.  The verify pass reads what the hashing kernels read
// behind a string (up to 67 bytes) behind the NEW blob's last entry: inside the 256 bytes it is allocated with.
#include "mi_gather.h"
#include "mi_plan.h"
#include "mi_slot_table.h"

#include <string.h>

#include <string>

using namespace mi;

namespace mi {

constexpr u64 kFetchNone = ~0ull;

// ---- resolve ------------------------------------------------------------------------------------------------------------------
// src[r], len64[r]: where the set holds row r's chunk and with how many bytes (0, 0: it does not); held[r]: whether it does.
// A bad row: a stated length of 0; a held digest whose length is not the stated one; with must_hold, a digest the set does not
// hold or holds with 0 bytes (only a hand-made blob carries such an entry; a pack has no room for it)
__global__ __launch_bounds__(256)
void fetch_lookup_kernel(const u8* __restrict__ digests, const u32* __restrict__ lengths, u64 n, const u64* __restrict__ tags,
                         const u64* __restrict__ slots, u64 mask, int must_hold, u64* __restrict__ src, u64* __restrict__ len64,
                         u8* __restrict__ held, u64* __restrict__ first_bad) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const u8* d = digests + 32 * r;
    u64 at = 0, has = 0;
    const u64 slot = slot_table_find(tags, slots, mask, d);
    const bool found = slot != kSlotNone;
    if (found) {
        at = slots[kSlotWords * slot + 4];
        has = slots[kSlotWords * slot + 5] & 0xFFFFFFFFull;
    }
    src[r] = at;
    len64[r] = has;
    held[r] = found ? 1 : 0;
    bool bad = must_hold && (!found || has == 0);
    if (lengths) {
        const u32 len = lengths[r];
        bad = bad || len == 0 || (found && has != len);
    }
    if (bad) atomicMin((unsigned long long*)first_bad, (unsigned long long)r);
}

// ---- plan: mi_plan.h's over the resolved rows -------------------------------------------------------------------------------------
enum : int { kTotEntries = 0, kTotBlob = 1, kTotRaw = 2, kTotFirst = 3, kTotHeld = 4, kTotHeldBytes = 5, kTotBad = 6, kTotDiffer = 7 };

// the selection: a first occurrence that the set holds (want_held: the sub-pack's entries) or lacks (the want list)
static __device__ __forceinline__ bool fetch_selected(const i64* __restrict__ dup_of, const u8* __restrict__ held, u64 row, int want_held) {
    return dup_of[row] < 0 && (held[row] != 0) == (want_held != 0);
}

// per block of kPlanTile rows: the selected rows and their rounded-up bytes (the set's lengths); into the totals: the selected
// rows' bytes as they are (the set's lengths, or for the want list the STATED ones: the set knows nothing of a chunk it lacks),
// the first occurrences, those of them the set holds, and their bytes
__global__ __launch_bounds__(kPlanBlock)
void fetch_block_sums_kernel(const i64* __restrict__ dup_of, const u8* __restrict__ held, const u64* __restrict__ len64,
                             const u32* __restrict__ stated, u64 n, int want_held, u64* __restrict__ block_cnt,
                             u64* __restrict__ block_bytes, u64* __restrict__ totals) {
    __shared__ u64 lds[6][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[6] = {0, 0, 0, 0, 0, 0};                       // selected, their rounded-up bytes, their bytes, firsts, held firsts, their bytes
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const u64 row = base + k;
        if (row >= n || dup_of[row] >= 0) continue;
        const bool h = held[row] != 0;
        const u64 len = len64[row];
        ++v[3];
        if (h) { ++v[4]; v[5] += len; }
        if (h == (want_held != 0)) {
            ++v[0];
            v[1] += round16(len);
            v[2] += want_held ? len : stated ? (u64)stated[row] : 0ull;
        }
    }
    plan_block_sum<6>(v, lds);
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = v[0];
        block_bytes[blockIdx.x] = v[1];
        if (v[2]) atomicAdd((unsigned long long*)&totals[kTotRaw], (unsigned long long)v[2]);
        if (v[3]) atomicAdd((unsigned long long*)&totals[kTotFirst], (unsigned long long)v[3]);
        if (v[4]) atomicAdd((unsigned long long*)&totals[kTotHeld], (unsigned long long)v[4]);
        if (v[5]) atomicAdd((unsigned long long*)&totals[kTotHeldBytes], (unsigned long long)v[5]);
    }
}

// single block: exclusive scan of both block arrays in place; the totals: selected rows, their rounded-up bytes
__global__ __launch_bounds__(kPlanBlock)
void fetch_block_offsets_kernel(u64* __restrict__ block_cnt, u64* __restrict__ block_bytes, u64 n_blocks, u64* __restrict__ totals) {
    plan_block_offsets<true>(block_cnt, block_bytes, n_blocks, &totals[kTotEntries], &totals[kTotBlob]);
}

// the want list: the selected rows' numbers, ascending
__global__ __launch_bounds__(kPlanBlock)
void fetch_compact_rows_kernel(const i64* __restrict__ dup_of, const u8* __restrict__ held, u64 n, const u64* __restrict__ block_cnt,
                               u64* __restrict__ want_rows) {
    want_rows_body([=](u64 row) { return fetch_selected(dup_of, held, row, 0); }, n, block_cnt, want_rows);
}

// the sub-pack's entries, in order of first occurrence: where the chunk lies, its length, where it goes in the blob, and the
// mi_pack_entry row (digest | offset | chunk_index = the request row | length, reserved = 0)
__global__ __launch_bounds__(kPlanBlock)
void fetch_compact_entries_kernel(const i64* __restrict__ dup_of, const u8* __restrict__ held, const u64* __restrict__ src,
                                  const u64* __restrict__ len64, const u8* __restrict__ digests, u64 n,
                                  const u64* __restrict__ block_cnt, const u64* __restrict__ block_bytes, u64* __restrict__ e_src,
                                  u64* __restrict__ e_len, u64* __restrict__ e_dst, u64* __restrict__ rows) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 len[kPlanPer];
    u64 cnt = 0, bytes = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const bool sel = base + k < n && fetch_selected(dup_of, held, base + k, 1);
        len[k] = sel ? len64[base + k] : kFetchNone;
        if (sel) { ++cnt; bytes += round16(len[k]); }
    }
    u64 at = plan_first(cnt, block_cnt);
    u64 dst = plan_first(bytes, block_bytes);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (len[k] == kFetchNone) continue;
        const u64 row = base + k;
        e_src[at] = src[row];
        e_len[at] = len[k];
        e_dst[at] = dst;
        put_entry_row(rows + kEntryWords * at, digests + 32 * row, dst, row, len[k] & 0xFFFFFFFFull);   // length | reserved = 0
        ++at;
        dst += round16(len[k]);
    }
}

// ---- gather: mi_gather.h's tile body over aligned sources -------------------------------------------------------------------------

__global__ __launch_bounds__(kGatherWG)
void fetch_gather_kernel(const u64* __restrict__ e_src, const u64* __restrict__ e_len, const u64* __restrict__ e_dst, u64 n_entries,
                         u64 blob_bytes, u8* __restrict__ blob) {
    gather_tile<true>(e_src, e_len, e_dst, n_entries, blob_bytes, blob);
}

// ---- MI_SUBPACK_VERIFY: the digests of the new blob's entries against the requested ones (the rows carry them) ---------------
__global__ __launch_bounds__(256)
void fetch_compare_kernel(const u8* __restrict__ got, const u64* __restrict__ rows, u64 n, u64* __restrict__ first_bad) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    digest_differs_mark(got, rows + kEntryWords * k, k, first_bad);
}

}  // namespace mi

namespace {

// what one call holds on the device until it returns
struct Request {
    DevBuf dig, len32, src, len64, held, dup, scan, want;
    Event ev[4];
    u64 nb = 0;
    u64* block_cnt = nullptr;
    u64* block_bytes = nullptr;
    u64* totals = nullptr;                              // kTot*
    const u32* stated() const { return len32.p ? len32.as<u32>() : nullptr; }
};

// Enqueues the request's way up, the lookup, the marking of first occurrences and the plan's first two launches; the want list's
// compaction behind them when asked for (it needs nothing from the host).  One synchronisation: the eight totals lie in c->h_word
int resolve_and_plan(mi_ctx* c, const uint64_t* tags, const uint64_t* slots, u64 cap, const uint8_t* digests, const uint32_t* lengths,
                     u64 n, bool must_hold, Request* q) {
    hipStream_t s = c->stream;
    for (auto& e : q->ev) HIPCHK(c, e.create());
    q->nb = (n + kPlanTile - 1) / kPlanTile;
    u64 dd_cap = 1024;
    while (dd_cap < 2 * n) dd_cap <<= 1;
    HIPCHK(c, q->dig.ensure(n * 32));
    if (lengths) HIPCHK(c, q->len32.ensure(n * 4));
    HIPCHK(c, q->src.ensure(n * 8));
    HIPCHK(c, q->len64.ensure(n * 8));
    HIPCHK(c, q->held.ensure(n));
    HIPCHK(c, q->dup.ensure(n * 8));
    HIPCHK(c, q->scan.ensure((2 * q->nb + 8) * 8));
    if (!must_hold) HIPCHK(c, q->want.ensure(n * 8));
    HIPCHK(c, c->dd_table.ensure(dd_cap * 8));
    HIPCHK(c, c->dd_slot.ensure(n * 4 + 16));
    HIPCHK(c, c->dd_nuniq.ensure(8));
    q->block_cnt = q->scan.as<u64>();
    q->block_bytes = q->block_cnt + q->nb;
    q->totals = q->block_bytes + q->nb;
    HIPCHK(c, hipEventRecord(q->ev[0], s));
    HIPCHK(c, hipMemcpyAsync(q->dig.p, digests, n * 32, hipMemcpyHostToDevice, s));
    if (lengths) HIPCHK(c, hipMemcpyAsync(q->len32.p, lengths, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(q->totals, 0, 6 * 8, s));
    HIPCHK(c, hipMemsetAsync(q->totals + kTotBad, 0xFF, 2 * 8, s));
    const u32 row_blocks = (u32)((n + 255) / 256);
    hipLaunchKernelGGL(fetch_lookup_kernel, dim3(row_blocks), dim3(256), 0, s, q->dig.as<u8>(), q->stated(), n, tags, slots, cap - 1,
                       must_hold ? 1 : 0, q->src.as<u64>(), q->len64.as<u64>(), q->held.as<u8>(), q->totals + kTotBad);
    launch_dedup_mark(q->dig.as<u8>(), n, nullptr, c->dd_table.as<u32>(), c->dd_slot.as<u32>(), dd_cap, q->dup.as<i64>(),
                      c->dd_nuniq.as<u64>(), true, s);
    hipLaunchKernelGGL(fetch_block_sums_kernel, dim3((u32)q->nb), dim3(kPlanBlock), 0, s, q->dup.as<i64>(), q->held.as<u8>(),
                       q->len64.as<u64>(), q->stated(), n, must_hold ? 1 : 0, q->block_cnt, q->block_bytes, q->totals);
    hipLaunchKernelGGL(fetch_block_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, s, q->block_cnt, q->block_bytes, q->nb, q->totals);
    if (!must_hold)
        hipLaunchKernelGGL(fetch_compact_rows_kernel, dim3((u32)q->nb), dim3(kPlanBlock), 0, s, q->dup.as<i64>(), q->held.as<u8>(), n,
                           q->block_cnt, q->want.as<u64>());
    HIPCHK(c, hipEventRecord(q->ev[1], s));
    HIPCHK(c, hipMemcpyAsync(c->h_word.p, q->totals, 8 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    return MI_OK;
}

// the smallest bad row, in mi_batch_add_recipes' words
int refuse_row(mi_ctx* c, const char* who, const Request& q, u64 bad, const uint8_t* digests, const uint32_t* lengths) {
    u64 has = 0;
    u8 found = 0;
    HIPCHK(c, hipMemcpy(&has, q.len64.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&found, q.held.as<u8>() + bad, 1, hipMemcpyDeviceToHost));
    const std::string dg = hex32(digests + 32 * bad);
    if (lengths && lengths[bad] == 0) return fail(c, MI_ERR_INVALID, "%s: row %llu has length 0", who, (unsigned long long)bad);
    if (!found) return fail(c, MI_ERR_INVALID, "%s: row %llu: the pack set does not hold digest %s", who, (unsigned long long)bad, dg.c_str());
    if (lengths && has != lengths[bad])
        return fail(c, MI_ERR_INVALID, "%s: row %llu: the pack set holds digest %s with %u bytes, the request states %u", who,
                    (unsigned long long)bad, dg.c_str(), (u32)has, lengths[bad]);
    return fail(c, MI_ERR_INVALID, "%s: row %llu: the pack set holds digest %s with 0 bytes, a pack has no entry for it", who,
                (unsigned long long)bad, dg.c_str());
}

}  // namespace

namespace mi {

int want_list_finish(mi_ctx* c, const char* who, u64 n, u64 n_distinct, u64 n_held, u64 n_want, u64 held_bytes, u64 want_bytes,
                     hipEvent_t ev0, hipEvent_t ev1, const void* d_held, const void* d_want, uint8_t* held, uint64_t* want_rows,
                     uint64_t cap, mi_want_info* info) {
    mi_want_info out = {};
    out.n_rows = n;
    out.n_distinct = n_distinct;
    out.n_held = n_held;
    out.n_want = n_want;
    out.held_bytes = held_bytes;
    out.want_bytes = want_bytes;
    if (out.n_held + out.n_want != out.n_distinct)
        return fail(c, MI_ERR_HIP, "%s: the plan counted %llu held and %llu missing among %llu distinct digests", who,
                    (unsigned long long)out.n_held, (unsigned long long)out.n_want, (unsigned long long)out.n_distinct);
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev0, ev1));
    out.ms_resolve = ms;
    if (info) *info = out;
    const bool fits = out.n_want <= cap;
    if (held) HIPCHK(c, hipMemcpyAsync(held, d_held, n, hipMemcpyDeviceToHost, c->stream));
    if (fits && out.n_want) HIPCHK(c, hipMemcpyAsync(want_rows, d_want, out.n_want * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!fits && (cap || want_rows))
        return fail(c, MI_ERR_CAPACITY, "%s: the want list buffer holds %llu rows, need %llu", who, (unsigned long long)cap,
                    (unsigned long long)out.n_want);
    return MI_OK;
}

}  // namespace mi

extern "C" {

int mi_packset_missing(const mi_packset* set, const uint8_t* digests, const uint32_t* lengths, uint64_t n, uint8_t* held,
                       uint64_t* want_rows, uint64_t cap, mi_want_info* info) {
    if (info) memset(info, 0, sizeof *info);
    if (!set || (n && !digests) || (cap && !want_rows)) return MI_ERR_INVALID;
    static const char* who = "mi_packset_missing";
    mi_ctx* c = nullptr;
    const uint64_t* tags = nullptr;
    const uint64_t* slots = nullptr;
    u64 t_cap = 0;
    int rc = mi_packset_table(set, who, &c, &tags, &slots, &t_cap);
    if (rc) return rc;
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu rows, a request holds fewer than 2^32", who, (unsigned long long)n);
    if (n == 0) return MI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    Request q;
    StreamDrain drain{c->stream};   // (goes first: buffers and events after it)
    rc = resolve_and_plan(c, tags, slots, t_cap, digests, lengths, n, false, &q);
    if (rc) return rc;
    const u64* h = c->h_word.as<u64>();
    if (h[kTotBad] != kFetchNone) return refuse_row(c, who, q, h[kTotBad], digests, lengths);
    return want_list_finish(c, who, n, h[kTotFirst], h[kTotHeld], h[kTotEntries], h[kTotHeldBytes], h[kTotRaw], q.ev[0], q.ev[1], q.held.p,
                            q.want.p, held, want_rows, cap, info);
}

int mi_packset_pack(const mi_packset* set, const uint8_t* digests, const uint32_t* lengths, uint64_t n, uint32_t flags, mi_pack** out,
                    uint64_t* first_bad) {
    if (first_bad) *first_bad = 0;
    if (out) *out = nullptr;
    if (!set || !out || (n && !digests)) return MI_ERR_INVALID;
    static const char* who = "mi_packset_pack";
    mi_ctx* c = nullptr;
    const uint64_t* tags = nullptr;
    const uint64_t* slots = nullptr;
    u64 t_cap = 0;
    int rc = mi_packset_table(set, who, &c, &tags, &slots, &t_cap);
    if (rc) return rc;
    if (flags & ~(uint32_t)MI_SUBPACK_VERIFY) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu rows, a pack holds fewer than 2^32", who, (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0) return mi_pack_empty(c, out);
    hipStream_t s = c->stream;
    struct Owned { mi_pack* p = nullptr; ~Owned() { if (p) mi_pack_free(p); } } mine;   // (drains the ctx stream before the blob goes)
    Request q;
    DevBuf e_src, e_len, e_dst, d_rows, d_got;
    StreamDrain drain{s};   // (goes first: buffers and events after it)
    rc = resolve_and_plan(c, tags, slots, t_cap, digests, lengths, n, true, &q);
    if (rc) return rc;
    u64* h = c->h_word.as<u64>();
    if (h[kTotBad] != kFetchNone) {
        if (first_bad) *first_bad = h[kTotBad];
        return refuse_row(c, who, q, h[kTotBad], digests, lengths);
    }
    const u64 n_sel = h[kTotEntries], blob_bytes = h[kTotBlob], chunk_bytes = h[kTotRaw];
    if (n_sel == 0 || n_sel != h[kTotFirst] || blob_bytes < 16 * n_sel)
        return fail(c, MI_ERR_HIP, "%s: the plan counted %llu entries in %llu bytes among %llu distinct digests", who, (unsigned long long)n_sel,
                    (unsigned long long)blob_bytes, (unsigned long long)h[kTotFirst]);
    const u64 n_tiles = (blob_bytes + kGatherTile - 1) / kGatherTile;
    if (n_tiles >> 31) return fail(c, MI_ERR_INVALID, "%s: a blob of %llu bytes is more than one launch covers", who, (unsigned long long)blob_bytes);
    void* d_blob = nullptr;
    mi_pack_entry* h_rows = nullptr;
    rc = mi_pack_alloc(c, who, n_sel, blob_bytes, chunk_bytes, &mine.p, &d_blob, &h_rows);      // does not fit: MI_ERR_NOMEM, nothing has changed
    if (rc) return rc;
    HIPCHK(c, d_rows.ensure(n_sel * sizeof(mi_pack_entry)));
    HIPCHK(c, e_src.ensure(n_sel * 8));
    HIPCHK(c, e_len.ensure(n_sel * 8));
    HIPCHK(c, e_dst.ensure(n_sel * 8));
    if (flags & MI_SUBPACK_VERIFY) HIPCHK(c, d_got.ensure(n_sel * 32));
    // plan, second half; the gather; the verification
    hipLaunchKernelGGL(fetch_compact_entries_kernel, dim3((u32)q.nb), dim3(kPlanBlock), 0, s, q.dup.as<i64>(), q.held.as<u8>(),
                       q.src.as<u64>(), q.len64.as<u64>(), q.dig.as<u8>(), n, q.block_cnt, q.block_bytes, e_src.as<u64>(), e_len.as<u64>(),
                       e_dst.as<u64>(), d_rows.as<u64>());
    HIPCHK(c, hipEventRecord(q.ev[1], s));
    hipLaunchKernelGGL(fetch_gather_kernel, dim3((u32)n_tiles), dim3(kGatherWG), 0, s, e_src.as<u64>(), e_len.as<u64>(), e_dst.as<u64>(), n_sel,
                       blob_bytes, (u8*)d_blob);
    HIPCHK(c, hipEventRecord(q.ev[2], s));
    if (flags & MI_SUBPACK_VERIFY) {
        const auto hash_items = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? launch_blake2s_items : launch_sha256_items;
        hash_items(kShaBlobs, (const u8*)d_blob, e_dst.as<u64>(), e_len.as<u64>(), nullptr, (u32)n_sel, nullptr, c->heads.as<u32>(), nullptr,
                   true, d_got.as<u8>(), c->sha, c->prop.multiProcessorCount, blob_bytes, s);     // entries in blob order: flat sharing
        hipLaunchKernelGGL(fetch_compare_kernel, dim3((u32)((n_sel + 255) / 256)), dim3(256), 0, s, d_got.as<u8>(), d_rows.as<u64>(), n_sel,
                           q.totals + kTotDiffer);
        HIPCHK(c, hipMemcpyAsync(h, q.totals + kTotDiffer, 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipEventRecord(q.ev[3], s));
    // the entries to the host with the same synchronisation: mi_pack_entries only reads from then on
    HIPCHK(c, hipMemcpyAsync(h_rows, d_rows.p, n_sel * sizeof(mi_pack_entry), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    float ms_gather = 0, ms_verify = 0;
    HIPCHK(c, hipEventElapsedTime(&ms_gather, q.ev[1], q.ev[2]));
    if (flags & MI_SUBPACK_VERIFY) {
        HIPCHK(c, hipEventElapsedTime(&ms_verify, q.ev[2], q.ev[3]));
        const u64 bad = h[0];
        if (bad != kFetchNone) {
            const mi_pack_entry row = bad < n_sel ? h_rows[bad] : mi_pack_entry{};
            u64 src = 0;
            (void)hipMemcpy(&src, e_src.as<u64>() + bad, 8, hipMemcpyDeviceToHost);
            if (first_bad) *first_bad = row.chunk_index;
            return fail(c, MI_ERR_IO, "%s: row %llu (entry %llu), %u bytes from source address %#llx at blob offset %llu: the gathered bytes do "
                        "not hash to the requested digest %s -- the set was fed a damaged blob without MI_PACKSET_VERIFY", who,
                        (unsigned long long)row.chunk_index, (unsigned long long)bad, row.length, (unsigned long long)src,
                        (unsigned long long)row.offset, hex32(row.digest).c_str());
        }
    }
    mi_pack_set_result(mine.p, (flags & MI_SUBPACK_VERIFY) ? 1u : 0u, ms_gather, ms_verify);
    *out = mine.p;
    mine.p = nullptr;
    return MI_OK;
}

}  // extern "C"
