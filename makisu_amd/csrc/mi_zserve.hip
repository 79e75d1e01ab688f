// mi_zserve.hip -- a compressed pack set CUT FOR A READER THAT KNOWS LESS THAN THE SET: mi_zset_zpack_unwrapped, the
// cut without the entropy stage (a form H entry carries its inner form: the LZ4 block, or the chunk's plain bytes as a raw entry;
// every other entry is moved as mi_zset_zpack moves it), and mi_zset_pack, the plain cut (an ordinary mi_pack, every entry decoded
// straight to its place).  Neither builds a plain set, a table or an intermediate zpack; the set is only read.
//
//   resolve   mi_zset.hip's lookup (mi_zset_lookup_enqueue) and the engine's first-occurrence marking, as mi_zset_zpack;
//   sizes     zcut_sizes_kernel, mi_plan.h's block shape: a first occurrence's form from its word and its first bytes (zh_form),
//             and what it takes in the NEW blob -- form H: the inner length that stands in its header (a header that breaks rule 8
//             is laid out as it lies and refused by the wave that meets it); the plain cut: the chunk's length -- per block; into
//             the totals: entries, stored bytes, raw entries, chunk bytes, form H rows, and for the plain cut the scratch the
//             requested kind-1 rows need (their inner lengths on a 64-byte grid);
//   scan      zcut_offsets_kernel: the exclusive scan of the three block arrays.  ONE synchronisation: the totals;
//   entries   zcut_entries_kernel: the compact list in order of first occurrence -- span, word, place, bytes -- and the 56-byte rows;
//   unwrapped zcut_gather_kernel (mi_gather.h's tile body) moves the verbatim rows; a form H row's place is zero-filled by it
//             from a block of zeroes of the call's (the tile body writes every unit of a tile, and its list must be gapless), then
//             zcut_unwrap_kernel, ONE WAVE A FORM H ROW, writes the inner form there: no scratch of inner forms, nothing reads one;
//   plain     zcut_decode_kernel, one launch, ONE WAVE AN ENTRY: a raw row copied, an LZ4 row through z_decode_block, form H over
//             raw unwrapped into the pack, form H over LZ4 unwrapped into the row's span of the scratch and decoded from there by
//             the same wave behind a barrier; the pad behind the chunk zeroed, the pad behind the stored span held against zero;
//   verify    MI_ZPACK_VERIFY: mi_zset.hip's (the new blob decoded into a scratch and hashed); MI_SUBPACK_VERIFY: the new blob's
//             entries through the ctx's hashing launcher where they lie, zcut_compare_kernel against the REQUESTED digests.
//
// LDS.  zcut_unwrap_kernel and zcut_decode_kernel: kZhUnwrapLds = 4 928 bytes (mi_huff_wave.h).  zcut_gather_kernel: 16 400
// bytes (mi_gather.h).  The plan-shaped kernels: the block sums' and the scan's few words.
//
// BOUNDS.  sizes and entries READ a held row's first 8 bytes only where stored >= 8 (bytes 0 and 1 where stored >= 1 and 2), inside
// the span; a row the set lacks (address 0) is not looked at.  gather: mi_gather.h's paragraph -- a form H row's source is the
// block of zeroes, 65 536 bytes for entries of at most 65 536 (rule 8).  unwrap READS as mi_huff_wave.h states and WRITES
// [place, place + round16(inner length)) of the new blob only where the layout gave the row that room: the room handed to
// zh_unwrap_row is round16 of the bytes the entries pass laid out for a row it took the header's length from, else 0, and
// zh_unwrap_row refuses an inner length above its room (rule 8) before its first store.  decode WRITES [place, place +
// round16(length)) of the new blob -- the decoder checks len <= length - op before every copy, the raw copy's units and tail
// partition [0, length), zh_unwrap_row's room is round16(length) -- and, kind 1, [at, at + need) of the scratch, clamped against
// the scan's total in the kernel; it READS [src, src + round16(stored)) of a span and what it wrote itself.
#include "mi_gather.h"
#include "mi_huff_wave.h"
#include "mi_lz4_wave.h"
#include "mi_plan.h"
#include "mi_zset_local.h"
#include "mi_zentropy.h"

#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>

using namespace mi;

namespace mi {

constexpr u64 kCNone = ~0ull;
constexpr u64 kCScratchGrid = 64;                     // a kind-1 row's span of the scratch: no two rows share 64 bytes
constexpr u64 kCZeroBlock = kZhMaxChunk;              // what the gather reads for a form H row's place
enum : int { kCTotEntries = 0, kCTotBlob = 1, kCTotStored = 2, kCTotRaw = 3, kCTotChunk = 4, kCTotH = 5, kCTotBad = 6, kCTotDiffer = 7,
             kCTotNeed = 8, kCTotRule = 9, kCTotWords = 10 };

typedef const u8 __attribute__((address_space(1))) * c_global_bytes;

// a form H span's inner length as its header states it, if the header's length obeys rule 8 (zh_inner_need's test); else 0
static __device__ __forceinline__ u64 zcut_inner_len(const u8* src, u64 word) {
    if (zh_inner_need(src, word) == 0) return 0;
    return (u64)src[4] | ((u64)src[5] << 8) | ((u64)src[6] << 16) | ((u64)src[7] << 24);
}

// what a held row takes in the new blob (bytes), and in the plain cut's scratch (need); h: it is form H; raw: a raw entry there;
// placed (the unwrapped cut): a form H row that was laid out with its inner length, which the unwrap writes in place
struct ZcutSize { u64 bytes, need; bool h, raw, placed; };
static __device__ __forceinline__ ZcutSize zcut_size(u64 addr, u64 word, int plain) {
    const u64 len = word & 0xFFFFFFFFull, stored = word >> 32;
    const u8* p = (const u8*)(c_global_bytes)addr;
    const u32 form = zh_form(p, word);
    ZcutSize s = {plain ? len : stored, 0, form >= kZhOverLz4, plain || stored == len, false};
    if (!s.h) return s;
    const u64 inner = zcut_inner_len(p, word);
    if (plain) {
        if (form == kZhOverLz4 && inner) s.need = (inner + kCScratchGrid - 1) & ~(kCScratchGrid - 1);
    } else if (inner) {
        s.bytes = inner;
        s.raw = inner == len;
        s.placed = true;
    }
    return s;
}

// ---- sizes: per block of kPlanTile rows the first occurrences, their rounded-up bytes in the new blob and their scratch ----------
__global__ __launch_bounds__(kPlanBlock)
void zcut_sizes_kernel(const i64* __restrict__ dup_of, const u64* __restrict__ src, const u64* __restrict__ word, u64 n, int plain,
                       u64* __restrict__ block_cnt, u64* __restrict__ block_bytes, u64* __restrict__ block_need, u64* __restrict__ totals) {
    __shared__ u64 lds[7][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[7] = {};                                    // entries, rounded-up bytes, bytes, raw entries, chunk bytes, form H rows, scratch
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const u64 row = base + k;
        if (row >= n || dup_of[row] >= 0 || src[row] == 0) continue;         // (a row the set lacks: the host refuses the call)
        const u64 w = word[row];
        const ZcutSize s = zcut_size(src[row], w, plain);
        ++v[0];
        v[1] += round16(s.bytes);
        v[2] += s.bytes;
        v[3] += s.raw ? 1 : 0;
        v[4] += w & 0xFFFFFFFFull;
        v[5] += s.h ? 1 : 0;
        v[6] += s.need;
    }
    plan_block_sum<7>(v, lds);
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = v[0];
        block_bytes[blockIdx.x] = v[1];
        block_need[blockIdx.x] = v[6];
        if (v[2]) atomicAdd((unsigned long long*)&totals[kCTotStored], (unsigned long long)v[2]);
        if (v[3]) atomicAdd((unsigned long long*)&totals[kCTotRaw], (unsigned long long)v[3]);
        if (v[4]) atomicAdd((unsigned long long*)&totals[kCTotChunk], (unsigned long long)v[4]);
        if (v[5]) atomicAdd((unsigned long long*)&totals[kCTotH], (unsigned long long)v[5]);
    }
}

// single block: the exclusive scan of the three block arrays in place; the totals: entries, the blob's bytes, the scratch's
__global__ __launch_bounds__(kPlanBlock)
void zcut_offsets_kernel(u64* __restrict__ block_cnt, u64* __restrict__ block_bytes, u64* __restrict__ block_need, u64 n_blocks,
                         u64* __restrict__ totals) {
    plan_block_offsets<true>(block_cnt, block_bytes, n_blocks, &totals[kCTotEntries], &totals[kCTotBlob]);
    plan_block_offsets<false>(block_need, nullptr, n_blocks, &totals[kCTotNeed], nullptr);
}

// the new blob's entries in order of first occurrence: where the stored span lies and its word, where the entry goes and with how
// many bytes, e_aux (the unwrapped cut: the gather's source -- the span, or `zeroes` for a form H row that unwraps in place; the
// plain cut: the row's place in the scratch) and the 56-byte row (digest | offset | chunk_index = the request row | length and, the
// unwrapped cut, the stored size THERE)
__global__ __launch_bounds__(kPlanBlock)
void zcut_entries_kernel(const i64* __restrict__ dup_of, const u64* __restrict__ src, const u64* __restrict__ word,
                         const u8* __restrict__ digests, u64 n, int plain, u64 zeroes, const u64* __restrict__ block_cnt,
                         const u64* __restrict__ block_bytes, const u64* __restrict__ block_need, u64* __restrict__ e_span,
                         u64* __restrict__ e_word, u64* __restrict__ e_dst, u64* __restrict__ e_len, u64* __restrict__ e_aux,
                         u64* __restrict__ rows) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    ZcutSize sz[kPlanPer];
    u32 sel = 0;
    u64 cnt = 0, bytes = 0, need = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const bool s = base + k < n && dup_of[base + k] < 0 && src[base + k] != 0;
        sz[k] = s ? zcut_size(src[base + k], word[base + k], plain) : ZcutSize{0, 0, false, false, false};
        if (s) { sel |= 1u << k; ++cnt; bytes += round16(sz[k].bytes); need += sz[k].need; }
    }
    u64 at = plan_first(cnt, block_cnt);
    u64 dst = plan_first(bytes, block_bytes);
    u64 scr = plan_first(need, block_need);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (!(sel & (1u << k))) continue;
        const u64 row = base + k, w = word[row], len = w & 0xFFFFFFFFull;
        e_span[at] = src[row];
        e_word[at] = w;
        e_dst[at] = dst;
        e_len[at] = sz[k].bytes;
        e_aux[at] = plain ? scr : sz[k].placed ? zeroes : src[row];
        put_entry_row(rows + kEntryWords * at, digests + 32 * row, dst, row, plain ? len : len | (sz[k].bytes << 32));
        ++at;
        dst += round16(sz[k].bytes);
        scr += sz[k].need;
    }
}

// ---- the unwrapped cut: the tile gather, then one wave a form H row -----------------------------------------------------------------
__global__ __launch_bounds__(kGatherWG)
void zcut_gather_kernel(const u64* __restrict__ e_src, const u64* __restrict__ e_len, const u64* __restrict__ e_dst, u64 n_entries,
                        u64 blob_bytes, u8* __restrict__ blob) {
    gather_tile<true>(e_src, e_len, e_dst, n_entries, blob_bytes, blob);
}

// rule_out[k]: 0, 8..11, or 7 for a form H that unwraps and whose pad is not zero; *first_bad: the smallest such entry.  An entry
// that is not form H is not looked at beyond its first two bytes
__global__ __launch_bounds__(64)
void zcut_unwrap_kernel(const u64* __restrict__ e_span, const u64* __restrict__ e_word, const u64* __restrict__ e_dst,
                        const u64* __restrict__ e_len, const u64* __restrict__ e_aux, u64 zeroes, u64 n, u8* blob, u32* __restrict__ rule_out,
                        u64* __restrict__ first_bad) {
    __shared__ ZhUnwrapLds lds;
    const int lane = threadIdx.x;
    for (u64 k = blockIdx.x; k < n; k += gridDim.x) {
        const u64 w = e_word[k];
        const u8* p = (const u8*)(c_global_bytes)e_span[k];
        u32 rule = 0;
        if (zh_form(p, w) >= kZhOverLz4) {
            const u64 len = w & 0xFFFFFFFFull, stored = w >> 32;
            const u64 room = e_aux[k] == zeroes ? round16(e_len[k]) : 0;      // what the layout gave the row for its inner form
            u32 m = 0, kind = 0;
            rule = zh_unwrap_row(p, stored, len, blob + e_dst[k], room, &m, &kind, &lds, lane);
            const bool pad_set = stored + lane < round16(stored) && p[stored + lane] != 0;
            if (__ballot(pad_set) != 0 && rule == 0) rule = mi_host::kLz4PadNotZero;
        }
        if (lane == 0) {
            rule_out[k] = rule;
            if (rule) atomicMin((unsigned long long*)first_bad, (unsigned long long)k);
        }
        __syncthreads();                              // the next row clears the table
    }
}

// ---- the plain cut: one wave an entry, decoded (or copied) straight to its place in the new blob ------------------------------------
// rule_out[k]: 0 or the rule that refuses entry k, in mi::ZhUnwrap::merge's order (8..11, the inner block's 1..6, the pad's 7)
__global__ __launch_bounds__(64)
void zcut_decode_kernel(const u64* __restrict__ e_span, const u64* __restrict__ e_word, const u64* __restrict__ e_dst,
                        const u64* __restrict__ e_aux, u64 n, u8* blob, u8* scratch, u64 scratch_bytes, u32* __restrict__ rule_out,
                        u64* __restrict__ first_bad) {
    __shared__ ZhUnwrapLds lds;
    const int lane = threadIdx.x;
    for (u64 k = blockIdx.x; k < n; k += gridDim.x) {
        const u64 w = e_word[k], s_addr = e_span[k];
        const u8* src = (const u8*)(c_global_bytes)s_addr;
        const u64 len = w & 0xFFFFFFFFull, stored = w >> 32;
        u8* dst = blob + e_dst[k];                    // on the 16-byte grid, as the span is
        const u32 form = zh_form(src, w);
        u32 rule = 0, m = 0, kind = 0;
        if (form == kZhRaw) {                         // whole units, the tail by bytes: they partition [0, len)
            const u64 units = len >> 4;
            for (u64 u = lane; u < units; u += 64) *(u32x4*)(dst + (u << 4)) = load16_global(s_addr + (u << 4));
            if ((units << 4) + lane < len) dst[(units << 4) + lane] = src[(units << 4) + lane];
        } else if (form == kZhLz4) {
            rule = z_decode_block(src, stored, dst, len, lane);
        } else if (form == kZhOverRaw) {
            rule = zh_unwrap_row(src, stored, len, dst, round16(len), &m, &kind, &lds, lane);
        } else {
            const u64 need = (zcut_inner_len(src, w) + kCScratchGrid - 1) & ~(kCScratchGrid - 1);
            const u64 at = e_aux[k] <= scratch_bytes ? e_aux[k] : scratch_bytes;
            u8* inner = scratch + at;
            rule = zh_unwrap_row(src, stored, len, inner, need <= scratch_bytes - at ? need : 0, &m, &kind, &lds, lane);
            __syncthreads();                          // the wave's stores of the inner block have landed
            if (rule == 0) rule = z_decode_block(inner, m, dst, len, lane);
        }
        if (len + lane < round16(len)) dst[len + lane] = 0;
        const bool pad_set = stored + lane < round16(stored) && src[stored + lane] != 0;
        if (__ballot(pad_set) != 0 && rule == 0) rule = mi_host::kLz4PadNotZero;
        if (lane == 0) {
            rule_out[k] = rule;
            if (rule) atomicMin((unsigned long long*)first_bad, (unsigned long long)k);
        }
        __syncthreads();                              // the next row clears the table
    }
}

// MI_SUBPACK_VERIFY: the digests the device computed for the new blob's entries against the requested ones (the rows carry them)
__global__ __launch_bounds__(256)
void zcut_compare_kernel(const u8* __restrict__ got, const u64* __restrict__ rows, u64 n, u64* __restrict__ first_bad) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    digest_differs_mark(got, rows + kEntryWords * k, k, first_bad);
}

}  // namespace mi

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// what one call holds on the device until it returns
struct Cut {
    DevBuf dig, len32, src, word, len64, dup, scan, e_span, e_word, e_dst, e_len, e_aux, rows, rule, extra, got;
    Event ev[4];
    u64 nb = 0, n_sel = 0, blob_bytes = 0, stored_bytes = 0, n_raw = 0, chunk_bytes = 0, n_h = 0, need = 0;
    u64* block_cnt = nullptr;
    u64* block_bytes = nullptr;
    u64* block_need = nullptr;
    u64* totals = nullptr;                             // kCTot*
};

// The request's way up, the lookup, the first occurrences, sizes and scan; one synchronisation: the totals.  A row the lookup
// refuses: mi_zset_zpack's words under `who`, *first_bad.  Nothing is allocated for the result yet
int resolve_and_size(const mi_zset* set, mi_ctx* c, const char* who, const uint8_t* digests, const uint32_t* lengths, u64 n, bool plain, Cut* q,
                     uint64_t* first_bad) {
    hipStream_t s = c->stream;
    for (auto& e : q->ev) HIPCHK(c, e.create());
    q->nb = (n + kPlanTile - 1) / kPlanTile;
    u64 dd_cap = 1024;
    while (dd_cap < 2 * n) dd_cap <<= 1;
    HIPCHK(c, q->dig.ensure(n * 32));
    if (lengths) HIPCHK(c, q->len32.ensure(n * 4));
    HIPCHK(c, q->src.ensure(n * 8));
    HIPCHK(c, q->word.ensure(n * 8));
    HIPCHK(c, q->len64.ensure(n * 8));
    HIPCHK(c, q->dup.ensure(n * 8));
    HIPCHK(c, q->scan.ensure((3 * q->nb + kCTotWords) * 8));
    HIPCHK(c, c->dd_table.ensure(dd_cap * 8));
    HIPCHK(c, c->dd_slot.ensure(n * 4 + 16));
    HIPCHK(c, c->dd_nuniq.ensure(8));
    q->block_cnt = q->scan.as<u64>();
    q->block_bytes = q->block_cnt + q->nb;
    q->block_need = q->block_bytes + q->nb;
    q->totals = q->block_need + q->nb;
    HIPCHK(c, hipEventRecord(q->ev[0], s));
    HIPCHK(c, hipMemcpyAsync(q->dig.p, digests, n * 32, hipMemcpyHostToDevice, s));
    if (lengths) HIPCHK(c, hipMemcpyAsync(q->len32.p, lengths, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(q->totals, 0, kCTotWords * 8, s));
    HIPCHK(c, hipMemsetAsync(q->totals + kCTotBad, 0xFF, 2 * 8, s));
    HIPCHK(c, hipMemsetAsync(q->totals + kCTotRule, 0xFF, 8, s));
    int rc = mi_zset_lookup_enqueue(set, q->dig.as<u8>(), lengths ? q->len32.as<u32>() : (const u32*)nullptr, n, q->src.as<u64>(),
                                    q->word.as<u64>(), q->len64.as<u64>(), q->totals + kCTotBad);
    if (rc) return fail(c, rc, "%s: the lookup was not enqueued", who);
    launch_dedup_mark(q->dig.as<u8>(), n, nullptr, c->dd_table.as<u32>(), c->dd_slot.as<u32>(), dd_cap, q->dup.as<i64>(), c->dd_nuniq.as<u64>(),
                      true, s);
    hipLaunchKernelGGL(zcut_sizes_kernel, dim3((u32)q->nb), dim3(kPlanBlock), 0, s, q->dup.as<i64>(), q->src.as<u64>(), q->word.as<u64>(), n,
                       plain ? 1 : 0, q->block_cnt, q->block_bytes, q->block_need, q->totals);
    hipLaunchKernelGGL(zcut_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, s, q->block_cnt, q->block_bytes, q->block_need, q->nb, q->totals);
    HIPCHK(c, hipEventRecord(q->ev[1], s));
    u64 h[kCTotWords];
    HIPCHK(c, hipMemcpyAsync(h, q->totals, kCTotWords * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (h[kCTotBad] != kCNone) {
        const u64 bad = h[kCTotBad];
        if (first_bad) *first_bad = bad;
        u64 w = 0, at = 0;
        HIPCHK(c, hipMemcpy(&w, q->word.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&at, q->src.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
        const std::string dg = hex32(digests + 32 * bad);
        if (lengths && lengths[bad] == 0) return fail(c, MI_ERR_INVALID, "%s: row %llu has length 0 (digest %s)", who, (unsigned long long)bad, dg.c_str());
        if (!at)
            return fail(c, MI_ERR_INVALID, "%s: row %llu: the compressed pack set does not hold digest %s", who, (unsigned long long)bad, dg.c_str());
        return fail(c, MI_ERR_INVALID, "%s: row %llu: the compressed pack set holds digest %s with %u bytes, the request states %u", who,
                    (unsigned long long)bad, dg.c_str(), (u32)w, lengths ? lengths[bad] : 0u);
    }
    q->n_sel = h[kCTotEntries];
    q->blob_bytes = h[kCTotBlob];
    q->stored_bytes = h[kCTotStored];
    q->n_raw = h[kCTotRaw];
    q->chunk_bytes = h[kCTotChunk];
    q->n_h = h[kCTotH];
    q->need = h[kCTotNeed];
    if (q->n_sel == 0 || q->n_sel > n || q->blob_bytes < 16 * q->n_sel || q->stored_bytes > q->chunk_bytes || q->stored_bytes > q->blob_bytes ||
        q->n_h > q->n_sel || q->n_raw > q->n_sel || q->need > q->n_h * (u64)kZhMaxChunk)
        return fail(c, MI_ERR_HIP, "%s: the plan counted %llu entries (%llu entropy forms, %llu scratch bytes) with %llu stored bytes in a blob of "
                    "%llu for %llu chunk bytes", who, (unsigned long long)q->n_sel, (unsigned long long)q->n_h, (unsigned long long)q->need,
                    (unsigned long long)q->stored_bytes, (unsigned long long)q->blob_bytes, (unsigned long long)q->chunk_bytes);
    return MI_OK;
}

// the list's buffers, and the entries pass behind them (`zeroes`: the unwrapped cut's block, or 0)
int list_entries(mi_ctx* c, Cut* q, u64 n, bool plain, u64 zeroes) {
    HIPCHK(c, q->rows.ensure(q->n_sel * sizeof(mi_zpack_entry)));
    HIPCHK(c, q->e_span.ensure(q->n_sel * 8));
    HIPCHK(c, q->e_word.ensure(q->n_sel * 8));
    HIPCHK(c, q->e_dst.ensure(q->n_sel * 8));
    HIPCHK(c, q->e_len.ensure(q->n_sel * 8));
    HIPCHK(c, q->e_aux.ensure(q->n_sel * 8));
    HIPCHK(c, q->rule.ensure(q->n_sel * 4));
    HIPCHK(c, hipEventRecord(q->ev[2], c->stream));
    hipLaunchKernelGGL(zcut_entries_kernel, dim3((u32)q->nb), dim3(kPlanBlock), 0, c->stream, q->dup.as<i64>(), q->src.as<u64>(), q->word.as<u64>(),
                       q->dig.as<u8>(), n, plain ? 1 : 0, zeroes, q->block_cnt, q->block_bytes, q->block_need, q->e_span.as<u64>(),
                       q->e_word.as<u64>(), q->e_dst.as<u64>(), q->e_len.as<u64>(), q->e_aux.as<u64>(), q->rows.as<u64>());
    return MI_OK;
}

int does_not_fit(mi_ctx* c, const char* who, hipError_t e, const char* what, u64 bytes, u64 n) {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: %s of %llu bytes for %llu entropy-coded entries does not fit: the device "
                "has %llu bytes free (%s); nothing has changed", who, what, (unsigned long long)bytes, (unsigned long long)n, (unsigned long long)free_b,
                hipGetErrorString(e));
}

// a stored form that does not unwrap or decode: the request row, the digest and the rule
int refuse_form(mi_ctx* c, const char* who, const Cut& q, u64 entry, const uint8_t* digests, uint64_t* first_bad) {
    u64 row[kEntryWords] = {};
    u32 rule = 0;
    HIPCHK(c, hipMemcpy(row, q.rows.as<u64>() + kEntryWords * entry, sizeof row, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&rule, q.rule.as<u32>() + entry, 4, hipMemcpyDeviceToHost));
    if (first_bad) *first_bad = row[5];
    return fail(c, MI_ERR_INVALID, "%s: row %llu (entry %llu), digest %s: the stored form does not decode: %s", who, (unsigned long long)row[5],
                (unsigned long long)entry, hex32(digests + 32 * row[5]).c_str(), mi_host::zrule_name(rule));
}

}  // namespace

extern "C" {

int mi_zset_zpack_unwrapped(const mi_zset* set, const uint8_t* digests, const uint32_t* lengths, uint64_t n, uint32_t flags, mi_zpack** out,
                            uint64_t* first_bad) {
    if (first_bad) *first_bad = 0;
    if (out) *out = nullptr;
    if (!set || !out || (n && !digests)) return MI_ERR_INVALID;
    static const char* who = "mi_zset_zpack_unwrapped";
    mi_ctx* c = nullptr;
    int rc = mi_zset_ctx(set, who, &c);
    if (rc) return rc;
    if (flags & ~(uint32_t)MI_ZPACK_VERIFY) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu rows, a pack holds fewer than 2^32", who, (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    struct Owned { mi_zpack* z = nullptr; ~Owned() { if (z) mi_zpack_free(z); } } mine;   // (drains the ctx stream before the blob goes)
    void* d_blob = nullptr;
    mi_zpack_entry* h_rows = nullptr;
    if (n == 0) {                                          // a valid zpack of nothing
        rc = mi_zpack_alloc(c, who, 0, 0, &mine.z, &d_blob, &h_rows);
        if (rc) return rc;
        mi_zpack_set_result(mine.z, 0, 0, 0, (flags & MI_ZPACK_VERIFY) ? 1u : 0u, 0, 0, 0);
        *out = mine.z;
        mine.z = nullptr;
        return MI_OK;
    }
    hipStream_t s = c->stream;
    Cut q;
    StreamDrain drain{s};   // (goes first: buffers and events after it)
    rc = resolve_and_size(set, c, who, digests, lengths, n, false, &q, first_bad);
    if (rc) return rc;
    const u64 n_tiles = (q.blob_bytes + kGatherTile - 1) / kGatherTile;
    if (n_tiles >> 31) return fail(c, MI_ERR_INVALID, "%s: a blob of %llu bytes is more than one launch covers", who, (unsigned long long)q.blob_bytes);
    rc = mi_zpack_alloc(c, who, q.n_sel, q.blob_bytes, &mine.z, &d_blob, &h_rows);      // does not fit: MI_ERR_NOMEM, nothing has changed
    if (rc) return rc;
    if (q.n_h) {                                           // what the gather lays under the form H rows' places
        const hipError_t e = q.extra.alloc_exact(kCZeroBlock);
        if (e != hipSuccess) return does_not_fit(c, who, e, "the block of zeroes", kCZeroBlock, q.n_h);
        HIPCHK(c, hipMemsetAsync(q.extra.p, 0, kCZeroBlock, s));
    }
    const u64 zeroes = (u64)(size_t)q.extra.p;             // 0 where no form H was met: no entry's source is 0
    rc = list_entries(c, &q, n, false, zeroes);
    if (rc) return rc;
    hipLaunchKernelGGL(zcut_gather_kernel, dim3((u32)n_tiles), dim3(kGatherWG), 0, s, q.e_aux.as<u64>(), q.e_len.as<u64>(), q.e_dst.as<u64>(), q.n_sel,
                       q.blob_bytes, (u8*)d_blob);
    if (q.n_h)
        hipLaunchKernelGGL(zcut_unwrap_kernel, dim3((u32)std::min<u64>(q.n_sel, 65536)), dim3(64), 0, s, q.e_span.as<u64>(), q.e_word.as<u64>(),
                           q.e_dst.as<u64>(), q.e_len.as<u64>(), q.e_aux.as<u64>(), zeroes, q.n_sel, (u8*)d_blob, q.rule.as<u32>(),
                           q.totals + kCTotRule);
    HIPCHK(c, hipEventRecord(q.ev[3], s));
    u64 h_bad = kCNone;
    HIPCHK(c, hipMemcpyAsync(&h_bad, q.totals + kCTotRule, 8, hipMemcpyDeviceToHost, s));
    // the entries to the host with the same synchronisation: mi_zpack_entries only reads from then on
    HIPCHK(c, hipMemcpyAsync(h_rows, q.rows.p, q.n_sel * sizeof(mi_zpack_entry), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (h_bad != kCNone) return refuse_form(c, who, q, h_bad, digests, first_bad);
    float ms = 0, ms2 = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, q.ev[0], q.ev[1]));
    HIPCHK(c, hipEventElapsedTime(&ms2, q.ev[2], q.ev[3]));
    double ms_verify = 0, ms_decode = 0;
    if (flags & MI_ZPACK_VERIFY) {
        // as mi_zset_zpack verifies: the new blob decoded into a plain scratch and hashed there, held against the rows -- which
        // carry the REQUESTED digests
        const auto t0 = std::chrono::steady_clock::now();
        u64 bad = kCNone;
        u32 rule = 0;
        rc = zset_verify_stored(c, who, d_blob, h_rows, q.rows.as<u64>(), q.n_sel, &bad, &rule, &ms_decode);
        if (rc) return rc;
        ms_verify = ms_since(t0);
        if (bad != kCNone) {
            const mi_zpack_entry row = bad < q.n_sel ? h_rows[bad] : mi_zpack_entry{};
            if (first_bad) *first_bad = row.chunk_index;
            return fail(c, MI_ERR_IO, "%s: row %llu (entry %llu), %u bytes stored for %u at blob offset %llu: %s%s, requested digest %s -- the "
                        "set was fed a damaged blob without MI_ZSET_VERIFY", who, (unsigned long long)row.chunk_index, (unsigned long long)bad,
                        row.stored, row.length, (unsigned long long)row.offset,
                        rule ? "the stored form does not decode: " : "the decoded bytes do not hash to the requested digest",
                        rule ? mi_host::zrule_name(rule) : "", hex32(row.digest).c_str());
        }
    }
    mi_zpack_set_result(mine.z, q.stored_bytes, q.n_raw, q.chunk_bytes, (flags & MI_ZPACK_VERIFY) ? 1u : 0u, (double)ms + ms2, ms_verify, ms_decode);
    *out = mine.z;
    mine.z = nullptr;
    return MI_OK;
}

int mi_zset_pack(const mi_zset* set, const uint8_t* digests, const uint32_t* lengths, uint64_t n, uint32_t flags, mi_pack** out,
                 uint64_t* first_bad) {
    if (first_bad) *first_bad = 0;
    if (out) *out = nullptr;
    if (!set || !out || (n && !digests)) return MI_ERR_INVALID;
    static const char* who = "mi_zset_pack";
    mi_ctx* c = nullptr;
    int rc = mi_zset_ctx(set, who, &c);
    if (rc) return rc;
    if (flags & ~(uint32_t)MI_SUBPACK_VERIFY) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu rows, a pack holds fewer than 2^32", who, (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0) return mi_pack_empty(c, out);
    hipStream_t s = c->stream;
    struct Owned { mi_pack* p = nullptr; ~Owned() { if (p) mi_pack_free(p); } } mine;   // (drains the ctx stream before the blob goes)
    Cut q;
    StreamDrain drain{s};   // (goes first: buffers and events after it)
    rc = resolve_and_size(set, c, who, digests, lengths, n, true, &q, first_bad);
    if (rc) return rc;
    void* d_blob = nullptr;
    mi_pack_entry* h_rows = nullptr;
    rc = mi_pack_alloc(c, who, q.n_sel, q.blob_bytes, q.chunk_bytes, &mine.p, &d_blob, &h_rows);      // does not fit: MI_ERR_NOMEM, nothing has changed
    if (rc) return rc;
    if (q.need) {                                          // the inner blocks of the requested kind-1 rows, nothing else
        const hipError_t e = q.extra.alloc_exact(q.need);
        if (e != hipSuccess) return does_not_fit(c, who, e, "the scratch for the inner blocks", q.need, q.n_h);
    }
    if (flags & MI_SUBPACK_VERIFY) HIPCHK(c, q.got.ensure(q.n_sel * 32));
    rc = list_entries(c, &q, n, true, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(zcut_decode_kernel, dim3((u32)std::min<u64>(q.n_sel, 65536)), dim3(64), 0, s, q.e_span.as<u64>(), q.e_word.as<u64>(),
                       q.e_dst.as<u64>(), q.e_aux.as<u64>(), q.n_sel, (u8*)d_blob, q.extra.as<u8>(), q.need, q.rule.as<u32>(), q.totals + kCTotRule);
    HIPCHK(c, hipEventRecord(q.ev[3], s));
    u64 h_bad[2] = {kCNone, kCNone};
    HIPCHK(c, hipMemcpyAsync(&h_bad[0], q.totals + kCTotRule, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(h_rows, q.rows.p, q.n_sel * sizeof(mi_pack_entry), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (h_bad[0] != kCNone) return refuse_form(c, who, q, h_bad[0], digests, first_bad);
    float ms_decode = 0;
    HIPCHK(c, hipEventElapsedTime(&ms_decode, q.ev[2], q.ev[3]));
    double ms_verify = 0;
    if (flags & MI_SUBPACK_VERIFY) {
        // as mi_packset_pack verifies: the entries hashed where they lie (in blob order: e_dst, and e_len = the lengths)
        const auto t0 = std::chrono::steady_clock::now();
        const auto hash_items = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? launch_blake2s_items : launch_sha256_items;
        hash_items(kShaBlobs, (const u8*)d_blob, q.e_dst.as<u64>(), q.e_len.as<u64>(), nullptr, (u32)q.n_sel, nullptr, c->heads.as<u32>(), nullptr,
                   true, q.got.as<u8>(), c->sha, c->prop.multiProcessorCount, q.blob_bytes, s);
        hipLaunchKernelGGL(zcut_compare_kernel, dim3((u32)((q.n_sel + 255) / 256)), dim3(256), 0, s, q.got.as<u8>(), q.rows.as<u64>(), q.n_sel,
                           q.totals + kCTotDiffer);
        HIPCHK(c, hipMemcpyAsync(&h_bad[1], q.totals + kCTotDiffer, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipGetLastError());
        ms_verify = ms_since(t0);
        if (h_bad[1] != kCNone) {
            const u64 bad = h_bad[1];
            const mi_pack_entry row = bad < q.n_sel ? h_rows[bad] : mi_pack_entry{};
            u64 src = 0;
            (void)hipMemcpy(&src, q.e_span.as<u64>() + bad, 8, hipMemcpyDeviceToHost);
            if (first_bad) *first_bad = row.chunk_index;
            return fail(c, MI_ERR_IO, "%s: row %llu (entry %llu), %u bytes from source address %#llx at blob offset %llu: the decoded bytes do "
                        "not hash to the requested digest %s -- the set was fed a damaged blob without MI_ZSET_VERIFY", who,
                        (unsigned long long)row.chunk_index, (unsigned long long)bad, row.length, (unsigned long long)src,
                        (unsigned long long)row.offset, hex32(row.digest).c_str());
        }
    }
    mi_pack_set_result(mine.p, (flags & MI_SUBPACK_VERIFY) ? 1u : 0u, ms_decode, ms_verify);
    *out = mine.p;
    mine.p = nullptr;
    return MI_OK;
}

}  // extern "C"
