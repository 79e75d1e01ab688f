// mi_zentropy.hip -- the zpack ENTROPY STAGE (include/makisu_mi.h FORMAT): a chunk's stored form -- its LZ4 block,
// or its plain bytes where no block was kept -- wrapped in a byte-wise Huffman code of at most 11 bits over 32 interleaved streams
// ("form H", marked in band by a first byte of 0x00), where that is smaller by more than a sixteenth.  The coder's half
// (MI_ZPACK_ENTROPY in mi_pack_compress and mi_zset_recode), the readers' half (an unwrap pre-pass in front of the LZ4 kernels,
// which stay as they are) and the census (mi_zpack_count_forms, mi_zset_count_forms).  The wave's work is mi_huff_wave.h's.
//
//   encode     zh_encode_kernel, one wave a row, BEHIND the coder's kernel, which has left every row's stored size and its LZ4
//              block in the row's worst-case scratch span: the form under it is that block or, for a raw row, the chunk in the
//              pack.  A kept form H goes into a SECOND scratch at the same span (h < the form under it <= the span), the row's
//              stored size is switched and its source recorded; the layout's scan and placing pass run as ever over the new sizes,
//              zh_sources_kernel points the gather at the second scratch for those rows: three kinds of source;
//   classify   zh_classify_kernel, mi_plan.h's block shape: a row's form from its word and its first bytes, the counts and
//              stored bytes per form into the totals, the rounded-up inner lengths of the form H rows per block;
//   unwrap     only if a form H row exists: the scan (zh_offsets_kernel), every row's place in one scratch (zh_place_kernel),
//              zh_unwrap_kernel one wave a row -- header, table, streams (mi_huff_wave.h), the pad behind the span -- and the
//              row arrays rewritten for the LZ4 kernel that follows: a kind 1 row points at its inner block, a kind 2 row is raw;
//   recode     mi_zrecode.hip's rounds with the stage: zh_rules_merge_kernel (the unwrap's rules into a round's), zh_recode_encode_kernel
//              and zh_recode_place_kernel (form H over a round's candidates, built in a second scratch; copied over the candidate),
//              zh_rep_rows_kernel and
//              zh_redecode_kernel (VERIFY's recheck over unwrapped rows, a raw row copied).
//
// LDS.  zh_unwrap_kernel: 4 928 bytes, the 2 048-entry table (4 KiB) plus 832 bytes (mi_huff_wave.h: code lengths, codes,
// counts per length).  zh_encode_kernel: 5 376 bytes.  The plan-shaped kernels: the block sums' and the scan's few words.
//
// BOUNDS.  classify and place READ a row's first 8 bytes only where stored >= 8 (byte 0 and 1 where stored >= 1 and 2: the
// structural check of every add gives stored >= 1), inside the span.  unwrap: mi_huff_wave.h's paragraph; the room it is given is
// total - place >= round16(inner length), checked in the kernel against the scan's total, so a header that changed between the
// two launches could not make it write outside the scratch; it rewrites row k's two words and rule_out[k], k < n.  encode READS
// the form under it below its stored size and WRITES scratch2 below h < that size, inside the row's span; rows[k]'s length word
// and d_hsrc[k], k < n.  sources WRITES e_src[k], k < n.  recode_encode READS the candidate (r_cand[k] bytes) or the row's plain bytes
// (length bytes) in the row's span of the round's scratch or, raw, in its blob, WRITES scratch2 below h < the candidate's size at
// the row's span (the same offsets in a buffer of the same size); recode_place copies round16(h) bytes, whole units, over the candidate:
// below z_worst_span(length), which the row's span holds behind its plain bytes.  redecode WRITES [span, span + length) of the
// row's span, as zrecode_redecode_kernel does; rules_merge and rep_rows write row k's word, k inside the round or the list.
#include "mi_zentropy.h"
#include "mi_huff_wave.h"
#include "mi_plan.h"
#include "mi_local.h"

#include <string.h>

#include <algorithm>

using namespace mi;

namespace mi {

constexpr u64 kHNone = ~0ull;
enum : int { kHTotN = 0, kHTotStored = 4, kHTotInner = 8, kHTotBad = 9, kHTotWords = 16 };

typedef const u8 __attribute__((address_space(1))) * h_global_bytes;

static __device__ __forceinline__ const u8* zh_span(u64 base, const u64* __restrict__ src, u32 stride, u64 k) {
    return (const u8*)(h_global_bytes)(base + src[(u64)stride * k]);
}

// ---- classify -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlanBlock)
void zh_classify_kernel(u64 base, const u64* __restrict__ src, u32 src_stride, const u64* __restrict__ word, u32 word_stride, u64 n,
                        const u64* __restrict__ tags, u64* __restrict__ block_need, u64* __restrict__ totals) {
    __shared__ u64 lds[9][kPlanBlock / 64];
    const u64 first = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[9] = {};                                    // rows per form, stored bytes per form, the form H rows' inner need
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (first + k >= n || (tags && tags[first + k] == 0ull)) continue;     // (a set's table: the occupied slots only)
        const u64 w = word[(u64)word_stride * (first + k)];
        const u8* p = zh_span(base, src, src_stride, first + k);
        const u32 form = zh_form(p, w);
#pragma unroll
        for (u32 f = 0; f < 4; ++f) {
            v[f] += form == f ? 1 : 0;
            v[4 + f] += form == f ? w >> 32 : 0;
        }
        if (form >= kZhOverLz4) v[8] += zh_inner_need(p, w);
    }
    plan_block_sum<9>(v, lds);
    if (threadIdx.x == 0) {
        if (block_need) block_need[blockIdx.x] = v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (v[q]) atomicAdd((unsigned long long*)&totals[kHTotN + q], (unsigned long long)v[q]);
    }
}

__global__ __launch_bounds__(kPlanBlock)
void zh_offsets_kernel(u64* __restrict__ block_need, u64 n_blocks, u64* __restrict__ totals) {
    plan_block_offsets<false>(block_need, nullptr, n_blocks, &totals[kHTotInner], nullptr);
}

// place[k]: where row k's inner form goes in the scratch (every row has one; only a form H row's is used)
__global__ __launch_bounds__(kPlanBlock)
void zh_place_kernel(u64 base, const u64* __restrict__ src, u32 src_stride, const u64* __restrict__ word, u32 word_stride, u64 n,
                     const u64* __restrict__ block_need, u64* __restrict__ place) {
    const u64 first = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 need[kPlanPer];
    u64 bytes = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        need[k] = 0;
        if (first + k < n) {
            const u64 w = word[(u64)word_stride * (first + k)];
            const u8* p = zh_span(base, src, src_stride, first + k);
            if (zh_form(p, w) >= kZhOverLz4) need[k] = zh_inner_need(p, w);
        }
        bytes += need[k];
    }
    u64 at = plan_first(bytes, block_need);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (first + k < n) place[first + k] = at;
        at += need[k];
    }
}

// ---- unwrap: one wave a row (the workgroup IS the wave), grid-stride ------------------------------------------------------------
// rule_out[k]: 0, 8..11, or 7 for a form H that unwraps and whose pad is not zero; totals[kHTotBad]: the smallest such row
__global__ __launch_bounds__(64)
void zh_unwrap_kernel(u64 base, u64* src, u32 src_stride, u64* word, u32 word_stride, u64 n, const u64* __restrict__ place, u8* inner, u64 total,
                      u32* __restrict__ rule_out, u64* __restrict__ totals) {
    __shared__ ZhUnwrapLds lds;
    const int lane = threadIdx.x;
    for (u64 k = blockIdx.x; k < n; k += gridDim.x) {
        const u64 w = word[(u64)word_stride * k];
        const u8* p = zh_span(base, src, src_stride, k);
        u32 rule = 0;
        if (zh_form(p, w) >= kZhOverLz4) {
            const u64 len = w & 0xFFFFFFFFull, stored = w >> 32;
            const u64 at = place[k] <= total ? place[k] : total;
            u32 m = 0, kind = 0;
            rule = zh_unwrap_row(p, stored, len, inner + at, total - at, &m, &kind, &lds, lane);
            const bool pad_set = stored + lane < round16(stored) && p[stored + lane] != 0;
            const bool pad_bad = __ballot(pad_set) != 0;
            __syncthreads();                          // every lane has read the row's words
            if (rule == 0 && lane == 0) {
                src[(u64)src_stride * k] = (u64)(size_t)(inner + at) - base;          // (modulo 2^64: the reader adds its base again)
                word[(u64)word_stride * k] = len | ((kind == mi_host::kHuffKindRaw ? len : (u64)m) << 32);
            }
            if (rule == 0 && pad_bad) rule = mi_host::kLz4PadNotZero;
        }
        if (lane == 0) {
            rule_out[k] = rule;
            if (rule) atomicMin((unsigned long long*)&totals[kHTotBad], (unsigned long long)k);
        }
        __syncthreads();
    }
}

// ---- encode: one wave a row behind the coder's kernel -------------------------------------------------------------------------------
__global__ __launch_bounds__(64)
void zh_encode_kernel(const u8* __restrict__ blob, u64* __restrict__ rows, const u64* __restrict__ w_off, const u8* __restrict__ scratch,
                      u8* __restrict__ scratch2, u64* __restrict__ h_src, u64 n) {
    __shared__ ZhEncodeLds lds;
    const int lane = threadIdx.x;
    for (u64 k = blockIdx.x; k < n; k += gridDim.x) {
        const u64* r = rows + kEntryWords * k;
        const u32 len = (u32)r[6], stored = (u32)(r[6] >> 32);
        u32 h = 0;
        if (len <= kZhMaxChunk && stored != 0 && stored <= len) {
            const bool coded = stored < len;
            h = zh_encode_row(coded ? scratch + w_off[k] : blob + r[4], stored, coded ? mi_host::kHuffKindLz4 : mi_host::kHuffKindRaw,
                              scratch2 + w_off[k], &lds, lane);
        }
        __syncthreads();                              // every lane has read the row
        if (lane == 0) {
            h_src[k] = h ? (u64)(size_t)(scratch2 + w_off[k]) : 0;
            if (h) rows[kEntryWords * k + 6] = (u64)len | ((u64)h << 32);
        }
    }
}

__global__ __launch_bounds__(256)
void zh_sources_kernel(const u64* __restrict__ h_src, u64* __restrict__ e_src, u64 n) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k < n && h_src[k]) e_src[k] = h_src[k];
}

// ---- mi_zset_recode with the stage (mi_zrecode.hip runs these between its own kernels) -----------------------------------------------
// the unwrap's rules into the recode's per-row rules for the round [r0, r0 + n): 8..11 always (the LZ4 decoder refused the row's
// 0x00 token with a rule of its own), the pad's 7 where the inner form decoded
__global__ __launch_bounds__(256)
void zh_rules_merge_kernel(const u32* __restrict__ h_rule, u32* __restrict__ r_rule, u64 r0, u64 n) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 h = h_rule[r0 + i];
    if (h >= mi_host::kHuffHeader || (h == mi_host::kLz4PadNotZero && r_rule[r0 + i] == 0)) r_rule[r0 + i] = h;
}

// behind the recode's encode kernel, one wave a row of the round: the LZ4 candidate of r_cand[k] bytes lies in the row's span of
// `scratch` behind its plain bytes (u_word's layout), or the row is raw and its plain bytes are the form under it.  A kept form H
// is built in the row's span of `scratch2`, r_cand[k] becomes its size with kZhKept set: the next launch copies it over the candidate
constexpr u32 kZhKept = 0x80000000u;
__global__ __launch_bounds__(64)
void zh_recode_encode_kernel(const u64* __restrict__ u_src, const u64* __restrict__ u_word, const u64* __restrict__ r_off,
                             const u32* __restrict__ r_rule, u64 n, const u8* __restrict__ scratch, u8* __restrict__ scratch2,
                             u32* __restrict__ r_cand) {
    // (the row arrays begin at the round's first row; scratch and scratch2 are the buffers MINUS the round's base offset, so that
    // r_off[k] indexes them as it is: fewer words for the wave to carry through the coder)
    __shared__ ZhEncodeLds lds;
    const int lane = threadIdx.x;
    for (u64 k = blockIdx.x; k < n; k += gridDim.x) {
        const u32 len = (u32)u_word[k], stored = (u32)(u_word[k] >> 32), cand = r_cand[k];
        const u64 plain_bytes = stored < len ? round16((u64)len) : 0;             // where the coder left its candidate (zrecode_plain_bytes)
        u32 h = 0;
        if (r_rule[k] == 0 && len <= kZhMaxChunk && cand != 0 && cand <= len) {
            const bool coded = cand < len;
            const u64 under = coded ? (u64)(size_t)scratch + r_off[k] + plain_bytes : stored < len ? (u64)(size_t)scratch + r_off[k] : u_src[k];
            h = zh_encode_row((const u8*)(h_global_bytes)under, cand, coded ? mi_host::kHuffKindLz4 : mi_host::kHuffKindRaw, scratch2 + r_off[k], &lds, lane);
        }
        __syncthreads();                              // every lane has read the row
        if (h && lane == 0) r_cand[k] = h | kZhKept;  // (zh_recode_place_kernel takes the mark off again)
    }
}

// ... and the kept forms copied over the candidates, one wave a row: whole units, both places are on the 16-byte grid
__global__ __launch_bounds__(64)
void zh_recode_place_kernel(const u64* __restrict__ u_word, const u64* __restrict__ r_off, u64 n, u8* __restrict__ scratch,
                            const u8* __restrict__ scratch2, u32* __restrict__ r_cand) {
    const int lane = threadIdx.x;
    for (u64 k = blockIdx.x; k < n; k += gridDim.x) {
        const u32 c = r_cand[k];
        __syncthreads();                              // every lane has read the mark
        if (!(c & kZhKept)) continue;
        const u32 h = c & ~kZhKept, len = (u32)u_word[k], stored = (u32)(u_word[k] >> 32);
        u8* at = scratch + r_off[k] + (stored < len ? round16((u64)len) : 0);
        const u8* out = scratch2 + r_off[k];
        for (u32 u = (u32)lane * 16; u < h; u += 64 * 16) *(u32x4*)(at + u) = *(const u32x4*)(out + u);
        if (lane == 0) r_cand[k] = h;
    }
}

// the recheck's rows: entry i of the list of replaced rows as (address in the new blob, length | new size << 32)
__global__ __launch_bounds__(256)
void zh_rep_rows_kernel(const u64* __restrict__ rep, u64 n, const u64* __restrict__ r_word, const u32* __restrict__ r_new,
                        const u64* __restrict__ r_addr, u64* __restrict__ v_src, u64* __restrict__ v_word) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = rep[i];
    v_src[i] = r_addr[k];
    v_word[i] = (r_word[k] & 0xFFFFFFFFull) | ((u64)r_new[k] << 32);
}

// the recheck's decode for a call with the stage, one wave an entry of rep[0, n): the unwrapped row (v_src, v_word: entry i at i)
// into the row's span of the scratch -- a raw row (form H over the plain bytes) is copied, a coded one decoded
__global__ __launch_bounds__(64)
void zh_redecode_kernel(const u64* __restrict__ rep, u64 n, const u64* __restrict__ v_src, const u64* __restrict__ v_word,
                        const u64* __restrict__ r_off, u64 base_off, u8* scratch, u64* __restrict__ v_off, u64* __restrict__ v_len,
                        u64* __restrict__ n_bad, u64* __restrict__ first_bad) {
    const int lane = threadIdx.x;
    for (u64 i = blockIdx.x; i < n; i += gridDim.x) {
        const u64 k = rep[i];
        const u8* src = (const u8*)(h_global_bytes)v_src[i];
        const u64 len = v_word[i] & 0xFFFFFFFFull, stored = v_word[i] >> 32;
        u8* dst = scratch + (r_off[k] - base_off);
        u32 rule = 0;
        if (stored == len) {
            for (u64 j = lane; j < len; j += 64) dst[j] = src[j];
        } else {
            rule = z_decode_block(src, stored, dst, len, lane);
        }
        const bool pad_set = stored + lane < round16(stored) && src[stored + lane] != 0;
        if (__ballot(pad_set) != 0 && rule == 0) rule = mi_host::kLz4PadNotZero;
        if (lane == 0) {
            v_off[i] = (u64)(size_t)dst;
            v_len[i] = len;
            if (rule) {
                atomicAdd((unsigned long long*)n_bad, 1ull);
                atomicMin((unsigned long long*)first_bad, (unsigned long long)k);
            }
        }
        __syncthreads();
    }
}

namespace {

int classify(mi_ctx* c, u64 base, const u64* d_src, u32 src_stride, const u64* d_word, u32 word_stride, u64 n, const u64* d_tags, DevBuf* cells,
             u64* block_need, u64* h /*kHTotWords*/) {
    hipStream_t st = c->stream;
    const u64 nb = (n + kPlanTile - 1) / kPlanTile;
    u64* tot = cells->as<u64>();
    HIPCHK(c, hipMemsetAsync(tot, 0, kHTotWords * 8, st));
    HIPCHK(c, hipMemsetAsync(tot + kHTotBad, 0xFF, 8, st));
    hipLaunchKernelGGL(zh_classify_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, st, base, d_src, src_stride, d_word, word_stride, n, d_tags, block_need,
                       tot);
    HIPCHK(c, hipMemcpyAsync(h, tot, kHTotWords * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return MI_OK;
}

void forms_of(const u64* h, mi_zforms* out) {
    for (int f = 0; f < 4; ++f) {
        out->n[f] = h[kHTotN + f];
        out->stored[f] = h[kHTotStored + f];
    }
}

}  // namespace

int zh_count_forms(mi_ctx* c, u64 base, const u64* d_src, u32 src_stride, const u64* d_word, u32 word_stride, u64 n, const u64* d_tags,
                   mi_zforms* out) {
    memset(out, 0, sizeof *out);
    if (!n) return MI_OK;
    DevBuf cells;
    StreamDrain drain{c->stream};
    HIPCHK(c, cells.ensure(kHTotWords * 8));
    u64 h[kHTotWords];
    const int rc = classify(c, base, d_src, src_stride, d_word, word_stride, n, d_tags, &cells, nullptr, h);
    if (rc) return rc;
    forms_of(h, out);
    return MI_OK;
}

int ZhUnwrap::run(mi_ctx* c, const char* who, u64 base, u64* d_src, u32 src_stride, u64* d_word, u32 word_stride, u64 n) {
    hipStream_t st = c->stream;
    const u64 nb = (n + kPlanTile - 1) / kPlanTile;
    n_h = 0;
    n_rows = 0;
    bad = kHNone;
    rule = 0;
    if (!n) return MI_OK;
    HIPCHK(c, cells.ensure((kHTotWords + nb) * 8));
    u64* tot = cells.as<u64>();
    u64* block_need = tot + kHTotWords;
    u64 h[kHTotWords];
    int rc = classify(c, base, d_src, src_stride, d_word, word_stride, n, nullptr, &cells, block_need, h);
    if (rc) return rc;
    forms_of(h, &forms);
    n_h = forms.n[kZhOverLz4] + forms.n[kZhOverRaw];
    if (n_h == 0) return MI_OK;                        // the stage's whole cost where no form H is: the launch above
    if (n_h > n) return fail(c, MI_ERR_HIP, "%s: the classify pass counted %llu entropy forms among %llu rows", who, (unsigned long long)n_h, (unsigned long long)n);
    hipLaunchKernelGGL(zh_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, st, block_need, nb, tot);
    HIPCHK(c, hipMemcpyAsync(h, tot, kHTotWords * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    inner_bytes = h[kHTotInner];
    if (inner_bytes > n_h * (u64)kZhMaxChunk)
        return fail(c, MI_ERR_HIP, "%s: the scan counted %llu inner bytes for %llu entropy forms", who, (unsigned long long)inner_bytes, (unsigned long long)n_h);
    const hipError_t e = inner.alloc_exact(inner_bytes);
    if (e != hipSuccess) {
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        (void)hipGetLastError();
        return fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: the scratch of %llu bytes for the inner forms of %llu entropy-coded "
                    "entries does not fit: the device has %llu bytes free (%s); nothing has changed", who, (unsigned long long)inner_bytes,
                    (unsigned long long)n_h, (unsigned long long)free_b, hipGetErrorString(e));
    }
    HIPCHK(c, aux.ensure(n * 8 + n * 4));
    n_rows = n;
    u64* place = aux.as<u64>();
    u32* rules = (u32*)(place + n);
    hipLaunchKernelGGL(zh_place_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, st, base, d_src, src_stride, d_word, word_stride, n, block_need, place);
    hipLaunchKernelGGL(zh_unwrap_kernel, dim3((u32)std::min<u64>(n, 65536)), dim3(64), 0, st, base, d_src, src_stride, d_word, word_stride, n, place,
                       inner.as<u8>(), inner_bytes, rules, tot);
    HIPCHK(c, hipMemcpyAsync(h, tot, kHTotWords * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (h[kHTotBad] != kHNone) {
        bad = h[kHTotBad];
        if (bad < n) HIPCHK(c, hipMemcpy(&rule, rules + bad, 4, hipMemcpyDeviceToHost));
    }
    return MI_OK;
}

void zh_encode_enqueue(mi_ctx* c, const void* d_base, u64* d_rows, const u64* d_woff, const void* d_scratch, void* d_scratch2, u64* d_hsrc, u64 n,
                       u32 waves) {
    hipLaunchKernelGGL(zh_encode_kernel, dim3(waves), dim3(64), 0, c->stream, (const u8*)d_base, d_rows, d_woff, (const u8*)d_scratch, (u8*)d_scratch2,
                       d_hsrc, n);
}

void zh_rules_merge_enqueue(mi_ctx* c, const u32* h_rule, u32* r_rule, u64 r0, u64 n) {
    hipLaunchKernelGGL(zh_rules_merge_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, c->stream, h_rule, r_rule, r0, n);
}

void zh_recode_encode_enqueue(mi_ctx* c, const u64* u_src, const u64* u_word, const u64* r_off, const u32* r_rule, u64 r0, u64 n, u64 base_off,
                              void* scratch, void* scratch2, u32* r_cand, u32 waves) {
    hipLaunchKernelGGL(zh_recode_encode_kernel, dim3(waves), dim3(64), 0, c->stream, u_src + r0, u_word + r0, r_off + r0, r_rule + r0, n,
                       (const u8*)scratch - base_off, (u8*)scratch2 - base_off, r_cand + r0);
    hipLaunchKernelGGL(zh_recode_place_kernel, dim3(waves), dim3(64), 0, c->stream, u_word + r0, r_off + r0, n, (u8*)scratch - base_off,
                       (const u8*)scratch2 - base_off, r_cand + r0);
}

void zh_rep_rows_enqueue(mi_ctx* c, const u64* rep, u64 n, const u64* r_word, const u32* r_new, const u64* r_addr, u64* v_src, u64* v_word) {
    hipLaunchKernelGGL(zh_rep_rows_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, c->stream, rep, n, r_word, r_new, r_addr, v_src, v_word);
}

void zh_redecode_enqueue(mi_ctx* c, const u64* rep, u64 n, const u64* v_src, const u64* v_word, const u64* r_off, u64 base_off, void* scratch,
                         u64* v_off, u64* v_len, u64* n_bad, u64* first_bad, u32 waves) {
    hipLaunchKernelGGL(zh_redecode_kernel, dim3(waves), dim3(64), 0, c->stream, rep, n, v_src, v_word, r_off, base_off, (u8*)scratch, v_off, v_len,
                       n_bad, first_bad);
}

void zh_sources_enqueue(mi_ctx* c, const u64* d_hsrc, u64* e_src, u64 n) {
    hipLaunchKernelGGL(zh_sources_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, c->stream, d_hsrc, e_src, n);
}

}  // namespace mi
