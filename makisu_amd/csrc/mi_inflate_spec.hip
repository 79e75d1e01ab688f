// mi_inflate_spec.hip -- a gzip member NOBODY INDEXED inflated on the device (host_inflate_spec.h: the pieces, the chain,
// the spans).  The span table and the window area of the indexed inflate are made here, on the device, from the member
// alone -- the technique of pugz and rapidgzip:
//   inflate_find_kernel          one wave a PIECE of the stream: the smallest bit of the piece at which a non-final dynamic block
//                                header parses (mi_inflate_wave.h's own header and table build decide), the piece's CANDIDATE
//   inflate_speculate_kernel     one wave a candidate: the decode from that bit WITHOUT the 32 KiB in front of it, nothing delivered --
//                                the output goes to a ring of 32 768 u16 entries, a literal as it is, a byte the span cannot know as a
//                                MARKER 0x8000 + k: "the byte 32 768 - k positions before my first byte".  It ends at the first block
//                                header that begins at its piece's candidate, and leaves a row
//   (host)                       the chain from candidate 0 along the rows' ends; the live spans, their output offsets by prefix sum
//   inflate_spec_windows_kernel  one workgroup, the live spans in chain order: span i's window from span i - 1's ring, the markers
//                                resolved through span i - 1's window -- straight into the inflater's window area
// and from there mi_inflater_run / _run_device are the indexed inflate's code: inflate_span_kernel holds every span to its end, the
// CRC-32 and ISIZE decide.  The speculation is only ever A HINT: a bug in it can cost time, never bytes.
//
// THE SPECULATIVE DECODE is mi_inflate_wave.h's body in a third form, written out here because its output stage shares nothing with
// the other two (u16 entries, a ring in global memory, no distance rule): the bit reader, the header, the tables and the symbol
// decode are that header's own functions, and its BOUNDS hold word for word -- input only through inf_load_word, LDS indexes as
// there.  Dead candidates decode garbage: that is this code's normal input.  OUTPUT: every global store's index is masked to the
// ring (p & 32 767) of the wave's own candidate.  THE RING INVARIANT: a match's source position p lies in [op - 32 768, op); what
// is flushed are the positions below `flushed` <= op, so the entry p & 32 767 could have been overwritten only by position
// p + 32 768 >= op >= flushed, which no flush has written yet -- a source at distance <= 32 768 is never an entry a flush has
// already overwritten.
#include "mi_internal.h"
#include "mi_inflate_local.h"
#include "mi_inflate_wave.h"
#include "host_inflate_index.h"
#include "host_inflate_spec.h"

#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

namespace mi {

using mi_host::InflateRow;
using mi_host::kSpecNone;
using mi_host::kSpecRing;

struct InfSpecLds {
    InfLds t;                                           // the tables (its byte ring is not used)
    u16 ring[kInfRing];                                 // the staging of entries: kInfRing's rules (a token is placed with 258 of room)
};

static __device__ __forceinline__ u64 inf_uni64(u64 v) { return (u64)inf_uni((u32)v) | (u64)inf_uni((u32)(v >> 32)) << 32; }

// ---- the finder -----------------------------------------------------------------------------------------------------------------
// the 128 bits of the member from word `word` on -> what a dynamic header at bit `sh` of them must satisfy before anything else:
// BFINAL 0, BTYPE 2, HLIT <= 29, HDIST <= 29, and the code-length code complete (its Kraft sum, in 128ths, is 128)
static __device__ __forceinline__ bool inf_find_prefilter(u64 a, u64 b, u32 sh) {
    const u64 lo = sh ? (a >> sh) | (b << (64 - sh)) : a, hi = b >> sh;     // bits [0, 64) and [64, 128 - sh) from the position
    if ((lo & 7) != 4 || ((lo >> 3) & 31) > 29 || ((lo >> 8) & 31) > 29) return false;
    const u32 hclen = (u32)((lo >> 13) & 15) + 4;
    const u64 cl = (lo >> 17) | (hi << 47);             // the (up to) 19 lengths, three bits each: 57 bits
    u32 kraft = 0;
    for (u32 i = 0; i < 19; ++i) {
        const u32 v = (u32)(cl >> (3 * i)) & 7u;
        if (i < hclen && v) kraft += 128u >> v;
    }
    return kraft == 128;
}

// cand[k] for every piece k: piece 0's is 8 hdr; otherwise the smallest bit p in [8 (hdr + k piece), 8 (hdr + (k + 1) piece)) below
// 8 (n - 8) at which BFINAL 0, BTYPE 2 stand, inf_dynamic_header gives no rule and inf_tables gives none -- or ~0.  64 positions a
// step: each lane prefilters its own, the wave runs the header and the tables on the survivors in ascending order
__global__ __launch_bounds__(64)
void inflate_find_kernel(const u8* __restrict__ gz, u64 n, u64 hdr, u64 piece, u64 n_pieces, u64* __restrict__ cand) {
    __shared__ InfLds lds;
    const u64 k = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (k >= n_pieces) return;
    if (k == 0) { if (lane == 0) cand[0] = 8 * hdr; return; }
    const u64 nbits = 8 * n, stream_end = 8 * (n - 8), first = 8 * (hdr + k * piece);
    const u64 last = first + 8 * piece < stream_end ? first + 8 * piece : stream_end;
    u64 found = kSpecNone;
    for (u64 base = first; base < last && found == kSpecNone; base += 64) {
        const u64 p = base + (u64)lane, word = p / 32;
        const u64 a = (u64)inf_load_word(gz, n, word) | (u64)inf_load_word(gz, n, word + 1) << 32;
        const u64 b = (u64)inf_load_word(gz, n, word + 2) | (u64)inf_load_word(gz, n, word + 3) << 32;
        u64 todo = __ballot(p < last && inf_find_prefilter(a, b, (u32)p & 31u));
        while (todo) {
            const u64 q = base + (u64)(__ffsll((unsigned long long)todo) - 1);
            todo &= todo - 1;
            InfBits bits;
            bits.gz = gz;
            bits.n = n;
            inf_seek(&bits, q / 8, lane);
            inf_drop(&bits, (u32)q & 7u);                       // (the seek left at least 8 bits)
            inf_need(&bits, lane);
            inf_drop(&bits, 3);                                 // BFINAL 0, BTYPE 2: the prefilter's
            u32 hlit = 0, hdist = 0;
            u32 rule = inf_dynamic_header(&bits, &lds, nbits, lane, &hlit, &hdist);
            if (!rule) rule = inf_tables(&lds, hlit, hdist, lane);
            if (!rule) { found = q; break; }
        }
    }
    if (lane == 0) cand[k] = found;
}

// ---- the speculative pass -------------------------------------------------------------------------------------------------------
struct SpecOut {
    u16* ring;            // the candidate's 32 768 entries in global memory: position p at entry p & 32 767
    u32 fill, ring_seen;  // the staging holds the positions [op - fill, op); below ring_seen it is visible to every lane
    u64 symbols, cap;     // literals and matches decoded, and how many there may be
};

static __device__ __forceinline__ void spec_flush(SpecOut* o, InfSpecLds* lds, u64 op, int lane) {
    __syncthreads();
#pragma nounroll
    for (u32 i = lane; i < o->fill; i += 64) o->ring[(op - o->fill + i) & (kSpecRing - 1)] = lds->ring[i];
    __syncthreads();
    o->fill = 0;
    o->ring_seen = 0;
}

// the symbols of one fixed or dynamic block whose tables stand; 0 or the rule.  inf_block's loop with entries for bytes: there is no
// distance rule (what reaches before the member's first byte is the write pass's rule 10) and there is a cap on the symbols
static __device__ __forceinline__ u32 spec_block(InfBits* b, InfSpecLds* lds, SpecOut* o, u64* op_io, u64 limit, u64 nbits, int lane) {
    u64 op = *op_io;
    u32 rule = 0;
    for (;;) {
        if (o->fill > kInfRing - 258) spec_flush(o, lds, op, lane);
        inf_need(b, lane);
        const u32 s = inf_symbol(b, lds->t.lit_tab, kInfLitBits, lds->t.lit_sym, &lds->t.lit);
        if (s == kInfNoSymbol) { rule = mi_host::kInfSymbol; break; }
        if (s < 256) {
            if (inf_bit(b) > nbits) { rule = mi_host::kInfInputEnds; break; }
            if (op + 1 > limit) { rule = mi_host::kInfWindow; break; }
            if (o->symbols + 1 > o->cap) { rule = mi_host::kInfSymbolCap; break; }
            if (lane == 0) lds->ring[o->fill] = (u16)s;
            ++o->fill;
            ++o->symbols;
            ++op;
            continue;
        }
        if (s == 256) {
            if (inf_bit(b) > nbits) rule = mi_host::kInfInputEnds;
            break;
        }
        if (s > 285) { rule = mi_host::kInfSymbol; break; }
        u32 len;
        if (s < 265) len = s - 254;
        else if (s == 285) len = 258;
        else {
            const u32 e = (s - 261) >> 2;
            len = 3 + ((4 + ((s - 261) & 3)) << e) + inf_take(b, e);
        }
        inf_need(b, lane);
        const u32 d = inf_symbol(b, lds->t.dist_tab, kInfDistBits, lds->t.dist_sym, &lds->t.dist);
        if (d == kInfNoSymbol || d > 29) { rule = mi_host::kInfSymbol; break; }
        u32 dist;
        if (d < 4) dist = d + 1;
        else {
            const u32 e = (d >> 1) - 1;
            dist = 1 + ((2 + (d & 1)) << e) + inf_take(b, e);
        }
        if (inf_bit(b) > nbits) { rule = mi_host::kInfInputEnds; break; }
        if (op + len > limit) { rule = mi_host::kInfWindow; break; }
        if (o->symbols + 1 > o->cap) { rule = mi_host::kInfSymbolCap; break; }
        // the source positions are src + (i mod dist), src = op - dist >= -32 768: a negative one is a marker, one at or above
        // `flushed` lies in the staging, the others in the ring (THE RING INVARIANT)
        const i64 src = (i64)op - (i64)dist, flushed = (i64)(op - o->fill);
        const u32 fresh = len < dist ? len : dist;
        if (src + (i64)fresh > flushed + (i64)o->ring_seen) {
            __syncthreads();                                  // what the wave put into the staging has landed
            o->ring_seen = o->fill;
        }
#pragma nounroll
        for (u32 i = lane; i < len; i += 64) {
            const i64 p = src + (i64)(i < dist ? i : i % dist);
            u16 v;
            if (p < 0) v = (u16)(0x8000 + 32768 + p);         // the byte -p positions before the span's first byte
            else if (p >= flushed) v = lds->ring[(u32)(p - flushed)];
            else v = o->ring[(u64)p & (kSpecRing - 1)];
            lds->ring[o->fill + i] = v;
        }
        o->fill += len;
        ++o->symbols;
        op += len;
    }
    *op_io = op;
    return rule;
}

static __device__ __forceinline__ InflateRow spec_row(u64 end, u64 op, u32 status, u32 rule, u64 bit) {
    return InflateRow{end, op, status, rule, bit};
}
static __device__ __forceinline__ InflateRow spec_broken(u32 rule, u64 op, u64 bit) {
    const bool too_long = rule == mi_host::kInfWindow || rule == mi_host::kInfSymbolCap;
    return InflateRow{0, op, too_long ? (u32)mi_host::kInfSegTooLong : (u32)mi_host::kInfSegBroken, rule, bit};
}

// the span from bit `start`: how it ends.  Before every block header at a bit b > start: b is its piece's candidate -> the span ENDS there
static __device__ __forceinline__ InflateRow spec_segment(const u8* __restrict__ gz, u64 n, u64 hdr, u64 piece, u64 n_pieces,
                                                          const u64* __restrict__ cand, u64 start, u16* ring, u64 limit, u64 cap, InfSpecLds* lds, int lane) {
    InfBits b;
    b.gz = gz;
    b.n = n;
    inf_seek(&b, start / 8, lane);
    inf_drop(&b, (u32)start & 7u);                            // (the seek left at least 8 bits)
    SpecOut o = {ring, 0, 0, 0, cap};
    const u64 nbits = n * 8, stream_end = 8 * (n - 8);
    u64 op = 0;
    for (;;) {
        const u64 at = inf_bit(&b);
        if (at > start && at < stream_end) {
            const u64 pk = (at / 8 - hdr) / piece;            // (at >= start >= 8 hdr)
            if (pk < n_pieces && inf_uni64(cand[pk]) == at) {
                spec_flush(&o, lds, op, lane);
                return spec_row(at, op, mi_host::kInfSegEnds, 0, at);
            }
        }
        inf_need(&b, lane);
        const u32 bfinal = inf_take(&b, 1), btype = inf_take(&b, 2);
        if (inf_bit(&b) > nbits) return spec_broken(mi_host::kInfInputEnds, op, inf_bit(&b));
        if (btype == 3) return spec_broken(mi_host::kInfBlockType, op, inf_bit(&b));
        if (btype == 0) {
            inf_drop(&b, (u32)(0 - inf_bit(&b)) & 7u);         // to the byte boundary
            inf_need(&b, lane);
            const u32 len = inf_take(&b, 16), nlen = inf_take(&b, 16);
            if (inf_bit(&b) > nbits) return spec_broken(mi_host::kInfInputEnds, op, inf_bit(&b));
            if ((len ^ 0xFFFFu) != nlen) return spec_broken(mi_host::kInfStoredLen, op, inf_bit(&b));
            const u64 byte = inf_bit(&b) / 8;
            if (byte + len > n) return spec_broken(mi_host::kInfInputEnds, op, nbits);
            if (op + len > limit) return spec_broken(mi_host::kInfWindow, op, inf_bit(&b));
            spec_flush(&o, lds, op, lane);
            // the stored bytes are literal entries, copied at the wave's width (only the last 32 768 of them can stay)
#pragma nounroll
            for (u32 i = (len > kSpecRing ? len - (u32)kSpecRing : 0u) + (u32)lane; i < len; i += 64)
                ring[(op + i) & (kSpecRing - 1)] = (u16)gz[byte + i];
            __syncthreads();
            op += len;
            inf_seek(&b, byte + len, lane);
        } else {
            u32 hlit = kInfMaxLit, hdist = kInfMaxDist, rule = 0;
            if (btype == 1) inf_fixed_lengths(&lds->t, lane);
            else rule = inf_dynamic_header(&b, &lds->t, nbits, lane, &hlit, &hdist);
            if (!rule) rule = inf_tables(&lds->t, hlit, hdist, lane);
            if (rule) return spec_broken(rule, op, inf_bit(&b));
            rule = spec_block(&b, lds, &o, &op, limit, nbits, lane);
            if (rule) return spec_broken(rule, op, inf_bit(&b));
        }
        if (bfinal) {
            spec_flush(&o, lds, op, lane);
            return spec_row((inf_bit(&b) + 7) / 8 * 8, op, mi_host::kInfSegFinal, 0, inf_bit(&b));
        }
    }
}

// one wave a candidate; rings: 32 768 entries each, candidate k's at rings + 32 768 k.  A candidate of ~0 (or one that is no bit of
// the stream) gets no work: its row stays what it was
__global__ __launch_bounds__(64)
void inflate_speculate_kernel(const u8* __restrict__ gz, u64 n, u64 hdr, u64 piece, u64 n_pieces, const u64* __restrict__ cand, u64 window,
                              u64 cap, u16* __restrict__ rings, InflateRow* __restrict__ rows) {
    __shared__ InfSpecLds lds;
    const u64 k = blockIdx.x;
    if (k >= n_pieces) return;
    const u64 start = inf_uni64(cand[k]);
    if (start == kSpecNone || start < 8 * hdr || start >= 8 * (n - 8)) return;
    const InflateRow r = spec_segment(gz, n, hdr, piece, n_pieces, cand, start, rings + kSpecRing * k, window, cap, &lds, (int)threadIdx.x);
    if (threadIdx.x == 0) rows[k] = r;
}

// ---- the window pass ------------------------------------------------------------------------------------------------------------
// live: five words a live span, in chain order -- out_at, out_bytes, its window's offset in hist, the window's bytes, the candidate
// whose ring holds its output.  Span i's window W_i (i >= 1) is written to hist + win_at_i: byte j, the output position
// a = out_at_i - win_bytes_i + j, is span i - 1's ring entry when a lies in span i - 1's output -- a literal as it is, a marker k
// W_{i-1}[win_bytes_{i-1} - 32 768 + k] (0 when that index is negative: the write pass then refuses the span by rule 10) -- and
// W_{i-1}'s tail otherwise.  What one iteration writes the next reads: ONE workgroup, a barrier between the two.  The table is the
// host's, and still nothing of it is trusted: *bad (~0 before) takes the first span whose words do not fit, and the pass ends there
__global__ __launch_bounds__(1024)
void inflate_spec_windows_kernel(const u16* __restrict__ rings, u64 n_rings, const u64* __restrict__ live, u64 n_live, u8* hist, u64 hist_total,
                                 u64* __restrict__ bad) {
    for (u64 i = 1; i < n_live; ++i) {
        const u64 p_out = live[5 * i - 5], p_bytes = live[5 * i - 4], p_win = live[5 * i - 3], p_wb = live[5 * i - 2], p_ring = live[5 * i - 1];
        const u64 out_at = live[5 * i], win_at = live[5 * i + 2], wb = live[5 * i + 3];
        if (p_ring >= n_rings || p_wb > kSpecRing || p_win > hist_total || p_wb > hist_total - p_win || wb > kSpecRing || win_at > hist_total ||
            wb > hist_total - win_at || out_at != p_out + p_bytes || wb > out_at || p_wb > p_out) {
            if (threadIdx.x == 0) *bad = i;
            return;
        }
        const u16* ring = rings + kSpecRing * p_ring;
        const u8* from = hist + p_win;
        u8* to = hist + win_at;
        for (u64 j = threadIdx.x; j < wb; j += 1024) {
            const u64 a = out_at - wb + j;
            i64 at;                                           // the index in W_{i-1}, unless the ring holds a literal
            u8 v = 0;
            if (a >= p_out) {
                const u32 e = ring[(a - p_out) & (kSpecRing - 1)];
                at = (i64)p_wb - 32768 + (i64)(e & 0x7FFFu);
                if (e < 0x8000u) { v = (u8)e; at = -1; }
            } else {
                at = (i64)p_wb - (i64)(p_out - a);
            }
            if (at >= 0 && at < (i64)p_wb) v = from[at];
            to[j] = v;
        }
        __syncthreads();
    }
}

// ---- the launchers (the plan's, and the kernel probe's) ----------------------------------------------------------------------------
static bool spec_shape_ok(u64 n, u64 hdr, u64 piece, u64 n_pieces) {
    return n_pieces != 0 && n_pieces <= 0x7FFFFFFFull && piece != 0 && n >= 18 && hdr >= 10 && hdr <= n - 9;
}

void launch_inflate_find(const u8* d_gz, u64 n, u64 hdr, u64 piece, u64 n_pieces, u64* d_cand, hipStream_t s) {
    if (!spec_shape_ok(n, hdr, piece, n_pieces)) return;
    hipLaunchKernelGGL(inflate_find_kernel, dim3((u32)n_pieces), dim3(64), 0, s, d_gz, n, hdr, piece, n_pieces, d_cand);
}

void launch_inflate_speculate(const u8* d_gz, u64 n, u64 hdr, u64 piece, u64 n_pieces, const u64* d_cand, u64 window, u64 cap, u16* d_rings, void* d_rows,
                              hipStream_t s) {
    if (!spec_shape_ok(n, hdr, piece, n_pieces)) return;
    hipLaunchKernelGGL(inflate_speculate_kernel, dim3((u32)n_pieces), dim3(64), 0, s, d_gz, n, hdr, piece, n_pieces, d_cand, window, cap, d_rings,
                       (InflateRow*)d_rows);
}

void launch_inflate_spec_windows(const u16* d_rings, u64 n_rings, const u64* d_live, u64 n_live, u8* d_hist, u64 hist_total, u64* d_bad, hipStream_t s) {
    if (n_live < 2) return;
    hipLaunchKernelGGL(inflate_spec_windows_kernel, dim3(1), dim3(1024), 0, s, d_rings, n_rings, d_live, n_live, d_hist, hist_total, d_bad);
}

// the plan's spans and the window area (brought down from d_hist) as a MIGZIX01 index; the spacing field is the piece used
int inflate_spec_index(mi_inflater* d, void** index, u64* index_bytes) {
    *index = nullptr;
    *index_bytes = 0;
    const u64 n_points = d->spans.size() / 6;
    if (!d->spec_plan || n_points == 0) return d->fail(MI_ERR_STATE, "device inflate: no speculative plan to make an index of");
    const u64 bytes = mi_host::kIndexHeader + mi_host::kIndexRow * n_points + d->hist_bytes;
    u8* p = (u8*)malloc((size_t)bytes);
    if (!p) return d->fail(MI_ERR_NOMEM, "device inflate: no memory for an index of %llu bytes", (unsigned long long)bytes);
    memcpy(p, mi_host::kIndexMagic, 8);
    mi_host::index_put64(p + 8, d->n); mi_host::index_put64(p + 16, d->chain.total); mi_host::index_put32(p + 24, d->want_crc);
    mi_host::index_put32(p + 28, d->want_isize); mi_host::index_put64(p + 32, d->header); mi_host::index_put64(p + 40, n_points);
    mi_host::index_put64(p + 48, d->spec.piece_bytes); mi_host::index_put64(p + 56, d->hist_bytes);
    for (u64 k = 0; k < n_points; ++k) {
        u8* r = p + mi_host::kIndexHeader + mi_host::kIndexRow * k;
        const u64* s = d->spans.data() + 6 * k;
        mi_host::index_put64(r, s[0]); mi_host::index_put64(r + 8, s[2]); mi_host::index_put64(r + 16, s[4]);
        mi_host::index_put32(r + 24, (u32)s[5]); mi_host::index_put32(r + 28, 0);
    }
    if (d->hist_bytes) {
        const hipError_t e = hipMemcpy(p + mi_host::kIndexHeader + mi_host::kIndexRow * n_points, d->d_hist.p, d->hist_bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { free(p); return d->fail(MI_ERR_HIP, "device inflate: the windows did not come down: %s", hipGetErrorString(e)); }
    }
    *index = p;
    *index_bytes = bytes;
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_inflater_plan_spec(mi_inflater* d, const uint8_t* gz, uint64_t n, uint64_t piece_bytes, mi_inflate_seen_fn seen, void* arg) {
    if (!d || !gz) return MI_ERR_INVALID;
    IFCHK(d, hipSetDevice(d->ctx->device));
    d->info = mi_inflate_info();
    d->info.in_bytes = n;
    d->spec = mi_inflate_spec_info();
    d->spec_plan = false;
    d->n = n;
    if (!mi_host::gzip_header(gz, n, &d->header))
        return d->fail(MI_ERR_INVALID, "device inflate: no gzip header (magic, method 8, no reserved flag, complete) in a member of %llu bytes",
                       (unsigned long long)n);
    if (n < d->header + 8 + 1)
        return d->fail(MI_ERR_INVALID, "device inflate: a member of %llu bytes ends behind its %llu header bytes: no stream, no trailer",
                       (unsigned long long)n, (unsigned long long)d->header);
    mi_host::SpecPieces pc;
    if (!mi_host::spec_pieces(n, d->header, piece_bytes, &pc))
        return d->fail(MI_ERR_INVALID, "device inflate: piece_bytes %llu is not 0 or within %llu .. %llu", (unsigned long long)piece_bytes,
                       (unsigned long long)mi_host::kSpecPieceMin, (unsigned long long)mi_host::kSpecPieceMax);
    const u64 np = pc.n_pieces, hdr = d->header;
    d->want_crc = mi_host::inflate_le32(gz + n - 8);
    d->want_isize = mi_host::inflate_le32(gz + n - 4);
    d->indexed = true;
    d->chain = mi_host::InflateChain();
    d->spans.clear();
    d->round_first.clear();
    d->spec.piece_bytes = pc.piece;
    d->spec.n_pieces = np;
    d->spec.ring_bytes = 2 * kSpecRing * np;
    // all the scratch before the first launch: the rings (65 536 bytes a piece, at most 1 GiB), the rows, the candidates, the bad word
    DevBuf d_rings, d_bad, d_live;
    Event e0, e1, e2;
    IFCHK(d, d_rings.alloc_exact(2 * kSpecRing * np));
    IFCHK(d, d->d_cand.alloc_exact(np * 8));
    IFCHK(d, d->d_rows.alloc_exact(np * sizeof(InflateRow)));
    IFCHK(d, d_bad.alloc_exact(8));
    IFCHK(d, e0.create());
    IFCHK(d, e1.create());
    IFCHK(d, e2.create());
    StreamDrain drain{d->code};                         // nothing is queued on the scratch when it goes
    int rc = inflate_upload(d, gz, n, seen, arg);
    if (rc) return rc;
    IFCHK(d, hipMemsetAsync(d->d_rows.p, 0xFF, np * sizeof(InflateRow), d->code));       // a row nobody wrote is no status at all
    IFCHK(d, hipMemsetAsync(d->d_cand.p, 0xFF, np * 8, d->code));
    IFCHK(d, hipEventRecord(e0, d->code));
    launch_inflate_find(d->d_gz.as<u8>(), n, hdr, pc.piece, np, d->d_cand.as<u64>(), d->code);
    IFCHK(d, hipEventRecord(e1, d->code));
    launch_inflate_speculate(d->d_gz.as<u8>(), n, hdr, pc.piece, np, d->d_cand.as<u64>(), d->window, mi_host::kSpecSymbolsPerByte * pc.piece,
                             d_rings.as<u16>(), d->d_rows.p, d->code);
    IFCHK(d, hipGetLastError());
    IFCHK(d, hipEventRecord(e2, d->code));
    d->cand.resize(np);
    d->rows.resize(np);
    IFCHK(d, hipMemcpyAsync(d->cand.data(), d->d_cand.p, np * 8, hipMemcpyDeviceToHost, d->code));
    IFCHK(d, hipMemcpyAsync(d->rows.data(), d->d_rows.p, np * sizeof(InflateRow), hipMemcpyDeviceToHost, d->code));
    IFCHK(d, hipStreamSynchronize(d->code));
    float ms = 0;
    IFCHK(d, hipEventElapsedTime(&ms, e0, e1));
    d->spec.ms_find = ms;
    IFCHK(d, hipEventElapsedTime(&ms, e1, e2));
    d->spec.ms_speculate = ms;
    d->info.ms_size = d->spec.ms_find + d->spec.ms_speculate;
    for (u64 k = 0; k < np; ++k) d->spec.n_found += d->cand[k] != kSpecNone;
    d->info.n_candidates = d->spec.n_found;
    mi_host::SpecChain ch;
    mi_host::spec_chain(d->cand.data(), d->rows.data(), np, hdr, pc.piece, n, &ch);
    d->spec.n_live = ch.n_live;
    d->info.n_segments = ch.n_live;
    d->info.at_in = ch.at_bit / 8;
    d->info.at_out = ch.at_out;
    d->info.rule = ch.rule;
    if (ch.end == mi_host::kInfChainNotParallel) {
        d->info.verdict = MI_INFLATE_NOT_PARALLEL;
        return MI_OK;
    }
    if (ch.end == mi_host::kInfChainCorrupt)
        return d->fail(MI_ERR_INVALID, "corrupt gzip stream: span %llu at input bit %llu (output offset %llu) breaks rule %u at bit %llu: %s",
                       (unsigned long long)ch.span, (unsigned long long)ch.at_bit, (unsigned long long)ch.at_out, ch.rule, (unsigned long long)ch.bit,
                       mi_host::inflate_rule_name(ch.rule));
    if (ch.end != mi_host::kInfChainDone)
        return d->fail(MI_ERR_HIP, "device inflate: the speculative rows contradict the candidates at input bit %llu (%llu pieces)",
                       (unsigned long long)ch.at_bit, (unsigned long long)np);
    const u64 L = ch.spans.size();
    d->spans.resize(6 * L);
    std::vector<u64> live(5 * L);
    for (u64 k = 0; k < L; ++k) {
        const mi_host::SpecSpan& s = ch.spans[k];
        const u64 row[6] = {s.in_bit, s.end_bit, s.out_at, s.out_bytes, s.win_at, s.win_bytes};
        memcpy(d->spans.data() + 6 * k, row, sizeof row);
        const u64 lv[5] = {s.out_at, s.out_bytes, s.win_at, s.win_bytes, s.ring};
        memcpy(live.data() + 5 * k, lv, sizeof lv);
        d->chain.segs.push_back(mi_host::InflateSeg{s.in_bit / 8, s.out_at, s.out_bytes, k});
        if (s.out_bytes > d->window) {                      // (a merged span only) no span is split: zlib takes the member
            d->info.verdict = MI_INFLATE_NOT_PARALLEL;
            d->info.rule = mi_host::kInfWindow;
            d->info.at_in = s.in_bit / 8;
            d->info.at_out = s.out_at;
            return MI_OK;
        }
    }
    d->chain.end = mi_host::kInfChainDone;
    d->chain.total = ch.total;
    d->chain.at_in = d->chain.segs.back().in_at;
    d->chain.at_out = d->chain.segs.back().out_at;
    d->hist_bytes = ch.windows_bytes;
    d->d_hist.release();
    if (ch.windows_bytes) {
        if (guard_alloc()) {                                // exactly the area: its last byte is the allocation's last
            void* p = nullptr;
            IFCHK(d, dev_alloc(&p, (size_t)ch.windows_bytes));
            d->d_hist.p = p;
            d->d_hist.bytes = (size_t)ch.windows_bytes;
        } else {
            IFCHK(d, d->d_hist.alloc_exact(ch.windows_bytes));
        }
        IFCHK(d, d_live.alloc_exact(40 * L));
        u64 bad = ~0ull;
        IFCHK(d, hipMemsetAsync(d->d_hist.p, 0, ch.windows_bytes, d->code));               // the pads are zeros
        IFCHK(d, hipMemcpyAsync(d_live.p, live.data(), 40 * L, hipMemcpyHostToDevice, d->code));
        IFCHK(d, hipMemcpyAsync(d_bad.p, &bad, 8, hipMemcpyHostToDevice, d->code));
        IFCHK(d, hipEventRecord(e0, d->code));
        launch_inflate_spec_windows(d_rings.as<u16>(), np, d_live.as<u64>(), L, d->d_hist.as<u8>(), ch.windows_bytes, d_bad.as<u64>(), d->code);
        IFCHK(d, hipGetLastError());
        IFCHK(d, hipEventRecord(e1, d->code));
        IFCHK(d, hipMemcpyAsync(&bad, d_bad.p, 8, hipMemcpyDeviceToHost, d->code));
        IFCHK(d, hipStreamSynchronize(d->code));
        IFCHK(d, hipEventElapsedTime(&ms, e0, e1));
        d->spec.ms_windows = ms;
        if (bad != ~0ull) return d->fail(MI_ERR_HIP, "device inflate: the window pass refused the table at span %llu of %llu", (unsigned long long)bad,
                                         (unsigned long long)L);
    }
    d->spec_plan = true;
    d->info.n_segments = L;
    d->info.verdict = MI_INFLATE_DONE;
    d->info.out_bytes = ch.total;
    mi_host::inflate_rounds(d->chain.segs, d->window, &d->round_first);
    d->info.n_rounds = d->round_first.size() - 1;
    return MI_OK;
}

void mi_inflater_spec_info(const mi_inflater* d, mi_inflate_spec_info* out) { if (d && out) *out = d->spec; }

// ---- the calls -------------------------------------------------------------------------------------------------------------------
namespace {
struct SpecSink { u8* dst; u64 at; };
int spec_buffer_emit(void* arg, const uint8_t* bytes, uint64_t n) {
    SpecSink* b = (SpecSink*)arg;
    memcpy(b->dst + b->at, bytes, n);                   // (cap >= the plan's total: checked before the first round)
    b->at += n;
    return MI_OK;
}
}  // namespace

int mi_inflate_buffer_spec(mi_ctx* c, const void* gz, uint64_t n, uint64_t piece_bytes, void* dst, uint64_t cap, uint64_t* out_bytes,
                           mi_inflate_info* info, mi_inflate_spec_info* spec_info, void** index, uint64_t* index_bytes) {
    if (index) *index = nullptr;
    if (index_bytes) *index_bytes = 0;
    if (info) memset(info, 0, sizeof *info);
    if (spec_info) memset(spec_info, 0, sizeof *spec_info);
    if (!c || !gz || !out_bytes || (!dst && cap) || (!index != !index_bytes)) return MI_ERR_INVALID;
    *out_bytes = 0;
    mi_inflater* d = nullptr;
    int rc = mi_inflater_create(c, &d);
    if (rc) return rc;
    rc = mi_inflater_plan_spec(d, (const u8*)gz, n, piece_bytes, nullptr, nullptr);
    if (rc == MI_OK && d->info.verdict == MI_INFLATE_DONE) {
        if (d->info.out_bytes > cap) {                      // known after the plan: before the write pass
            *out_bytes = d->info.out_bytes;
            if (info) *info = d->info;
            if (spec_info) *spec_info = d->spec;
            mi_inflater_free(d);
            return fail(c, MI_ERR_CAPACITY, "mi_inflate_buffer_spec: the member inflates to %llu bytes, dst holds %llu", (unsigned long long)*out_bytes,
                        (unsigned long long)cap);
        }
        SpecSink sink{(u8*)dst, 0};
        rc = mi_inflater_run(d, spec_buffer_emit, &sink);
        if (rc == MI_OK) *out_bytes = sink.at;
        if (rc == MI_OK && index) rc = inflate_spec_index(d, index, index_bytes);
        if (rc == kInflateRefused) rc = MI_OK;              // a verdict, not an error: nothing is delivered
    }
    if (rc) fail(c, rc, "mi_inflate_buffer_spec: %s", d->err.c_str());
    if (info) *info = d->info;
    if (spec_info) *spec_info = d->spec;
    mi_inflater_free(d);
    return rc;
}

int mi_tar_inflate_ctx_spec(mi_ctx* c, const char* blob_path, uint64_t piece_bytes, const char* tar_path_out, uint64_t* tar_bytes, uint8_t* tar_sha256,
                            uint8_t* blob_sha256, mi_inflate_info* info, mi_inflate_spec_info* spec_info, void** index, uint64_t* index_bytes, char* err,
                            uint64_t err_cap) {
    if (index) *index = nullptr;
    if (index_bytes) *index_bytes = 0;
    if (spec_info) memset(spec_info, 0, sizeof *spec_info);
    if (!c || !blob_path || (!index != !index_bytes)) return MI_ERR_INVALID;
    const InfSpecAsk ask = {piece_bytes, spec_info, index, index_bytes};
    return tar_inflate_ctx_route(c, blob_path, nullptr, 0, &ask, tar_path_out, tar_bytes, tar_sha256, blob_sha256, info, err, err_cap);
}

}  // extern "C"
