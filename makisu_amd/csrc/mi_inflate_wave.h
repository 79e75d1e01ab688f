// mi_inflate_wave.h -- the decoder of one SEGMENT of a gzip member's deflate stream by ONE WAVE: what
// inflate_size_kernel (no byte written: the segment's end, its output bytes, or the rule it breaks) and inflate_write_kernel
// (the same decode again, straight to the segment's place in a round's output) both call.  The host half -- the gzip header, the
// rows, the chain, the rounds -- is host_inflate.h; the rule numbers are the ones stated there.
//
// THE FORMAT RULE.  A CANDIDATE is a byte offset p of the member gz[0, n) with gz[p - 4, p) == 00 00 FF FF and p <= n - 8; the first
// byte behind the gzip header is a candidate too.  The SEGMENT from a candidate c: deflate blocks are decoded from bit 8 c until
//   (a) an EMPTY stored block (LEN = 0) with BFINAL 0 has been read: the segment ends at the byte behind it, a candidate by
//       construction (what Z_SYNC_FLUSH writes, and what ends every dynamic piece of the device leg);
//   (b) a block with BFINAL 1 has been read: END -- the member's deflate stream ends at the next byte boundary;
//   (c) a rule is broken.
// Stored, fixed and dynamic blocks are all decoded.  No match of a segment may reach before the segment's first byte: both of this
// library's writers start every segment without history, and a blob that does not is handed to zlib (NOT_PARALLEL).  The LIVE
// CHAIN starts at the first byte behind the header and follows each segment's end to the next candidate until END, which must
// lie at exactly n - 8.  Candidates that are not on the chain are dead: their rows are never read.
//
// THE DECODE is wave-uniform and serial: one symbol after another, the bit buffer, the positions and every branch the same in
// all lanes (what comes out of LDS or out of a lane goes through readfirstlane so that the compiler knows it).  The lanes work
// together where there is width: the input window (64 words, one a lane), the code tables (counts by LDS atomics, ranks by
// ballots, the primary table's repeats), the copies (a match, a stored block, the flush of the staging ring).  The parallelism
// comes from the number of segments.
//
// TABLES, per block.  Code lengths in LDS -> the counts per length -> the canonical first codes and the offsets into the list of
// symbols sorted by (length, symbol) -> a PRIMARY table indexed by the next 10 (literal/length) or 8 (distance) bits of the
// stream, entry = symbol << 4 | length, 0 = no code this short.  A longer code (and a pattern with no symbol) walks first code /
// count / offset bit by bit.  The fixed code is built by the same path from its lengths.
//
// BOUNDS.  INPUT: the bit reader sees the member only through inf_load_word, which compares every byte's index with n before the
// load (whole words below n, single bytes at the end, zero behind it) -- nothing is loaded past the member's last byte, and bits
// "read" behind it are zeros that end the decode with kInfInputEnds at the next check (after every block header, every code
// length and every symbol); a stored block's bytes are copied only after byte + LEN <= n.  OUTPUT: a literal, a match or a stored
// run is placed only after op + len <= limit -- the window in the size pass, the segment's out_bytes from the size pass in the
// write pass -- and the ring is flushed to out[op - fill, op) only: nothing outside [out, out + limit).  A match's source is
// op - dist + (i mod dist) with 0 < dist <= op: inside the segment's own output.  LDS: a primary-table index is masked to the
// table's bits; a sorted-list index is offset + (code - first) < the number of coded symbols <= the list's size; lens[] is indexed
// below HLIT + HDIST <= 316 (+ the 19 code-length lengths behind 320); the ring below kInfRing (a token is placed only with
// 258 bytes of room).  A SPAN's match (kSpan) may reach before the span: its source is then hist[hist_bytes - back + i], 0 < back =
// dist - op <= hist_bytes checked before the copy and i < back -- window reads lie in [hist, hist + hist_bytes) only, and the kernel has
// held [hist, hist + hist_bytes) against the uploaded window area before the decode begins.  No kernel faults on any input: corrupt
// input -- and a corrupt or stale index -- is the normal case for this code.
//
// VISIBILITY.  The workgroup IS the wave.  What one lane wrote (a literal in the ring, a code length) and another lane reads is
// separated by __syncthreads(): `ring_seen` is the ring's fill at the last barrier, and a match whose source lies at or above it
// takes a barrier first (mi_lz4_wave.h's `seen`).  Global output is read only below op - fill (what has been flushed), and every flush ends in a barrier.
//
// LDS: kInfLds = 4 384 bytes a wave (the size pass carries the ring too: one layout).
#pragma once

#include "mi_common.h"
#include "host_inflate.h"

namespace mi {

typedef uint16_t u16;

constexpr u32 kInfLitBits = 10, kInfDistBits = 8;   // the primary tables' index bits
constexpr u32 kInfRing = 512;                       // the write pass's staging: literals and matches, flushed 255 bytes or more at a time (in front of a token
                                                    // once fill > kInfRing - 258), whatever it holds at a stored block and at the segment's end
constexpr u32 kInfMaxLit = 288, kInfMaxDist = 32;   // symbols a code may have lengths for (the fixed code: all of them)
constexpr u32 kInfLenCodeAt = 320;                  // lens[320, 339): the code-length code's own lengths
constexpr u32 kInfNoSymbol = 0xFFFFu;

struct InfCode { u16 count[16], first[16], offset[16]; };   // per code length: how many, the first canonical code, where they start in the list

struct InfLds {
    u16 lit_tab[1u << kInfLitBits];                 // 2 048
    u16 dist_tab[1u << kInfDistBits];               //   512
    u16 lit_sym[kInfMaxLit];                        //   576
    u16 dist_sym[kInfMaxDist];                      //    64
    u32 cnt[16];                                    //    64
    InfCode lit, dist;                              //   192
    u8 lens[kInfLenCodeAt + 32];                    //   352
    u8 ring[kInfRing];                              //   512
    u32 pad[16];                                    //    64 (the total stays a multiple of 128)
};
static_assert(sizeof(InfLds) == 4384, "kInfLds = 4 384 bytes");

static __device__ __forceinline__ u32 inf_uni(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }

// ---- the bit reader ------------------------------------------------------------------------------------------------------------
struct InfBits {
    const u8* gz;
    u64 n;
    u64 bb;               // the next bc bits of the stream, the first one lowest
    u32 bc;
    u64 next_word;        // the member's 4-byte word that is fed next
    u32 win_at;           // ... is the one lane win_at holds: lanes hold words [next_word - win_at, next_word - win_at + 64); 64: none
    u32 win;              // (a lane each)
};

// bytes [4 word, 4 word + 4) of the member, zero from n on
static __device__ __forceinline__ u32 inf_load_word(const u8* __restrict__ gz, u64 n, u64 word) {
    const u64 at = word * 4;
    if (at + 4 <= n) return *(const u32*)(gz + at);           // (gz is 256-byte aligned: a device allocation's first byte)
    u32 w = 0;
    for (u32 k = 0; k < 4; ++k)
        if (at + k < n) w |= (u32)gz[at + k] << (8 * k);
    return w;
}

static __device__ __forceinline__ void inf_feed(InfBits* b, int lane) {   // bc <= 32
    if (b->win_at >= 64) {
        b->win_at = 0;
        b->win = inf_load_word(b->gz, b->n, b->next_word + (u64)lane);
    }
    const u32 w = (u32)__builtin_amdgcn_readlane((int)b->win, (int)b->win_at);
    b->bb |= (u64)w << b->bc;
    b->bc += 32;
    ++b->win_at;
    ++b->next_word;
}
// at least 33 bits are there
static __device__ __forceinline__ void inf_need(InfBits* b, int lane) { if (b->bc <= 32) inf_feed(b, lane); }
static __device__ __forceinline__ void inf_drop(InfBits* b, u32 k) { b->bb >>= k; b->bc -= k; }
static __device__ __forceinline__ u32 inf_take(InfBits* b, u32 k) {       // k <= 16
    const u32 v = (u32)b->bb & ((1u << k) - 1u);
    inf_drop(b, k);
    return v;
}
static __device__ __forceinline__ u64 inf_bit(const InfBits* b) { return b->next_word * 32 - b->bc; }   // the next bit's number
static __device__ __forceinline__ void inf_seek(InfBits* b, u64 byte, int lane) {
    b->next_word = byte / 4;
    b->win_at = 64;                                           // no window yet: the feed loads one
    b->bb = 0;
    b->bc = 0;
    inf_feed(b, lane);
    inf_drop(b, (u32)(byte & 3) * 8);
}

// ---- the tables -----------------------------------------------------------------------------------------------------------------
struct InfBuilt { bool over; int left; u32 total, max_len; };

// lens[0, nsym) (LDS) -> the code's counts / first codes / offsets, its sorted list and its primary table of 2^bits entries.  over:
// over-subscribed (nothing else is valid then); left: what of the code space stays unused; total: symbols with a length
static __device__ __forceinline__ InfBuilt inf_build(const u8* lens, u32 nsym, u16* tab, u32 bits, u16* sym, InfCode* code, u32* cnt, int lane) {
    __syncthreads();                                          // the lengths are written; nobody reads the old tables any more
    if (lane < 16) cnt[lane] = 0;
    for (u32 i = lane; i < (1u << bits) / 2; i += 64) ((u32*)tab)[i] = 0;
    __syncthreads();
    for (u32 s = lane; s < nsym; s += 64) {
        const u32 l = lens[s];
        if (l) atomicAdd(&cnt[l & 15u], 1u);
    }
    __syncthreads();
    InfBuilt r = {false, 1, 0, 0};
#pragma nounroll
    for (u32 len = 1; len <= 15; ++len) {
        const u32 c = inf_uni(cnt[len]);
        r.left = (r.left << 1) - (int)c;
        if (r.left < 0) { r.over = true; return r; }
        if (c) r.max_len = len;
        r.total += c;
    }
    if (lane == 0) {
        u32 f = 0, o = 0, prev = 0;
        code->count[0] = 0; code->first[0] = 0; code->offset[0] = 0;
#pragma nounroll
        for (u32 len = 1; len <= 15; ++len) {
            f = (f + prev) << 1;
            prev = cnt[len];
            code->first[len] = (u16)f;
            code->offset[len] = (u16)o;
            code->count[len] = (u16)prev;
            o += prev;
        }
    }
    __syncthreads();
    // the rank of every symbol among those of its length, 64 symbols a step: one ballot per length that occurs among them; cnt[]
    // now counts the symbols of a length that lie in front of the step
    if (lane < 16) cnt[lane] = 0;
    __syncthreads();
    for (u32 base = 0; base < nsym; base += 64) {
        const u32 s = base + (u32)lane;
        const u32 l = s < nsym ? (u32)lens[s] & 15u : 0u;
        u32 rank = 0;
        for (u64 todo = __ballot(l != 0); todo;) {
            const u32 len = inf_uni((u32)__shfl((int)l, __ffsll((unsigned long long)todo) - 1));
            const u64 m = __ballot(l == len);
            const u32 before = inf_uni(cnt[len]);
            if (l == len) rank = before + (u32)__popcll(m & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == 0) cnt[len] = before + (u32)__popcll(m);
            __syncthreads();
            todo &= ~m;
        }
        if (l) {
            const u32 c = (u32)code->first[l] + rank;
            sym[(u32)code->offset[l] + rank] = (u16)s;        // offset + rank < total <= nsym
            if (l <= bits) {
                const u16 e = (u16)(s << 4 | l);
                for (u32 j = __brev(c) >> (32 - l); j < (1u << bits); j += 1u << l) tab[j] = e;
            }
        }
    }
    __syncthreads();
    return r;
}

// the next symbol of a code (at least 15 bits are there), or kInfNoSymbol: the bits are no code of it
static __device__ __forceinline__ u32 inf_symbol(InfBits* b, const u16* tab, u32 bits, const u16* sym, const InfCode* code) {
    const u32 e = inf_uni(tab[(u32)b->bb & ((1u << bits) - 1u)]);
    if (e) { inf_drop(b, e & 15u); return e >> 4; }
    u32 c = 0;
    u64 rest = b->bb;
#pragma nounroll
    for (u32 len = 1; len <= 15; ++len) {
        c = c << 1 | (u32)(rest & 1);
        rest >>= 1;
        const u32 first = inf_uni(code->first[len]), count = inf_uni(code->count[len]);
        if (c >= first && c - first < count) {
            inf_drop(b, len);
            return inf_uni(sym[inf_uni(code->offset[len]) + (c - first)]);
        }
    }
    return kInfNoSymbol;
}

// ---- the segment ----------------------------------------------------------------------------------------------------------------
struct InfEnd { u64 end, out_bytes, bit; u32 status, rule; };

static __device__ __forceinline__ InfEnd inf_broken(u32 rule, u64 op, u64 bit) {
    return InfEnd{0, op, bit, rule == mi_host::kInfWindow ? (u32)mi_host::kInfSegTooLong : (u32)mi_host::kInfSegBroken, rule};
}

template <bool kWrite>
struct InfOut {
    u8* out;              // the segment's first output byte
    u32 fill, ring_seen;  // the ring holds out[op - fill, op); below ring_seen it is visible to every lane.  FLUSHED = op - fill:
                          // out[0, flushed) is written and visible to every lane
    const u8* hist;       // (a span only) the hist_bytes of output in front of the span's first byte, in global memory
    u32 hist_bytes;
};

template <bool kWrite>
static __device__ __forceinline__ void inf_flush(InfOut<kWrite>* o, InfLds* lds, u64 op, int lane) {
    if (!kWrite) return;
    __syncthreads();
#pragma nounroll
    for (u32 i = lane; i < o->fill; i += 64) o->out[op - o->fill + i] = lds->ring[i];
    __syncthreads();
    o->fill = 0;
    o->ring_seen = 0;
}

// the symbols of one fixed or dynamic block whose tables stand; 0 or the rule
template <bool kWrite, bool kSpan = false>
static __device__ __forceinline__ u32 inf_block(InfBits* b, InfLds* lds, InfOut<kWrite>* o, u64* op_io, u64 limit, u64 nbits, int lane) {
    u64 op = *op_io;
    u32 rule = 0;
    for (;;) {
        if (kWrite && o->fill > kInfRing - 258) inf_flush(o, lds, op, lane);
        inf_need(b, lane);
        const u32 s = inf_symbol(b, lds->lit_tab, kInfLitBits, lds->lit_sym, &lds->lit);
        if (s == kInfNoSymbol) { rule = mi_host::kInfSymbol; break; }
        if (s < 256) {
            if (inf_bit(b) > nbits) { rule = mi_host::kInfInputEnds; break; }
            if (op + 1 > limit) { rule = mi_host::kInfWindow; break; }
            if (kWrite) {
                if (lane == 0) lds->ring[o->fill] = (u8)s;
                ++o->fill;
            }
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
        const u32 d = inf_symbol(b, lds->dist_tab, kInfDistBits, lds->dist_sym, &lds->dist);
        if (d == kInfNoSymbol || d > 29) { rule = mi_host::kInfSymbol; break; }
        u32 dist;
        if (d < 4) dist = d + 1;
        else {
            const u32 e = (d >> 1) - 1;
            dist = 1 + ((2 + (d & 1)) << e) + inf_take(b, e);
        }
        if (inf_bit(b) > nbits) { rule = mi_host::kInfInputEnds; break; }
        if (kSpan ? (u64)dist > op + o->hist_bytes : (u64)dist > op) { rule = mi_host::kInfDistance; break; }
        if (op + len > limit) { rule = mi_host::kInfWindow; break; }
        if (kSpan && kWrite && (u64)dist > op) {
            // (a span only) the source begins in the window: its first `back` bytes are hist[hist_bytes - back, hist_bytes), the
            // rest -- i mod dist is what it was -- the span's own bytes from 0 on, flushed or in the ring
            const u32 back = dist - (u32)op, fresh = len < dist ? len : dist;     // (op < dist <= 32 768)
            const u64 flushed = op - o->fill;
            if (fresh > back && (u64)(fresh - back) > flushed + o->ring_seen) {
                __syncthreads();
                o->ring_seen = o->fill;
            }
#pragma nounroll
            for (u32 i = lane; i < len; i += 64) {
                const u32 at = i < dist ? i : i % dist;
                u8 v;
                if (at < back) v = o->hist[o->hist_bytes - back + at];           // back <= hist_bytes: checked above
                else {
                    const u64 p = at - back;
                    v = p >= flushed ? lds->ring[(u32)(p - flushed)] : o->out[p];
                }
                lds->ring[o->fill + i] = v;
            }
            o->fill += len;
        } else if (kWrite) {
            // the match repeats the `dist` bytes in front of op; they lie in out[0, flushed) or in the ring behind it
            const u64 src = op - dist, flushed = op - o->fill;
            const u32 fresh = len < dist ? len : dist;
            if (src + fresh > flushed + o->ring_seen) {
                __syncthreads();                              // what the wave put into the ring has landed
                o->ring_seen = o->fill;
            }
#pragma nounroll
            for (u32 i = lane; i < len; i += 64) {
                const u64 p = src + (i < dist ? i : i % dist);
                lds->ring[o->fill + i] = p >= flushed ? lds->ring[(u32)(p - flushed)] : o->out[p];
            }
            o->fill += len;
        }
        op += len;
    }
    *op_io = op;
    return rule;
}

// a dynamic block's header -> the code lengths lens[0, *hlit_out + *hdist_out); 0 or the rule
static __device__ __forceinline__ u32 inf_dynamic_header(InfBits* b, InfLds* lds, u64 nbits, int lane, u32* hlit_out, u32* hdist_out) {
    inf_need(b, lane);
    const u32 hlit = inf_take(b, 5) + 257, hdist = inf_take(b, 5) + 1, hclen = inf_take(b, 4) + 4;
    if (inf_bit(b) > nbits) return mi_host::kInfInputEnds;
    if (hlit > 286 || hdist > 30) return mi_host::kInfTooManyCodes;
    __syncthreads();
    if (lane < 19) lds->lens[kInfLenCodeAt + lane] = 0;
    __syncthreads();
    for (u32 i = 0; i < hclen; ++i) {
        inf_need(b, lane);
        const u32 v = inf_take(b, 3);
        // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
        const u32 where = i < 12 ? (u32)((0x22CAA324E804A30ull >> (5 * i)) & 31) : (u32)((0x3C2E1346Cull >> (5 * (i - 12))) & 31);
        if (lane == 0) lds->lens[kInfLenCodeAt + where] = (u8)v;
    }
    if (inf_bit(b) > nbits) return mi_host::kInfInputEnds;
    InfBuilt t = inf_build(lds->lens + kInfLenCodeAt, 19, lds->lit_tab, 7, lds->lit_sym, &lds->lit, lds->cnt, lane);
    if (t.over || t.left != 0) return mi_host::kInfLengthCode;
    const u32 total = hlit + hdist;
    u32 have = 0, prev = 0;
    while (have < total) {
        inf_need(b, lane);
        const u32 s = inf_symbol(b, lds->lit_tab, 7, lds->lit_sym, &lds->lit);
        if (s == kInfNoSymbol) return mi_host::kInfSymbol;    // (a complete code has a symbol for every pattern)
        if (s < 16) {
            if (lane == 0) lds->lens[have] = (u8)s;
            ++have;
            prev = s;
        } else {
            u32 rep, val = 0;
            if (s == 16) {
                if (have == 0) return mi_host::kInfRepeat;
                val = prev;
                rep = 3 + inf_take(b, 2);
            } else if (s == 17) rep = 3 + inf_take(b, 3);
            else rep = 11 + inf_take(b, 7);
            if (have + rep > total) return mi_host::kInfRepeat;
            for (u32 i = lane; i < rep; i += 64) lds->lens[have + i] = (u8)val;
            have += rep;
            prev = val;
        }
        if (inf_bit(b) > nbits) return mi_host::kInfInputEnds;
    }
    __syncthreads();
    if (inf_uni(lds->lens[256]) == 0) return mi_host::kInfNoEndOfBlock;
    *hlit_out = hlit;
    *hdist_out = hdist;
    return 0;
}

// lens[0, hlit) and lens[hlit, hlit + hdist) -> the literal/length and the distance tables (one body, twice); 0 or the rule.  A code
// may be incomplete only as a single code of length 1; a distance code with no length at all is a block without matches
static __device__ __forceinline__ u32 inf_tables(InfLds* lds, u32 hlit, u32 hdist, int lane) {
#pragma nounroll
    for (u32 which = 0; which < 2; ++which) {
        const InfBuilt t = inf_build(lds->lens + (which ? hlit : 0u), which ? hdist : hlit, which ? lds->dist_tab : lds->lit_tab,
                                     which ? kInfDistBits : kInfLitBits, which ? lds->dist_sym : lds->lit_sym, which ? &lds->dist : &lds->lit,
                                     lds->cnt, lane);
        if (t.over || (t.total != 0 && t.left > 0 && !(t.max_len == 1 && t.total == 1))) return mi_host::kInfCode;
    }
    return 0;
}

// the fixed code's lengths (RFC 1951 3.2.6), all 288 + 32 of them
static __device__ __forceinline__ void inf_fixed_lengths(InfLds* lds, int lane) {
    __syncthreads();
    for (u32 i = lane; i < kInfMaxLit; i += 64) lds->lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    if (lane < (int)kInfMaxDist) lds->lens[kInfMaxLit + lane] = 5;
}

// the segment from byte `start` of gz[0, n): how it ends.  kWrite: its bytes go to out[0, limit), limit = what the size pass found
//
// kSpan: the SPAN between two checkpoints of an index (host_inflate_index.h), five differences.  `start` is a BIT of the
// member; an empty stored block is a block like any other; the span ends where the next block's header would begin at bit
// sp->end_bit, with exactly `limit` bytes made -- a header that begins behind end_bit, a BFINAL block in front of it and output
// beyond `limit` are all kInfIndex, "the span does not end where the index says" --; the last span (end_bit 0) ends at its BFINAL
// block; and a match may reach up to sp->hist_bytes before the span's first byte, into sp->hist (inf_block).
struct InfSpan { u64 end_bit; const u8* hist; u32 hist_bytes; };

template <bool kWrite, bool kSpan = false>
static __device__ __forceinline__ InfEnd inf_segment(const u8* __restrict__ gz, u64 n, u64 start, u8* out, u64 limit, InfLds* lds, int lane,
                                                     const InfSpan* sp = nullptr) {
    InfBits b;
    b.gz = gz;
    b.n = n;
    inf_seek(&b, kSpan ? start / 8 : start, lane);
    InfOut<kWrite> o = {out, 0, 0, nullptr, 0};
    if (kSpan) {
        inf_drop(&b, (u32)start & 7u);                        // (the seek left at least 8 bits)
        o.hist = sp->hist;
        o.hist_bytes = sp->hist_bytes;
    }
    const u64 nbits = n * 8;
    u64 op = 0;
    for (;;) {
        if (kSpan && sp->end_bit) {
            if (inf_bit(&b) == sp->end_bit) {
                inf_flush(&o, lds, op, lane);
                if (op != limit) return inf_broken(mi_host::kInfIndex, op, inf_bit(&b));
                return InfEnd{inf_bit(&b) / 8, op, inf_bit(&b), mi_host::kInfSegEnds, 0};
            }
            if (inf_bit(&b) > sp->end_bit) return inf_broken(mi_host::kInfIndex, op, inf_bit(&b));
        }
        inf_need(&b, lane);
        const u32 bfinal = inf_take(&b, 1), btype = inf_take(&b, 2);
        if (inf_bit(&b) > nbits) return inf_broken(mi_host::kInfInputEnds, op, inf_bit(&b));
        if (kSpan && bfinal && sp->end_bit) return inf_broken(mi_host::kInfIndex, op, inf_bit(&b));
        if (btype == 3) return inf_broken(mi_host::kInfBlockType, op, inf_bit(&b));
        if (btype == 0) {
            inf_drop(&b, (u32)(0 - inf_bit(&b)) & 7u);         // to the byte boundary
            inf_need(&b, lane);
            const u32 len = inf_take(&b, 16), nlen = inf_take(&b, 16);
            if (inf_bit(&b) > nbits) return inf_broken(mi_host::kInfInputEnds, op, inf_bit(&b));
            if ((len ^ 0xFFFFu) != nlen) return inf_broken(mi_host::kInfStoredLen, op, inf_bit(&b));
            const u64 byte = inf_bit(&b) / 8;
            if (!kSpan && len == 0 && !bfinal) {
                inf_flush(&o, lds, op, lane);
                return InfEnd{byte, op, inf_bit(&b), mi_host::kInfSegEnds, 0};
            }
            if (byte + len > n) return inf_broken(mi_host::kInfInputEnds, op, nbits);
            if (op + len > limit) return inf_broken(kSpan ? mi_host::kInfIndex : mi_host::kInfWindow, op, inf_bit(&b));
            if (kWrite) {
                inf_flush(&o, lds, op, lane);
#pragma nounroll
                for (u32 i = lane; i < len; i += 64) out[op + i] = gz[byte + i];
                __syncthreads();
            }
            op += len;
            inf_seek(&b, byte + len, lane);
        } else {
            u32 hlit = kInfMaxLit, hdist = kInfMaxDist, rule = 0;
            if (btype == 1) inf_fixed_lengths(lds, lane);
            else rule = inf_dynamic_header(&b, lds, nbits, lane, &hlit, &hdist);
            if (!rule) rule = inf_tables(lds, hlit, hdist, lane);
            if (rule) return inf_broken(rule, op, inf_bit(&b));
            rule = inf_block<kWrite, kSpan>(&b, lds, &o, &op, limit, nbits, lane);
            if (rule) return inf_broken(kSpan && rule == mi_host::kInfWindow ? (u32)mi_host::kInfIndex : rule, op, inf_bit(&b));
        }
        if (bfinal) {
            inf_flush(&o, lds, op, lane);
            return InfEnd{(inf_bit(&b) + 7) / 8, op, inf_bit(&b), mi_host::kInfSegFinal, 0};
        }
    }
}

}  // namespace mi
