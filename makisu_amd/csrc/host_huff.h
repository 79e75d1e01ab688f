// host_huff.h -- the decoder of one entropy form ("form H", include/makisu_mi.h FORMAT) on a host core, under the
// rules zh_unwrap_kernel (mi_zentropy.hip) decodes by: what mi_zpack_check runs over an entry whose stored form is shorter than
// the chunk and begins with 0x00.  Plain C++, no HIP: a stand-alone program may include it
// (tests/test_host_huff_decoder_sanitized.py does).
//
// Form H wraps the form under it -- the chunk's LZ4 block (kind 1) or its plain bytes (kind 2) -- in a byte-wise Huffman code,
// symbol i of the inner bytes in stream i mod S:
//     0x00 | kind | S - 1 | 0 | inner length u32 LE | 128 bytes: 256 code lengths of 4 bits, 0 = absent, 1..11 |
//     S stream sizes u16 LE | the streams: canonical codes by (length, symbol), LSB first, bit-reversed, zero pad bits
// The decoder trusts NOTHING of it: it writes inside [inner, inner + inner length), where inner length <= length <= 65 536 was
// checked first, and reads inside [src, src + stored), or it refuses.  The rules continue host_lz4.h's numbering and are checked
// in this order; the inner block of kind 1 then falls under rules 1..6, the pad behind the span under rule 7 as ever.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "host_lz4.h"

namespace mi_host {

enum HuffRule : uint32_t {
    kHuffHeader = 8,          // kind not 1 or 2, the reserved byte set, more than 64 streams, an inner length that breaks the rule of
                              // its kind, a span shorter than header, table and sizes, or a chunk above 65 536 bytes
    kHuffCode = 9,            // a code length above 11, no symbol at all, or an over-subscribed code
    kHuffSizes = 10,          // the stream sizes do not sum to exactly the rest of the span
    kHuffBits = 11,           // a stream ends before its symbols do, meets an unassigned code, has a whole byte left over or a pad bit set
};

constexpr uint32_t kHuffMaxBits = 11;
constexpr uint32_t kHuffTable = 1u << kHuffMaxBits;       // entries: symbol | length << 8, 0 = nobody's code
constexpr uint32_t kHuffMaxStreams = 64;
constexpr uint32_t kHuffStreams = 32;                     // what the coder uses
constexpr uint32_t kHuffMaxChunk = 65536;
constexpr uint32_t kHuffHead = 8 + 128;                   // in front of the stream sizes
constexpr uint32_t kHuffKindLz4 = 1, kHuffKindRaw = 2;

static inline const char* zrule_name(uint32_t rule) {
    static const char* const names[] = {"an entropy form with a bad header (kind, reserved byte, stream count, inner length, span or a chunk above 65536 bytes)",
                                        "an entropy form whose code lengths are above 11 bits, all absent or over-subscribed",
                                        "an entropy form whose stream sizes do not sum to the rest of the span",
                                        "an entropy form with a stream that ends early, meets an unassigned code, has a byte left over or a pad bit set"};
    return rule >= kHuffHeader && rule <= kHuffBits ? names[rule - kHuffHeader] : lz4_rule_name(rule);
}

// a span with stored < length that begins with 0x00 is form H: no LZ4 block begins with a token without literals
static inline bool is_form_h(const uint8_t* src, uint64_t stored, uint64_t length) { return stored < length && src[0] == 0; }

static inline uint32_t huff_reverse(uint32_t v, uint32_t bits) {
    uint32_t out = 0;
    for (uint32_t i = 0; i < bits; ++i, v >>= 1) out = (out << 1) | (v & 1);
    return out;
}

// the 2 048-entry table of the 128 bytes of code lengths; kLz4Ok or kHuffCode
static inline uint32_t huff_build_table(const uint8_t* lens4, uint16_t* table) {
    uint32_t count[kHuffMaxBits + 2] = {}, next[kHuffMaxBits + 2] = {};
    for (uint32_t s = 0; s < 256; ++s) {
        const uint32_t l = (lens4[s >> 1] >> ((s & 1) * 4)) & 15;
        if (l > kHuffMaxBits) return kHuffCode;
        ++count[l];
    }
    uint32_t kraft = 0, code = 0;
    for (uint32_t l = 1; l <= kHuffMaxBits; ++l) {
        kraft += count[l] << (kHuffMaxBits - l);
        code = (code + count[l - 1] * (l > 1)) << 1;
        next[l] = code;
    }
    if (kraft == 0 || kraft > kHuffTable) return kHuffCode;
    for (uint32_t i = 0; i < kHuffTable; ++i) table[i] = 0;
    for (uint32_t s = 0; s < 256; ++s) {
        const uint32_t l = (lens4[s >> 1] >> ((s & 1) * 4)) & 15;
        if (!l) continue;
        const uint32_t r = huff_reverse(next[l]++, l);
        for (uint32_t i = r; i < kHuffTable; i += 1u << l) table[i] = (uint16_t)(s | (l << 8));
    }
    return kLz4Ok;
}

// src[0, stored), the stored form of a chunk of `length` bytes -> inner[0, *inner_len) and its kind; `inner` holds `length`
// bytes.  kLz4Ok, or the rule that refuses the form (inner then holds garbage inside its bytes)
static inline uint32_t huff_decode(const uint8_t* src, uint64_t stored, uint64_t length, uint8_t* inner, uint32_t* inner_len, uint32_t* kind_out) {
    if (stored < 8 || src[0] != 0 || (src[1] != kHuffKindLz4 && src[1] != kHuffKindRaw) || src[2] >= kHuffMaxStreams || src[3] != 0 ||
        length > kHuffMaxChunk)
        return kHuffHeader;
    const uint32_t kind = src[1], streams = (uint32_t)src[2] + 1;
    const uint64_t n = (uint64_t)src[4] | ((uint64_t)src[5] << 8) | ((uint64_t)src[6] << 16) | ((uint64_t)src[7] << 24);
    if (kind == kHuffKindLz4 ? (n == 0 || n >= length) : n != length) return kHuffHeader;
    if (stored < kHuffHead + 2 * streams) return kHuffHeader;
    uint16_t table[kHuffTable];
    const uint32_t rc = huff_build_table(src + 8, table);
    if (rc) return rc;
    const uint64_t body = kHuffHead + 2 * streams;
    uint64_t sum = 0;
    for (uint32_t s = 0; s < streams; ++s) sum += (uint64_t)src[kHuffHead + 2 * s] | ((uint64_t)src[kHuffHead + 2 * s + 1] << 8);
    if (sum != stored - body) return kHuffSizes;
    uint64_t at = body;
    for (uint32_t s = 0; s < streams; ++s) {
        const uint64_t size = (uint64_t)src[kHuffHead + 2 * s] | ((uint64_t)src[kHuffHead + 2 * s + 1] << 8);
        const uint8_t* p = src + at;                     // [p, p + size) is inside the span: the sizes sum to its rest
        uint64_t acc = 0, ip = 0;
        uint32_t have = 0;
        for (uint64_t i = s; i < n; i += streams) {
            while (have <= 56 && ip < size) { acc |= (uint64_t)p[ip++] << have; have += 8; }
            const uint32_t e = table[acc & (kHuffTable - 1)], l = e >> 8;
            if (l == 0 || l > have) return kHuffBits;    // nobody's code, or the stream ended inside the code
            inner[i] = (uint8_t)e;
            acc >>= l;
            have -= l;
        }
        if (ip != size || have >= 8 || acc != 0) return kHuffBits;       // a byte left over, or a pad bit set
        at += size;
    }
    *inner_len = (uint32_t)n;
    *kind_out = kind;
    return kLz4Ok;
}

// one stored form with stored < length -> dst[0, length): the LZ4 block, or form H over it or over the plain bytes; `inner`
// holds `length` bytes of scratch.  kLz4Ok or the rule
static inline uint32_t zform_decode(const uint8_t* src, uint64_t stored, uint8_t* dst, uint64_t length, uint8_t* inner) {
    if (!is_form_h(src, stored, length)) return lz4_block_decode(src, stored, dst, length);
    uint32_t n = 0, kind = 0;
    const uint32_t rc = huff_decode(src, stored, length, inner, &n, &kind);
    if (rc) return rc;
    if (kind == kHuffKindLz4) return lz4_block_decode(inner, n, dst, length);
    for (uint64_t i = 0; i < length; ++i) dst[i] = inner[i];
    return kLz4Ok;
}

}  // namespace mi_host
