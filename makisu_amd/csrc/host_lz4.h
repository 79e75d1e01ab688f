// host_lz4.h -- the decoder of one standard LZ4 block on a host core, under the rules zpack_decode_kernel (mi_zpack.hip)
// decodes by: what mi_zpack_check runs over every entry of a compressed pack whose stored form is shorter than the chunk.
// Plain C++, no HIP: a stand-alone program may include it (tests/test_host_zpack_decoder_sanitized.py does).
//
// A block is a run of sequences: a token (literal length in the high nibble, match length - 4 in the low one, 15 = extension
// bytes follow, each added, the first below 255 ends them), the literals, a 2-byte little-endian offset in 1..65535 and the
// match length's extension bytes.  The last sequence ends behind its literals.  The decoder trusts NOTHING of it: it writes
// inside [dst, dst + n) and reads inside [src, src + stored) and in front of the bytes it has produced, or it refuses.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mi_host {

// why an entry is refused; the kernel reports the same numbers
enum Lz4Rule : uint32_t {
    kLz4Ok = 0,
    kLz4OffsetZero = 1,       // a match offset of 0
    kLz4OffsetBeyond = 2,     // an offset beyond the bytes produced so far
    kLz4LiteralsLeave = 3,    // a literal run that leaves the stored span
    kLz4ExtensionCut = 4,     // a length extension (or the offset) cut off by the span's end
    kLz4OutputPasses = 5,     // literals or a match that pass the chunk's length
    kLz4OutputShort = 6,      // the stream ends with output short of the chunk's length
    kLz4PadNotZero = 7,       // a byte behind the stored span, inside its 16-byte unit, is not zero
};

static inline const char* lz4_rule_name(uint32_t rule) {
    static const char* const names[] = {"ok", "a match offset of 0", "a match offset beyond the bytes produced so far",
                                        "a literal run that leaves the stored span", "a length extension or an offset cut off by the span's end",
                                        "output that passes the chunk's length", "a stream that ends with output short of the chunk's length",
                                        "a pad byte behind the stored span that is not zero"};
    return rule < sizeof names / sizeof names[0] ? names[rule] : "?";
}

// a length's extension bytes behind a nibble of 15; false: the span ended first
static inline bool lz4_extension(const uint8_t* src, uint64_t stored, uint64_t* ip, uint64_t* len) {
    for (;;) {
        if (*ip >= stored) return false;
        const uint8_t b = src[(*ip)++];
        *len += b;
        if (b != 255) return true;
    }
}

// src[0, stored) -> dst[0, n): kLz4Ok, or the rule that refuses the stream (dst then holds garbage inside its n bytes)
static inline uint32_t lz4_block_decode(const uint8_t* src, uint64_t stored, uint8_t* dst, uint64_t n) {
    uint64_t ip = 0, op = 0;
    for (;;) {
        if (ip >= stored) return kLz4OutputShort;                        // a token is due and there is none
        const uint8_t token = src[ip++];
        uint64_t lit = token >> 4;
        if (lit == 15 && !lz4_extension(src, stored, &ip, &lit)) return kLz4ExtensionCut;
        if (lit > stored - ip) return kLz4LiteralsLeave;
        if (lit > n - op) return kLz4OutputPasses;
        for (uint64_t i = 0; i < lit; ++i) dst[op + i] = src[ip + i];
        ip += lit;
        op += lit;
        if (ip == stored) return op == n ? kLz4Ok : kLz4OutputShort;     // the last sequence: literals only
        if (stored - ip < 2) return kLz4ExtensionCut;
        const uint64_t off = (uint64_t)src[ip] | ((uint64_t)src[ip + 1] << 8);
        ip += 2;
        if (off == 0) return kLz4OffsetZero;
        if (off > op) return kLz4OffsetBeyond;
        uint64_t len = token & 15;
        if (len == 15 && !lz4_extension(src, stored, &ip, &len)) return kLz4ExtensionCut;
        len += 4;
        if (len > n - op) return kLz4OutputPasses;
        for (uint64_t i = 0; i < len; ++i) dst[op + i] = dst[op - off + i];   // byte by byte: an overlapping match repeats itself
        op += len;
    }
}

}  // namespace mi_host
