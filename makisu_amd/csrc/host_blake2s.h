// host_blake2s.h -- streaming BLAKE2s-256 (RFC 7693: unkeyed, no salt, no personalisation, sequential mode) on a host
// core: hashlib.blake2s(b).digest().  What the host hashes with it are chunk DIGESTS -- the root of a split file
// (mi_group.hip), mi_chunk_root_alg -- 32 bytes per chunk, so it is the plain portable form; the data itself is hashed
// on the GPU (blake2s.hip).  Product code: independent of oracle/.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace mi_host {

class Blake2s {
public:
    Blake2s() { reset(); }
    void reset() {
        memcpy(h_, iv(), sizeof h_);
        h_[0] ^= 0x01010020u;                 // parameter block: digest_length 32, no key, fanout 1, depth 1
        t_ = 0;
        fill_ = 0;
    }
    // (a full buffer is only compressed when more input follows: the block that ENDS the string carries the final flag)
    void update(const void* data, size_t len) {
        const uint8_t* p = (const uint8_t*)data;
        while (len) {
            if (fill_ == 64) {
                t_ += 64;
                compress(buf_, false);
                fill_ = 0;
            }
            size_t take = 64 - fill_;
            if (take > len) take = len;
            memcpy(buf_ + fill_, p, take);
            fill_ += take;
            p += take;
            len -= take;
        }
    }
    void final(uint8_t out[32]) {
        t_ += fill_;
        memset(buf_ + fill_, 0, 64 - fill_);
        compress(buf_, true);
        for (int i = 0; i < 8; ++i) {
            out[4 * i + 0] = (uint8_t)(h_[i]);
            out[4 * i + 1] = (uint8_t)(h_[i] >> 8);
            out[4 * i + 2] = (uint8_t)(h_[i] >> 16);
            out[4 * i + 3] = (uint8_t)(h_[i] >> 24);
        }
    }

private:
    uint32_t h_[8];
    uint64_t t_;
    uint8_t buf_[64];
    size_t fill_;

    static const uint32_t* iv() {
        static const uint32_t IV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                       0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
        return IV;
    }
    static uint32_t ror(uint32_t x, int s) { return (x >> s) | (x << (32 - s)); }

    void compress(const uint8_t* p, bool last) {
        static const uint8_t S[10][16] = {
            {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
            {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
            {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
            {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
            {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
        const uint32_t* IV = iv();
        uint32_t m[16], v[16];
        for (int i = 0; i < 16; ++i)
            m[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
        for (int i = 0; i < 8; ++i) { v[i] = h_[i]; v[i + 8] = IV[i]; }
        v[12] ^= (uint32_t)t_;
        v[13] ^= (uint32_t)(t_ >> 32);
        if (last) v[14] = ~v[14];
#define MI_B2S_G(a, b, c, d, x, y)                                                    \
    do {                                                                              \
        v[a] += v[b] + (x); v[d] = ror(v[d] ^ v[a], 16); v[c] += v[d]; v[b] = ror(v[b] ^ v[c], 12); \
        v[a] += v[b] + (y); v[d] = ror(v[d] ^ v[a], 8);  v[c] += v[d]; v[b] = ror(v[b] ^ v[c], 7);  \
    } while (0)
        for (int r = 0; r < 10; ++r) {
            const uint8_t* s = S[r];
            MI_B2S_G(0, 4, 8, 12, m[s[0]], m[s[1]]);
            MI_B2S_G(1, 5, 9, 13, m[s[2]], m[s[3]]);
            MI_B2S_G(2, 6, 10, 14, m[s[4]], m[s[5]]);
            MI_B2S_G(3, 7, 11, 15, m[s[6]], m[s[7]]);
            MI_B2S_G(0, 5, 10, 15, m[s[8]], m[s[9]]);
            MI_B2S_G(1, 6, 11, 12, m[s[10]], m[s[11]]);
            MI_B2S_G(2, 7, 8, 13, m[s[12]], m[s[13]]);
            MI_B2S_G(3, 4, 9, 14, m[s[14]], m[s[15]]);
        }
#undef MI_B2S_G
        for (int i = 0; i < 8; ++i) h_[i] ^= v[i] ^ v[i + 8];
    }
};

}  // namespace mi_host
