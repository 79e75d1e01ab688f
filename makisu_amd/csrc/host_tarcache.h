// host_tarcache.h -- plain C++, no HIP: the HEADER CACHE of a tar that lies on the device.  The device marked the
// 512-byte blocks that may be headers (mi_tarscan.hip: the blocks mi_tar.hip's checksum_ok holds for) and, behind a header of
// typeflag x, g, L or K, the next kTarMetaInline blocks as its body; their numbers came down ascending with their kinds and
// their bytes in one dense buffer.  The parser only moves forward, so a lookup walks a cursor; asked backwards or far ahead it
// searches.  A range is HELD when every block it touches is in the cache -- consecutive block numbers lie side by side in the
// dense buffer, so a held range is one pointer.  Anything else the caller fetches from the device.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mi_host {

constexpr uint8_t  kTarHeader = 1, kTarBody = 2;       // a marked block's kind: either, or both
constexpr uint64_t kTarBlock = 512;
constexpr int      kTarMetaInline = 2;                  // body blocks that travel with a meta header

struct TarCache {
    const uint64_t* blocks = nullptr;
    const uint8_t*  kinds = nullptr;
    const uint8_t*  dense = nullptr;
    uint64_t        n = 0;
    uint64_t        cur = 0;                            // the cursor: no block in front of it is >= the last block asked for

    TarCache() = default;
    TarCache(const uint64_t* blocks_, const uint8_t* kinds_, const uint8_t* dense_, uint64_t n_)
        : blocks(blocks_), kinds(kinds_), dense(dense_), n(n_) {}

    // the first k with blocks[k] >= j (n: none)
    uint64_t seek(uint64_t j) {
        if (cur == 0 || blocks[cur - 1] < j) {          // the answer is not in front of the cursor: a few steps may find it
            for (int step = 0; step < 8 && cur < n && blocks[cur] < j; ++step) ++cur;
            if (cur == n || blocks[cur] >= j) return cur;
        }
        uint64_t lo = 0, hi = n;                        // asked backwards, or far ahead
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (blocks[mid] < j) lo = mid + 1; else hi = mid;
        }
        return cur = lo;
    }

    // tar[off, off + len), len > 0: its bytes if every block it touches is held, else NULL (fetch it).  *kind (may be NULL): the
    // first block's kind
    const uint8_t* lookup(uint64_t off, uint64_t len, uint8_t* kind = nullptr) {
        if (len == 0 || off + len < off) return nullptr;
        const uint64_t j0 = off / kTarBlock, j1 = (off + len - 1) / kTarBlock;
        const uint64_t k = seek(j0);
        if (k >= n || blocks[k] != j0 || j1 - j0 >= n - k || blocks[k + (j1 - j0)] != j1) return nullptr;   // ascending, distinct: j1 there means all there
        if (kind) *kind = kinds[k];
        return dense + k * kTarBlock + off % kTarBlock;
    }
};

// what an on-demand fetch of tar[off, off + len) asks the device for: whole blocks, two at least (the end marker's two zero
// blocks cost one fetch), nothing behind the tar's end
inline void tar_fetch_range(uint64_t off, uint64_t len, uint64_t tar_bytes, uint64_t* first, uint64_t* bytes) {
    const uint64_t a = off / kTarBlock * kTarBlock;
    uint64_t e = (off + len + kTarBlock - 1) / kTarBlock * kTarBlock;
    if (e - a < 2 * kTarBlock) e = a + 2 * kTarBlock;
    if (e > tar_bytes) e = tar_bytes;
    *first = a;
    *bytes = e > a ? e - a : 0;
}

}  // namespace mi_host
