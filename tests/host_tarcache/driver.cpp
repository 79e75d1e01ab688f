// driver.cpp -- test infrastructure: csrc/host_tarcache.h in a stand-alone program of its own (tests/test_host_tarcache.py compiles it
// plain and under AddressSanitizer + UBSan).  Lines on stdin, one answer line each:
//   N k  b0 kind0  b1 kind1 ...   a new cache of k marked blocks; block b's byte i in the dense buffer is pattern(b, i)   -> "N k"
//   L off len                     lookup                                      -> "L held kind bytes_are_the_tar's cursor"
//   F off len tar_bytes           what a fetch of the range asks for          -> "F first bytes"
// The dense buffer is allocated at exactly 512 k bytes, so a lookup that hands out more than it holds is the sanitizer's to find.
#include "host_tarcache.h"

#include <stdio.h>
#include <string.h>

#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

static uint8_t pattern(uint64_t block, uint64_t i) { return (uint8_t)(block * 131 + i * 7 + 3); }

int main() {
    std::unique_ptr<uint64_t[]> blocks;
    std::unique_ptr<uint8_t[]> kinds, dense;
    mi_host::TarCache cache;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char what = 0;
        in >> what;
        if (what == 'N') {
            uint64_t k = 0;
            in >> k;
            blocks.reset(new uint64_t[k]);
            kinds.reset(new uint8_t[k]);
            dense.reset(new uint8_t[k * 512]);
            for (uint64_t i = 0; i < k; ++i) {
                unsigned kind = 0;
                in >> blocks[i] >> kind;
                kinds[i] = (uint8_t)kind;
                for (uint64_t j = 0; j < 512; ++j) dense[i * 512 + j] = pattern(blocks[i], j);
            }
            cache = mi_host::TarCache(blocks.get(), kinds.get(), dense.get(), k);
            printf("N %llu\n", (unsigned long long)k);
        } else if (what == 'L') {
            uint64_t off = 0, len = 0;
            in >> off >> len;
            uint8_t kind = 0;
            const uint8_t* p = cache.lookup(off, len, &kind);
            int same = 1;
            if (p)
                for (uint64_t i = 0; i < len; ++i)
                    if (p[i] != pattern((off + i) / 512, (off + i) % 512)) same = 0;
            printf("L %d %u %d %llu\n", p ? 1 : 0, (unsigned)kind, p ? same : 0, (unsigned long long)cache.cur);
        } else if (what == 'F') {
            uint64_t off = 0, len = 0, tar_bytes = 0, first = 0, bytes = 0;
            in >> off >> len >> tar_bytes;
            mi_host::tar_fetch_range(off, len, tar_bytes, &first, &bytes);
            printf("F %llu %llu\n", (unsigned long long)first, (unsigned long long)bytes);
        } else {
            printf("? 0\n");
        }
    }
    return 0;
}
