// driver.cpp -- test infrastructure: csrc/host_inflate_index.h behind a line protocol, in a stand-alone program of its own (compiled plain
// and under AddressSanitizer + UBSan by tests/test_host_inflate_index_driver.py; never loaded into another process).  Every buffer is a
// heap allocation of EXACTLY the size the line states, so one byte too far is a report.  Bytes travel as hex, - for none.
//   B <spacing> <hex member>            -> "B 1 <n_points> <n_blocks> <out_bytes> <hex sha256 of the inflation> <hex index>", or "B 0 <reason>"
//   K <hex index> <hex member or ->     -> "K <refusal number>"
#include "host_inflate_index.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>

static uint8_t* from_hex(const std::string& hex, size_t* n) {
    *n = hex == "-" ? 0 : hex.size() / 2;
    uint8_t* p = (uint8_t*)malloc(*n ? *n : 1);                   // exactly as long as the bytes (malloc(0) may be NULL)
    for (size_t i = 0; i < *n; ++i) {
        const char d[3] = {hex[2 * i], hex[2 * i + 1], 0};
        p[i] = (uint8_t)strtoul(d, nullptr, 16);
    }
    return p;
}

static void put_hex(const uint8_t* p, size_t n) {
    if (!n) printf("-");
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

int main() {
    std::string line;
    static char chunk[1 << 16];
    for (;;) {
        line.clear();
        while (fgets(chunk, sizeof chunk, stdin)) {
            line += chunk;
            if (!line.empty() && line.back() == '\n') break;
        }
        if (line.empty()) break;
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "B") {
            unsigned long long spacing = 0;
            std::string hex;
            in >> spacing >> hex;
            size_t n = 0;
            uint8_t* gz = from_hex(hex, &n);
            std::vector<uint8_t> ix;
            mi_host::IndexBuilt built;
            mi_host::Sha256 sha;
            std::string why;
            if (mi_host::index_build(gz, n, spacing, &ix, &built, &sha, &why)) {
                uint8_t digest[32];
                sha.final(digest);
                printf("B 1 %llu %llu %llu ", (unsigned long long)built.n_points, (unsigned long long)built.n_blocks, (unsigned long long)built.out_bytes);
                put_hex(digest, 32);
                printf(" ");
                put_hex(ix.data(), ix.size());
                printf("\n");
            } else {
                printf("B 0 %s\n", why.c_str());
            }
            free(gz);
        } else if (what == "K") {
            std::string hex_ix, hex_gz;
            in >> hex_ix >> hex_gz;
            size_t n_ix = 0, n = 0;
            uint8_t* ix = from_hex(hex_ix, &n_ix);
            uint8_t* gz = from_hex(hex_gz, &n);
            printf("K %d\n", mi_host::index_check(ix, n_ix, hex_gz == "-" ? nullptr : gz, n));
            free(ix);
            free(gz);
        }
    }
    return 0;
}
