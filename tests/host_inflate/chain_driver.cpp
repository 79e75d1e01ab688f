// chain_driver.cpp -- test infrastructure: csrc/host_inflate.h behind a line protocol, in a stand-alone program of its own (compiled
// plain and under AddressSanitizer + UBSan by tests/test_host_inflate_chain.py; never loaded into another process).  Every buffer is
// a heap allocation of EXACTLY the size the line states, so one byte too far is a report.
//   H <hex of the bytes, - for none>                  -> "H <1|0> <header length>"
//   C <n> <first> <window> <k> <k candidates> <k rows: end out_bytes status rule bit>
//                                                      -> "C <chain end> <rule> <at_in> <at_out> <total> <segments> <rounds> <segment starts...>"
#include "host_inflate.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>

int main() {
    static char line[1 << 20];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "H") {
            std::string hex;
            in >> hex;
            const size_t n = hex == "-" ? 0 : hex.size() / 2;
            uint8_t* gz = (uint8_t*)malloc(n ? n : 1);            // exactly as long as the bytes (malloc(0) may be NULL)
            for (size_t i = 0; i < n; ++i) gz[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
            uint64_t header = 0;
            const bool ok = mi_host::gzip_header(gz, n, &header);
            printf("H %d %llu\n", ok ? 1 : 0, (unsigned long long)(ok ? header : 0));
            free(gz);
        } else if (what == "C") {
            unsigned long long n = 0, first = 0, window = 0, k = 0;
            in >> n >> first >> window >> k;
            uint64_t* cand = (uint64_t*)malloc(k ? k * sizeof(uint64_t) : 1);
            mi_host::InflateRow* rows = (mi_host::InflateRow*)malloc(k ? k * sizeof(mi_host::InflateRow) : 1);
            for (unsigned long long i = 0; i < k; ++i) { unsigned long long c = 0; in >> c; cand[i] = c; }
            for (unsigned long long i = 0; i < k; ++i) {
                unsigned long long end = 0, out = 0, bit = 0;
                unsigned status = 0, rule = 0;
                in >> end >> out >> status >> rule >> bit;
                rows[i] = mi_host::InflateRow{end, out, status, rule, bit};
            }
            mi_host::InflateChain chain;
            mi_host::inflate_chain(cand, rows, k, first, n, &chain);
            std::vector<uint64_t> rounds;
            size_t n_rounds = 0;
            if (chain.end == mi_host::kInfChainDone) {
                mi_host::inflate_rounds(chain.segs, window, &rounds);
                n_rounds = rounds.size() - 1;
            }
            printf("C %u %u %llu %llu %llu %zu %zu", chain.end, chain.rule, (unsigned long long)chain.at_in, (unsigned long long)chain.at_out,
                   (unsigned long long)chain.total, chain.segs.size(), n_rounds);
            for (const mi_host::InflateSeg& s : chain.segs) printf(" %llu", (unsigned long long)s.in_at);
            printf("\n");
            free(cand);
            free(rows);
        }
    }
    return 0;
}
