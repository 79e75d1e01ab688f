// driver.cpp -- test infrastructure: csrc/host_inflate_spec.h behind a line protocol, in a stand-alone program of its own (compiled plain
// and under AddressSanitizer + UBSan by tests/test_host_inflate_spec_driver.py; never loaded into another process).  The candidate
// table and the rows are heap allocations of EXACTLY n_pieces entries, so one entry too far is a report.
//   P <n> <hdr> <piece_bytes>                                         -> "P 1 <piece> <n_pieces>", or "P 0"
//   C <n> <hdr> <piece> <n_pieces> <cand>... <end out status rule bit>...
//       -> "C <chain end> <rule> <span> <at_bit> <at_out> <bit> <total> <n_live> <windows_bytes> <n_spans> <in_bit end_bit out_at out_bytes win_at win_bytes ring>..."
// (~0 is written as 18446744073709551615)
#include "host_inflate_spec.h"

#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>

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
        if (what == "P") {
            unsigned long long n = 0, hdr = 0, piece_bytes = 0;
            in >> n >> hdr >> piece_bytes;
            mi_host::SpecPieces pc;
            if (mi_host::spec_pieces(n, hdr, piece_bytes, &pc)) printf("P 1 %llu %llu\n", (unsigned long long)pc.piece, (unsigned long long)pc.n_pieces);
            else printf("P 0\n");
        } else if (what == "C") {
            unsigned long long n = 0, hdr = 0, piece = 0, np = 0;
            in >> n >> hdr >> piece >> np;
            uint64_t* cand = (uint64_t*)malloc(np ? np * sizeof(uint64_t) : 1);
            mi_host::InflateRow* rows = (mi_host::InflateRow*)malloc(np ? np * sizeof(mi_host::InflateRow) : 1);
            for (unsigned long long k = 0; k < np; ++k) { unsigned long long v = 0; in >> v; cand[k] = v; }
            for (unsigned long long k = 0; k < np; ++k) {
                unsigned long long end = 0, out = 0, bit = 0;
                unsigned status = 0, rule = 0;
                in >> end >> out >> status >> rule >> bit;
                rows[k] = mi_host::InflateRow{end, out, status, rule, bit};
            }
            mi_host::SpecChain ch;
            mi_host::spec_chain(cand, rows, np, hdr, piece, n, &ch);
            printf("C %u %u %llu %llu %llu %llu %llu %llu %llu %llu", ch.end, ch.rule, (unsigned long long)ch.span, (unsigned long long)ch.at_bit,
                   (unsigned long long)ch.at_out, (unsigned long long)ch.bit, (unsigned long long)ch.total, (unsigned long long)ch.n_live,
                   (unsigned long long)ch.windows_bytes, (unsigned long long)ch.spans.size());
            for (const mi_host::SpecSpan& s : ch.spans)
                printf(" %llu %llu %llu %llu %llu %llu %llu", (unsigned long long)s.in_bit, (unsigned long long)s.end_bit, (unsigned long long)s.out_at,
                       (unsigned long long)s.out_bytes, (unsigned long long)s.win_at, (unsigned long long)s.win_bytes, (unsigned long long)s.ring);
            printf("\n");
            free(cand);
            free(rows);
        }
    }
    return 0;
}
