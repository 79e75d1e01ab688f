// host_inflate.h -- the host half of the device inflate (mi_inflate_wave.h): the gzip header and trailer of a member,
// the rows the size pass leaves, the walk along the live chain and the cut of the live segments into rounds.  Plain C++, no HIP:
// a stand-alone program may include it (tests/host_inflate/chain_driver.cpp does).
//
// The size pass decodes from EVERY candidate and leaves one row each.  Only the chain tells which rows count: it starts at the
// first byte behind the header and follows each segment's end to the next candidate until a block with BFINAL ends the stream.
// A row that is not on the chain is never read, whatever it says.  The walk trusts nothing of the rows: an end that is no
// candidate, or one that does not move forward, is an error of the passes, not of the member.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace mi_host {

// why a segment is refused; the kernels and the model (tests/inflate_cases.py) report the same numbers
enum InflateRule : uint32_t {
    kInfOk = 0,
    kInfBlockType = 1,        // block type 3
    kInfStoredLen = 2,        // a stored block whose LEN is not ~NLEN
    kInfTooManyCodes = 3,     // HLIT > 286 or HDIST > 30
    kInfLengthCode = 4,       // a code-length code that is over-subscribed or incomplete
    kInfRepeat = 5,           // a repeat with no previous length, or a run that passes HLIT + HDIST
    kInfNoEndOfBlock = 6,     // no end-of-block code
    kInfCode = 7,             // a literal/length or distance code over-subscribed, or incomplete other than one code of length 1
    kInfSymbol = 8,           // literal/length 286 / 287, distance 30 / 31, or a bit pattern that has no symbol
    kInfInputEnds = 9,        // the input ends inside a block
    kInfDistance = 10,        // a distance that reaches before the segment's first byte
    kInfWindow = 11,          // output beyond the window
    kInfIndex = 12,           // (a span of an index, host_inflate_index.h) the span does not end where the index says
    kInfSymbolCap = 13,       // (a speculative span, host_inflate_spec.h) more symbols than the cap without reaching a candidate
};

static inline const char* inflate_rule_name(uint32_t rule) {
    static const char* const names[] = {"ok", "block type 3", "a stored block whose LEN is not ~NLEN", "HLIT above 286 or HDIST above 30",
                                        "a code-length code that is over-subscribed or incomplete",
                                        "a repeat with no previous length or a run that passes HLIT + HDIST", "no end-of-block code",
                                        "a literal/length or distance code that is over-subscribed or incomplete",
                                        "a symbol that does not exist", "input that ends inside a block",
                                        "a distance that reaches before the segment's first byte", "output beyond the window",
                                        "the span does not end where the index says",
                                        "more symbols than the speculative pass allows without reaching a block start it found"};
    return rule < sizeof names / sizeof names[0] ? names[rule] : "?";
}

// how the decode from a candidate ended
enum InflateStatus : uint32_t {
    kInfSegEnds = 0,          // an empty stored block with BFINAL 0: `end` is the byte behind it, a candidate by construction
    kInfSegFinal = 1,         // a block with BFINAL 1: `end` is the next byte boundary behind the deflate stream
    kInfSegBroken = 2,        // `rule` was broken at input bit `bit`
    kInfSegTooLong = 3,       // out_bytes would have passed the window (rule kInfWindow)
};

struct InflateRow {           // 32 bytes a candidate
    uint64_t end, out_bytes;
    uint32_t status, rule;
    uint64_t bit;
};
static_assert(sizeof(InflateRow) == 32, "an inflate row is 32 bytes");

static inline uint32_t inflate_le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the gzip header of gz[0, n) (RFC 1952): *header = its length, FEXTRA / FNAME / FCOMMENT / FHCRC walked.  false: a wrong magic,
// a method other than 8, a reserved flag bit, a wrong FHCRC, or a header that does not end inside the member
static inline bool gzip_header(const uint8_t* gz, uint64_t n, uint64_t* header) {
    if (n < 10 || gz[0] != 0x1f || gz[1] != 0x8b || gz[2] != 8 || (gz[3] & 0xE0)) return false;
    const uint32_t flg = gz[3];
    uint64_t at = 10;
    if (flg & 4) {                                    // FEXTRA: XLEN, then XLEN bytes
        if (n - at < 2) return false;
        const uint64_t xlen = (uint64_t)gz[at] | (uint64_t)gz[at + 1] << 8;
        at += 2;
        if (n - at < xlen) return false;
        at += xlen;
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1) {    // FNAME, FCOMMENT: up to and with a zero byte
        if (!(flg & bit)) continue;
        while (at < n && gz[at]) ++at;
        if (at >= n) return false;
        ++at;
    }
    if (flg & 2) {                                    // FHCRC: the low half of the CRC-32 of the header so far, held as zlib holds it
        if (n - at < 2) return false;
        uint32_t c = 0xFFFFFFFFu;
        for (uint64_t i = 0; i < at; ++i) {
            c ^= gz[i];
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        }
        if (((~c) & 0xFFFFu) != ((uint32_t)gz[at] | (uint32_t)gz[at + 1] << 8)) return false;
        at += 2;
    }
    *header = at;
    return true;
}

struct InflateSeg { uint64_t in_at, out_at, out_bytes, row; };   // a live segment: where it starts, where its bytes go, its row

enum InflateChainEnd : uint32_t {
    kInfChainDone = 0,        // the chain reached END at exactly n - 8
    kInfChainNotParallel = 1, // a live segment reaches before its start or inflates past the window, or END lies before n - 8
    kInfChainCorrupt = 2,     // a live segment broke another rule, or END lies behind n - 8
    kInfChainInternal = 3,    // the rows contradict the candidates: the passes are wrong, not the member
};

struct InflateChain {
    uint32_t end = kInfChainInternal, rule = 0;
    uint64_t at_in = 0, at_out = 0, bit = 0;          // the segment that stopped the walk (or the last one), the bit of its rule
    uint64_t total = 0;                               // output bytes of the live segments walked
    std::vector<InflateSeg> segs;
};

// the candidates are ascending; the index of `at` among them, or n_cand
static inline uint64_t inflate_find(const uint64_t* cand, uint64_t n_cand, uint64_t at) {
    uint64_t lo = 0, hi = n_cand;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (cand[mid] < at) lo = mid + 1; else hi = mid;
    }
    return lo < n_cand && cand[lo] == at ? lo : n_cand;
}

// the walk: from candidate `first` (the header's length) along the rows to END; n: the member's bytes
static inline void inflate_chain(const uint64_t* cand, const InflateRow* rows, uint64_t n_cand, uint64_t first, uint64_t n, InflateChain* out) {
    *out = InflateChain();
    uint64_t at = first;
    for (;;) {
        const uint64_t k = inflate_find(cand, n_cand, at);
        if (k == n_cand) { out->end = kInfChainInternal; out->at_in = at; out->at_out = out->total; return; }
        const InflateRow& r = rows[k];
        out->at_in = at;
        out->at_out = out->total;
        out->rule = r.rule;
        out->bit = r.bit;
        out->segs.push_back(InflateSeg{at, out->total, r.out_bytes, k});
        if (r.status == kInfSegBroken) {
            out->end = r.rule == kInfDistance ? kInfChainNotParallel : kInfChainCorrupt;
            return;
        }
        if (r.status == kInfSegTooLong) { out->end = kInfChainNotParallel; out->rule = kInfWindow; return; }
        if (r.status != kInfSegEnds && r.status != kInfSegFinal) { out->end = kInfChainInternal; return; }
        if (r.end <= at || r.end > n) { out->end = kInfChainInternal; return; }
        out->total += r.out_bytes;
        if (r.status == kInfSegFinal) {
            out->rule = 0;
            if (n >= 8 && r.end == n - 8) out->end = kInfChainDone;
            else if (n >= 8 && r.end < n - 8) out->end = kInfChainNotParallel;   // more members, or bytes behind the trailer
            else { out->end = kInfChainCorrupt; out->rule = kInfInputEnds; out->bit = 8 * n; }   // no room for the trailer
            return;
        }
        if (n < 8 || r.end > n - 8) {                                             // the segment ends where only the trailer may lie
            out->end = kInfChainCorrupt; out->rule = kInfInputEnds; out->bit = 8 * n;
            return;
        }
        at = r.end;
    }
}

// the live segments in rounds whose output fits `window` (every segment does): first[r] = the first segment of round r, and
// first[n_rounds] = the number of segments
static inline void inflate_rounds(const std::vector<InflateSeg>& segs, uint64_t window, std::vector<uint64_t>* first) {
    first->clear();
    uint64_t in_round = 0;
    for (uint64_t k = 0; k < segs.size(); ++k) {
        if (k == 0 || in_round + segs[k].out_bytes > window) { first->push_back(k); in_round = 0; }
        in_round += segs[k].out_bytes;
    }
    first->push_back(segs.size());
}

}  // namespace mi_host
