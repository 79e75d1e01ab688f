// host_inflate_spec.h -- the host half of the SPECULATIVE device inflate (mi_inflate_spec.hip): the cut of a member's deflate
// stream into pieces, the walk along the speculative rows from candidate 0 to the stream's end, and the live spans as the six-word
// span table of the indexed inflate with their windows' places.  Plain C++, no HIP: a stand-alone program may include it
// (tests/host_inflate_spec/driver.cpp does).
//
// THE PIECES.  The stream behind the gzip header (length hdr) is cut into pieces of `piece` member bytes; piece k covers the bits
// [8 (hdr + k piece), 8 (hdr + (k + 1) piece)) below 8 (n - 8).  cand[k] is piece k's CANDIDATE: 8 hdr for piece 0, otherwise the
// smallest bit of the piece at which a non-final dynamic block header parses, or ~0.  The speculative pass decodes from every
// candidate and leaves one row each (host_inflate.h InflateRow; `end` is a BIT here): kInfSegEnds -- a block header would begin at
// `end`, and `end` is its piece's candidate --, kInfSegFinal -- a BFINAL block was read, `end` is the next byte boundary, in bits --,
// kInfSegBroken, kInfSegTooLong.  Only the chain tells which rows count, and the walk trusts nothing of them: an end that is no
// candidate, does not advance or lies outside the stream is an error of the passes (kInfChainInternal), never an access out of bounds.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "host_inflate.h"

namespace mi_host {

// kSpecPiece: measured (profiles/gunzip_spec.txt) -- to a file, 65 536 beats 32 768 on the foreign stream by more than the run's spread, and
// its index is half the size; into a batch 32 768 is the faster by less
constexpr uint64_t kSpecPiece = 65536, kSpecPieceMin = 1024, kSpecPieceMax = 16777216, kSpecMaxPieces = 16384;
constexpr uint64_t kSpecRing = 32768;                 // ring entries (u16) a candidate: 65 536 bytes
// the speculative pass gives up (kInfSegTooLong, rule kInfSymbolCap) behind this many symbols a piece byte without a hit.  A guess:
// at a typical 9 bits a symbol 32 x piece symbols are 30 or more pieces of input; it bounds the time before a NOT_PARALLEL verdict.
// KEPT at 32 after profiles/gunzip_spec.txt, for want of a figure against it: the cap bound on no blob measured there (100 MB of zeros
// reached its verdict by the window rule after 0.39 M symbols and 384 ms, about 1 microsecond a 258-byte match); a stream of fixed
// blocks, the one input it exists for, was not measured
constexpr uint64_t kSpecSymbolsPerByte = 32;
constexpr uint64_t kSpecNone = ~0ull;

struct SpecPieces { uint64_t piece = 0, n_pieces = 0; };

// piece_bytes as asked (0: kSpecPiece) -> the piece used and the number of pieces of a member of n bytes with a header of hdr bytes
// (n >= hdr + 9); false: piece_bytes out of range.  The piece is doubled until there are at most kSpecMaxPieces
static inline bool spec_pieces(uint64_t n, uint64_t hdr, uint64_t piece_bytes, SpecPieces* out) {
    uint64_t piece = piece_bytes ? piece_bytes : kSpecPiece;
    if (piece < kSpecPieceMin || piece > kSpecPieceMax || n < hdr + 9) return false;
    const uint64_t stream = n - 8 - hdr;
    while ((stream + piece - 1) / piece > kSpecMaxPieces) piece *= 2;
    out->piece = piece;
    out->n_pieces = (stream + piece - 1) / piece;
    return true;
}

// the piece of bit b (8 hdr <= b)
static inline uint64_t spec_piece_of(uint64_t b, uint64_t hdr, uint64_t piece) { return (b / 8 - hdr) / piece; }

struct SpecSpan { uint64_t in_bit, end_bit, out_at, out_bytes, win_at, win_bytes, ring; };   // ring: the candidate whose ring holds its output

struct SpecChain {
    uint32_t end = kInfChainInternal, rule = 0;
    uint64_t span = 0, at_bit = 0, at_out = 0, bit = 0;   // the live span that stopped the walk (or the last one): its number, start, output offset
    uint64_t total = 0, n_live = 0;                       // output bytes and number of the live spans walked (before the merge)
    std::vector<SpecSpan> spans;                          // (kInfChainDone only) the merged spans, in chain order
    uint64_t windows_bytes = 0;
};

// the walk.  cand / rows: n_pieces of each, as the passes left them
static inline void spec_chain(const uint64_t* cand, const InflateRow* rows, uint64_t n_pieces, uint64_t hdr, uint64_t piece, uint64_t n, SpecChain* out) {
    *out = SpecChain();
    if (n_pieces == 0 || n < hdr + 9 || piece == 0 || cand[0] != 8 * hdr) return;
    const uint64_t stream_end = 8 * (n - 8);
    std::vector<SpecSpan> live;
    uint64_t k = 0, at = cand[0];
    for (;;) {
        const InflateRow& r = rows[k];
        out->span = live.size();
        out->at_bit = at;
        out->at_out = out->total;
        out->rule = r.rule;
        out->bit = r.bit;
        ++out->n_live;
        if (r.status == kInfSegBroken) { out->end = kInfChainCorrupt; return; }
        if (r.status == kInfSegTooLong) { out->end = kInfChainNotParallel; return; }
        if (r.status != kInfSegEnds && r.status != kInfSegFinal) { out->end = kInfChainInternal; return; }
        if (r.end <= at || r.end > 8 * n || r.out_bytes > (~0ull >> 1) - out->total) { out->end = kInfChainInternal; return; }
        live.push_back(SpecSpan{at, 0, out->total, r.out_bytes, 0, 0, k});
        out->total += r.out_bytes;
        if (r.status == kInfSegFinal) {
            out->rule = 0;
            if (r.end == stream_end) break;
            if (r.end < stream_end) out->end = kInfChainNotParallel;                  // more members, or bytes behind the trailer
            else { out->end = kInfChainCorrupt; out->rule = kInfInputEnds; out->bit = 8 * n; }   // no room for the trailer
            return;
        }
        if (r.end >= stream_end) { out->end = kInfChainInternal; return; }            // no piece lies there
        const uint64_t next = spec_piece_of(r.end, hdr, piece);
        if (next >= n_pieces || next <= k || cand[next] != r.end) { out->end = kInfChainInternal; return; }
        k = next;
        at = r.end;
    }
    // a live span without output is merged into the one in front: its start is no point (and neither is a start with no output in front of it)
    for (const SpecSpan& s : live) {
        if (!out->spans.empty() && (s.out_bytes == 0 || s.out_at == 0)) {
            SpecSpan& front = out->spans.back();
            if (front.out_bytes == 0) front.ring = s.ring;
            front.out_bytes += s.out_bytes;
        } else {
            out->spans.push_back(s);
        }
    }
    uint64_t win_at = 0;
    for (size_t i = 0; i < out->spans.size(); ++i) {
        SpecSpan& s = out->spans[i];
        s.end_bit = i + 1 < out->spans.size() ? out->spans[i + 1].in_bit : 0;
        s.win_bytes = i == 0 ? 0 : (s.out_at < kSpecRing ? s.out_at : kSpecRing);
        s.win_at = i == 0 ? 0 : win_at;
        win_at += (s.win_bytes + 15) / 16 * 16;
    }
    out->windows_bytes = win_at;
    out->end = kInfChainDone;
}

}  // namespace mi_host
