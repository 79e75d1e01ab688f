// host_inflate_index.h -- the INDEX OF CHECKPOINTS of one gzip member: its format, the builder (zlib's raw inflate with
// Z_BLOCK, zran's technique) and the checker every untrusted index passes before anything of it reaches the device.  Plain C++ plus
// zlib, no HIP: a stand-alone program may include it (tests/host_inflate_index/driver.cpp does).
//
// A CHECKPOINT is a deflate block boundary: the member's bit number of the block's first header bit, the output offset there, and the
// (up to) 32 KiB of output in front of it.  The SPAN between two checkpoints is independent of every other: its output size is
// known, and a match that reaches before it reads the checkpoint's window (mi_inflate_wave.h kSpan).
//
// FORMAT, little-endian, a pure function of (member, spacing):
//   header, 64 bytes   "MIGZIX01" | u64 n (member bytes) | u64 out_bytes | u32 CRC-32 | u32 ISIZE (both from the trailer) |
//                      u64 gzip header length | u64 n_points (>= 1) | u64 spacing | u64 windows_bytes
//   n_points rows, 32  u64 in_bit | u64 out_at | u64 win_at (offset in the window area, a multiple of 16) |
//                      u32 win_bytes = min(32 768, out_at) | u32 zero
//   the window area    each window: the win_bytes of output in front of its point, raw, zero-padded to 16; in the points' order
//
// (An index may also come out of a speculative plan -- mi_inflate_buffer_spec, DESIGN 4.23: the same format, passes the same checker and
// drives the same calls, but its points are the candidates that plan's chain passed and its spacing field is the piece used.  It is NOT
// the builder's index for any spacing.)
//
// THE POINT RULE.  Point 0 is (8 * header length, 0) with no window.  After every non-final block, ending at bit b with output o: if
// o - the last point's out_at >= spacing, (b, o) is a new point.  An empty stored block is a block like any other.  Spacing 0 means
// kIndexSpacing; spacing 1 makes every boundary at which output has advanced a point.  A point at which the output is already
// complete (only blocks without output follow: the host leg's final empty block) heads a span with nothing to do and is dropped:
// every point but point 0 has out_at < out_bytes.  Only a single member that ends at n - 8 is indexed.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "host_inflate.h"
#include "host_sha256.h"

namespace mi_host {

constexpr uint64_t kIndexSpacing = 262144, kIndexWindow = 32768, kIndexHeader = 64, kIndexRow = 32;
static const char kIndexMagic[9] = "MIGZIX01";

struct IndexPoint { uint64_t in_bit, out_at, win_at; uint32_t win_bytes, zero; };
static_assert(sizeof(IndexPoint) == 32, "an index row is 32 bytes");

struct IndexHead { uint64_t n, out_bytes; uint32_t crc, isize; uint64_t header, n_points, spacing, windows_bytes; };

static inline uint64_t index_le64(const uint8_t* p) { uint64_t v = 0; for (int k = 7; k >= 0; --k) v = v << 8 | p[k]; return v; }
static inline void index_put64(uint8_t* p, uint64_t v) { for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (8 * k)); }
static inline void index_put32(uint8_t* p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k)); }

static inline void index_head(const uint8_t* ix, IndexHead* h) {      // (ix holds kIndexHeader bytes)
    h->n = index_le64(ix + 8); h->out_bytes = index_le64(ix + 16); h->crc = inflate_le32(ix + 24); h->isize = inflate_le32(ix + 28);
    h->header = index_le64(ix + 32); h->n_points = index_le64(ix + 40); h->spacing = index_le64(ix + 48); h->windows_bytes = index_le64(ix + 56);
}
static inline IndexPoint index_point(const uint8_t* ix, uint64_t k) { // (row k lies inside ix)
    const uint8_t* r = ix + kIndexHeader + kIndexRow * k;
    return IndexPoint{index_le64(r), index_le64(r + 8), index_le64(r + 16), inflate_le32(r + 24), inflate_le32(r + 28)};
}

// ---- the checker -----------------------------------------------------------------------------------------------------------------
enum IndexRefusal : int {
    kIxOk = 0,
    kIxMagic = 1,             // shorter than a header, or another magic
    kIxSizes = 2,             // no point, a member too short for its header and trailer, ISIZE that is not out_bytes mod 2^32, spacing 0,
                              // or a total length that is not 64 + 32 n_points + windows_bytes
    kIxFirstPoint = 3,        // point 0 is not (8 * header length, 0) without a window
    kIxInBit = 4,             // in_bit not strictly ascending
    kIxOutAt = 5,             // out_at not strictly ascending
    kIxInBitEnd = 6,          // in_bit at or behind 8 (n - 8)
    kIxOutAtEnd = 7,          // out_at at or behind out_bytes
    kIxWinBytes = 8,          // win_bytes is not min(32 768, out_at), or the row's last word is not zero
    kIxWindow = 9,            // a window out of bounds, not aligned to 16, or overlapping the one in front
    kIxMember = 10,           // the member given is not the one indexed: n, the header's length, CRC-32 or ISIZE differ
};

static inline const char* index_refusal_text(int r) {
    static const char* const names[] = {"ok", "no index: too short or a wrong magic", "sizes that contradict each other", "a first point that is not the stream's start",
                                        "bit offsets that do not ascend", "output offsets that do not ascend", "a point behind the deflate stream",
                                        "a point behind the output", "a window of the wrong size", "a window out of bounds, unaligned or overlapping",
                                        "the index of another member"};
    return r >= 0 && (size_t)r < sizeof names / sizeof names[0] ? names[r] : "?";
}

// ix[0, bytes): an index nobody vouches for.  gz (may be NULL): the member it is said to belong to, n its bytes
static inline int index_check(const uint8_t* ix, uint64_t bytes, const uint8_t* gz, uint64_t n) {
    if (!ix || bytes < kIndexHeader || memcmp(ix, kIndexMagic, 8) != 0) return kIxMagic;
    IndexHead h;
    index_head(ix, &h);
    const uint64_t body = bytes - kIndexHeader;
    if (h.n_points == 0 || h.n_points > body / kIndexRow || h.windows_bytes != body - kIndexRow * h.n_points) return kIxSizes;
    if (h.header < 10 || h.n < 9 || h.header > h.n - 9 || h.spacing == 0 || h.isize != (uint32_t)h.out_bytes || h.n > (~0ull >> 4)) return kIxSizes;
    uint64_t win_end = 0;
    IndexPoint prev = {};
    for (uint64_t k = 0; k < h.n_points; ++k) {
        const IndexPoint p = index_point(ix, k);
        if (k == 0) {
            if (p.in_bit != 8 * h.header || p.out_at != 0 || p.win_at != 0 || p.win_bytes != 0 || p.zero != 0) return kIxFirstPoint;
        } else {
            if (p.in_bit <= prev.in_bit) return kIxInBit;
            if (p.out_at <= prev.out_at) return kIxOutAt;
            if (p.in_bit >= 8 * (h.n - 8)) return kIxInBitEnd;
            if (p.out_at >= h.out_bytes) return kIxOutAtEnd;
            if (p.win_bytes != (p.out_at < kIndexWindow ? p.out_at : kIndexWindow) || p.zero != 0) return kIxWinBytes;
            if ((p.win_at & 15) || p.win_at < win_end || p.win_at > h.windows_bytes || p.win_bytes > h.windows_bytes - p.win_at) return kIxWindow;
            win_end = p.win_at + ((uint64_t)p.win_bytes + 15) / 16 * 16;      // (the pad may end behind the area: nobody reads it)
        }
        prev = p;
    }
    if (gz) {
        uint64_t header = 0;
        if (n != h.n || !gzip_header(gz, n, &header) || header != h.header || inflate_le32(gz + n - 8) != h.crc || inflate_le32(gz + n - 4) != h.isize)
            return kIxMember;
    }
    return kIxOk;
}

// ---- the builder -----------------------------------------------------------------------------------------------------------------
struct IndexBuilt { uint64_t n_points = 0, n_blocks = 0, out_bytes = 0, windows_bytes = 0, spacing = 0; };

static inline uint32_t index_crc(uint32_t c, const uint8_t* p, uint64_t n) {
    while (n) { const uInt t = n > (1u << 30) ? (1u << 30) : (uInt)n; c = (uint32_t)crc32(c, p, t); p += t; n -= t; }
    return c;
}

// the index of gz[0, n) into *ix (cleared first); sha (may be NULL) sees the member's whole inflation, in order.  false: *why says
// what about the member cannot be indexed
static inline bool index_build(const uint8_t* gz, uint64_t n, uint64_t spacing, std::vector<uint8_t>* ix, IndexBuilt* built, Sha256* sha,
                               std::string* why) {
    ix->clear();
    if (spacing == 0) spacing = kIndexSpacing;
    uint64_t header = 0;
    if (!gz || !gzip_header(gz, n, &header)) { *why = "no gzip header (magic, method 8, no reserved flag, complete)"; return false; }
    if (n < header + 8 + 1) { *why = "the member ends behind its header: no stream, no trailer"; return false; }
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) { *why = "zlib: inflateInit2 failed"; return false; }
    std::vector<uint8_t> ring(2 * kIndexWindow), windows;
    std::vector<IndexPoint> points(1, IndexPoint{8 * header, 0, 0, 0, 0});
    uint64_t fill = 0, in = header, out = 0, blocks = 0;     // ring[0, fill) ends with the last min(out, 32 768 .. 65 536) bytes of output
    uint32_t crc = 0;
    int rc = Z_OK;
    bool ok = false;
    for (;;) {
        if (z.avail_in == 0 && in < n) {
            const uint64_t take = n - in < (1u << 30) ? n - in : (1u << 30);
            z.next_in = const_cast<Bytef*>(gz + in);
            z.avail_in = (uInt)take;
            in += take;
        }
        if (fill == ring.size()) {                            // the last 32 768 bytes move to the front
            memmove(ring.data(), ring.data() + fill - kIndexWindow, kIndexWindow);
            fill = kIndexWindow;
        }
        z.next_out = ring.data() + fill;
        z.avail_out = (uInt)(ring.size() - fill);
        const uint64_t room = z.avail_out;
        rc = inflate(&z, Z_BLOCK);
        const uint64_t made = room - z.avail_out;
        crc = index_crc(crc, ring.data() + fill, made);
        if (sha) sha->update(ring.data() + fill, (size_t)made);
        fill += made;
        out += made;
        if (rc == Z_STREAM_END) { ok = true; break; }
        if (rc == Z_BUF_ERROR) {                              // no progress: there is always room, so the input has run out
            if (z.avail_in == 0 && in < n) continue;
            break;                                            // ... inside the stream
        }
        if (rc != Z_OK) break;
        if ((z.data_type & 128) && !(z.data_type & 64)) {     // a block has ended, and it was not the last one
            ++blocks;
            const uint64_t consumed = in - z.avail_in;
            const uint64_t bit = 8 * consumed - (uint64_t)(z.data_type & 7);
            if (out - points.back().out_at >= spacing) {
                const uint32_t wb = (uint32_t)(out < kIndexWindow ? out : kIndexWindow);
                points.push_back(IndexPoint{bit, out, (uint64_t)windows.size(), wb, 0});
                windows.insert(windows.end(), ring.data() + fill - wb, ring.data() + fill);
                windows.resize((windows.size() + 15) / 16 * 16, 0);
            }
        }
    }
    const uint64_t end = in - z.avail_in;
    const char* msg = z.msg;
    std::string zmsg = msg ? msg : "the stream does not end";
    inflateEnd(&z);
    if (!ok) { *why = "corrupt deflate stream at input offset " + std::to_string(end) + " (output offset " + std::to_string(out) + "): " + zmsg; return false; }
    if (end > n - 8) { *why = "the deflate stream ends at " + std::to_string(end) + ": no room for the trailer in " + std::to_string(n) + " bytes"; return false; }
    if (end < n - 8) {
        const bool more = n - end >= 8 + 10 && gz[end + 8] == 0x1f && gz[end + 9] == 0x8b;
        *why = (more ? "a second member begins at offset " : "trailing bytes behind the trailer at offset ") + std::to_string(end + 8) +
               ": only a single member is indexed";
        return false;
    }
    const uint32_t want_crc = inflate_le32(gz + n - 8), want_isize = inflate_le32(gz + n - 4);
    if (crc != want_crc || (uint32_t)out != want_isize) {
        char buf[200];
        snprintf(buf, sizeof buf, "%llu bytes with CRC-32 %08x, the trailer states %u (mod 2^32) and %08x", (unsigned long long)out, crc, want_isize, want_crc);
        *why = buf;
        return false;
    }
    if (points.size() > 1 && points.back().out_at == out) {   // a span without output
        windows.resize((size_t)points.back().win_at);
        points.pop_back();
    }
    ix->resize((size_t)(kIndexHeader + kIndexRow * points.size() + windows.size()));
    uint8_t* p = ix->data();
    memcpy(p, kIndexMagic, 8);
    index_put64(p + 8, n); index_put64(p + 16, out); index_put32(p + 24, want_crc); index_put32(p + 28, want_isize);
    index_put64(p + 32, header); index_put64(p + 40, points.size()); index_put64(p + 48, spacing); index_put64(p + 56, windows.size());
    for (size_t k = 0; k < points.size(); ++k) {
        uint8_t* r = p + kIndexHeader + kIndexRow * k;
        index_put64(r, points[k].in_bit); index_put64(r + 8, points[k].out_at); index_put64(r + 16, points[k].win_at);
        index_put32(r + 24, points[k].win_bytes); index_put32(r + 28, 0);
    }
    if (!windows.empty()) memcpy(p + kIndexHeader + kIndexRow * points.size(), windows.data(), windows.size());
    if (built) *built = IndexBuilt{(uint64_t)points.size(), blocks, out, (uint64_t)windows.size(), spacing};
    return true;
}

}  // namespace mi_host
