// mi_zpack.hip -- compressed chunk packs ("zpacks"): every chunk of a pack coded ON ITS OWN as one standard LZ4 block, on the
// device (mi_pack_compress and the mi_zpack_* calls of include/makisu_mi.h), and such a pack decoded on the device into the
// plain blob an ordinary pack set holds (mi_packset_add_zblob, mi_packset_add_zpack); mi_zpack_check is the host's opinion
// (csrc/host_lz4.h).  What a chunk store keeps at rest and sends over the wire instead of plain bytes.
//
//   encode    (z_encode_block, csrc/mi_lz4_wave_enc.h: mi_zbatch.hip codes a batch's chunks where they lie with the same function)
//             one wave a chunk, a hash table of 4 096 32-bit positions in LDS (16 KiB, cleared per chunk; the workgroup IS the
//             wave).  The wave advances in STEPS of 64 consecutive positions [p, p + 64), capped at n - 12: lane i reads its 4
//             bytes and the slot (u32 * 2654435761) >> 20 AS THE TABLE WAS BEFORE THE STEP.  A candidate c counts if c < pos,
//             pos - c <= 65535 and the 4 bytes are equal (a table of zeros needs no "empty" mark).  No candidate: all 64
//             positions go into the table, the bytes stay pending literals.  Otherwise the LOWEST lane with a candidate wins (one
//             ballot), the match is extended 64 bytes a round up to n - 5, the sequence is written (lane 0: token and offset;
//             the wave: extension bytes and literals), p becomes the match's end and the step's positions BELOW the new p go
//             into the table.  Two lanes of a step in one slot: the greater position wins (atomicMax: the order the hardware
//             writes LDS in does not show).  The block is kept if it is smaller than n - (n >> 4); chunks under 13 bytes are raw;
//   layout    the wave writes into scratch at the chunk's WORST-CASE span (n + n / 255 + 16, rounded up to 16; the prefix sums
//             are taken on the host, which has the pack's entries); the stored sizes are known only then: mi_zrows.h's layout
//             (mi_plan.h's plan over round16(stored), the placing pass), and a destination-driven gather of 16 KiB tiles
//             (mi_gather.h, from absolute addresses: a raw chunk is gathered from the INPUT pack, a coded one from scratch)
//             into a blob of exactly its size;
//   decode    one wave an entry.  A raw entry is a copy in 16-byte units.  An LZ entry's sequences are taken in order: token and
//             offset are read by every lane alike, extension bytes 64 at a time with a ballot for the first below 255, the wave
//             copies literals and match bytes.  A match is PERIODIC with its offset: byte i is the byte (i mod offset) behind
//             op - offset, so every lane reads in front of the match, whatever the overlap.  The pad behind the chunk is zero;
//   verify    MI_ZPACK_VERIFY: the new blob decoded again into the scratch spans, the result through the ctx's own hashing
//             launcher (pass kShaBlobs), held against the entries' digests.
//
// BOUNDS.  The decoder is what parses bytes from elsewhere.  WRITES: a literal run or a match is copied only after
// len <= length - op was checked, the pad is [length, round16(length)): nothing outside [dst, dst + round16(length)), the
// entry's own span of the plain layout.  READS of the stored form: every index is compared with `stored` before the load
// (token, extension bytes, the two offset bytes, the literal run as a whole); the pad check reads [stored, round16(stored)),
// which the structural check on the host (offset + round16(stored) <= blob_bytes, always, before any upload) keeps inside the
// blob.  READS of the output: op - offset + (i mod offset) with 0 < offset <= op: inside [dst, dst + op).  A raw entry is read
// in aligned 16-byte units inside [src, src + round16(stored)).  The encoder reads src[pos .. pos + 3] with pos <= n - 12 and
// match bytes below n - 5: inside the chunk; it writes below the worst-case span (checked per sequence: a block that would pass
// it -- none does -- is stored raw).  The gather reads aligned units inside [src, src + round16(stored)) of the input pack or of
// a scratch span.  The hashing of the verify pass reads up to 67 bytes behind the last scratch span: DevBuf's 256 bytes.
#include "mi_internal.h"
#include "mi_gather.h"
#include "mi_lz4_wave.h"
#include "mi_zrows.h"
#include "mi_zentropy.h"
#include "host_blake2s.h"
#include "host_huff.h"
#include "host_lz4.h"
#include "host_sha256.h"

#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

using namespace mi;

namespace mi {

constexpr u64 kZNone = ~0ull;
// z_worst_span (what one chunk of n bytes takes in scratch): csrc/mi_lz4_wave_enc.h

// ---- encode ---------------------------------------------------------------------------------------------------------------------
// z_put_extension, z_encode_block: csrc/mi_lz4_wave_enc.h (mi_zbatch.hip codes with them too)
// rows[k]: digest | the chunk's offset in the pack's blob | chunk_index | length (the high half is written here: stored)
__global__ __launch_bounds__(64)
void zpack_encode_kernel(const u8* __restrict__ blob, u64* __restrict__ rows, const u64* __restrict__ w_off, u8* __restrict__ scratch, u64 n) {
    __shared__ u32 table[kZTable];
    z_encode_rows<ZLevel1>(blob, rows, w_off, scratch, n, table);
}

// ---- layout: mi_zrows.h's, over round16(stored) ----------------------------------------------------------------------------------
enum : int { kZTotBlob = 0, kZTotStored = 1, kZTotRaw = 2, kZTotChunk = 3, kZTotBad = 4 };

// per block of kPlanTile rows: the rounded-up stored bytes; into the totals: stored bytes, raw entries, chunk bytes
__global__ __launch_bounds__(kPlanBlock)
void zpack_block_sums_kernel(const u64* __restrict__ rows, u64 n, u64* __restrict__ block_bytes, u64* __restrict__ totals) {
    z_layout_sums<true>(rows, n, block_bytes, totals, kZTotStored, kZTotRaw, kZTotChunk);
}

// single block: exclusive scan of the block array in place; totals[kZTotBlob] = the blob's bytes
__global__ __launch_bounds__(kPlanBlock)
void zpack_block_offsets_kernel(u64* __restrict__ block_bytes, u64 n_blocks, u64* __restrict__ totals) {
    plan_block_offsets<false>(block_bytes, nullptr, n_blocks, &totals[kZTotBlob], nullptr);
}

// every entry's place in the new blob, where its stored form lies now (a raw chunk: in the input pack; a coded one: in its
// scratch span) and the row's offset word: from here on the rows are the zpack's entries
__global__ __launch_bounds__(kPlanBlock)
void zpack_place_kernel(u64* __restrict__ rows, const u64* __restrict__ w_off, u64 n, const u64* __restrict__ block_bytes, u64 pack_base,
                        u64 scratch_base, u64* __restrict__ e_src, u64* __restrict__ e_len, u64* __restrict__ e_dst) {
    z_place(rows, w_off, n, block_bytes, pack_base, scratch_base, e_src, e_len, e_dst);
}

// ---- gather: mi_gather.h's tile body over aligned sources (a raw chunk in the input pack, a coded one in scratch) -------------

__global__ __launch_bounds__(kGatherWG)
void zpack_gather_kernel(const u64* __restrict__ e_src, const u64* __restrict__ e_len, const u64* __restrict__ e_dst, u64 n_entries,
                         u64 blob_bytes, u8* __restrict__ blob) {
    gather_tile<true>(e_src, e_len, e_dst, n_entries, blob_bytes, blob);
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------
// z_get_extension, z_decode_block: csrc/mi_lz4_wave.h (mi_zset.hip decodes with them too)
// rows: the zpack's entries (offset into zblob | chunk_index | length, stored); p_off: where the plain chunk goes in `out`
__global__ __launch_bounds__(64)
void zpack_decode_kernel(const u8* __restrict__ zblob, const u64* __restrict__ rows, const u64* __restrict__ p_off, u64 n, u8* out,
                         u32* __restrict__ rule_out, u64* __restrict__ first_bad) {
    const int lane = threadIdx.x;
    for (u64 k = blockIdx.x; k < n; k += gridDim.x) {
        const u64* r = rows + kEntryWords * k;
        const u8* src = zblob + r[4];
        const u64 len = r[6] & 0xFFFFFFFFull, stored = r[6] >> 32;
        u8* dst = out + p_off[k];
        u32 rule = 0;
        if (stored == len) {                          // raw: aligned units, the bytes at and beyond the length zeroed in registers
            for (u64 u = (u64)lane * 16; u < len; u += 64 * 16) {
                u32x4 v = *(const u32x4*)(src + u);
                if (len - u < 16) v = keep_first_bytes(v, (u32)(len - u));
                *(u32x4*)(dst + u) = v;
            }
        } else {
            rule = z_decode_block(src, stored, dst, len, lane);
            if (len + lane < round16(len)) dst[len + lane] = 0;
        }
        const bool pad_set = stored + lane < round16(stored) && src[stored + lane] != 0;
        if (__ballot(pad_set) != 0 && rule == 0) rule = mi_host::kLz4PadNotZero;
        if (lane == 0) {
            rule_out[k] = rule;
            if (rule) atomicMin((unsigned long long*)first_bad, (unsigned long long)k);
        }
        __syncthreads();
    }
}

// MI_ZPACK_VERIFY: the digests of the decoded chunks against the rows'
__global__ __launch_bounds__(256)
void zpack_compare_kernel(const u8* __restrict__ got, const u64* __restrict__ rows, u64 n, u64* __restrict__ first_bad) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    digest_differs_mark(got, rows + kEntryWords * k, k, first_bad);
}

// ---- mi_zpack_read: mi_pack.hip's PackReader, restated -- the blob through two pinned windows, the copy of one overlapping the
// consumption of the other ---------------------------------------------------------------------------------------------------
constexpr u64 kZWinBytes = 8ull << 20;
struct MI_LOCAL ZpackReader {
    Stream stream;
    struct Win { PinBuf buf; u64 start = 0, len = 0; bool pending = false; Event ev; };
    Win win[2];
    int cur = 0;
    ZpackReader() = default;
    ZpackReader(ZpackReader&&) = default;
    ZpackReader& operator=(ZpackReader&&) = default;
    ~ZpackReader() { if (stream) (void)hipStreamSynchronize(stream); }    // no copy into a window is under way when the windows go
    int prepare(mi_ctx* c) {
        if (win[0].buf.p) return MI_OK;
        ZpackReader r;                                // whole or not at all
        HIPCHK(c, r.stream.create());
        for (auto& w : r.win) {
            HIPCHK(c, w.buf.ensure(kZWinBytes));
            HIPCHK(c, w.ev.create(hipEventDisableTiming));
        }
        *this = std::move(r);
        return MI_OK;
    }
    int read(mi_ctx* c, const u8* base, u64 total, u64 at, void* dst, u64 len) {
        if (!len) return MI_OK;
        const int rc = prepare(c);
        if (rc) return rc;
        auto prefetch = [&](Win& w, u64 from) -> int {
            w.len = 0;
            if (from >= total) return MI_OK;
            const u64 want = std::min(kZWinBytes, total - from);
            HIPCHK(c, hipMemcpyAsync(w.buf.p, base + from, want, hipMemcpyDeviceToHost, stream));
            HIPCHK(c, hipEventRecord(w.ev, stream));
            w.start = from;
            w.len = want;
            w.pending = true;
            return MI_OK;
        };
        u8* d = (u8*)dst;
        while (len) {
            Win* w = &win[cur];
            if (!(w->len && at >= w->start && at < w->start + w->len)) {
                Win* nx = &win[cur ^ 1];
                const bool follows = w->len && at == w->start + w->len;          // the reader streams
                if (nx->len && at >= nx->start && at < nx->start + nx->len) {
                    if (nx->pending) { HIPCHK(c, hipEventSynchronize(nx->ev)); nx->pending = false; }
                    cur ^= 1;
                    const int prc = prefetch(*w, nx->start + nx->len);           // the window just left takes what follows the new one
                    if (prc) return prc;
                    continue;
                }
                if (nx->pending) { HIPCHK(c, hipEventSynchronize(nx->ev)); nx->pending = false; }
                nx->len = 0;
                const u64 want = std::min(kZWinBytes, total - at);
                w->len = 0;
                HIPCHK(c, hipMemcpyAsync(w->buf.p, base + at, want, hipMemcpyDeviceToHost, stream));
                HIPCHK(c, hipStreamSynchronize(stream));
                w->start = at;
                w->len = want;
                w->pending = false;
                if (follows || want < len) {
                    const int prc = prefetch(*nx, at + want);
                    if (prc) return prc;
                }
            }
            const u64 take = std::min(len, w->start + w->len - at);
            memcpy(d, (const u8*)w->buf.p + (at - w->start), take);
            d += take;
            at += take;
            len -= take;
        }
        return MI_OK;
    }
};

}  // namespace mi

struct mi_zpack {
    mi_ctx* ctx = nullptr;
    mi_zpack_info info = {};
    DevBuf blob;                                 // info.blob_bytes + the slack every blob has
    std::vector<mi_zpack_entry> h_rows;          // on the host before mi_pack_compress returns and never written again
    ZpackReader reader;
};

namespace {

int does_not_fit(mi_ctx* c, const char* who, const char* what, hipError_t e, u64 bytes, u64 n) {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: %s of %llu bytes (%llu entries) does not fit: the device has "
                "%llu bytes free (%s); split the pack", who, what, (unsigned long long)bytes, (unsigned long long)n, (unsigned long long)free_b,
                hipGetErrorString(e));
}

void zpack_delete(mi_zpack* z) {
    mi_ctx* c = z->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    --c->live_children;
    delete z;
}

mi_zpack* zpack_new(mi_ctx* c) {
    mi_zpack* z = new mi_zpack();
    z->ctx = c;
    ++c->live_children;                                    // mi_zpack_free undoes it
    z->info.alg = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? MI_DIGEST_BLAKE2S : MI_DIGEST_SHA256;
    return z;
}

u32 wave_grid(u64 n) { return (u32)std::min<u64>(n, 1u << 20); }     // one wave an entry; more entries: the waves go round

// The structure of a zpack, on the host, before anything else looks at it: offsets on the 16-byte grid, ascending, without
// overlap, inside the blob (no 64-bit wrap), 0 < stored <= length.  false: *first_bad = the first entry that is not
bool structure_ok(u64 blob_bytes, const mi_zpack_entry* entries, u64 n, u64* first_bad) {
    u64 end = 0;                                       // where the previous entry's unit(s) end
    for (u64 k = 0; k < n; ++k) {
        const mi_zpack_entry& en = entries[k];
        const u64 span = round16(en.stored);
        if (en.stored != 0 && en.stored <= en.length && en.offset % 16 == 0 && en.offset >= end && en.offset <= blob_bytes &&
            span <= blob_bytes - en.offset) {
            end = en.offset + span;
            continue;
        }
        *first_bad = k;
        return false;
    }
    return true;
}

int refuse_structure(mi_ctx* c, const char* who, u64 blob_bytes, const mi_zpack_entry& en, u64 k) {
    return fail(c, MI_ERR_INVALID, "%s: entry %llu (offset %llu, %u bytes stored for %u) is off the 16-byte grid, overlaps the entry before it, "
                "leaves the blob of %llu bytes or states a stored size of 0 or above its length", who, (unsigned long long)k,
                (unsigned long long)en.offset, en.stored, en.length, (unsigned long long)blob_bytes);
}

// The entries lie on the host, the compressed blob on the device (a copy into it may still be queued on the ctx stream): the
// plain layout, the plain blob, the decode (mi_zpack_decode_plain below) -- and the set takes it as it takes any plain blob
// (mi_packset_adopt)
int add_compressed(mi_packset* s, mi_ctx* c, const char* who, const u8* d_zblob, const mi_zpack_entry* entries, u64 n, uint32_t flags,
                   double ms_upload, u64* first_bad) {
    std::vector<mi_pack_entry> plain(n);
    DevBuf d_plain;
    StreamDrain drain{c->stream};   // (goes first: the buffer above after it)
    u64 plain_bytes = 0, bad = kZNone;
    u32 rule = 0;
    const int rc = mi_zpack_decode_plain(c, who, d_zblob, entries, n, &d_plain, &plain_bytes, plain.data(), &bad, &rule, nullptr);
    if (rc) return rc;
    if (bad != kZNone) {                               // the plain blob goes with this frame: the set's table was not touched
        if (first_bad) *first_bad = bad;
        const mi_zpack_entry en = bad < n ? entries[bad] : mi_zpack_entry{};
        return fail(c, MI_ERR_INVALID, "%s: entry %llu (offset %llu, %u bytes stored for %u) does not decode: %s", who, (unsigned long long)bad,
                    (unsigned long long)en.offset, en.stored, en.length, mi_host::zrule_name(rule));
    }
    return mi_packset_adopt(s, who, &d_plain, plain_bytes, plain.data(), n, flags, ms_upload, first_bad);
}

}  // namespace

extern "C" {

// (hidden: mi_local.h) the decoding half of a compressed add, for mi_packset_add_z* here and for mi_zset.hip's verifications
int mi_zpack_decode_plain(mi_ctx* c, const char* who, const void* d_zblob, const mi_zpack_entry* entries, uint64_t n, void* plain_buf,
                          uint64_t* plain_bytes_out, mi_pack_entry* plain, uint64_t* bad_out, uint32_t* rule_out, double* ms_decode) {
    if (!c || !who || !d_zblob || !entries || !n || !plain_buf || !plain_bytes_out || !plain || !bad_out || !rule_out) return MI_ERR_INVALID;
    hipStream_t st = c->stream;
    DevBuf* d_plain = (DevBuf*)plain_buf;
    std::vector<u64> p_off(n);
    u64 plain_bytes = 0;
    for (u64 k = 0; k < n; ++k) {
        memcpy(plain[k].digest, entries[k].digest, 32);
        plain[k].offset = p_off[k] = plain_bytes;
        plain[k].chunk_index = entries[k].chunk_index;
        plain[k].length = entries[k].length;
        plain[k].reserved = 0;
        plain_bytes += round16(entries[k].length);
    }
    *plain_bytes_out = plain_bytes;
    *bad_out = kZNone;
    *rule_out = 0;
    DevBuf d_rows, d_poff, d_rule, d_bad;
    Event ev[2];
    StreamDrain drain{st};   // (goes first: the buffers above after it)
    const hipError_t e = d_plain->alloc_exact(plain_bytes);
    if (e != hipSuccess) return does_not_fit(c, who, "the plain blob", e, plain_bytes, n);
    for (auto& v : ev) HIPCHK(c, v.create());
    HIPCHK(c, d_rows.ensure(n * sizeof(mi_zpack_entry)));
    HIPCHK(c, d_poff.ensure(n * 8));
    HIPCHK(c, d_rule.ensure(n * 4));
    HIPCHK(c, d_bad.ensure(8));
    HIPCHK(c, hipMemcpyAsync(d_rows.p, entries, n * sizeof(mi_zpack_entry), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_poff.p, p_off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_bad.p, 0xFF, 8, st));
    // the entropy forms unwrapped first (mi_zentropy.h): d_rows is this call's copy, its form H rows then point at their inner
    // forms in `unwrap`'s scratch, which lives until the decode below has run.  No form H: one launch, nothing else
    ZhUnwrap unwrap;
    const int urc = unwrap.run(c, who, (u64)(size_t)d_zblob, d_rows.as<u64>() + 4, (u32)kEntryWords, d_rows.as<u64>() + 6, (u32)kEntryWords, n);
    if (urc) return urc;
    HIPCHK(c, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(zpack_decode_kernel, dim3(wave_grid(n)), dim3(64), 0, st, (const u8*)d_zblob, d_rows.as<u64>(), d_poff.as<u64>(), n,
                       d_plain->as<u8>(), d_rule.as<u32>(), d_bad.as<u64>());
    HIPCHK(c, hipEventRecord(ev[1], st));
    u64* h = c->h_word.as<u64>();
    HIPCHK(c, hipMemcpyAsync(h, d_bad.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (ms_decode) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
        *ms_decode = ms;
    }
    const u64 bad = h[0];
    if (bad != kZNone) {
        u32 rule = 0;
        if (bad < n) HIPCHK(c, hipMemcpy(&rule, d_rule.as<u32>() + bad, 4, hipMemcpyDeviceToHost));
        *bad_out = bad;
        *rule_out = rule;
    }
    unwrap.merge(bad_out, rule_out);
    return MI_OK;
}

// (hidden: mi_local.h) the structural host check every compressed add begins with, in mi_packset_add_zblob's words
int mi_zpack_structure(mi_ctx* c, const char* who, uint64_t blob_bytes, const mi_zpack_entry* entries, uint64_t n, uint64_t* first_bad) {
    u64 bad = 0;
    if (structure_ok(blob_bytes, entries, n, &bad)) return MI_OK;
    if (first_bad) *first_bad = bad;
    return refuse_structure(c, who, blob_bytes, entries[bad], bad);
}

// (hidden: mi_local.h) a zpack whose blob and rows the caller writes (mi_zset.hip's cut), and what the caller found out about it
int mi_zpack_alloc(mi_ctx* c, const char* who, uint64_t n_entries, uint64_t blob_bytes, mi_zpack** out, void** d_blob, mi_zpack_entry** h_rows) {
    if (!c || !who || !out || !d_blob || !h_rows) return MI_ERR_INVALID;
    *out = nullptr;
    mi_zpack* z = zpack_new(c);
    z->h_rows.resize(n_entries);
    const hipError_t e = n_entries ? z->blob.alloc_exact(blob_bytes) : hipSuccess;
    if (e != hipSuccess) {
        zpack_delete(z);
        return does_not_fit(c, who, "the compressed blob", e, blob_bytes, n_entries);
    }
    z->info.n_entries = n_entries;
    z->info.blob_bytes = blob_bytes;
    *out = z;
    *d_blob = z->blob.p;
    *h_rows = z->h_rows.data();
    return MI_OK;
}

void mi_zpack_set_result(mi_zpack* z, uint64_t stored_bytes, uint64_t n_raw, uint64_t chunk_bytes, uint32_t verified, double ms_compact,
                         double ms_verify, double ms_decode) {
    mi_zpack_info& zi = z->info;
    zi.stored_bytes = stored_bytes;
    zi.n_raw = n_raw;
    zi.chunk_bytes = chunk_bytes;
    zi.verified = verified;
    zi.ms_encode = 0;
    zi.ms_compact = ms_compact;
    zi.ms_verify = ms_verify;
    zi.ms_decode = ms_decode;
}

// (hidden: mi_local.h) the decode kernel behind whatever the ctx stream holds, for mi_zbatch.hip's verification
int mi_zpack_decode_enqueue(mi_ctx* c, const void* d_zblob, const uint64_t* d_rows, const uint64_t* d_poff, uint64_t n, void* d_out,
                            uint32_t* d_rule, uint64_t* d_first_bad) {
    if (!c || !d_zblob || !d_rows || !d_poff || !n || !d_out || !d_rule || !d_first_bad) return MI_ERR_INVALID;
    hipLaunchKernelGGL(zpack_decode_kernel, dim3(wave_grid(n)), dim3(64), 0, c->stream, (const u8*)d_zblob, d_rows, d_poff, n, (u8*)d_out, d_rule,
                       d_first_bad);
    return MI_OK;
}

void mi_zpack_set_encode_ms(mi_zpack* z, double ms_encode) { z->info.ms_encode = ms_encode; }

// (hidden: mi_local.h) a zpack where it lies: its ctx, its blob on the device (NULL for an empty one) and its rows on the host
int mi_zpack_device(const mi_zpack* z, mi_ctx** ctx, const void** d_blob, uint64_t* blob_bytes, const mi_zpack_entry** rows, uint64_t* n) {
    if (!z || !ctx || !d_blob || !blob_bytes || !rows || !n) return MI_ERR_INVALID;
    *ctx = z->ctx;
    *d_blob = z->blob.p;
    *blob_bytes = z->info.blob_bytes;
    *rows = z->h_rows.data();
    *n = z->info.n_entries;
    return MI_OK;
}

int mi_pack_compress(const mi_pack* p, uint32_t flags, mi_zpack** out) {
    if (out) *out = nullptr;
    if (!p || !out) return MI_ERR_INVALID;
    static const char* who = "mi_pack_compress";
    mi_ctx* c = mi_pack_ctx(p);
    if (flags & ~(uint32_t)(MI_ZPACK_VERIFY | MI_ZPACK_LEVEL2 | MI_ZPACK_ENTROPY)) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    const bool entropy = (flags & MI_ZPACK_ENTROPY) != 0;
    mi_pack_info pi;
    const void* d_pack = nullptr;
    u64 pack_bytes = 0;
    int rc;
    if ((rc = mi_pack_get_info(p, &pi)) || (rc = mi_pack_device(p, &d_pack, &pack_bytes))) return rc;
    const u64 n = pi.n_entries;
    HIPCHK(c, hipSetDevice(c->device));
    struct Owned { mi_zpack* z = nullptr; ~Owned() { if (z) zpack_delete(z); } } mine;     // (drains the ctx stream before the blob goes)
    mine.z = zpack_new(c);
    if (n == 0) {                                          // a valid zpack of nothing
        mine.z->info.verified = (flags & MI_ZPACK_VERIFY) ? 1 : 0;
        *out = mine.z;
        mine.z = nullptr;
        return MI_OK;
    }
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu entries, a pack holds fewer than 2^32", who, (unsigned long long)n);
    // the input's entries are on the host: the scratch spans' prefix sums are taken here
    std::vector<mi_zpack_entry>& rows = mine.z->h_rows;
    rows.resize(n);
    static_assert(sizeof(mi_zpack_entry) == sizeof(mi_pack_entry), "one layout");
    if ((rc = mi_pack_entries(p, (mi_pack_entry*)rows.data(), n))) return rc;
    std::vector<u64> w_off(n);
    u64 scratch_bytes = 0;
    for (u64 k = 0; k < n; ++k) {
        const u64 len = rows[k].length;
        if (len == 0 || rows[k].offset % 16 || rows[k].offset > pack_bytes || round16(len) > pack_bytes - rows[k].offset)
            return fail(c, MI_ERR_INVALID, "%s: entry %llu of the pack (offset %llu, %u bytes) has no bytes or leaves its blob of %llu bytes", who,
                        (unsigned long long)k, (unsigned long long)rows[k].offset, rows[k].length, (unsigned long long)pack_bytes);
        w_off[k] = scratch_bytes;
        scratch_bytes += z_worst_span(len);
    }
    hipStream_t s = c->stream;
    const u64 nb = (n + kPlanTile - 1) / kPlanTile;
    DevBuf d_rows, d_woff, d_scratch, d_scan, e_src, e_len, e_dst, d_rule, d_got, d_scratch2, d_hsrc, d_rows2;
    ZhUnwrap unwrap;                                       // (MI_ZPACK_ENTROPY with MI_ZPACK_VERIFY)
    Event ev[7];
    StreamDrain drain{s};   // (goes first: buffers and events after it)
    for (auto& e : ev) HIPCHK(c, e.create());
    hipError_t e = d_scratch.alloc_exact(scratch_bytes);
    if (e != hipSuccess) return does_not_fit(c, who, "the coder's scratch", e, scratch_bytes, n);
    if (entropy) {                                         // the entropy forms' spans: the same places in a second scratch
        if ((e = d_scratch2.alloc_exact(scratch_bytes)) != hipSuccess) return does_not_fit(c, who, "the entropy stage's scratch", e, scratch_bytes, n);
        HIPCHK(c, d_hsrc.ensure(n * 8));
    }
    HIPCHK(c, d_rows.ensure(n * sizeof(mi_zpack_entry)));
    HIPCHK(c, d_woff.ensure(n * 8));
    HIPCHK(c, d_scan.ensure((nb + 8) * 8));
    u64* block_bytes = d_scan.as<u64>();
    u64* totals = block_bytes + nb;                        // kZTot*
    HIPCHK(c, hipMemcpyAsync(d_rows.p, rows.data(), n * sizeof(mi_zpack_entry), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_woff.p, w_off.data(), n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(totals, 0, 4 * 8, s));
    HIPCHK(c, hipMemsetAsync(totals + kZTotBad, 0xFF, 8, s));
    HIPCHK(c, hipEventRecord(ev[0], s));
    if (flags & MI_ZPACK_LEVEL2) {                         // the denser parse (mi_zpack2.hip): the same rows, spans and scratch
        if ((rc = mi_zencode_l2_enqueue(c, d_pack, d_rows.as<u64>(), d_woff.as<u64>(), d_scratch.p, n, wave_grid(n))))
            return fail(c, rc, "%s: the level-2 coder was refused", who);
    } else {
        hipLaunchKernelGGL(zpack_encode_kernel, dim3(wave_grid(n)), dim3(64), 0, s, (const u8*)d_pack, d_rows.as<u64>(), d_woff.as<u64>(),
                           d_scratch.as<u8>(), n);
    }
    if (entropy)                                           // behind the coder: form H where it is smaller by more than a sixteenth (mi_zentropy.hip)
        zh_encode_enqueue(c, d_pack, d_rows.as<u64>(), d_woff.as<u64>(), d_scratch.p, d_scratch2.p, d_hsrc.as<u64>(), n, wave_grid(n));
    HIPCHK(c, hipEventRecord(ev[1], s));
    hipLaunchKernelGGL(zpack_block_sums_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, s, d_rows.as<u64>(), n, block_bytes, totals);
    hipLaunchKernelGGL(zpack_block_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, s, block_bytes, nb, totals);
    HIPCHK(c, hipEventRecord(ev[2], s));
    u64* h = c->h_word.as<u64>();
    HIPCHK(c, hipMemcpyAsync(h, totals, 4 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    mi_zpack_info& zi = mine.z->info;
    zi.n_entries = n;
    zi.blob_bytes = h[kZTotBlob];
    zi.stored_bytes = h[kZTotStored];
    zi.n_raw = h[kZTotRaw];
    zi.chunk_bytes = h[kZTotChunk];
    const u64 blob_bytes = zi.blob_bytes;
    if (blob_bytes < 16 * n || zi.stored_bytes > zi.chunk_bytes || zi.chunk_bytes != pi.chunk_bytes)
        return fail(c, MI_ERR_HIP, "%s: the plan counted %llu stored bytes in a blob of %llu for %llu chunk bytes (the pack states %llu)", who,
                    (unsigned long long)zi.stored_bytes, (unsigned long long)blob_bytes, (unsigned long long)zi.chunk_bytes,
                    (unsigned long long)pi.chunk_bytes);
    const u64 n_tiles = (blob_bytes + kGatherTile - 1) / kGatherTile;
    if (n_tiles >> 31) return fail(c, MI_ERR_INVALID, "%s: a blob of %llu bytes is more than one launch covers", who, (unsigned long long)blob_bytes);
    if ((e = mine.z->blob.alloc_exact(blob_bytes)) != hipSuccess) return does_not_fit(c, who, "the compressed blob", e, blob_bytes, n);
    HIPCHK(c, e_src.ensure(n * 8));
    HIPCHK(c, e_len.ensure(n * 8));
    HIPCHK(c, e_dst.ensure(n * 8));
    if (flags & MI_ZPACK_VERIFY) {
        HIPCHK(c, d_rule.ensure(n * 4));
        HIPCHK(c, d_got.ensure(n * 32));
    }
    HIPCHK(c, hipEventRecord(ev[3], s));
    hipLaunchKernelGGL(zpack_place_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, s, d_rows.as<u64>(), d_woff.as<u64>(), n, block_bytes,
                       (u64)(size_t)d_pack, (u64)(size_t)d_scratch.p, e_src.as<u64>(), e_len.as<u64>(), e_dst.as<u64>());
    if (entropy) zh_sources_enqueue(c, d_hsrc.as<u64>(), e_src.as<u64>(), n);          // a form H row: from the second scratch
    hipLaunchKernelGGL(zpack_gather_kernel, dim3((u32)n_tiles), dim3(kGatherWG), 0, s, e_src.as<u64>(), e_len.as<u64>(), e_dst.as<u64>(), n, blob_bytes,
                       mine.z->blob.as<u8>());
    HIPCHK(c, hipEventRecord(ev[4], s));
    if (flags & MI_ZPACK_VERIFY) {
        // the new blob decoded into the scratch spans (the gather has read them: same stream), hashed there.  The chunks' lengths
        // for the launcher: e_len is free again
        std::vector<u64> lens(n);
        for (u64 k = 0; k < n; ++k) lens[k] = rows[k].length;
        HIPCHK(c, hipMemcpyAsync(e_len.p, lens.data(), n * 8, hipMemcpyHostToDevice, s));
        const u64* v_rows = d_rows.as<u64>();
        if (entropy) {                                     // a COPY of the rows is unwrapped: d_rows are the zpack's entries
            HIPCHK(c, d_rows2.ensure(n * sizeof(mi_zpack_entry)));
            HIPCHK(c, hipMemcpyAsync(d_rows2.p, d_rows.p, n * sizeof(mi_zpack_entry), hipMemcpyDeviceToDevice, s));
            if ((rc = unwrap.run(c, who, (u64)(size_t)mine.z->blob.p, d_rows2.as<u64>() + 4, (u32)kEntryWords, d_rows2.as<u64>() + 6, (u32)kEntryWords, n)))
                return rc;
            if (unwrap.bad != kZNone)
                return fail(c, MI_ERR_IO, "%s: entry %llu: the entropy form just coded does not unwrap on the device: %s", who,
                            (unsigned long long)unwrap.bad, mi_host::zrule_name(unwrap.rule));
            v_rows = d_rows2.as<u64>();
        }
        hipLaunchKernelGGL(zpack_decode_kernel, dim3(wave_grid(n)), dim3(64), 0, s, mine.z->blob.as<u8>(), v_rows, d_woff.as<u64>(), n,
                           d_scratch.as<u8>(), d_rule.as<u32>(), totals + kZTotBad);
        HIPCHK(c, hipEventRecord(ev[6], s));
        const auto hash_items = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? launch_blake2s_items : launch_sha256_items;
        hash_items(kShaBlobs, d_scratch.as<u8>(), d_woff.as<u64>(), e_len.as<u64>(), nullptr, (u32)n, nullptr, c->heads.as<u32>(), nullptr, true,
                   d_got.as<u8>(), c->sha, c->prop.multiProcessorCount, scratch_bytes, s);
        hipLaunchKernelGGL(zpack_compare_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, s, d_got.as<u8>(), d_rows.as<u64>(), n,
                           totals + kZTotBad);
        HIPCHK(c, hipMemcpyAsync(h, totals + kZTotBad, 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipEventRecord(ev[5], s));
    // the entries to the host with the same synchronisation: mi_zpack_entries only reads from then on
    HIPCHK(c, hipMemcpyAsync(rows.data(), d_rows.p, n * sizeof(mi_zpack_entry), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    float ms = 0, ms2 = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    zi.ms_encode = ms;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[1], ev[2]));
    HIPCHK(c, hipEventElapsedTime(&ms2, ev[3], ev[4]));
    zi.ms_compact = (double)ms + ms2;
    if (flags & MI_ZPACK_VERIFY) {
        HIPCHK(c, hipEventElapsedTime(&ms, ev[4], ev[5]));
        zi.ms_verify = ms;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[4], ev[6]));
        zi.ms_decode = ms;
        const u64 bad = h[0];
        if (bad != kZNone) {
            const mi_zpack_entry row = bad < n ? rows[bad] : mi_zpack_entry{};
            return fail(c, MI_ERR_IO, "%s: entry %llu -- chunk row %llu, %u bytes stored for %u at blob offset %llu, digest %s -- does not decode on the "
                        "device to bytes that hash to its digest", who, (unsigned long long)bad, (unsigned long long)row.chunk_index, row.stored,
                        row.length, (unsigned long long)row.offset, hex32(row.digest).c_str());
        }
        zi.verified = 1;
    }
    *out = mine.z;
    mine.z = nullptr;
    return MI_OK;
}

int mi_zpack_get_info(const mi_zpack* z, mi_zpack_info* out) {
    if (!z || !out) return MI_ERR_INVALID;
    *out = z->info;
    return MI_OK;
}

int mi_zpack_entries(const mi_zpack* z, mi_zpack_entry* out, uint64_t cap) {
    if (!z || (!out && cap)) return MI_ERR_INVALID;
    const u64 n = z->info.n_entries;
    if (cap < n) return fail(z->ctx, MI_ERR_CAPACITY, "zpack entry buffer holds %llu rows, need %llu", (unsigned long long)cap, (unsigned long long)n);
    if (n) memcpy(out, z->h_rows.data(), n * sizeof(mi_zpack_entry));
    return MI_OK;
}

int mi_zpack_read(mi_zpack* z, uint64_t offset, void* dst, uint64_t len) {
    if (!z || (!dst && len)) return MI_ERR_INVALID;
    mi_ctx* c = z->ctx;
    if (offset > z->info.blob_bytes || len > z->info.blob_bytes - offset)
        return fail(c, MI_ERR_INVALID, "mi_zpack_read: [%llu, +%llu) is outside the blob of %llu bytes", (unsigned long long)offset,
                    (unsigned long long)len, (unsigned long long)z->info.blob_bytes);
    if (!len) return MI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return z->reader.read(c, z->blob.as<u8>(), z->info.blob_bytes, offset, dst, len);
}

void mi_zpack_free(mi_zpack* z) {
    if (z) zpack_delete(z);
}

int mi_zpack_count_forms(const mi_zpack* z, mi_zforms* out) {
    if (!z || !out) return MI_ERR_INVALID;
    mi_ctx* c = z->ctx;
    memset(out, 0, sizeof *out);
    const u64 n = z->info.n_entries;
    if (!n) return MI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf d_rows;
    StreamDrain drain{c->stream};
    HIPCHK(c, d_rows.ensure(n * sizeof(mi_zpack_entry)));
    HIPCHK(c, hipMemcpyAsync(d_rows.p, z->h_rows.data(), n * sizeof(mi_zpack_entry), hipMemcpyHostToDevice, c->stream));
    return zh_count_forms(c, (u64)(size_t)z->blob.p, d_rows.as<u64>() + 4, (u32)kEntryWords, d_rows.as<u64>() + 6, (u32)kEntryWords, n, nullptr, out);
}

int mi_packset_add_zblob(mi_packset* s, const void* blob, uint64_t blob_bytes, const mi_zpack_entry* entries, uint64_t n, uint32_t flags,
                         uint64_t* first_bad) {
    if (first_bad) *first_bad = 0;
    if (!s || (!blob && blob_bytes) || (!entries && n)) return MI_ERR_INVALID;
    static const char* who = "mi_packset_add_zblob";
    mi_ctx* c = nullptr;
    const uint64_t* tags = nullptr;
    const uint64_t* slots = nullptr;
    u64 t_cap = 0;
    int rc = mi_packset_table(s, who, &c, &tags, &slots, &t_cap);       // (a set in its sticky failed state: MI_ERR_STATE)
    if (rc) return rc;
    if (flags & ~(uint32_t)MI_PACKSET_VERIFY) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu entries, a pack holds fewer than 2^32", who, (unsigned long long)n);
    u64 bad = 0;
    if (!structure_ok(blob_bytes, entries, n, &bad)) {                   // before a byte is uploaded
        if (first_bad) *first_bad = bad;
        return refuse_structure(c, who, blob_bytes, entries[bad], bad);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0) return mi_packset_adopt(s, who, nullptr, 0, nullptr, 0, flags, 0, first_bad);
    DevBuf d_zblob;
    StreamDrain drain{c->stream};
    const hipError_t e = d_zblob.ensure(blob_bytes);
    if (e != hipSuccess) return does_not_fit(c, who, "the compressed blob", e, blob_bytes, n);
    double ms_upload = 0;
    rc = mi_packset_upload(s, d_zblob.p, blob, blob_bytes, &ms_upload);
    if (rc) return rc;
    return add_compressed(s, c, who, d_zblob.as<u8>(), entries, n, flags, ms_upload, first_bad);
}

int mi_packset_add_zpack(mi_packset* s, const mi_zpack* z, uint32_t flags) {
    if (!s || !z) return MI_ERR_INVALID;
    static const char* who = "mi_packset_add_zpack";
    mi_ctx* c = nullptr;
    const uint64_t* tags = nullptr;
    const uint64_t* slots = nullptr;
    u64 t_cap = 0;
    int rc = mi_packset_table(s, who, &c, &tags, &slots, &t_cap);
    if (rc) return rc;
    if (flags & ~(uint32_t)MI_PACKSET_VERIFY) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    if (z->ctx != c) return fail(c, MI_ERR_INVALID, "%s: the zpack belongs to another ctx; hand its bytes to mi_packset_add_zblob", who);
    const u64 n = z->info.n_entries;
    u64 bad = 0;
    if (!structure_ok(z->info.blob_bytes, z->h_rows.data(), n, &bad)) return refuse_structure(c, who, z->info.blob_bytes, z->h_rows[bad], bad);
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0) return mi_packset_adopt(s, who, nullptr, 0, nullptr, 0, flags, 0, nullptr);
    return add_compressed(s, c, who, z->blob.as<u8>(), z->h_rows.data(), n, flags, 0, nullptr);       // decoded where it lies
}

// Host logic: what the pulling side runs before it trusts a zpack.  No ctx, no GPU.  The order the device path finds things
// in: the structure of ALL entries first, then the first entry that does not decode (or whose pad is not zero), then the first
// whose bytes do not hash to its digest
int mi_zpack_check(const void* blob, uint64_t blob_bytes, const mi_zpack_entry* entries, uint64_t n, uint32_t alg, uint64_t* first_bad) {
    if (first_bad) *first_bad = 0;
    if ((!blob && blob_bytes) || (!entries && n)) return MI_ERR_INVALID;
    if (alg != MI_DIGEST_SHA256 && alg != MI_DIGEST_BLAKE2S) return MI_ERR_INVALID;
    u64 bad = 0;
    if (n >> 32 || !structure_ok(blob_bytes, entries, n, &bad)) {
        if (first_bad) *first_bad = bad;
        return MI_ERR_INVALID;
    }
    const u8* base = (const u8*)blob;
    std::vector<u8> plain, inner;                      // (inner: what an entropy form wraps, host_huff.h)
    u64 hash_bad = kZNone;
    for (u64 k = 0; k < n; ++k) {
        const mi_zpack_entry& en = entries[k];
        const u8* src = base + en.offset;
        const u8* chunk = src;
        bool ok = true;
        if (en.stored < en.length) {
            plain.resize(en.length);
            if (mi_host::is_form_h(src, en.stored, en.length) && en.length <= mi_host::kHuffMaxChunk) inner.resize(en.length);
            ok = mi_host::zform_decode(src, en.stored, plain.data(), en.length, inner.data()) == mi_host::kLz4Ok;
            chunk = plain.data();
        }
        for (u64 i = en.stored; i < round16(en.stored); ++i) ok = ok && src[i] == 0;
        if (!ok) {                                     // the smallest entry that does not decode: nothing behind it matters
            if (first_bad) *first_bad = k;
            return MI_ERR_INVALID;
        }
        if (hash_bad != kZNone) continue;
        u8 got[32];
        if (alg == MI_DIGEST_BLAKE2S) {
            mi_host::Blake2s hsh;
            hsh.update(chunk, en.length);
            hsh.final(got);
        } else {
            mi_host::Sha256 hsh;
            hsh.update(chunk, en.length);
            hsh.final(got);
        }
        if (memcmp(got, en.digest, 32) != 0) hash_bad = k;
    }
    if (hash_bad != kZNone) {
        if (first_bad) *first_bad = hash_bad;
        return MI_ERR_INVALID;
    }
    return MI_OK;
}

}  // extern "C"
