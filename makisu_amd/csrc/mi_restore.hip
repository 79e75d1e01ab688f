// mi_restore.hip -- the consuming side of the chunk packs (mi_pack.hip): packs resident on the device and addressed by digest
// (a PACK SET: mi_packset_*), and the files of a batch ASSEMBLED from such a set and their recipes (mi_batch_add_recipes) --
// the inverse of pack_gather_kernel plus a digest-addressed lookup.  What feeds a batch from packs instead of from disk.
//
//   set       every added pack's blob lies in device memory of its own (exactly its bytes + DevBuf's 256 bytes of slack).  Its
//             entries go into ONE open-addressing table (mi_slot_table.h, the one mi_zset.hip holds too): tag = the digest's
//             first 8 bytes (0 is stored as 1, 0 = empty), slot = {digest 32 | the chunk's ABSOLUTE device address 8 | its
//             length 4 | 4}.  The insert runs in probe-then-verify rounds across a kernel boundary (no thread compares digest
//             bytes another thread of the same launch may still be writing); a digest met again is kept once; the same digest
//             with another length is reported and makes the set unusable (the table is not rolled back).  Rebuilt at twice the
//             size when it passes half full: the new table is filled before the old one goes, so a failed growth leaves the
//             set as it was;
//   upload    mi_packset_add_blob: after the structural check on the host (no lying entry reaches a kernel) the blob goes up
//             through two pinned windows, filling one while the other's copy runs -- PackReader's mirror image;
//   verify    MI_PACKSET_VERIFY: the blob's entries through the ctx's own hashing launcher (pass kShaBlobs) as MI_PACK_VERIFY
//             does it; one kernel holds digests and pad bytes against the entries;
//   resolve   mi_batch_add_recipes: 36 bytes a row go up (digest, length); a lookup kernel finds every row's source address --
//             tag first, then all 32 bytes -- the smallest bad row by atomicMin.  The rows' arena offsets (an exclusive scan
//             of the lengths per file) are taken on the host in the pass that sums the files' sizes for the placement;
//   assemble  destination-driven like the gather: [first file's offset, last file's end rounded up to 16) is cut into tiles of
//             kRestoreTile bytes, a workgroup takes a tile, the rows that reach into it are found by the wave search over
//             the rows' arena offsets and lie in LDS (a tile of more than kRestoreRows rows -- rows of under 16 bytes on
//             average -- reads them from global memory instead: the same code, instantiated twice).  Every lane owns aligned
//             16-byte units.  A unit inside one row: one 16-byte load from src + (unit - row start) at whatever alignment that
//             has, one aligned dwordx4 store.  Any other unit is put together: the tail of the row it begins in, then every
//             row that begins inside it (up to sixteen 1-byte rows), each with one 16-byte load from the ROW'S OWN FIRST
//             BYTE, masked and shifted into place; bytes that belong to no file (the gap between files, the tail behind the
//             last) are zero.  A lane issues all its loads before its first store.  Bytes in front of the first file's
//             offset and behind the range are never written;
//   verify    MI_RECIPE_VERIFY: the assembled ranges through the hashing launcher (base = the arena, items = the rows' arena
//             offsets and lengths), the digests held against the recipes' on the device.
//
// READ BOUND.  Every load of the assemble kernel is 16 bytes long and begins at src + a with 0 <= a < len, src the address of
// an entry of a blob and len its length: it never begins in front of its entry -- so never in front of the blob, whose first
// entry may sit at the allocation's first byte; in particular the head of a row that begins inside a unit is fetched by a load
// that starts AT the row's source, not before it -- and it ends at src + a + 15 <= src + len + 14 <= src + round16(len) + 15:
// at most 15 bytes behind offset + round16(length) <= blob_bytes, inside the 256 bytes of slack behind every blob.  The
// structural check (offset + round16(length) <= blob_bytes, always, on the host) is what makes the entry's address a bound.
// The hashing of the set's verify pass reads up to 67 bytes behind the blob's last entry (the same slack), that of the recipes'
// up to 67 bytes behind the last restored file (the arena's 4 KiB).
#include "mi_plan.h"
#include "mi_slot_table.h"

#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

using namespace mi;

namespace mi {

constexpr u64 kNone = ~0ull;

// ---- the set: entries -> table records, the verification, the table ------------------------------------------------------
// entries as they were uploaded -> what the table takes (digest | base + offset | length) and what the hashing launcher takes
__global__ __launch_bounds__(256)
void packset_unpack_kernel(const u64* __restrict__ entries, u64 n, u64 base, u64* __restrict__ recs, u64* __restrict__ off,
                           u64* __restrict__ len) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const u64* e = entries + kEntryWords * k;
    u64* r = recs + kSlotWords * k;
    r[0] = e[0]; r[1] = e[1]; r[2] = e[2]; r[3] = e[3];
    r[4] = base + e[4];
    r[5] = e[6] & 0xFFFFFFFFull;
    off[k] = e[4];
    len[k] = e[6] & 0xFFFFFFFFull;
}

// MI_PACKSET_VERIFY: the digests the device computed against the entries', and the pad bytes behind every chunk
__global__ __launch_bounds__(256)
void packset_check_kernel(const u8* __restrict__ got, const u64* __restrict__ entries, const u8* __restrict__ blob, u64 n,
                          u64* __restrict__ first_bad) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const u64* g = (const u64*)(got + 32 * k);
    const u64* e = entries + kEntryWords * k;
    bool ok = g[0] == e[0] && g[1] == e[1] && g[2] == e[2] && g[3] == e[3];
    const u64 len = e[6] & 0xFFFFFFFFull;
    for (u64 i = e[4] + len; i < e[4] + round16(len); ++i) ok = ok && blob[i] == 0;
    if (!ok) atomicMin((unsigned long long*)first_bad, (unsigned long long)k);
}

// ---- resolve: every recipe row's source address ---------------------------------------------------------------------------
// found[r]: the length the set holds the row's digest with (0: it does not hold it); src[r] only where that is the row's own
__global__ __launch_bounds__(256)
void restore_lookup_kernel(const u8* __restrict__ digests, const u32* __restrict__ lengths, u64 n, const u64* __restrict__ tags,
                           const u64* __restrict__ slots, u64 mask, u64* __restrict__ src, u64* __restrict__ len64,
                           u32* __restrict__ found, u64* __restrict__ first_bad) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const u8* d = digests + 32 * r;
    const u32 len = lengths[r];
    u64 at = 0;
    u32 held = 0;
    if (len) {
        const u64 slot = slot_table_find(tags, slots, mask, d);
        if (slot != kSlotNone) {
            held = (u32)slots[kSlotWords * slot + 5];
            if (held == len) at = slots[kSlotWords * slot + 4];
        }
    }
    src[r] = at;
    len64[r] = len;
    found[r] = held;
    if (!at) atomicMin((unsigned long long*)first_bad, (unsigned long long)r);
}

// ---- assemble ------------------------------------------------------------------------------------------------------------------
constexpr int kRestoreWG = 256;
constexpr u32 kRestoreTile = 16384;                  // bytes of the destination a workgroup writes
constexpr int kRestorePer = kRestoreTile / 16 / kRestoreWG;   // units per lane
constexpr u32 kRestoreRows = 1024;                   // rows of a tile that LDS holds (a tile of rows of 16 bytes and more has no more)

// masks of the first n bytes (n < 16) of a 16-byte unit held as (lo, hi).  Plain values on purpose: written with references to
// lo and hi the compiler turns the choice between them into an indexed access to a two-element array in scratch
static __device__ __forceinline__ u64 keep_lo(u32 n) { return n >= 8 ? ~0ull : n ? ~0ull >> (64 - 8 * n) : 0ull; }
static __device__ __forceinline__ u64 keep_hi(u32 n) { return n > 8 ? ~0ull >> (64 - 8 * (n - 8)) : 0ull; }

// the rows of one tile, in LDS (kLds) or where the resolve left them (g_* point at the tile's first row)
template <bool kLds>
static __device__ __forceinline__ u32 restore_tile(u8* __restrict__ arena, const u64* __restrict__ g_dst, const u64* __restrict__ g_src,
                                                  const u64* __restrict__ g_len, const u64* s_dst, const u64* s_src, const u32* s_len,
                                                  u32 cnt, u64 tile0, u64 tile1) {
#define row_dst(i) (kLds ? s_dst[i] : g_dst[i])
#define row_src(i) (kLds ? s_src[i] : g_src[i])
#define row_len(i) (kLds ? s_len[i] : (u32)g_len[i])
    u64 ld[kRestorePer];                             // where the unit's first 16 bytes come from
    u32 valid[kRestorePer], row[kRestorePer];        // how many of them are the row's; the row the unit begins in
#pragma unroll
    for (int j = 0; j < kRestorePer; ++j) {
        const u64 u = tile0 + ((u32)threadIdx.x + (u32)j * kRestoreWG) * 16;
        ld[j] = 0;
        valid[j] = 0;
        row[j] = 0;
        if (u >= tile1) continue;
        u32 lo = 0, hi = cnt;                         // the last row that begins at or before the unit
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (row_dst(mid) <= u) lo = mid; else hi = mid;
        }
        const u64 o = u - row_dst(lo);
        const u64 len = row_len(lo);
        row[j] = lo;
        if (o < len) {                                // (else: the gap behind a file's last row)
            ld[j] = row_src(lo) + o;
            valid[j] = len - o < 16 ? (u32)(len - o) : 16u;
        }
    }
    u32x4 v[kRestorePer];
#pragma unroll
    for (int j = 0; j < kRestorePer; ++j) {
        v[j] = u32x4{0, 0, 0, 0};
        if (valid[j]) v[j] = load16_global_unaligned(ld[j]);
    }
    u32 joined = 0;
#pragma unroll
    for (int j = 0; j < kRestorePer; ++j) {
        const u64 u = tile0 + ((u32)threadIdx.x + (u32)j * kRestoreWG) * 16;
        if (u >= tile1 || valid[j] == 16) continue;
        // the unit is not one row's: the tail of the row it begins in (or nothing), then the rows that begin inside it
        u64 lo = (((u64)v[j].y << 32) | v[j].x) & keep_lo(valid[j]), hi = (((u64)v[j].w << 32) | v[j].z) & keep_hi(valid[j]);
        u32 rows_in = valid[j] ? 1u : 0u;
        for (u32 nx = row[j] + 1; nx < cnt; ++nx) {
            const u64 d = row_dst(nx);
            if (d >= u + 16) break;
            const u32 q = (u32)(d - u);               // 1..15: where the row begins in the unit
            const u32 len = row_len(nx);
            const u32 m = len < 16 - q ? len : 16 - q;
            const u32x4 w = load16_global_unaligned(row_src(nx));      // from the row's first byte: never in front of it
            const u64 wl = (((u64)w.y << 32) | w.x) & keep_lo(m), wh = (((u64)w.w << 32) | w.z) & keep_hi(m);
            // ... moved up by q bytes (q >= 8: the low half lands in the high one; a shift by 64 is never formed)
            lo |= q >= 8 ? 0ull : wl << (8 * q);
            hi |= q >= 8 ? wl << (8 * (q - 8)) : (wh << (8 * q)) | (wl >> (64 - 8 * q));
            ++rows_in;
        }
        v[j] = u32x4{(u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)};
        if (rows_in > 1) ++joined;
    }
#pragma unroll
    for (int j = 0; j < kRestorePer; ++j) {
        const u64 u = tile0 + ((u32)threadIdx.x + (u32)j * kRestoreWG) * 16;
        if (u < tile1) *(u32x4*)(arena + u) = v[j];
    }
    return joined;
#undef row_dst
#undef row_src
#undef row_len
}

// d0: the first file's arena offset (a multiple of kFileAlign, = r_dst[0]); d1: the last file's end rounded up to 16
__global__ __launch_bounds__(kRestoreWG)
void restore_assemble_kernel(u8* __restrict__ arena, const u64* __restrict__ r_dst, const u64* __restrict__ r_src,
                             const u64* __restrict__ r_len, u64 n_rows, u64 d0, u64 d1, u64* __restrict__ n_joined) {
    __shared__ u64 s_dst[kRestoreRows];
    __shared__ u64 s_src[kRestoreRows];
    __shared__ u32 s_len[kRestoreRows];
    __shared__ u64 s_k[2];
    __shared__ u32 s_joined;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 tile0 = d0 + (u64)blockIdx.x * kRestoreTile;
    const u64 tile1 = tile0 + kRestoreTile < d1 ? tile0 + kRestoreTile : d1;
    if (threadIdx.x == 0) s_joined = 0;
    // the first and the last row that reach into the tile: the last one that begins at or before the tile's first / last byte
    if (wave < 2) {
        const u64 k = wave_last_le(r_dst, n_rows, wave == 0 ? tile0 : tile1 - 1, lane);
        if (lane == 0) s_k[wave] = k;
    }
    __syncthreads();
    const u64 k0 = s_k[0];
    const u32 cnt = (u32)(s_k[1] - k0 + 1);           // at most kRestoreTile + 1: a row has a byte at least
    const bool in_lds = cnt <= kRestoreRows;
    if (in_lds)
        for (u32 i = threadIdx.x; i < cnt; i += kRestoreWG) {
            s_dst[i] = r_dst[k0 + i];
            s_src[i] = r_src[k0 + i];
            s_len[i] = (u32)r_len[k0 + i];
        }
    __syncthreads();
    const u32 joined = in_lds ? restore_tile<true>(arena, nullptr, nullptr, nullptr, s_dst, s_src, s_len, cnt, tile0, tile1)
                              : restore_tile<false>(arena, r_dst + k0, r_src + k0, r_len + k0, nullptr, nullptr, nullptr, cnt, tile0, tile1);
    if (joined) atomicAdd(&s_joined, joined);
    __syncthreads();
    if (threadIdx.x == 0 && s_joined) atomicAdd((unsigned long long*)n_joined, (unsigned long long)s_joined);
}

// MI_RECIPE_VERIFY: the digests of the assembled ranges against the recipes'
__global__ __launch_bounds__(256)
void restore_compare_kernel(const u8* __restrict__ got, const u8* __restrict__ want, u64 n, u64* __restrict__ first_bad) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    digest_differs_mark(got, (const u64*)(want + 32 * r), r, first_bad);
}

// ---- mi_packset_add_blob's way up: two pinned windows, one filled by the host while the other's copy runs ------------------
constexpr u64 kSetWinBytes = 8ull << 20;
struct MI_LOCAL SetUploader {
    Stream stream;
    PinBuf buf[2];
    Event ev[2];
    bool busy[2] = {false, false};
    ~SetUploader() { if (stream) (void)hipStreamSynchronize(stream); }    // no copy out of a window is under way when the windows go
    int prepare(mi_ctx* c, u64 bytes) {
        const u64 want = std::min<u64>(kSetWinBytes, (bytes + 4095) & ~(u64)4095);    // a small blob does not pay for 16 MiB of pinned memory
        HIPCHK(c, stream.create());
        for (int i = 0; i < 2; ++i) {
            HIPCHK(c, buf[i].ensure(want));
            HIPCHK(c, ev[i].create(hipEventDisableTiming));
        }
        return MI_OK;
    }
    int pieces(mi_ctx* c, u8* dst, const u8* src, u64 bytes) {
        const u64 win = std::min(buf[0].bytes, buf[1].bytes);
        int w = 0;
        for (u64 at = 0; at < bytes; w ^= 1) {
            const u64 take = std::min(win, bytes - at);
            if (busy[w]) { HIPCHK(c, hipEventSynchronize(ev[w])); busy[w] = false; }
            memcpy(buf[w].p, src + at, take);
            HIPCHK(c, hipMemcpyAsync(dst + at, buf[w].p, take, hipMemcpyHostToDevice, stream));
            HIPCHK(c, hipEventRecord(ev[w], stream));
            busy[w] = true;
            at += take;
        }
        return MI_OK;
    }
    // blocking; whatever happened, no copy is in flight when it returns
    int upload(mi_ctx* c, u8* dst, const void* src, u64 bytes) {
        if (!bytes) return MI_OK;
        int rc = prepare(c, bytes);
        if (rc == MI_OK) rc = pieces(c, dst, (const u8*)src, bytes);
        const hipError_t e = stream ? hipStreamSynchronize(stream) : hipSuccess;
        busy[0] = busy[1] = false;
        if (rc == MI_OK && e != hipSuccess) rc = fail(c, MI_ERR_HIP, "mi_packset_add_blob: upload: %s", hipGetErrorString(e));
        return rc;
    }
};

}  // namespace mi

struct mi_packset {
    mi_ctx* ctx = nullptr;
    mi_packset_info info = {};
    std::vector<DevBuf> blobs;                   // every added pack's bytes, each in memory of its own: the table points into them
    SlotTable table;                             // digest -> the chunk's device address and length (mi_slot_table.h)
    DevBuf bad_cell;                             // MI_PACKSET_VERIFY's answer
    std::string broken;                          // sticky: the first message of an add that left the table in doubt
    SetUploader up;
};

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int set_state(const mi_packset* s, const char* who) {
    if (s->broken.empty()) return MI_OK;
    return fail(s->ctx, MI_ERR_STATE, "%s: the pack set is unusable since: %s", who, s->broken.c_str());
}

// the structural half of mi_pack_check: the entries lie inside the blob on 16-byte offsets, ascending, without overlap
int check_structure(mi_ctx* c, const char* who, u64 blob_bytes, const mi_pack_entry* entries, u64 n, u64* first_bad) {
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu entries, a pack holds fewer than 2^32", who, (unsigned long long)n);
    u64 end = 0;                                       // where the previous entry's unit(s) end
    for (u64 k = 0; k < n; ++k) {
        const mi_pack_entry& en = entries[k];
        const u64 span = round16(en.length);
        if (en.offset % 16 == 0 && en.offset >= end && en.offset <= blob_bytes && span <= blob_bytes - en.offset) {
            end = en.offset + span;
            continue;
        }
        if (first_bad) *first_bad = k;
        return fail(c, MI_ERR_INVALID, "%s: entry %llu (offset %llu, %u bytes) is off the 16-byte grid, overlaps the entry before it or leaves "
                    "the blob of %llu bytes", who, (unsigned long long)k, (unsigned long long)en.offset, en.length, (unsigned long long)blob_bytes);
    }
    return MI_OK;
}

// The blob lies on the device (the copy into it may still be queued on the ctx stream); entries are structurally sound.
// Verification, the table, the set's counters.  Until the insert begins every failure leaves the set as it was.
int set_add(mi_packset* s, const char* who, DevBuf&& blob, u64 blob_bytes, const mi_pack_entry* entries, u64 n, uint32_t flags,
            u64* first_bad) {
    mi_ctx* c = s->ctx;
    hipStream_t st = c->stream;
    DevBuf mine = std::move(blob);                     // freed on every early return -- after the stream has drained
    DevBuf d_ent, d_recs, d_off, d_len, d_got;
    StreamDrain drain{st};   // (goes first: the buffers above after it)
    s->info.ms_verify = s->info.ms_insert = 0;
    if (n == 0) {                                      // a pack of nothing
        ++s->info.n_packs;
        return MI_OK;
    }
    HIPCHK(c, d_ent.ensure(n * sizeof(mi_pack_entry)));
    HIPCHK(c, d_recs.ensure(n * kSlotWords * 8));
    HIPCHK(c, d_off.ensure(n * 8));
    HIPCHK(c, d_len.ensure(n * 8));
    HIPCHK(c, hipMemcpyAsync(d_ent.p, entries, n * sizeof(mi_pack_entry), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(packset_unpack_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_ent.as<u64>(), n, (u64)(size_t)mine.p,
                       d_recs.as<u64>(), d_off.as<u64>(), d_len.as<u64>());
    u64* h = c->h_word.as<u64>();
    if (flags & MI_PACKSET_VERIFY) {
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(c, d_got.ensure(n * 32));
        HIPCHK(c, s->bad_cell.ensure(8));
        u64* d_bad = s->bad_cell.as<u64>();
        HIPCHK(c, hipMemsetAsync(d_bad, 0xFF, 8, st));
        const auto hash_items = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? launch_blake2s_items : launch_sha256_items;
        hash_items(kShaBlobs, mine.as<u8>(), d_off.as<u64>(), d_len.as<u64>(), nullptr, (u32)n, nullptr, c->heads.as<u32>(), nullptr, true,
                   d_got.as<u8>(), c->sha, c->prop.multiProcessorCount, blob_bytes, st);
        hipLaunchKernelGGL(packset_check_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_got.as<u8>(), d_ent.as<u64>(),
                           mine.as<u8>(), n, d_bad);
        HIPCHK(c, hipMemcpyAsync(h, d_bad, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        s->info.ms_verify = ms_since(t0);
        const u64 bad = h[0];
        if (bad != kNone) {
            if (first_bad) *first_bad = bad;
            const mi_pack_entry en = bad < n ? entries[bad] : mi_pack_entry{};
            return fail(c, MI_ERR_INVALID, "%s: entry %llu (offset %llu, %u bytes) does not hash to its digest on the device, or the pad "
                        "behind it is not zero", who, (unsigned long long)bad, (unsigned long long)en.offset, en.length);
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    int rc = s->table.make_room(c, n, "pack set");
    if (rc) return rc;
    u64 sums[3], conflict = kNone;                     // (a plain record has no stored size: only sums[0] says anything)
    rc = s->table.insert(c, d_recs.as<u64>(), n, sums, &conflict, "pack set");
    s->table.count += sums[0];
    s->info.n_digests = s->table.count;
    s->blobs.push_back(std::move(mine));               // the table may point into it by now
    if (rc == MI_OK && conflict != kNone) {
        if (first_bad) *first_bad = conflict;
        rc = fail(c, MI_ERR_INVALID, "%s: entry %llu (%u bytes) has a digest the set holds with another length -- unverified input; the set "
                  "is unusable from here on", who, (unsigned long long)conflict, conflict < n ? entries[conflict].length : 0u);
    }
    if (rc) {                                          // the table is not rolled back: sticky
        s->broken = ctx_error(c);
        return rc;
    }
    s->info.ms_insert = ms_since(t0);
    ++s->info.n_packs;
    s->info.n_entries += n;
    s->info.blob_bytes += blob_bytes;
    return MI_OK;
}

int blob_does_not_fit(mi_ctx* c, const char* who, hipError_t e, u64 blob_bytes, u64 n) {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: a blob of %llu bytes (%llu entries) does not fit: the device "
                "has %llu bytes free (%s)", who, (unsigned long long)blob_bytes, (unsigned long long)n, (unsigned long long)free_b,
                hipGetErrorString(e));
}

}  // namespace

extern "C" {

int mi_packset_create(mi_ctx* c, uint64_t entries_hint, mi_packset** out) {
    if (!c || !out) return MI_ERR_INVALID;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    if (entries_hint >> 40) return fail(c, MI_ERR_INVALID, "mi_packset_create: entries_hint %llu", (unsigned long long)entries_hint);
    mi_packset* s = new mi_packset();
    s->ctx = c;
    ++c->live_children;                                 // mi_packset_free undoes it
    s->info.alg = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? MI_DIGEST_BLAKE2S : MI_DIGEST_SHA256;
    u64 cap = 1024;
    while (cap < entries_hint * 2) cap <<= 1;
    int rc = s->table.alloc(c, cap);
    if (rc == MI_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, MI_ERR_HIP, "mi_packset_create: the table's memset failed");
    if (rc) { mi_packset_free(s); return rc; }
    *out = s;
    return MI_OK;
}

int mi_packset_add_blob(mi_packset* s, const void* blob, uint64_t blob_bytes, const mi_pack_entry* entries, uint64_t n, uint32_t flags,
                        uint64_t* first_bad) {
    if (first_bad) *first_bad = 0;
    if (!s || (!blob && blob_bytes) || (!entries && n)) return MI_ERR_INVALID;
    mi_ctx* c = s->ctx;
    int rc = set_state(s, "mi_packset_add_blob");
    if (rc) return rc;
    if (flags & ~(uint32_t)MI_PACKSET_VERIFY) return fail(c, MI_ERR_INVALID, "mi_packset_add_blob: unknown flags %#x", flags);
    rc = check_structure(c, "mi_packset_add_blob", blob_bytes, entries, n, first_bad);      // before a byte is uploaded
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    s->info.ms_upload = 0;
    DevBuf d_blob;
    if (blob_bytes && n) {
        const hipError_t e = d_blob.alloc_exact(blob_bytes);
        if (e != hipSuccess) return blob_does_not_fit(c, "mi_packset_add_blob", e, blob_bytes, n);
        const auto t0 = std::chrono::steady_clock::now();
        rc = s->up.upload(c, d_blob.as<u8>(), blob, blob_bytes);
        if (rc) return rc;
        s->info.ms_upload = ms_since(t0);
    }
    return set_add(s, "mi_packset_add_blob", std::move(d_blob), n ? blob_bytes : 0, entries, n, flags, first_bad);
}

int mi_packset_add_pack(mi_packset* s, const mi_pack* p, uint32_t flags) {
    if (!s || !p) return MI_ERR_INVALID;
    mi_ctx* c = s->ctx;
    int rc = set_state(s, "mi_packset_add_pack");
    if (rc) return rc;
    if (flags & ~(uint32_t)MI_PACKSET_VERIFY) return fail(c, MI_ERR_INVALID, "mi_packset_add_pack: unknown flags %#x", flags);
    if (mi_pack_ctx(p) != c) return fail(c, MI_ERR_INVALID, "mi_packset_add_pack: the pack belongs to another ctx; hand its bytes to mi_packset_add_blob");
    mi_pack_info pi;
    const void* src = nullptr;
    u64 blob_bytes = 0;
    if ((rc = mi_pack_get_info(p, &pi)) || (rc = mi_pack_device(p, &src, &blob_bytes))) return rc;
    const u64 n = pi.n_entries;
    std::vector<mi_pack_entry> rows(n);
    if ((rc = mi_pack_entries(p, rows.data(), n))) return rc;
    rc = check_structure(c, "mi_packset_add_pack", blob_bytes, rows.data(), n, nullptr);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    s->info.ms_upload = 0;
    DevBuf d_blob;
    if (blob_bytes && n) {
        const hipError_t e = d_blob.alloc_exact(blob_bytes);
        if (e != hipSuccess) return blob_does_not_fit(c, "mi_packset_add_pack", e, blob_bytes, n);
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t ce = hipMemcpyAsync(d_blob.p, src, blob_bytes, hipMemcpyDeviceToDevice, c->stream);
        if (ce == hipSuccess) ce = hipStreamSynchronize(c->stream);
        if (ce != hipSuccess) return fail(c, MI_ERR_HIP, "mi_packset_add_pack: the device-to-device copy: %s", hipGetErrorString(ce));
        s->info.ms_upload = ms_since(t0);
    }
    return set_add(s, "mi_packset_add_pack", std::move(d_blob), n ? blob_bytes : 0, rows.data(), n, flags, nullptr);
}

int mi_packset_get_info(const mi_packset* s, mi_packset_info* out) {
    if (!s || !out) return MI_ERR_INVALID;
    const int rc = set_state(s, "mi_packset_get_info");
    if (rc) return rc;
    *out = s->info;
    return MI_OK;
}

// (hidden: mi_local.h) what mi_fetch.hip's lookup walks: mi_packset_missing, mi_packset_pack
int mi_packset_table(const mi_packset* s, const char* who, mi_ctx** ctx, const uint64_t** tags, const uint64_t** slots, uint64_t* cap) {
    if (!s || !ctx || !tags || !slots || !cap) return MI_ERR_INVALID;
    *ctx = s->ctx;
    const int rc = set_state(s, who);
    if (rc) return rc;
    *tags = s->table.tags.as<u64>();
    *slots = s->table.slots.as<u64>();
    *cap = s->table.cap;
    return MI_OK;
}

// (hidden: mi_local.h) for mi_zpack.hip: bytes up through the set's two windows, blocking; and a PLAIN blob that lies on the
// device already (blob: a mi::DevBuf the set takes over, NULL with n = 0) added as mi_packset_add_blob adds one behind its upload
int mi_packset_upload(mi_packset* s, void* d_dst, const void* src, uint64_t bytes, double* ms) {
    if (!s || (bytes && (!d_dst || !src))) return MI_ERR_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = s->up.upload(s->ctx, (u8*)d_dst, src, bytes);
    if (ms) *ms = ms_since(t0);
    return rc;
}

int mi_packset_adopt(mi_packset* s, const char* who, void* blob, uint64_t blob_bytes, const mi_pack_entry* entries, uint64_t n, uint32_t flags,
                     double ms_upload, uint64_t* first_bad) {
    if (!s || !who || (n && (!blob || !entries))) return MI_ERR_INVALID;
    const int rc = set_state(s, who);
    if (rc) return rc;
    s->info.ms_upload = ms_upload;
    DevBuf none;
    return set_add(s, who, std::move(blob ? *(DevBuf*)blob : none), n ? blob_bytes : 0, entries, n, flags, first_bad);
}

void mi_packset_free(mi_packset* s) {
    if (!s) return;
    mi_ctx* c = s->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    --c->live_children;
    delete s;
}

int mi_batch_add_recipes(mi_batch* b, const mi_packset* set, uint64_t n_files, const uint64_t* n_chunks, const uint8_t* digests,
                         const uint32_t* lengths, const uint64_t* user_tags, uint32_t flags, mi_recipe_stats* stats_out) {
    if (!b) return MI_ERR_INVALID;
    mi_ctx* c = b->ctx;
    if (stats_out) memset(stats_out, 0, sizeof *stats_out);
    if (!set || (n_files && !n_chunks)) return fail(c, MI_ERR_INVALID, "mi_batch_add_recipes: a NULL argument");
    if (b->group) return fail(c, MI_ERR_INVALID, "mi_batch_add_recipes: a batch group has one arena per GPU; restore into its members");
    if (set->ctx != c) return fail(c, MI_ERR_INVALID, "mi_batch_add_recipes: the pack set belongs to another ctx");
    if (flags & ~(uint32_t)MI_RECIPE_VERIFY) return fail(c, MI_ERR_INVALID, "mi_batch_add_recipes: unknown flags %#x", flags);
    int rc = set_state(set, "mi_batch_add_recipes");
    if (rc) return rc;
    if (b->staged) return fail(c, MI_ERR_STATE, "batch already ran; begin a new batch");
    u64 n_rows = 0;
    for (u64 i = 0; i < n_files; ++i) {
        if (n_chunks[i] > 0xFFFFFFFFull - n_rows)
            return fail(c, MI_ERR_INVALID, "mi_batch_add_recipes: more than 2^32 - 1 rows in one call (at file %llu)", (unsigned long long)i);
        n_rows += n_chunks[i];
    }
    if (n_rows && (!digests || !lengths)) return fail(c, MI_ERR_INVALID, "mi_batch_add_recipes: a NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    if (n_files == 0) return MI_OK;
    rc = b->window.flush(b);                          // the inline window may hold bytes of earlier small adds
    if (rc) return rc;
    // placement, as mi_batch_add_synthetic places: add order, kFileAlign-aligned; and every row's arena offset (the exclusive
    // scan of the lengths per file) in the pass that sums the sizes.  Nothing of the batch changes before the bytes lie there
    std::vector<u64> f_off(n_files), f_size(n_files), h_dst(n_rows);
    u64 end = b->arena_used, bytes = 0;
    for (u64 i = 0, r = 0; i < n_files; ++i) {
        const u64 at = (end + kFileAlign - 1) / kFileAlign * kFileAlign;
        u64 size = 0;
        for (u64 k = 0; k < n_chunks[i]; ++k, ++r) {
            h_dst[r] = at + size;
            size += lengths[r];
        }
        f_off[i] = at;
        f_size[i] = size;
        end = at + size;
        bytes += size;
    }
    const u64 end_aligned = (end + kFileAlign - 1) / kFileAlign * kFileAlign;
    rc = mi_batch_arena_reserve(b, end_aligned);
    if (rc) return rc;
    rc = arena_wait_mapped(c, &b->arena, std::min<u64>(b->arena.bytes, end_aligned + 4096));   // a walk-fed arena is mapped piece by piece
    if (rc) return rc;
    mi_recipe_stats st = {};
    st.n_files = n_files;
    st.n_rows = n_rows;
    st.bytes = bytes;
    if (n_rows) {
        hipStream_t s = c->stream;
        DevBuf d_dig, d_len32, d_dst, d_src, d_len64, d_found, d_cell, d_got;
        Event ev[4];
        StreamDrain drain{s};   // (goes first: buffers and events after it)
        for (auto& e : ev) HIPCHK(c, e.create());
        HIPCHK(c, d_dig.ensure(n_rows * 32));
        HIPCHK(c, d_len32.ensure(n_rows * 4));
        HIPCHK(c, d_dst.ensure(n_rows * 8));
        HIPCHK(c, d_src.ensure(n_rows * 8));
        HIPCHK(c, d_len64.ensure(n_rows * 8));
        HIPCHK(c, d_found.ensure(n_rows * 4));
        HIPCHK(c, d_cell.ensure(16));
        if (flags & MI_RECIPE_VERIFY) HIPCHK(c, d_got.ensure(n_rows * 32));
        u64* cell = d_cell.as<u64>();                  // [0] the smallest bad row, [1] joined units
        u64* h = c->h_word.as<u64>();
        // resolve
        HIPCHK(c, hipEventRecord(ev[0], s));
        HIPCHK(c, hipMemcpyAsync(d_dig.p, digests, n_rows * 32, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_len32.p, lengths, n_rows * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_dst.p, h_dst.data(), n_rows * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(cell, 0xFF, 8, s));
        HIPCHK(c, hipMemsetAsync(cell + 1, 0, 8, s));
        const u32 row_blocks = (u32)((n_rows + 255) / 256);
        hipLaunchKernelGGL(restore_lookup_kernel, dim3(row_blocks), dim3(256), 0, s, d_dig.as<u8>(), d_len32.as<u32>(), n_rows,
                           set->table.tags.as<u64>(), set->table.slots.as<u64>(), set->table.cap - 1, d_src.as<u64>(), d_len64.as<u64>(), d_found.as<u32>(), cell);
        HIPCHK(c, hipMemcpyAsync(h, cell, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(ev[1], s));
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipGetLastError());
        auto locate = [&](u64 row, u64* file, u64* in_file) {
            u64 f = 0, first = 0;
            while (f + 1 < n_files && row >= first + n_chunks[f]) first += n_chunks[f++];
            *file = f;
            *in_file = row - first;
        };
        if (h[0] != kNone) {
            const u64 bad = h[0];
            u64 f = 0, k = 0;
            locate(bad, &f, &k);
            u32 held = 0;
            HIPCHK(c, hipMemcpy(&held, d_found.as<u32>() + bad, 4, hipMemcpyDeviceToHost));
            const std::string dg = hex32(digests + 32 * bad);
            if (lengths[bad] == 0)
                return fail(c, MI_ERR_INVALID, "mi_batch_add_recipes: file %llu, row %llu (row %llu of the call) has length 0",
                            (unsigned long long)f, (unsigned long long)k, (unsigned long long)bad);
            if (held == 0)
                return fail(c, MI_ERR_INVALID, "mi_batch_add_recipes: file %llu, row %llu (row %llu of the call): the pack set does not hold "
                            "digest %s", (unsigned long long)f, (unsigned long long)k, (unsigned long long)bad, dg.c_str());
            return fail(c, MI_ERR_INVALID, "mi_batch_add_recipes: file %llu, row %llu (row %llu of the call): the pack set holds digest %s "
                        "with %u bytes, the recipe states %u", (unsigned long long)f, (unsigned long long)k, (unsigned long long)bad, dg.c_str(),
                        held, lengths[bad]);
        }
        // assemble: [the first file's offset, the last file's end rounded up to 16).  Files without rows in front lie where the
        // first file with rows lies (an empty file takes no room), so the range begins at the first row
        const u64 d0 = h_dst[0], d1 = round16(end);
        const u64 n_tiles = (d1 - d0 + kRestoreTile - 1) / kRestoreTile;
        if (n_tiles >> 31)
            return fail(c, MI_ERR_INVALID, "mi_batch_add_recipes: %llu bytes are more than one launch covers", (unsigned long long)(d1 - d0));
        hipLaunchKernelGGL(restore_assemble_kernel, dim3((u32)n_tiles), dim3(kRestoreWG), 0, s, b->arena.as<u8>(), d_dst.as<u64>(),
                           d_src.as<u64>(), d_len64.as<u64>(), n_rows, d0, d1, cell + 1);
        HIPCHK(c, hipEventRecord(ev[2], s));
        if (flags & MI_RECIPE_VERIFY) {
            const auto hash_items = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? launch_blake2s_items : launch_sha256_items;
            hash_items(kShaBlobs, b->arena.as<u8>(), d_dst.as<u64>(), d_len64.as<u64>(), nullptr, (u32)n_rows, nullptr, c->heads.as<u32>(),
                       nullptr, true, d_got.as<u8>(), c->sha, c->prop.multiProcessorCount, d1, s);
            hipLaunchKernelGGL(restore_compare_kernel, dim3(row_blocks), dim3(256), 0, s, d_got.as<u8>(), d_dig.as<u8>(), n_rows, cell);
        }
        HIPCHK(c, hipEventRecord(ev[3], s));
        HIPCHK(c, hipMemcpyAsync(h, cell, 16, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipGetLastError());
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
        st.ms_resolve = ms;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[1], ev[2]));
        st.ms_assemble = ms;
        if (flags & MI_RECIPE_VERIFY) {
            HIPCHK(c, hipEventElapsedTime(&ms, ev[2], ev[3]));
            st.ms_verify = ms;
        }
        st.n_joined_units = h[1];
        if (h[0] != kNone) {
            const u64 bad = h[0];
            u64 f = 0, k = 0, src = 0;
            locate(bad, &f, &k);
            HIPCHK(c, hipMemcpy(&src, d_src.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
            return fail(c, MI_ERR_IO, "mi_batch_add_recipes: file %llu, row %llu (row %llu of the call), %u bytes at arena offset %llu from "
                        "source address %#llx: the assembled bytes do not hash to the recipe's digest %s", (unsigned long long)f,
                        (unsigned long long)k, (unsigned long long)bad, lengths[bad], (unsigned long long)h_dst[bad], (unsigned long long)src,
                        hex32(digests + 32 * bad).c_str());
        }
    }
    // the bytes lie in the arena: now the batch changes
    b->files.reserve(b->files.size() + n_files);
    for (u64 i = 0; i < n_files; ++i) b->files.push_back({f_off[i], f_size[i], user_tags ? user_tags[i] : 0});
    b->arena_used = end;
    b->total_bytes += bytes;
    if (stats_out) *stats_out = st;
    return MI_OK;
}

}  // extern "C"
