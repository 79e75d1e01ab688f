// mi_zset.hip -- compressed pack sets: zpacks (mi_zpack.hip) resident on the device AS STORED and addressed by digest
// (mi_zset_*), CUT by digest into a new zpack without a coder (mi_zset_zpack), and the files of a batch assembled from such a
// set by decoding every recipe row straight to its place in the arena (mi_batch_add_zrecipes).  A chunk's stored form is a
// pure function of its bytes, so moving stored spans gives byte for byte what mi_packset_pack + mi_pack_compress gives.
//
//   set       the pack sets' table (mi_slot_table.h) with a slot that carries `stored`: tag = the digest's first 8 bytes (0 is
//             stored as 1, 0 = empty), slot = {digest 32 | the stored span's ABSOLUTE device address 8 | length | stored << 32}.
//             Insert in probe-then-verify rounds across a kernel boundary; a digest met again is kept once (the first form
//             wins); the same digest with another LENGTH makes the set unusable.  Rebuilt at twice the size when it passes half full;
//   verify    MI_ZSET_VERIFY / MI_ZPACK_VERIFY: the blob decoded by mi_zpack.hip's decode kernel into a scratch laid out as a
//             plain pack (mi_zpack_decode_plain), hashed by the ctx's launcher (pass kShaBlobs), held against the entries;
//   cut       mi_fetch.hip's scheme: lookup (slot_table_find: tag first, then all 32 bytes), first occurrences by the engine's
//             dedup marking, mi_plan.h's plan over round16(stored) with the totals (entries, stored bytes, raw entries, chunk
//             bytes), and the 16 KiB-tile gather (mi_gather.h) from absolute
//             16-byte-aligned sources, the bytes at and beyond `stored` zeroed in registers.  One synchronisation: the totals,
//             before the blob is allocated.  Every offset is 64-bit;
//   restore   zset_restore_kernel: ONE WAVE A RECIPE ROW (the workgroup is the wave, grid-stride, at most 65 536 waves).  A coded
//             row is z_decode_block (mi_lz4_wave.h) with the arena as its output, at whatever byte alignment the row has; a raw
//             row is a copy: bytes up to the first 16-aligned destination, aligned 16-byte stores from unaligned 16-byte loads,
//             the tail by bytes.  NO PAD IS WRITTEN: a row's neighbours are other waves' rows.  The stored span's pad is read
//             and must be zero, so an unverified set fails on the entries mi_zpack_check would refuse.
//
// BOUNDS.  The restore kernel WRITES only [dst, dst + length) of each row: the decoder checks len <= length - op before every
// copy, the raw copy's three pieces partition [0, length).  It READS only [src, src + round16(stored)) -- the decoder compares
// every index with `stored` before the load, the raw copy's 16-byte loads begin at src + a with a + 16 <= length = stored, the
// pad check reads [stored, round16(stored)) -- and [dst, dst + op) of its own row (a match's source).  The structural check of
// every add (offset + round16(stored) <= blob_bytes, always, on the host) keeps a stored span inside its blob.  The cut READS
// aligned 16-byte units inside [src, src + round16(stored)) and WRITES aligned units inside the new blob.  The hashing of a
// verify pass reads up to 67 bytes behind the last string: a scratch's 256 bytes of slack, the arena's 4 KiB.
#include "mi_gather.h"
#include "mi_lz4_wave.h"
#include "mi_plan.h"
#include "mi_zset_local.h"
#include "mi_zentropy.h"

#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

using namespace mi;

namespace mi {

constexpr u64 kQNone = ~0ull;

// ---- the set: entries -> the table's records (the table itself: mi_slot_table.hip) -------------------------------------------
__global__ __launch_bounds__(256)
void zset_unpack_kernel(const u64* __restrict__ entries, u64 n, u64 base, u64* __restrict__ recs) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const u64* e = entries + kEntryWords * k;
    u64* r = recs + kSlotWords * k;
    r[0] = e[0]; r[1] = e[1]; r[2] = e[2]; r[3] = e[3];
    r[4] = base + e[4];
    r[5] = e[6];
}

// ---- resolve (as mi_fetch.hip's fetch_lookup_kernel does) ----------------------------------------------------------------------
// src[r], word[r]: where the set holds row r's stored span and its length | stored << 32 (0, 0: it does not hold the digest);
// len64[r]: the SET'S length.  A bad row: a digest the set lacks; with lengths, a stated length of 0 or another one than the set's
__global__ __launch_bounds__(256)
void zset_lookup_kernel(const u8* __restrict__ digests, const u32* __restrict__ lengths, u64 n, const u64* __restrict__ tags,
                        const u64* __restrict__ slots, u64 mask, u64* __restrict__ src, u64* __restrict__ word,
                        u64* __restrict__ len64, u64* __restrict__ first_bad) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const u8* d = digests + 32 * r;
    u64 at = 0, w = 0;
    const u64 slot = slot_table_find(tags, slots, mask, d);
    if (slot != kSlotNone) {
        at = slots[kSlotWords * slot + 4];
        w = slots[kSlotWords * slot + 5];
    }
    src[r] = at;
    word[r] = w;
    len64[r] = w & 0xFFFFFFFFull;
    bool bad = at == 0;
    if (lengths) {
        const u32 len = lengths[r];
        bad = bad || len == 0 || (u32)w != len;
    }
    if (bad) atomicMin((unsigned long long*)first_bad, (unsigned long long)r);
}

// ---- plan: mi_plan.h's over round16(stored) of the first occurrences ---------------------------------------------------------
enum : int { kQTotEntries = 0, kQTotBlob = 1, kQTotStored = 2, kQTotRaw = 3, kQTotChunk = 4, kQTotBad = 6, kQTotDiffer = 7 };

// per block of kPlanTile rows: the first occurrences and their rounded-up stored bytes; into the totals: stored bytes, raw
// entries, chunk bytes
__global__ __launch_bounds__(kPlanBlock)
void zset_block_sums_kernel(const i64* __restrict__ dup_of, const u64* __restrict__ word, u64 n, u64* __restrict__ block_cnt,
                            u64* __restrict__ block_bytes, u64* __restrict__ totals) {
    __shared__ u64 lds[5][kPlanBlock / 64];
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 v[5] = {0, 0, 0, 0, 0};                       // entries, rounded-up stored bytes, stored bytes, raw entries, chunk bytes
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const u64 row = base + k;
        if (row >= n || dup_of[row] >= 0) continue;
        const u64 w = word[row];
        const u64 len = w & 0xFFFFFFFFull, stored = w >> 32;
        ++v[0];
        v[1] += round16(stored);
        v[2] += stored;
        v[3] += stored == len ? 1 : 0;
        v[4] += len;
    }
    plan_block_sum<5>(v, lds);
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = v[0];
        block_bytes[blockIdx.x] = v[1];
        if (v[2]) atomicAdd((unsigned long long*)&totals[kQTotStored], (unsigned long long)v[2]);
        if (v[3]) atomicAdd((unsigned long long*)&totals[kQTotRaw], (unsigned long long)v[3]);
        if (v[4]) atomicAdd((unsigned long long*)&totals[kQTotChunk], (unsigned long long)v[4]);
    }
}

// single block: exclusive scan of both block arrays in place; the totals: entries, the blob's bytes
__global__ __launch_bounds__(kPlanBlock)
void zset_block_offsets_kernel(u64* __restrict__ block_cnt, u64* __restrict__ block_bytes, u64 n_blocks, u64* __restrict__ totals) {
    plan_block_offsets<true>(block_cnt, block_bytes, n_blocks, &totals[kQTotEntries], &totals[kQTotBlob]);
}

// the new zpack's entries, in order of first occurrence: where the stored span lies, its stored size, where it goes in the blob,
// and the mi_zpack_entry row (digest | offset | chunk_index = the request row | length, stored)
__global__ __launch_bounds__(kPlanBlock)
void zset_compact_entries_kernel(const i64* __restrict__ dup_of, const u64* __restrict__ src, const u64* __restrict__ word,
                                 const u8* __restrict__ digests, u64 n, const u64* __restrict__ block_cnt,
                                 const u64* __restrict__ block_bytes, u64* __restrict__ e_src, u64* __restrict__ e_len,
                                 u64* __restrict__ e_dst, u64* __restrict__ rows) {
    const u64 base = (u64)blockIdx.x * kPlanTile + (u64)threadIdx.x * kPlanPer;
    u64 w[kPlanPer];
    u32 sel = 0;
    u64 cnt = 0, bytes = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        const bool s = base + k < n && dup_of[base + k] < 0;
        w[k] = s ? word[base + k] : 0;
        if (s) { sel |= 1u << k; ++cnt; bytes += round16(w[k] >> 32); }
    }
    u64 at = plan_first(cnt, block_cnt);
    u64 dst = plan_first(bytes, block_bytes);
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (!(sel & (1u << k))) continue;
        const u64 row = base + k;
        const u64 stored = w[k] >> 32;
        e_src[at] = src[row];
        e_len[at] = stored;
        e_dst[at] = dst;
        put_entry_row(rows + kEntryWords * at, digests + 32 * row, dst, row, w[k]);
        ++at;
        dst += round16(stored);
    }
}

// ---- gather: mi_gather.h's tile body over aligned sources -----------------------------------------------------------------------

__global__ __launch_bounds__(kGatherWG)
void zset_gather_kernel(const u64* __restrict__ e_src, const u64* __restrict__ e_len, const u64* __restrict__ e_dst, u64 n_entries,
                        u64 blob_bytes, u8* __restrict__ blob) {
    gather_tile<true>(e_src, e_len, e_dst, n_entries, blob_bytes, blob);
}

// ---- the fused restore: one wave a recipe row, decoded (or copied) straight to its place in the arena -----------------------
// r_dst: the row's arena offset (any byte alignment); r_src: the stored span's device address (16-byte aligned); r_word:
// length | stored << 32.  rule_out[k]: 0 or the rule that refuses row k; first_bad: the smallest refused row
__global__ __launch_bounds__(64)
void zset_restore_kernel(u8* arena, const u64* __restrict__ r_dst, const u64* __restrict__ r_src, const u64* __restrict__ r_word,
                         u64 n, u32* __restrict__ rule_out, u64* __restrict__ first_bad) {
    typedef const u8 __attribute__((address_space(1))) * global_bytes;
    const int lane = threadIdx.x;
    for (u64 k = blockIdx.x; k < n; k += gridDim.x) {
        const u64 s_addr = r_src[k];
        const u8* src = (const u8*)(global_bytes)s_addr;
        const u64 len = r_word[k] & 0xFFFFFFFFull, stored = r_word[k] >> 32;
        u8* dst = arena + r_dst[k];
        u32 rule = 0;
        if (stored == len) {
            // raw: bytes up to the first 16-aligned destination, aligned stores from unaligned loads, the tail by bytes -- the
            // three pieces partition [0, len), a chunk shorter than one unit goes by bytes only
            const u64 to_grid = (16 - ((u64)(size_t)dst & 15)) & 15;
            const u64 head = to_grid < len ? to_grid : len;
            const u64 units = (len - head) >> 4;
            const u64 tail = head + (units << 4);
            if ((u64)lane < head) dst[lane] = src[lane];
            for (u64 u = lane; u < units; u += 64) *(u32x4*)(dst + head + (u << 4)) = load16_global_unaligned(s_addr + head + (u << 4));
            if (tail + lane < len) dst[tail + lane] = src[tail + lane];
        } else {
            rule = z_decode_block(src, stored, dst, len, lane);
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

// the digests the device computed against the wanted ones: `stride` words from one wanted digest to the next (the rows of a
// zpack: 7; a recipe's digests: 4)
__global__ __launch_bounds__(256)
void zset_compare_kernel(const u8* __restrict__ got, const u64* __restrict__ want, u32 stride, u64 n, u64* __restrict__ first_bad) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    digest_differs_mark(got, want + (u64)stride * k, k, first_bad);
}

}  // namespace mi

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int blob_does_not_fit(mi_ctx* c, const char* who, hipError_t e, u64 blob_bytes, u64 n) {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: a compressed blob of %llu bytes (%llu entries) does not fit: the "
                "device has %llu bytes free (%s)", who, (unsigned long long)blob_bytes, (unsigned long long)n, (unsigned long long)free_b,
                hipGetErrorString(e));
}

int set_state(const mi_zset* s, const char* who) {
    if (s->broken.empty()) return MI_OK;
    return fail(s->ctx, MI_ERR_STATE, "%s: the compressed pack set is unusable since: %s", who, s->broken.c_str());
}

// MI_ZSET_VERIFY / MI_ZPACK_VERIFY: a compressed blob on the device, its entries on the host (structurally sound) and on the
// device (d_rows: what the digests are held against), n > 0.  Decoded into a scratch laid out as a plain pack, hashed there.
// *bad = the smallest entry that does not decode (then *rule says why) or, if all decode, that does not hash (*rule = 0);
// kQNone: none.  Blocking; the scratch is gone when it returns
int verify_stored(mi_ctx* c, const char* who, const void* d_zblob, const mi_zpack_entry* entries, const u64* d_rows, u64 n, u64* bad,
                  u32* rule, double* ms_decode) {
    hipStream_t st = c->stream;
    std::vector<mi_pack_entry> plain(n);
    DevBuf d_plain, d_off, d_len, d_got, d_bad;
    StreamDrain drain{st};   // (goes first: the buffers above after it)
    u64 plain_bytes = 0;
    int rc = mi_zpack_decode_plain(c, who, d_zblob, entries, n, &d_plain, &plain_bytes, plain.data(), bad, rule, ms_decode);
    if (rc || *bad != kQNone) return rc;
    std::vector<u64> offs(2 * n);
    for (u64 k = 0; k < n; ++k) { offs[k] = plain[k].offset; offs[n + k] = plain[k].length; }
    HIPCHK(c, d_off.ensure(2 * n * 8));
    HIPCHK(c, d_got.ensure(n * 32));
    HIPCHK(c, d_bad.ensure(8));
    HIPCHK(c, hipMemcpyAsync(d_off.p, offs.data(), 2 * n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_bad.p, 0xFF, 8, st));
    const auto hash_items = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? launch_blake2s_items : launch_sha256_items;
    hash_items(kShaBlobs, d_plain.as<u8>(), d_off.as<u64>(), d_off.as<u64>() + n, nullptr, (u32)n, nullptr, c->heads.as<u32>(), nullptr, true,
               d_got.as<u8>(), c->sha, c->prop.multiProcessorCount, plain_bytes, st);
    hipLaunchKernelGGL(zset_compare_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_got.as<u8>(), d_rows, (u32)kEntryWords, n,
                       d_bad.as<u64>());
    u64* h = c->h_word.as<u64>();
    HIPCHK(c, hipMemcpyAsync(h, d_bad.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    *bad = h[0];
    *rule = 0;
    return MI_OK;
}

// The blob lies on the device as stored (the copy into it may still be queued on the ctx stream); entries are structurally
// sound.  Verification, the table, the set's counters.  Until the insert begins every failure leaves the set as it was.
int set_add(mi_zset* s, const char* who, DevBuf&& blob, u64 blob_bytes, const mi_zpack_entry* entries, u64 n, uint32_t flags, u64* first_bad) {
    mi_ctx* c = s->ctx;
    hipStream_t st = c->stream;
    DevBuf mine = std::move(blob);                     // freed on every early return -- after the stream has drained
    DevBuf d_ent, d_recs, new_stamps;
    StreamDrain drain{st};   // (goes first: the buffers above after it)
    s->info.ms_verify = s->info.ms_insert = 0;
    if (n == 0) {                                      // a zpack of nothing
        ++s->info.n_packs;
        return MI_OK;
    }
    HIPCHK(c, d_ent.ensure(n * sizeof(mi_zpack_entry)));
    HIPCHK(c, d_recs.ensure(n * kSlotWords * 8));
    HIPCHK(c, hipMemcpyAsync(d_ent.p, entries, n * sizeof(mi_zpack_entry), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(zset_unpack_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_ent.as<u64>(), n, (u64)(size_t)mine.p,
                       d_recs.as<u64>());
    if (flags & MI_ZSET_VERIFY) {
        const auto t0 = std::chrono::steady_clock::now();
        u64 bad = kQNone;
        u32 rule = 0;
        const int rc = verify_stored(c, who, mine.p, entries, d_ent.as<u64>(), n, &bad, &rule, nullptr);
        if (rc) return rc;
        s->info.ms_verify = ms_since(t0);
        if (bad != kQNone) {
            if (first_bad) *first_bad = bad;
            const mi_zpack_entry en = bad < n ? entries[bad] : mi_zpack_entry{};
            if (rule)
                return fail(c, MI_ERR_INVALID, "%s: entry %llu (offset %llu, %u bytes stored for %u) does not decode: %s", who,
                            (unsigned long long)bad, (unsigned long long)en.offset, en.stored, en.length, mi_host::zrule_name(rule));
            return fail(c, MI_ERR_INVALID, "%s: entry %llu (offset %llu, %u bytes stored for %u) does not hash to its digest on the device", who,
                        (unsigned long long)bad, (unsigned long long)en.offset, en.stored, en.length);
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    int rc = MI_OK;
    if (s->ageing) {                                   // (mi_zage.hip) a table that grows takes the stamps along, before the old one goes
        rc = s->table.make_room(c, n, "compressed pack set", [&](const u64* new_tags, const u64* new_slots, u64 new_cap) -> int {
            const hipError_t e = new_stamps.alloc_exact(new_cap * 4);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: the grown table's stamps of %llu bytes do not fit (%s)", who,
                            (unsigned long long)(new_cap * 4), hipGetErrorString(e));
            }
            const int rc2 = zage_carry_enqueue(c, s->table.tags.as<u64>(), s->table.slots.as<u64>(), s->table.cap, s->stamps.as<u32>(), new_tags, new_slots,
                                               new_cap, new_stamps.as<u32>());
            if (rc2) return rc2;
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipGetLastError());
            return MI_OK;
        });
        if (rc == MI_OK && new_stamps.p) s->stamps = std::move(new_stamps);      // (DevBuf's move swaps: the old stamps go with the local)
    } else {
        rc = s->table.make_room(c, n, "compressed pack set");
    }
    if (rc) return rc;
    u64 sums[3], conflict = kQNone;
    rc = s->table.insert(c, d_recs.as<u64>(), n, sums, &conflict, "compressed pack set");
    s->table.count += sums[0];
    s->info.n_digests = s->table.count;
    s->info.stored_bytes += sums[1];
    s->info.chunk_bytes += sums[2];
    s->blobs.push_back(ZsetBlob{std::move(mine), blob_bytes});   // the table may point into it by now
    if (rc == MI_OK && conflict != kQNone) {
        if (first_bad) *first_bad = conflict;
        rc = fail(c, MI_ERR_INVALID, "%s: entry %llu (%u bytes) has a digest the set holds with another length -- unverified input; the set "
                  "is unusable from here on", who, (unsigned long long)conflict, conflict < n ? entries[conflict].length : 0u);
    }
    if (rc == MI_OK && s->ageing) {                    // an add is a use: every digest it brought, new or held, gets the set's epoch
        rc = zage_touch_records_enqueue(s, d_recs.as<u64>(), n);
        if (rc == MI_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(c, MI_ERR_HIP, "%s: stamping the added digests failed", who);
    }
    if (rc) {                                          // the table is not rolled back: sticky
        s->broken = ctx_error(c);
        return rc;
    }
    s->info.ms_insert = ms_since(t0);
    ++s->info.n_packs;
    s->info.n_entries += n;
    for (u64 k = 0; k < n; ++k) s->info.blob_bytes += round16(entries[k].stored);
    return MI_OK;
}

}  // namespace

namespace mi {

// (hidden: mi_zset_local.h) for mi_zserve.hip's MI_ZPACK_VERIFY
int zset_verify_stored(mi_ctx* c, const char* who, const void* d_zblob, const mi_zpack_entry* entries, const u64* d_rows, u64 n, u64* bad, u32* rule,
                       double* ms_decode) {
    return verify_stored(c, who, d_zblob, entries, d_rows, n, bad, rule, ms_decode);
}

}  // namespace mi

extern "C" {

int mi_zset_create(mi_ctx* c, uint64_t entries_hint, mi_zset** out) {
    if (!c || !out) return MI_ERR_INVALID;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    if (entries_hint >> 40) return fail(c, MI_ERR_INVALID, "mi_zset_create: entries_hint %llu", (unsigned long long)entries_hint);
    mi_zset* s = new mi_zset();
    s->ctx = c;
    ++c->live_children;                                 // mi_zset_free undoes it
    s->info.alg = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? MI_DIGEST_BLAKE2S : MI_DIGEST_SHA256;
    u64 cap = 1024;
    while (cap < entries_hint * 2) cap <<= 1;
    s->table.sum_bytes = true;                          // (mi_zset_info's stored_bytes and chunk_bytes)
    int rc = s->table.alloc(c, cap);
    if (rc == MI_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, MI_ERR_HIP, "mi_zset_create: the table's memset failed");
    if (rc) { mi_zset_free(s); return rc; }
    *out = s;
    return MI_OK;
}

int mi_zset_add_zblob(mi_zset* s, const void* blob, uint64_t blob_bytes, const mi_zpack_entry* entries, uint64_t n, uint32_t flags,
                      uint64_t* first_bad) {
    if (first_bad) *first_bad = 0;
    if (!s || (!blob && blob_bytes) || (!entries && n)) return MI_ERR_INVALID;
    static const char* who = "mi_zset_add_zblob";
    mi_ctx* c = s->ctx;
    int rc = set_state(s, who);
    if (rc) return rc;
    if (flags & ~(uint32_t)MI_ZSET_VERIFY) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu entries, a pack holds fewer than 2^32", who, (unsigned long long)n);
    rc = mi_zpack_structure(c, who, blob_bytes, entries, n, first_bad);        // before a byte is uploaded
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    s->info.ms_upload = 0;
    DevBuf d_blob;
    if (blob_bytes && n) {
        const hipError_t e = d_blob.alloc_exact(blob_bytes);
        if (e != hipSuccess) return blob_does_not_fit(c, who, e, blob_bytes, n);
        const auto t0 = std::chrono::steady_clock::now();
        rc = s->up.upload(c, d_blob.as<u8>(), blob, blob_bytes);
        if (rc) return rc;
        s->info.ms_upload = ms_since(t0);
    }
    return set_add(s, who, std::move(d_blob), blob_bytes, entries, n, flags, first_bad);
}

int mi_zset_add_zpack(mi_zset* s, const mi_zpack* z, uint32_t flags) {
    if (!s || !z) return MI_ERR_INVALID;
    static const char* who = "mi_zset_add_zpack";
    mi_ctx* c = s->ctx;
    int rc = set_state(s, who);
    if (rc) return rc;
    if (flags & ~(uint32_t)MI_ZSET_VERIFY) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    mi_ctx* zc = nullptr;
    const void* src = nullptr;
    const mi_zpack_entry* rows = nullptr;
    u64 blob_bytes = 0, n = 0;
    if ((rc = mi_zpack_device(z, &zc, &src, &blob_bytes, &rows, &n))) return rc;
    if (zc != c) return fail(c, MI_ERR_INVALID, "%s: the zpack belongs to another ctx; hand its bytes to mi_zset_add_zblob", who);
    rc = mi_zpack_structure(c, who, blob_bytes, rows, n, nullptr);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    s->info.ms_upload = 0;
    DevBuf d_blob;
    if (blob_bytes && n) {
        const hipError_t e = d_blob.alloc_exact(blob_bytes);
        if (e != hipSuccess) return blob_does_not_fit(c, who, e, blob_bytes, n);
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t ce = hipMemcpyAsync(d_blob.p, src, blob_bytes, hipMemcpyDeviceToDevice, c->stream);
        if (ce == hipSuccess) ce = hipStreamSynchronize(c->stream);
        if (ce != hipSuccess) return fail(c, MI_ERR_HIP, "%s: the device-to-device copy: %s", who, hipGetErrorString(ce));
        s->info.ms_upload = ms_since(t0);
    }
    return set_add(s, who, std::move(d_blob), blob_bytes, rows, n, flags, nullptr);
}

// (hidden: mi_local.h) for mi_zbatch.hip's mi_zset_missing: the set's ctx, and the lookup behind whatever the ctx stream holds
int mi_zset_ctx(const mi_zset* s, const char* who, mi_ctx** ctx) {
    if (!s || !who || !ctx) return MI_ERR_INVALID;
    *ctx = s->ctx;
    return set_state(s, who);
}

int mi_zset_lookup_enqueue(const mi_zset* s, const uint8_t* d_digests, const uint32_t* d_lengths, uint64_t n, uint64_t* d_src, uint64_t* d_word,
                           uint64_t* d_len64, uint64_t* d_first_bad) {
    if (!s || !d_digests || !n || !d_src || !d_word || !d_len64 || !d_first_bad) return MI_ERR_INVALID;
    hipLaunchKernelGGL(zset_lookup_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, s->ctx->stream, d_digests, d_lengths, n,
                       s->table.tags.as<u64>(), s->table.slots.as<u64>(), s->table.cap - 1, d_src, d_word, d_len64, d_first_bad);
    return MI_OK;
}

int mi_zset_entries(const mi_zset* s, uint8_t* digests, uint32_t* lengths, uint32_t* stored, uint64_t cap, uint64_t* n) {
    if (!s || !n) return MI_ERR_INVALID;
    static const char* who = "mi_zset_entries";
    mi_ctx* c = s->ctx;
    const int rc = set_state(s, who);
    if (rc) return rc;
    *n = s->table.count;
    if (cap == 0 || s->table.count == 0) return MI_OK;                       // the sizing call; a set of nothing
    if (cap < s->table.count)
        return fail(c, MI_ERR_INVALID, "%s: room for %llu entries, the set holds %llu", who, (unsigned long long)cap, (unsigned long long)s->table.count);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf d_recs, d_cursor;
    StreamDrain drain{st};   // (goes first: the buffers above after it)
    std::vector<u64> recs(s->table.count * kSlotWords);
    HIPCHK(c, d_recs.ensure(s->table.count * kSlotWords * 8));
    HIPCHK(c, d_cursor.ensure(8));
    HIPCHK(c, hipMemsetAsync(d_cursor.p, 0, 8, st));
    s->table.export_records(c, d_recs.as<u64>(), s->table.count, d_cursor.as<u64>());
    HIPCHK(c, hipMemcpyAsync(c->h_word.p, d_cursor.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(recs.data(), d_recs.p, s->table.count * kSlotWords * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    const u64 have = c->h_word.as<u64>()[0];
    if (have != s->table.count)
        return fail(c, MI_ERR_STATE, "%s: the set holds %llu digests, counted %llu", who, (unsigned long long)have, (unsigned long long)s->table.count);
    for (u64 k = 0; k < s->table.count; ++k) {
        const u64* r = recs.data() + kSlotWords * k;
        if (digests) memcpy(digests + 32 * k, r, 32);
        if (lengths) lengths[k] = (u32)r[5];
        if (stored) stored[k] = (u32)(r[5] >> 32);
    }
    return MI_OK;
}

int mi_zset_count_forms(const mi_zset* s, mi_zforms* out) {
    if (!s || !out) return MI_ERR_INVALID;
    mi_ctx* c = s->ctx;
    memset(out, 0, sizeof *out);
    const int rc = set_state(s, "mi_zset_count_forms");
    if (rc) return rc;
    if (!s->table.count) return MI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const u64* slots = s->table.slots.as<u64>();           // a slot: digest 4 | the span's address | length, stored
    return zh_count_forms(c, 0, slots + 4, (u32)kSlotWords, slots + 5, (u32)kSlotWords, s->table.cap, s->table.tags.as<u64>(), out);
}

int mi_zset_get_info(const mi_zset* s, mi_zset_info* out) {
    if (!s || !out) return MI_ERR_INVALID;
    const int rc = set_state(s, "mi_zset_get_info");
    if (rc) return rc;
    *out = s->info;
    return MI_OK;
}

void mi_zset_free(mi_zset* s) {
    if (!s) return;
    mi_ctx* c = s->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    --c->live_children;
    delete s;
}

int mi_zset_zpack(const mi_zset* set, const uint8_t* digests, const uint32_t* lengths, uint64_t n, uint32_t flags, mi_zpack** out,
                  uint64_t* first_bad) {
    if (first_bad) *first_bad = 0;
    if (out) *out = nullptr;
    if (!set || !out || (n && !digests)) return MI_ERR_INVALID;
    static const char* who = "mi_zset_zpack";
    mi_ctx* c = set->ctx;
    int rc = set_state(set, who);
    if (rc) return rc;
    if (flags & ~(uint32_t)MI_ZPACK_VERIFY) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu rows, a pack holds fewer than 2^32", who, (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    struct Owned { mi_zpack* z = nullptr; ~Owned() { if (z) mi_zpack_free(z); } } mine;   // (drains the ctx stream before the blob goes)
    void* d_blob = nullptr;
    mi_zpack_entry* h_rows = nullptr;
    if (n == 0) {                                          // a valid zpack of nothing
        rc = mi_zpack_alloc(c, who, 0, 0, &mine.z, &d_blob, &h_rows);
        if (rc) return rc;
        mi_zpack_set_result(mine.z, 0, 0, 0, (flags & MI_ZPACK_VERIFY) ? 1u : 0u, 0, 0, 0);
        *out = mine.z;
        mine.z = nullptr;
        return MI_OK;
    }
    hipStream_t s = c->stream;
    DevBuf d_dig, d_len32, d_src, d_word, d_len64, d_dup, d_scan, e_src, e_len, e_dst, d_rows;
    Event ev[4];
    StreamDrain drain{s};   // (goes first: buffers and events after it)
    for (auto& e : ev) HIPCHK(c, e.create());
    const u64 nb = (n + kPlanTile - 1) / kPlanTile;
    u64 dd_cap = 1024;
    while (dd_cap < 2 * n) dd_cap <<= 1;
    HIPCHK(c, d_dig.ensure(n * 32));
    if (lengths) HIPCHK(c, d_len32.ensure(n * 4));
    HIPCHK(c, d_src.ensure(n * 8));
    HIPCHK(c, d_word.ensure(n * 8));
    HIPCHK(c, d_len64.ensure(n * 8));
    HIPCHK(c, d_dup.ensure(n * 8));
    HIPCHK(c, d_scan.ensure((2 * nb + 8) * 8));
    HIPCHK(c, c->dd_table.ensure(dd_cap * 8));
    HIPCHK(c, c->dd_slot.ensure(n * 4 + 16));
    HIPCHK(c, c->dd_nuniq.ensure(8));
    u64* block_cnt = d_scan.as<u64>();
    u64* block_bytes = block_cnt + nb;
    u64* totals = block_bytes + nb;                        // kQTot*
    // lookup, first occurrences, the plan's first two launches; one synchronisation: the totals
    HIPCHK(c, hipEventRecord(ev[0], s));
    HIPCHK(c, hipMemcpyAsync(d_dig.p, digests, n * 32, hipMemcpyHostToDevice, s));
    if (lengths) HIPCHK(c, hipMemcpyAsync(d_len32.p, lengths, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(totals, 0, 6 * 8, s));
    HIPCHK(c, hipMemsetAsync(totals + kQTotBad, 0xFF, 2 * 8, s));
    hipLaunchKernelGGL(zset_lookup_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, s, d_dig.as<u8>(),
                       lengths ? d_len32.as<u32>() : (const u32*)nullptr, n, set->table.tags.as<u64>(), set->table.slots.as<u64>(), set->table.cap - 1,
                       d_src.as<u64>(), d_word.as<u64>(), d_len64.as<u64>(), totals + kQTotBad);
    launch_dedup_mark(d_dig.as<u8>(), n, nullptr, c->dd_table.as<u32>(), c->dd_slot.as<u32>(), dd_cap, d_dup.as<i64>(), c->dd_nuniq.as<u64>(),
                      true, s);
    hipLaunchKernelGGL(zset_block_sums_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, s, d_dup.as<i64>(), d_word.as<u64>(), n, block_cnt, block_bytes,
                       totals);
    hipLaunchKernelGGL(zset_block_offsets_kernel, dim3(1), dim3(kPlanBlock), 0, s, block_cnt, block_bytes, nb, totals);
    HIPCHK(c, hipEventRecord(ev[1], s));
    u64* h = c->h_word.as<u64>();
    HIPCHK(c, hipMemcpyAsync(h, totals, 8 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (h[kQTotBad] != kQNone) {
        const u64 bad = h[kQTotBad];
        if (first_bad) *first_bad = bad;
        u64 w = 0, at = 0;
        HIPCHK(c, hipMemcpy(&w, d_word.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&at, d_src.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
        const std::string dg = hex32(digests + 32 * bad);
        if (lengths && lengths[bad] == 0) return fail(c, MI_ERR_INVALID, "%s: row %llu has length 0 (digest %s)", who, (unsigned long long)bad, dg.c_str());
        if (!at)
            return fail(c, MI_ERR_INVALID, "%s: row %llu: the compressed pack set does not hold digest %s", who, (unsigned long long)bad, dg.c_str());
        return fail(c, MI_ERR_INVALID, "%s: row %llu: the compressed pack set holds digest %s with %u bytes, the request states %u", who,
                    (unsigned long long)bad, dg.c_str(), (u32)w, lengths ? lengths[bad] : 0u);
    }
    const u64 n_sel = h[kQTotEntries], blob_bytes = h[kQTotBlob], stored_bytes = h[kQTotStored], n_raw = h[kQTotRaw], chunk_bytes = h[kQTotChunk];
    if (n_sel == 0 || n_sel > n || blob_bytes < 16 * n_sel || stored_bytes > chunk_bytes || stored_bytes > blob_bytes)
        return fail(c, MI_ERR_HIP, "%s: the plan counted %llu entries with %llu stored bytes in a blob of %llu for %llu chunk bytes", who,
                    (unsigned long long)n_sel, (unsigned long long)stored_bytes, (unsigned long long)blob_bytes, (unsigned long long)chunk_bytes);
    const u64 n_tiles = (blob_bytes + kGatherTile - 1) / kGatherTile;
    if (n_tiles >> 31) return fail(c, MI_ERR_INVALID, "%s: a blob of %llu bytes is more than one launch covers", who, (unsigned long long)blob_bytes);
    rc = mi_zpack_alloc(c, who, n_sel, blob_bytes, &mine.z, &d_blob, &h_rows);      // does not fit: MI_ERR_NOMEM, nothing has changed
    if (rc) return rc;
    HIPCHK(c, d_rows.ensure(n_sel * sizeof(mi_zpack_entry)));
    HIPCHK(c, e_src.ensure(n_sel * 8));
    HIPCHK(c, e_len.ensure(n_sel * 8));
    HIPCHK(c, e_dst.ensure(n_sel * 8));
    HIPCHK(c, hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(zset_compact_entries_kernel, dim3((u32)nb), dim3(kPlanBlock), 0, s, d_dup.as<i64>(), d_src.as<u64>(), d_word.as<u64>(),
                       d_dig.as<u8>(), n, block_cnt, block_bytes, e_src.as<u64>(), e_len.as<u64>(), e_dst.as<u64>(), d_rows.as<u64>());
    hipLaunchKernelGGL(zset_gather_kernel, dim3((u32)n_tiles), dim3(kGatherWG), 0, s, e_src.as<u64>(), e_len.as<u64>(), e_dst.as<u64>(), n_sel,
                       blob_bytes, (u8*)d_blob);
    HIPCHK(c, hipEventRecord(ev[3], s));
    // the entries to the host with the same synchronisation: mi_zpack_entries only reads from then on
    HIPCHK(c, hipMemcpyAsync(h_rows, d_rows.p, n_sel * sizeof(mi_zpack_entry), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    float ms = 0, ms2 = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    HIPCHK(c, hipEventElapsedTime(&ms2, ev[2], ev[3]));
    double ms_verify = 0, ms_decode = 0;
    if (flags & MI_ZPACK_VERIFY) {
        // as mi_pack_compress verifies: the new blob decoded into a plain scratch and hashed there, held against the rows --
        // which carry the REQUESTED digests
        const auto t0 = std::chrono::steady_clock::now();
        u64 bad = kQNone;
        u32 rule = 0;
        rc = verify_stored(c, who, d_blob, h_rows, d_rows.as<u64>(), n_sel, &bad, &rule, &ms_decode);
        if (rc) return rc;
        ms_verify = ms_since(t0);
        if (bad != kQNone) {
            const mi_zpack_entry row = bad < n_sel ? h_rows[bad] : mi_zpack_entry{};
            if (first_bad) *first_bad = row.chunk_index;
            return fail(c, MI_ERR_IO, "%s: row %llu (entry %llu), %u bytes stored for %u at blob offset %llu: %s%s, requested digest %s -- the "
                        "set was fed a damaged blob without MI_ZSET_VERIFY", who, (unsigned long long)row.chunk_index, (unsigned long long)bad,
                        row.stored, row.length, (unsigned long long)row.offset,
                        rule ? "the stored form does not decode: " : "the decoded bytes do not hash to the requested digest",
                        rule ? mi_host::zrule_name(rule) : "", hex32(row.digest).c_str());
        }
    }
    mi_zpack_set_result(mine.z, stored_bytes, n_raw, chunk_bytes, (flags & MI_ZPACK_VERIFY) ? 1u : 0u, (double)ms + ms2, ms_verify, ms_decode);
    *out = mine.z;
    mine.z = nullptr;
    return MI_OK;
}

int mi_batch_add_zrecipes(mi_batch* b, const mi_zset* set, uint64_t n_files, const uint64_t* n_chunks, const uint8_t* digests,
                          const uint32_t* lengths, const uint64_t* user_tags, uint32_t flags, mi_recipe_stats* stats_out) {
    if (!b) return MI_ERR_INVALID;
    static const char* who = "mi_batch_add_zrecipes";
    mi_ctx* c = b->ctx;
    if (stats_out) memset(stats_out, 0, sizeof *stats_out);
    if (!set || (n_files && !n_chunks)) return fail(c, MI_ERR_INVALID, "%s: a NULL argument", who);
    if (b->group) return fail(c, MI_ERR_INVALID, "%s: a batch group has one arena per GPU; restore into its members", who);
    if (set->ctx != c) return fail(c, MI_ERR_INVALID, "%s: the compressed pack set belongs to another ctx", who);
    if (flags & ~(uint32_t)MI_RECIPE_VERIFY) return fail(c, MI_ERR_INVALID, "%s: unknown flags %#x", who, flags);
    int rc = set_state(set, who);
    if (rc) return rc;
    if (b->staged) return fail(c, MI_ERR_STATE, "batch already ran; begin a new batch");
    u64 n_rows = 0;
    for (u64 i = 0; i < n_files; ++i) {
        if (n_chunks[i] > 0xFFFFFFFFull - n_rows)
            return fail(c, MI_ERR_INVALID, "%s: more than 2^32 - 1 rows in one call (at file %llu)", who, (unsigned long long)i);
        n_rows += n_chunks[i];
    }
    if (n_rows && (!digests || !lengths)) return fail(c, MI_ERR_INVALID, "%s: a NULL argument", who);
    HIPCHK(c, hipSetDevice(c->device));
    if (n_files == 0) return MI_OK;
    rc = b->window.flush(b);                          // the inline window may hold bytes of earlier small adds
    if (rc) return rc;
    // placement, as mi_batch_add_recipes places: add order, kFileAlign-aligned; and every row's arena offset (the exclusive scan
    // of the lengths per file) in the pass that sums the sizes.  Nothing of the batch changes before the bytes lie there
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
        DevBuf d_dig, d_len32, d_dst, d_src, d_word, d_len64, d_rule, d_cell, d_got;
        Event ev[4];
        StreamDrain drain{s};   // (goes first: buffers and events after it)
        for (auto& e : ev) HIPCHK(c, e.create());
        HIPCHK(c, d_dig.ensure(n_rows * 32));
        HIPCHK(c, d_len32.ensure(n_rows * 4));
        HIPCHK(c, d_dst.ensure(n_rows * 8));
        HIPCHK(c, d_src.ensure(n_rows * 8));
        HIPCHK(c, d_word.ensure(n_rows * 8));
        HIPCHK(c, d_len64.ensure(n_rows * 8));
        HIPCHK(c, d_rule.ensure(n_rows * 4));
        HIPCHK(c, d_cell.ensure(16));
        if (flags & MI_RECIPE_VERIFY) HIPCHK(c, d_got.ensure(n_rows * 32));
        u64* cell = d_cell.as<u64>();                  // [0] the smallest bad row
        u64* h = c->h_word.as<u64>();
        // resolve
        HIPCHK(c, hipEventRecord(ev[0], s));
        HIPCHK(c, hipMemcpyAsync(d_dig.p, digests, n_rows * 32, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_len32.p, lengths, n_rows * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_dst.p, h_dst.data(), n_rows * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(cell, 0xFF, 16, s));
        const u32 row_blocks = (u32)((n_rows + 255) / 256);
        hipLaunchKernelGGL(zset_lookup_kernel, dim3(row_blocks), dim3(256), 0, s, d_dig.as<u8>(), d_len32.as<u32>(), n_rows,
                           set->table.tags.as<u64>(), set->table.slots.as<u64>(), set->table.cap - 1, d_src.as<u64>(), d_word.as<u64>(), d_len64.as<u64>(), cell);
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
        if (h[0] != kQNone) {
            const u64 bad = h[0];
            u64 f = 0, k = 0, w = 0, at = 0;
            locate(bad, &f, &k);
            HIPCHK(c, hipMemcpy(&w, d_word.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(&at, d_src.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
            const std::string dg = hex32(digests + 32 * bad);
            if (lengths[bad] == 0)
                return fail(c, MI_ERR_INVALID, "%s: file %llu, row %llu (row %llu of the call) has length 0", who, (unsigned long long)f,
                            (unsigned long long)k, (unsigned long long)bad);
            if (!at)
                return fail(c, MI_ERR_INVALID, "%s: file %llu, row %llu (row %llu of the call): the compressed pack set does not hold digest %s",
                            who, (unsigned long long)f, (unsigned long long)k, (unsigned long long)bad, dg.c_str());
            return fail(c, MI_ERR_INVALID, "%s: file %llu, row %llu (row %llu of the call): the compressed pack set holds digest %s with %u "
                        "bytes, the recipe states %u", who, (unsigned long long)f, (unsigned long long)k, (unsigned long long)bad, dg.c_str(),
                        (u32)w, lengths[bad]);
        }
        // the entropy forms unwrapped first (mi_zentropy.h): d_src and d_word are this call's, their form H rows then point at the
        // inner forms in `unwrap`'s scratch, which lives until the fused kernel has run.  No form H: one launch, nothing else
        ZhUnwrap unwrap;
        rc = unwrap.run(c, who, 0, d_src.as<u64>(), 1u, d_word.as<u64>(), 1u, n_rows);
        if (rc) return rc;
        // the fused kernel: one wave a row, at most 65 536 of them
        const u32 grid = (u32)std::min<u64>(n_rows, 65536);
        HIPCHK(c, hipMemsetAsync(cell, 0xFF, 8, s));
        hipLaunchKernelGGL(zset_restore_kernel, dim3(grid), dim3(64), 0, s, b->arena.as<u8>(), d_dst.as<u64>(), d_src.as<u64>(),
                           d_word.as<u64>(), n_rows, d_rule.as<u32>(), cell);
        HIPCHK(c, hipEventRecord(ev[2], s));
        if (flags & MI_RECIPE_VERIFY) {
            const auto hash_items = (c->cfg.flags & MI_FLAG_CHUNK_BLAKE2S) ? launch_blake2s_items : launch_sha256_items;
            hash_items(kShaBlobs, b->arena.as<u8>(), d_dst.as<u64>(), d_len64.as<u64>(), nullptr, (u32)n_rows, nullptr, c->heads.as<u32>(),
                       nullptr, true, d_got.as<u8>(), c->sha, c->prop.multiProcessorCount, round16(end), s);
            hipLaunchKernelGGL(zset_compare_kernel, dim3(row_blocks), dim3(256), 0, s, d_got.as<u8>(), d_dig.as<u64>(), 4u, n_rows, cell + 1);
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
        u64 lz_bad = h[0];
        u32 lz_rule = 0;
        if (lz_bad != kQNone && lz_bad < n_rows) HIPCHK(c, hipMemcpy(&lz_rule, d_rule.as<u32>() + lz_bad, 4, hipMemcpyDeviceToHost));
        unwrap.merge(&lz_bad, &lz_rule);
        if (lz_bad != kQNone) {                        // a stored form that does not decode: what an unverified set costs its reader
            const u64 bad = lz_bad;
            u64 f = 0, k = 0;
            const u32 rule = lz_rule;
            locate(bad, &f, &k);
            return fail(c, MI_ERR_INVALID, "%s: file %llu, row %llu (row %llu of the call), digest %s: the stored form does not decode: %s", who,
                        (unsigned long long)f, (unsigned long long)k, (unsigned long long)bad, hex32(digests + 32 * bad).c_str(),
                        mi_host::zrule_name(rule));
        }
        if (h[1] != kQNone) {
            const u64 bad = h[1];
            u64 f = 0, k = 0, src = 0;
            locate(bad, &f, &k);
            HIPCHK(c, hipMemcpy(&src, d_src.as<u64>() + bad, 8, hipMemcpyDeviceToHost));
            return fail(c, MI_ERR_IO, "%s: file %llu, row %llu (row %llu of the call), %u bytes at arena offset %llu from source address %#llx: "
                        "the assembled bytes do not hash to the recipe's digest %s", who, (unsigned long long)f, (unsigned long long)k,
                        (unsigned long long)bad, lengths[bad], (unsigned long long)h_dst[bad], (unsigned long long)src,
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
