// mi_zage.hip -- a compressed pack set (mi_zset.hip) that knows WHEN each chunk was last used, and expires by age: a 32-bit stamp
// a table slot on the device, a clock (the set's epoch) the caller advances, and "everything older than epoch E goes" through
// mi_zprune.hip's sweep, compaction and rebuild -- no digest list crosses the host (mi_zset_set_epoch, _get_epoch, _touch,
// _stamps, _age_census, _expire).  Until mi_zset_set_epoch is called none of it exists: no allocation, no launch.
//
//   touch     one thread a row: slot_table_find's walk (the tag first, then all 32 bytes), then atomicExch(&stamps[slot], epoch).
//             The row that gets an old value other than the epoch back is THE one that refreshed that digest: n_refreshed is
//             exact under repeats.  Misses and refreshes by ballot and popcount, one global atomic a wave and value.  The stride
//             from row to row is a parameter: 32 for a digest list, 48 for the six-word records an add has on the device;
//   stamps    one thread a row: find, load, store -- 0xFFFFFFFF for a digest the set lacks;
//   mark      one thread a slot: mark[s] = occupied and stamps[s] < min_epoch.  It fills the per-slot mark array
//             zprune_mark_kernel fills; zprune_sweep_kernel with keep = 0 and everything behind it run unchanged;
//   census    over the slots, grid-stride, at most 2 048 workgroups of 256: the bounds lie in LDS, every thread searches its
//             stamp among them and adds to per-workgroup bins in LDS (256 bins of four values); at the end one global atomic a
//             non-empty bin, value and workgroup;
//   carry     one thread an OLD slot, when a table was rebuilt: the slot's digest is found in the NEW table (complete, no writer)
//             and its stamp stored there.  A digest that was dropped is not found.
//
// Latency-bound table walkers like the ones beside them (an 8-byte tag, then a 48-byte slot, at a random slot); no roof is claimed.
//
// BOUNDS.  touch READS rows [0, stride n) -- the first 32 bytes of each, stride a multiple of 16 --, tags / slots [0, cap) (the
// walk is masked), WRITES stamps at a slot the walk returned (< cap).  stamps READS the same and stamps at such a slot, WRITES
// out [0, n).  mark READS tags, stamps [0, cap), WRITES mark [0, cap).  census READS bounds [0, n_bounds), n_bounds <= 255 (checked on
// the host), tags, slots, stamps [0, cap); the bin comes from the search, which stays in [0, n_bounds]; WRITES out [0, 4 (n_bounds + 1)).
// carry READS old tags, slots, stamps [0, old_cap) and the new table through the masked walk, WRITES new_stamps at a slot the
// walk returned (< new_cap).  Every stamp array holds one u32 a slot of the table it belongs to.
#include "mi_zset_local.h"

using namespace mi;

namespace mi {

constexpr u32 kANone = 0xFFFFFFFFu;                   // no stamp: the set does not hold the digest; as an epoch: reserved
constexpr int kAWG = 256;                             // the census's workgroup
constexpr int kABins = 256;                           // bins: at most 255 bounds
enum : int { kATotUnknown = 0, kATotRefreshed = 1 };

// ---- touch ----------------------------------------------------------------------------------------------------------------------
// the stamp of the slot that holds row r's digest becomes `epoch`; totals (may be NULL): [kATotUnknown] += rows whose digest the
// set does not hold, [kATotRefreshed] += digests whose stamp was another one
__global__ __launch_bounds__(256)
void zage_touch_kernel(const u8* __restrict__ rows, u32 stride, u64 n, const u64* __restrict__ tags, const u64* __restrict__ slots, u64 mask,
                       u32* __restrict__ stamps, u32 epoch, u64* __restrict__ totals) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    bool miss = false, fresh = false;
    if (r < n) {
        const u64 slot = slot_table_find(tags, slots, mask, rows + (u64)stride * r);
        miss = slot == kSlotNone;
        if (!miss) fresh = atomicExch(&stamps[slot], epoch) != epoch;      // (rows that repeat a digest: one of them gets the old stamp)
    }
    if (!totals) return;
    const u64 misses = (u64)__popcll(__ballot(miss)), refreshed = (u64)__popcll(__ballot(fresh));
    if ((threadIdx.x & 63) == 0) {
        if (misses) atomicAdd((unsigned long long*)&totals[kATotUnknown], (unsigned long long)misses);
        if (refreshed) atomicAdd((unsigned long long*)&totals[kATotRefreshed], (unsigned long long)refreshed);
    }
}

// ---- stamps ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void zage_stamps_kernel(const u8* __restrict__ digests, u64 n, const u64* __restrict__ tags, const u64* __restrict__ slots, u64 mask,
                        const u32* __restrict__ stamps, u32* __restrict__ out) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const u64 slot = slot_table_find(tags, slots, mask, digests + 32 * r);
    out[r] = slot == kSlotNone ? kANone : stamps[slot];
}

// ---- mark -----------------------------------------------------------------------------------------------------------------------
// mark[s] = 1 for an occupied slot whose stamp is below min_epoch: what zprune_sweep_kernel (keep = 0) drops
__global__ __launch_bounds__(256)
void zage_mark_kernel(const u64* __restrict__ tags, const u32* __restrict__ stamps, u64 cap, u32 min_epoch, u8* __restrict__ mark) {
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s < cap) mark[s] = tags[s] != 0ull && stamps[s] < min_epoch ? 1 : 0;
}

// ---- census ---------------------------------------------------------------------------------------------------------------------
// out[4 b + 0..3] += digests, stored bytes, round16(stored), chunk bytes of the occupied slots whose stamp lies in bin b: the
// number of bounds at or below it
__global__ __launch_bounds__(kAWG)
void zage_census_kernel(const u64* __restrict__ tags, const u64* __restrict__ slots, u64 cap, const u32* __restrict__ stamps,
                        const u32* __restrict__ bounds, u32 n_bounds, u64* __restrict__ out) {
    __shared__ unsigned long long bins[kABins * 4];
    __shared__ u32 s_bounds[kABins];
    for (int i = threadIdx.x; i < kABins * 4; i += kAWG) bins[i] = 0;
    for (u32 i = threadIdx.x; i < n_bounds; i += kAWG) s_bounds[i] = bounds[i];
    __syncthreads();
    for (u64 s = (u64)blockIdx.x * kAWG + threadIdx.x; s < cap; s += (u64)gridDim.x * kAWG) {
        if (tags[s] == 0ull) continue;
        const u32 stamp = stamps[s];
        const u64 word = slots[kSlotWords * s + 5];
        const u64 len = word & 0xFFFFFFFFull, stored = word >> 32;
        u32 lo = 0, hi = n_bounds;                    // the first bound above the stamp: [0, n_bounds]
        while (lo < hi) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if (s_bounds[mid] <= stamp) lo = mid + 1; else hi = mid;
        }
        unsigned long long* b = bins + 4 * lo;
        atomicAdd(&b[0], 1ull);
        atomicAdd(&b[1], (unsigned long long)stored);
        atomicAdd(&b[2], (unsigned long long)round16(stored));
        atomicAdd(&b[3], (unsigned long long)len);
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < 4 * (n_bounds + 1); i += kAWG)
        if (bins[i]) atomicAdd((unsigned long long*)&out[i], bins[i]);
}

// ---- carry ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void zage_carry_kernel(const u64* __restrict__ old_tags, const u64* __restrict__ old_slots, u64 old_cap, const u32* __restrict__ old_stamps,
                       const u64* __restrict__ new_tags, const u64* __restrict__ new_slots, u64 new_mask, u32* __restrict__ new_stamps) {
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= old_cap || old_tags[s] == 0ull) return;
    const u64 slot = slot_table_find(new_tags, new_slots, new_mask, (const u8*)(old_slots + kSlotWords * s));
    if (slot != kSlotNone) new_stamps[slot] = old_stamps[s];
}

// (hidden: mi_zset_local.h)
int zage_carry_enqueue(mi_ctx* c, const u64* old_tags, const u64* old_slots, u64 old_cap, const u32* old_stamps, const u64* new_tags,
                       const u64* new_slots, u64 new_cap, u32* new_stamps) {
    HIPCHK(c, hipMemsetAsync(new_stamps, 0, new_cap * 4, c->stream));
    hipLaunchKernelGGL(zage_carry_kernel, dim3((u32)((old_cap + 255) / 256)), dim3(256), 0, c->stream, old_tags, old_slots, old_cap, old_stamps, new_tags,
                       new_slots, new_cap - 1, new_stamps);
    return MI_OK;
}

int zage_touch_records_enqueue(const mi_zset* s, const u64* d_recs, u64 n) {
    if (!n) return MI_OK;
    hipLaunchKernelGGL(zage_touch_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, s->ctx->stream, (const u8*)d_recs, (u32)(kSlotWords * 8), n,
                       s->table.tags.as<u64>(), s->table.slots.as<u64>(), s->table.cap - 1, s->stamps.as<u32>(), s->epoch, (u64*)nullptr);
    return MI_OK;
}

}  // namespace mi

namespace {

int does_not_fit(mi_ctx* c, const char* who, hipError_t e, const char* what, u64 bytes) {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP, "%s: %s of %llu bytes does not fit: the device has %llu bytes free (%s)",
                who, what, (unsigned long long)bytes, (unsigned long long)free_b, hipGetErrorString(e));
}

#define AGE_ALLOC(buf, want, what)                                                        \
    do {                                                                                  \
        const hipError_t e_ = (buf).alloc_exact((want));                                  \
        if (e_ != hipSuccess) return does_not_fit(c, who, e_, (what), (want));            \
    } while (0)

int not_ageing(mi_ctx* c, const char* who) {
    return fail(c, MI_ERR_STATE, "%s: the set does not age: mi_zset_set_epoch was never called", who);
}

}  // namespace

extern "C" {

int mi_zset_set_epoch(mi_zset* s, uint32_t epoch) {
    if (!s) return MI_ERR_INVALID;
    static const char* who = "mi_zset_set_epoch";
    mi_ctx* c = nullptr;
    const int rc = mi_zset_ctx(s, who, &c);                    // MI_ERR_STATE with the first message for a set in its failed state
    if (rc) return rc;
    if (epoch == kANone) return fail(c, MI_ERR_INVALID, "%s: epoch 0xFFFFFFFF is reserved: it is what mi_zset_stamps answers for a digest not held", who);
    if (s->ageing) {                                           // the clock only
        if (epoch < s->epoch) return fail(c, MI_ERR_INVALID, "%s: epoch %u is behind the set's, %u", who, epoch, s->epoch);
        s->epoch = epoch;
        return MI_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf stamps;
    StreamDrain drain{st};   // (goes first: the buffer above after it)
    AGE_ALLOC(stamps, s->table.cap * 4, "the stamp array");
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)stamps.p, (int)epoch, s->table.cap, st));    // everything held, and the empty slots with it
    HIPCHK(c, hipStreamSynchronize(st));
    s->stamps = std::move(stamps);
    s->epoch = epoch;
    s->ageing = true;
    return MI_OK;
}

int mi_zset_get_epoch(const mi_zset* s, uint32_t* ageing, uint32_t* epoch, uint64_t* stamp_bytes) {
    if (!s) return MI_ERR_INVALID;
    mi_ctx* c = nullptr;
    const int rc = mi_zset_ctx(s, "mi_zset_get_epoch", &c);
    if (rc) return rc;
    if (ageing) *ageing = s->ageing ? 1u : 0u;
    if (epoch) *epoch = s->epoch;
    if (stamp_bytes) *stamp_bytes = s->stamps.bytes;
    return MI_OK;
}

int mi_zset_touch(mi_zset* s, const uint8_t* digests, uint64_t n, mi_touch_info* info) {
    if (info) memset(info, 0, sizeof *info);
    if (!s || (n && !digests)) return MI_ERR_INVALID;
    static const char* who = "mi_zset_touch";
    mi_ctx* c = nullptr;
    const int rc = mi_zset_ctx(s, who, &c);
    if (rc) return rc;
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu rows, a request holds fewer than 2^32", who, (unsigned long long)n);
    if (!s->ageing) return not_ageing(c, who);
    mi_touch_info ti = {};
    ti.n_rows = n;
    if (n == 0) {
        if (info) *info = ti;
        return MI_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf d_dig, d_tot;
    Event ev[2];
    StreamDrain drain{st};   // (goes first: buffers and events after it)
    for (auto& e : ev) HIPCHK(c, e.create());
    AGE_ALLOC(d_dig, n * 32, "the request");
    AGE_ALLOC(d_tot, 64, "the totals");
    u64* h = c->h_word.as<u64>();
    HIPCHK(c, hipEventRecord(ev[0], st));
    HIPCHK(c, hipMemcpyAsync(d_dig.p, digests, n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_tot.p, 0, 64, st));
    hipLaunchKernelGGL(zage_touch_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_dig.as<u8>(), 32u, n, s->table.tags.as<u64>(),
                       s->table.slots.as<u64>(), s->table.cap - 1, s->stamps.as<u32>(), s->epoch, d_tot.as<u64>());
    HIPCHK(c, hipEventRecord(ev[1], st));
    HIPCHK(c, hipMemcpyAsync(h, d_tot.p, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    ti.n_unknown = h[kATotUnknown];
    ti.n_refreshed = h[kATotRefreshed];
    ti.ms_touch = ms;
    if (ti.n_unknown > n || ti.n_refreshed > n - ti.n_unknown)
        return fail(c, MI_ERR_HIP, "%s: %llu rows, counted %llu unknown and %llu refreshed", who, (unsigned long long)n, (unsigned long long)ti.n_unknown,
                    (unsigned long long)ti.n_refreshed);
    if (info) *info = ti;
    return MI_OK;
}

int mi_zset_stamps(const mi_zset* s, const uint8_t* digests, uint64_t n, uint32_t* stamps) {
    if (!s || (n && (!digests || !stamps))) return MI_ERR_INVALID;
    static const char* who = "mi_zset_stamps";
    mi_ctx* c = nullptr;
    const int rc = mi_zset_ctx(s, who, &c);
    if (rc) return rc;
    if (n >> 32) return fail(c, MI_ERR_INVALID, "%s: %llu rows, a request holds fewer than 2^32", who, (unsigned long long)n);
    if (!s->ageing) return not_ageing(c, who);
    if (n == 0) return MI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf d_dig, d_out;
    StreamDrain drain{st};   // (goes first: the buffers above after it)
    AGE_ALLOC(d_dig, n * 32, "the request");
    AGE_ALLOC(d_out, n * 4, "the answer");
    HIPCHK(c, hipMemcpyAsync(d_dig.p, digests, n * 32, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(zage_stamps_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_dig.as<u8>(), n, s->table.tags.as<u64>(),
                       s->table.slots.as<u64>(), s->table.cap - 1, s->stamps.as<u32>(), d_out.as<u32>());
    HIPCHK(c, hipMemcpyAsync(stamps, d_out.p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return MI_OK;
}

int mi_zset_age_census(const mi_zset* s, const uint32_t* bounds, uint32_t n_bounds, mi_zage_bin* bins) {
    if (!s || !bounds || !bins) return MI_ERR_INVALID;
    static const char* who = "mi_zset_age_census";
    mi_ctx* c = nullptr;
    const int rc = mi_zset_ctx(s, who, &c);
    if (rc) return rc;
    if (n_bounds == 0 || n_bounds >= (u32)kABins) return fail(c, MI_ERR_INVALID, "%s: %u bounds, a census takes 1 to 255", who, n_bounds);
    for (u32 i = 1; i < n_bounds; ++i)
        if (bounds[i] <= bounds[i - 1])
            return fail(c, MI_ERR_INVALID, "%s: bound %u (%u) is not above bound %u (%u): the bounds ascend strictly", who, i, bounds[i], i - 1, bounds[i - 1]);
    if (!s->ageing) return not_ageing(c, who);
    const u64 out_bytes = (u64)(n_bounds + 1) * sizeof(mi_zage_bin);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf d_bounds, d_bins;
    StreamDrain drain{st};   // (goes first: the buffers above after it)
    AGE_ALLOC(d_bounds, n_bounds * 4, "the bounds");
    AGE_ALLOC(d_bins, out_bytes, "the bins");
    HIPCHK(c, hipMemcpyAsync(d_bounds.p, bounds, n_bounds * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_bins.p, 0, out_bytes, st));
    const u32 grid = (u32)std::min<u64>((s->table.cap + kAWG - 1) / kAWG, 2048);
    hipLaunchKernelGGL(zage_census_kernel, dim3(grid), dim3(kAWG), 0, st, s->table.tags.as<u64>(), s->table.slots.as<u64>(), s->table.cap,
                       s->stamps.as<u32>(), d_bounds.as<u32>(), n_bounds, d_bins.as<u64>());
    HIPCHK(c, hipMemcpyAsync(bins, d_bins.p, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    u64 held = 0;
    for (u32 i = 0; i <= n_bounds; ++i) held += bins[i].n_digests;
    if (held != s->table.count)
        return fail(c, MI_ERR_STATE, "%s: the set holds %llu digests, the census counted %llu", who, (unsigned long long)s->table.count, (unsigned long long)held);
    return MI_OK;
}

int mi_zset_expire(mi_zset* s, uint32_t min_epoch, uint32_t min_live_permille, mi_prune_info* info) {
    if (info) memset(info, 0, sizeof *info);
    if (!s) return MI_ERR_INVALID;
    static const char* who = "mi_zset_expire";
    mi_ctx* c = nullptr;
    int rc = mi_zset_ctx(s, who, &c);
    if (rc) return rc;
    if (min_live_permille > 1000) return fail(c, MI_ERR_INVALID, "%s: min_live_permille %u is more than 1000", who, min_live_permille);
    if (!s->ageing) return not_ageing(c, who);
    if (min_epoch > s->epoch)
        return fail(c, MI_ERR_INVALID, "%s: min_epoch %u is above the set's epoch, %u: it would empty the set (MI_ZSET_PRUNE_KEEP with n = 0 does that)", who,
                    min_epoch, s->epoch);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const u64 cap = s->table.cap;
    DevBuf d_dig;
    ZsetSweep sweep;                                           // mi_zprune.hip's, around this call's mark (mi_zset_local.h)
    StreamDrain drain{st};   // (goes first: buffers and events after it)
    // an empty request, as mi_zset_prune allocates one: the two calls' peak_extra_bytes differ by the new stamp array alone
    const hipError_t e = d_dig.alloc_exact(0, &sweep.extra);
    if (e != hipSuccess) return does_not_fit(c, who, e, "the request", 0);
    if ((rc = sweep.begin(s, who))) return rc;
    hipLaunchKernelGGL(zage_mark_kernel, dim3((u32)((cap + 255) / 256)), dim3(256), 0, st, s->table.tags.as<u64>(), s->stamps.as<u32>(), cap, min_epoch,
                       sweep.mark.as<u8>());
    return sweep.finish(s, who, 0, false, min_live_permille, info);
}

}  // extern "C"
