// mi_slot_table.hip -- the pack sets' digest table (mi_slot_table.h): its four kernels and the host's insert and growth.
//
// BOUNDS.  begin / verify index [0, n) of the records and the row scratch; probe walks tags / slots at a MASKED slot and stops
// at the first empty one, which a table under half full always has; export writes out[0, limit) (the cursor is checked).
#include "mi_slot_table.h"

using namespace mi;

namespace mi {

enum : u8 { kRowDone = 0, kRowVerify = 1, kRowProbe = 2 };

__global__ __launch_bounds__(256)
void slot_table_begin_kernel(const u64* __restrict__ recs, u64 n, u64 mask, u8* __restrict__ row_state, u64* __restrict__ row_slot) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    row_state[i] = kRowProbe;
    row_slot[i] = tag_of(recs[kSlotWords * i]) & mask;
}

// walks from the row's slot comparing TAGS only: an empty slot is claimed and the record stored, a slot with an equal tag is
// remembered for the verify kernel, anything else is walked past.  counters[0] += records stored; kSums: [3] += their stored
// bytes, [4] += their lengths -- what a compressed set counts; a plain set's insert is measurably faster without the two sums
// (a global atomic a workgroup and value)
template <bool kSums>
__global__ __launch_bounds__(256)
void slot_table_probe_kernel(const u64* __restrict__ recs, u64 n, u64* __restrict__ tags, u64* __restrict__ slots, u64 mask,
                             u8* __restrict__ row_state, u64* __restrict__ row_slot, u64* __restrict__ counters) {
    __shared__ unsigned long long wg[3];
    if (threadIdx.x < 3) wg[threadIdx.x] = 0;
    __syncthreads();
    u64 mine_new = 0, mine_stored = 0, mine_len = 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        if (row_state[i] != kRowProbe) continue;
        const u64* r = recs + kSlotWords * i;
        const u64 tag = tag_of(r[0]);
        u64 slot = row_slot[i];
        for (;;) {
            const u64 old = atomicCAS((unsigned long long*)&tags[slot], 0ull, (unsigned long long)tag);
            if (old == 0ull) {                               // empty: mine now
                u64* s = slots + kSlotWords * slot;
                s[0] = r[0]; s[1] = r[1]; s[2] = r[2]; s[3] = r[3]; s[4] = r[4]; s[5] = r[5];
                row_state[i] = kRowDone;
                ++mine_new;
                if (kSums) {
                    mine_stored += r[5] >> 32;
                    mine_len += r[5] & 0xFFFFFFFFull;
                }
                break;
            }
            if (old == tag) {                                // full compare after the kernel boundary
                row_slot[i] = slot;
                row_state[i] = kRowVerify;
                break;
            }
            slot = (slot + 1) & mask;
        }
    }
    if (mine_new) {
        atomicAdd(&wg[0], (unsigned long long)mine_new);
        if (kSums) {
            atomicAdd(&wg[1], (unsigned long long)mine_stored);
            atomicAdd(&wg[2], (unsigned long long)mine_len);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && wg[0]) {
        atomicAdd((unsigned long long*)&counters[0], wg[0]);
        if (kSums) {
            atomicAdd((unsigned long long*)&counters[3], wg[1]);
            atomicAdd((unsigned long long*)&counters[4], wg[2]);
        }
    }
}

// equal digests: the chunk is held already (kept once, the first form wins) -- with another LENGTH: counters[2] = the smallest
// such row.  Equal tags, different digests: the row goes on probing behind the slot (counters[1] += 1)
__global__ __launch_bounds__(256)
void slot_table_verify_kernel(const u64* __restrict__ recs, u64 n, const u64* __restrict__ slots, u64 mask, u8* __restrict__ row_state,
                              u64* __restrict__ row_slot, u64* __restrict__ counters) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || row_state[i] != kRowVerify) return;
    const u64 slot = row_slot[i];
    const u64* r = recs + kSlotWords * i;
    const u64* s = slots + kSlotWords * slot;
    if (s[0] == r[0] && s[1] == r[1] && s[2] == r[2] && s[3] == r[3]) {
        if ((u32)s[5] != (u32)r[5]) atomicMin((unsigned long long*)&counters[2], (unsigned long long)i);
        row_state[i] = kRowDone;
    } else {
        row_slot[i] = (slot + 1) & mask;
        row_state[i] = kRowProbe;
        atomicAdd((unsigned long long*)&counters[1], 1ull);
    }
}

// every occupied slot's record to out[0, limit); the cursor counts them all
__global__ __launch_bounds__(256)
void slot_table_export_kernel(const u64* __restrict__ tags, const u64* __restrict__ slots, u64 cap, u64* __restrict__ out, u64 limit,
                              u64* __restrict__ cursor) {
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= cap || tags[s] == 0ull) return;
    const u64 at = atomicAdd((unsigned long long*)cursor, 1ull);
    if (at >= limit) return;
#pragma unroll
    for (int w = 0; w < kSlotWords; ++w) out[kSlotWords * at + w] = slots[kSlotWords * s + w];
}

static int alloc_table(mi_ctx* c, DevBuf* tags, DevBuf* slots, u64 cap) {
    HIPCHK(c, tags->ensure(cap * 8));
    HIPCHK(c, slots->ensure(cap * kSlotWords * 8));
    HIPCHK(c, hipMemsetAsync(tags->p, 0, cap * 8, c->stream));
    return MI_OK;
}

int SlotTable::alloc(mi_ctx* c, u64 new_cap) {
    const int rc = alloc_table(c, &tags, &slots, new_cap);
    if (rc == MI_OK) cap = new_cap;
    return rc;
}

int SlotTable::insert_into(mi_ctx* c, u64* to_tags, u64* to_slots, u64 to_cap, const u64* d_recs, u64 n, u64 sums[3], u64* conflict,
                           const char* what) {
    sums[0] = sums[1] = sums[2] = 0;
    *conflict = kSlotNone;
    if (n == 0) return MI_OK;
    HIPCHK(c, row_state.ensure(n + 16));
    HIPCHK(c, row_slot.ensure(n * 8 + 16));
    HIPCHK(c, counter.ensure(64));
    u64* d_cnt = counter.as<u64>();                     // [0] stored, [1] rows to probe again, [2] smallest conflicting row, [3] [4] bytes
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, 40, c->stream));
    HIPCHK(c, hipMemsetAsync(d_cnt + 2, 0xFF, 8, c->stream));
    const u32 per_row = (u32)((n + 255) / 256);
    const u32 grid = per_row < 2048u ? per_row : 2048u;
    hipLaunchKernelGGL(slot_table_begin_kernel, dim3(per_row), dim3(256), 0, c->stream, d_recs, n, to_cap - 1, row_state.as<u8>(),
                       row_slot.as<u64>());
    u64* h = c->h_word.as<u64>();
    for (u64 round = 0;; ++round) {
        hipLaunchKernelGGL(sum_bytes ? slot_table_probe_kernel<true> : slot_table_probe_kernel<false>, dim3(grid), dim3(256), 0, c->stream,
                           d_recs, n, to_tags, to_slots, to_cap - 1, row_state.as<u8>(), row_slot.as<u64>(), d_cnt);
        hipLaunchKernelGGL(slot_table_verify_kernel, dim3(per_row), dim3(256), 0, c->stream, d_recs, n, to_slots, to_cap - 1,
                           row_state.as<u8>(), row_slot.as<u64>(), d_cnt);
        HIPCHK(c, hipMemcpyAsync(h, d_cnt, 40, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        sums[0] = h[0];
        sums[1] = h[3];
        sums[2] = h[4];
        *conflict = h[2];
        if (h[1] == 0) return MI_OK;                                      // no 64-bit tag collisions (the normal case)
        if (round >= to_cap) return fail(c, MI_ERR_HIP, "%s: probing does not converge", what);
        HIPCHK(c, hipMemsetAsync(d_cnt + 1, 0, 8, c->stream));
    }
}

int SlotTable::insert(mi_ctx* c, const u64* d_recs, u64 n, u64 sums[3], u64* conflict, const char* what) {
    return insert_into(c, tags.as<u64>(), slots.as<u64>(), cap, d_recs, n, sums, conflict, what);
}

void SlotTable::export_records(mi_ctx* c, u64* d_out, u64 limit, u64* d_cursor) const {
    hipLaunchKernelGGL(slot_table_export_kernel, dim3((u32)((cap + 255) / 256)), dim3(256), 0, c->stream, tags.as<u64>(), slots.as<u64>(), cap,
                       d_out, limit, d_cursor);
}

// The new table is complete before the old one goes: a failure leaves the owner as it was
int SlotTable::make_room(mi_ctx* c, u64 n_more, const char* what, const BeforeSwap& before_swap) {
    const u64 need = (count + n_more) * 2;
    if (need <= cap) return MI_OK;
    u64 new_cap = cap ? cap : 1024;
    while (new_cap < need) new_cap <<= 1;
    DevBuf new_tags, new_slots, old;
    int rc = alloc_table(c, &new_tags, &new_slots, new_cap);
    if (rc) return rc;
    if (count) {
        HIPCHK(c, old.ensure(count * kSlotWords * 8));
        HIPCHK(c, counter.ensure(64));
        HIPCHK(c, hipMemsetAsync(counter.p, 0, 8, c->stream));
        export_records(c, old.as<u64>(), count, counter.as<u64>());
        HIPCHK(c, hipMemcpyAsync(c->h_word.p, counter.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const u64 have = c->h_word.as<u64>()[0];
        if (have != count)
            return fail(c, MI_ERR_STATE, "%s holds %llu digests, counted %llu", what, (unsigned long long)have, (unsigned long long)count);
        u64 sums[3], conflict = kSlotNone;
        rc = insert_into(c, new_tags.as<u64>(), new_slots.as<u64>(), new_cap, old.as<u64>(), count, sums, &conflict, what);
        if (rc) return rc;
        if (sums[0] != count)
            return fail(c, MI_ERR_HIP, "%s rebuild lost entries (%llu of %llu)", what, (unsigned long long)sums[0], (unsigned long long)count);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (before_swap && (rc = before_swap(new_tags.as<u64>(), new_slots.as<u64>(), new_cap))) return rc;
    tags = std::move(new_tags);                         // (DevBuf's move swaps: the old table goes with the locals)
    slots = std::move(new_slots);
    cap = new_cap;
    return MI_OK;
}

}  // namespace mi
