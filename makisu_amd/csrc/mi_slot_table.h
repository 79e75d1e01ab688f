// mi_slot_table.h -- the digest-addressed table of the pack sets, once: what a plain pack set (mi_restore.hip) and a compressed
// one (mi_zset.hip, rebuilt by mi_zprune.hip) hold their chunks in.  Open addressing, linear probing, a power of two of slots,
// kept under half full.  tag = the digest's first 8 bytes (0 is stored as 1, 0 = empty); slot = six words: digest 4 | the
// span's ABSOLUTE device address | length in the low half, `stored` in the high half (a plain set leaves it 0).  The insert
// runs in probe-then-verify rounds across a kernel boundary (no thread compares digest bytes another thread of the same launch
// may still be writing); a digest met again is kept once (the first record wins); the same digest with another LENGTH is
// reported.  Grown through export and re-insert: the new table is complete before the old one goes, so a failure leaves the
// owner as it was.  mi_index.hip's table (32-byte slots, known flags) is another one.
#pragma once

#include "mi_internal.h"
#include "mi_wave.h"

#include <functional>

namespace mi {

constexpr int kSlotWords = 6;                               // digest 4 | device address | length, stored
constexpr u64 kSlotNone = ~0ull;

// the slot that holds `digest` (32 bytes on a 16-byte boundary) or kSlotNone: the tag first, then all 32 bytes; the walk is masked
// and ends at an empty slot (the table is under half full).  No thread may write the table during the launch
static __device__ __forceinline__ u64 slot_table_find(const u64* __restrict__ tags, const u64* __restrict__ slots, u64 mask, const u8* digest) {
    const u64 tag = tag_of(*(const u64*)digest);
    u64 slot = tag & mask;
    for (u64 walked = 0; walked <= mask; ++walked) {
        const u64 t = tags[slot];
        if (t == 0ull) break;
        if (t == tag && digest_eq32((const u8*)(slots + kSlotWords * slot), digest)) return slot;
        slot = (slot + 1) & mask;
    }
    return kSlotNone;
}

// The host's side: the table and the row scratch of its inserts.  Everything runs on the ctx stream.  `what` words the owner
// in a message ("pack set", "compressed pack set")
struct MI_LOCAL SlotTable {
    DevBuf tags, slots;                          // cap tags, cap slots of kSlotWords words
    u64 cap = 0;                                 // slots, a power of two
    u64 count = 0;                               // distinct digests held: the OWNER counts (insert says how many were new)
    DevBuf row_state, row_slot, counter;         // an insert's scratch
    bool sum_bytes = false;                      // an insert also sums what it stored (sums[1], sums[2]): a compressed set's counters

    // tags and slots hold cap slots, the tags' memset ENQUEUED -- buffers that are large enough already are kept
    int alloc(mi_ctx* c, u64 new_cap);
    // n records (device, six words each) through the probe-then-verify rounds, ONE synchronisation a round (one round unless
    // 64-bit tags collide): sums[0] of them were not held, with (sum_bytes) sums[1] stored bytes and sums[2] chunk bytes;
    // *conflict = the smallest row whose digest is held with another length (kSlotNone: none)
    int insert(mi_ctx* c, const u64* d_recs, u64 n, u64 sums[3], u64* conflict, const char* what);
    // room for n_more digests under half full: rebuilt at the next power of two that has it.  before_swap (may be empty): called
    // when a rebuilt table is complete and the stream idle, with the OLD table still this one's -- for an owner that keeps something
    // per slot and has to carry it over (mi_zage.hip's stamps); what it returns but MI_OK ends the call, the owner as it was
    using BeforeSwap = std::function<int(const u64* new_tags, const u64* new_slots, u64 new_cap)>;
    int make_room(mi_ctx* c, u64 n_more, const char* what, const BeforeSwap& before_swap = BeforeSwap());
    // ENQUEUED: every occupied slot's record to d_out[0, limit); *d_cursor (zeroed by the caller) counts them all
    void export_records(mi_ctx* c, u64* d_out, u64 limit, u64* d_cursor) const;

private:
    int insert_into(mi_ctx* c, u64* to_tags, u64* to_slots, u64 to_cap, const u64* d_recs, u64 n, u64 sums[3], u64* conflict, const char* what);
};

}  // namespace mi
