// mi_zset_local.h -- what a compressed pack set IS, for the translation units that work on one: mi_zset.hip (create, add,
// cut, restore), mi_zprune.hip (prune in place, usage), mi_zrecode.hip (recode in place) and mi_zage.hip (stamps, expiry by age).
// Host types only: no kernel lives here, and mi_zset.hip's device code does not depend on it.  The table all of them work on is
// a mi::SlotTable (mi_slot_table.h).
#pragma once
#include "mi_slot_table.h"

#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace mi {

// ---- the way up: two pinned windows, one filled by the host while the other's copy runs (mi_restore.hip's SetUploader) -------
constexpr u64 kQWinBytes = 8ull << 20;
struct MI_LOCAL ZsetUploader {
    Stream stream;
    PinBuf buf[2];
    Event ev[2];
    bool busy[2] = {false, false};
    ~ZsetUploader() { if (stream) (void)hipStreamSynchronize(stream); }    // no copy out of a window is under way when the windows go
    int prepare(mi_ctx* c, u64 bytes) {
        const u64 want = std::min<u64>(kQWinBytes, (bytes + 4095) & ~(u64)4095);    // a small blob does not pay for 16 MiB of pinned memory
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
        if (rc == MI_OK && e != hipSuccess) rc = fail(c, MI_ERR_HIP, "mi_zset_add_zblob: upload: %s", hipGetErrorString(e));
        return rc;
    }
};

// a blob the table points into: one added zpack's bytes as stored, or a prune's compaction blob -- memory of its own, and how
// many of its bytes were given (the allocation is that rounded up to 256, plus DevBuf's 256 bytes of slack)
struct ZsetBlob {
    DevBuf mem;
    u64 bytes = 0;
};

// mi_zset.hip, for mi_zserve.hip: MI_ZSET_VERIFY / MI_ZPACK_VERIFY over a compressed blob on the device, its entries on the host
// (structurally sound) and on the device (d_rows: what the digests are held against), n > 0 -- decoded into a scratch laid out as
// a plain pack, hashed there.  *bad = the smallest entry that does not decode (then *rule says why) or, if all decode, that does
// not hash (*rule = 0); ~0: none.  Blocking; the scratch is gone when it returns
MI_LOCAL int zset_verify_stored(mi_ctx* c, const char* who, const void* d_zblob, const mi_zpack_entry* entries, const u64* d_rows, u64 n, u64* bad,
                                u32* rule, double* ms_decode);

// mi_zprune.hip, for mi_zset_prune and mi_zset_expire (mi_zage.hip): a prune around its mark.  begin() allocates what the sweep
// needs -- the per-slot mark array among it --, records where ms_mark begins and enqueues the memsets and the blob bases; the
// CALLER then enqueues, on the ctx stream, whatever sets mark[slot] = 1 for the slots it names and counts the request rows the
// set does not hold into totals[0]; finish() takes that filled mark array and is everything behind it: sweep (keep: the marked
// slots stay / go), the blobs' fates, plan, move, repoint, rebuild, swap -- mi_zset_prune's contract (include/makisu_mi.h) word for
// word.  `extra` is what the call allocated so far (the caller adds its own); the caller holds a StreamDrain declared BEHIND
// this object.  An ageing set's stamps follow the survivors into the new table (zage_carry_enqueue below)
struct MI_LOCAL ZsetSweep {
    DevBuf mark, slot_blob, bases, blob_live, totals;
    Event ev_begin;
    u64 extra = 0;
    std::vector<u32> order;                      // the blobs by base address
    std::vector<u64> h_bases;                    // ... and the addresses, until their copy has run
    int begin(mi_zset* s, const char* who);
    int finish(mi_zset* s, const char* who, u64 n_rows, bool keep, u32 min_live_permille, mi_prune_info* info);
};

// mi_zage.hip, for everything that rebuilds an AGEING set's table (mi_zset.hip's growth inside an add, ZsetSweep::finish,
// mi_zset_recode).  ENQUEUED on the ctx stream: new_stamps [0, new_cap) zeroed, then every occupied old slot's stamp stored at the
// slot that holds its digest in the new table -- which is complete and has no writer; a digest the new table lacks is skipped
MI_LOCAL int zage_carry_enqueue(mi_ctx* c, const u64* old_tags, const u64* old_slots, u64 old_cap, const u32* old_stamps, const u64* new_tags,
                                const u64* new_slots, u64 new_cap, u32* new_stamps);
// ... and for an add: ENQUEUED, the set's epoch into the stamp of every digest among n six-word records on the device -- the
// table holds them all by now and has no writer
MI_LOCAL int zage_touch_records_enqueue(const mi_zset* s, const u64* d_recs, u64 n);

}  // namespace mi

struct mi_zset {
    mi_ctx* ctx = nullptr;
    mi_zset_info info = {};
    std::vector<mi::ZsetBlob> blobs;             // every blob that is resident: the table points into them
    mi::SlotTable table;                         // digest -> the stored span's device address, length | stored << 32 (mi_slot_table.h)
    std::string broken;                          // sticky: the first message of an add that left the table in doubt
    bool ageing = false;                         // mi_zset_set_epoch was called (mi_zage.hip); until then the two below do not exist
    mi::u32 epoch = 0;                           // the set's clock: every held digest's stamp is at most this
    mi::DevBuf stamps;                           // a u32 a table slot: when the digest in it was last used; an empty slot's means nothing
    mi::ZsetUploader up;
};
