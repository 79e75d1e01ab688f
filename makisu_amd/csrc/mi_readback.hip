// mi_readback.hip -- staged bytes back out of HBM: mi_batch_read_file and its kin behind the C ABI of include/makisu_mi.h,
// through the batch's two pinned read-back windows (mi::ReadBack, mi_internal.h).
#include "mi_internal.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <utility>
#include <vector>

using namespace mi;

// Bytes [offset, offset + len) of file `file_index` as they lie in HBM, through pinned windows: a copy brings more than was
// asked for (files that were staged together lie together; a layer's files are asked for in nearly that order); its length
// doubles while reads continue where the last window ended -- 256 KiB when a layer picks single files out of a tree, 8 MiB when
// it streams -- and a reader that streams finds the NEXT range already on its way into the second window: the copy of one
// overlaps the consumption of the other (round 6: with one window every 1 MiB the tar writer asked for was a copy of 1 MiB it
// waited for -- 6 192 of them for 48 x 128 MiB -- and while eight reader threads kept PCIe busy each wait was long enough to
// leave the layer's SHA-256 thread without work: 0.03-0.11 s of a 2.7 s commit, profiles/r06_commit_large_before.txt).
constexpr u64 kReadWinBytes = 8ull << 20, kReadWinMin = 256ull << 10;
int ReadBack::prepare(mi_ctx* c) {
    if (win[0].buf.p) return MI_OK;
    ReadBack rb;                                   // built here and moved in whole: a failure leaves nothing behind, the next call begins again
    HIPCHK(c, rb.stream.create());
    for (auto& w : rb.win) {
        HIPCHK(c, w.buf.ensure(kReadWinBytes));
        HIPCHK(c, w.ev.create(hipEventDisableTiming));
    }
    rb.next = kReadWinMin;
    *this = std::move(rb);                         // (the counters: still zero, nothing counts before the windows exist)
    return MI_OK;
}
// a copy into a window has completed.  MI_STAGE_FAULT=readback:N[:K] (tests): the N-th .. N+K-1-th arrive with a byte flipped
static void window_arrived(mi_ctx* c, ReadBack* rb, void* p, u64 len) {
    const long long k = (long long)rb->copies++;
    if (c->fault_readback >= 0 && k >= c->fault_readback && k < c->fault_readback + c->fault_readback_n && len) ((u8*)p)[len / 2] ^= 0x20;
}
void ReadBack::drop() {
    for (auto& w : win) {
        if (w.pending) (void)hipEventSynchronize(w.ev);
        w.pending = false;
        w.len = 0;
    }
    next = kReadWinMin;
}
void ReadBack::stats(double* wait_s_out, double* fetch_s_out, u64* fetches_out, u64* bytes_out) const {
    if (wait_s_out) *wait_s_out = wait_s;
    if (fetch_s_out) *fetch_s_out = fetch_s;
    if (fetches_out) *fetches_out = fetches;
    if (bytes_out) *bytes_out = bytes;
}
// while_staging: the caller is the pipelined commit (mi_commit.hip) -- the batch is still being staged and scanned by another
// thread; the file's bytes are waited for (stager_wait_landed), nothing else of the batch's state is touched
int ReadBack::read(mi_batch* b, u64 row_end, u64 at, void* dst, u64 len, bool while_staging) {
    mi_ctx* c = b->ctx;
    if (!len) return MI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    {
        const int rc = prepare(c);
        if (rc) return rc;
    }
    const bool staging = while_staging && c->stager;
    // the range behind `from` on its way into window `w` (not waited for): as far as the batch's bytes have landed
    auto prefetch = [&](Win& w, u64 from) -> int {
        w.len = 0;
        if (from >= b->arena_used) return MI_OK;
        u64 want = std::min(next, b->arena_used - from);
        if (staging) {
            const u64 landed = stager_landed(c->stager, b);
            if (landed != ~0ull) {
                if (landed <= from) return MI_OK;
                want = std::min(want, landed - from);
            }
        }
        HIPCHK(c, hipMemcpyAsync(w.buf.p, b->arena.as<u8>() + from, want, hipMemcpyDeviceToHost, stream));
        HIPCHK(c, hipEventRecord(w.ev, stream));
        w.start = from;
        w.len = want;
        w.pending = true;
        ++fetches;
        bytes += want;
        return MI_OK;
    };
    u8* d = (u8*)dst;
    while (len) {
        Win* w = &win[cur];
        if (!(w->len && at >= w->start && at < w->start + w->len)) {
            Win* nx = &win[cur ^ 1];
            const bool follows = w->len && at == w->start + w->len;     // the reader continues where the window ended: it streams
            if (nx->len && at >= nx->start && at < nx->start + nx->len) {
                if (nx->pending) {
                    const auto tf = std::chrono::steady_clock::now();
                    HIPCHK(c, hipEventSynchronize(nx->ev));
                    fetch_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tf).count();
                    nx->pending = false;
                    window_arrived(c, this, nx->buf.p, nx->len);
                }
                cur ^= 1;
                if (follows) next = std::min(next * 2, kReadWinBytes);
                const int rc = prefetch(*w, nx->start + nx->len);        // the window just left takes what follows the new one
                if (rc) return rc;
                continue;
            }
            if (nx->pending) { HIPCHK(c, hipEventSynchronize(nx->ev)); nx->pending = false; }
            nx->len = 0;
            next = follows ? std::min(next * 2, kReadWinBytes) : kReadWinMin;
            u64 want = std::max(next, std::min(len, kReadWinBytes));
            want = std::min(want, b->arena_used - at);
            if (staging) {
                // what was asked for is waited for; the window then takes what ELSE has landed behind it (the neighbours that
                // will be asked for next) and nothing that is still on its way
                const u64 need = std::min(len, std::min(kReadWinBytes, row_end - at));
                u64 landed = ~0ull;
                const auto tw = std::chrono::steady_clock::now();
                const int rc = stager_wait_landed(c->stager, b, at + need, &landed);
                wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
                if (rc) return rc;
                if (landed != ~0ull) want = std::min(want, std::max(need, landed > at ? landed - at : 0));
            }
            const auto tf = std::chrono::steady_clock::now();
            HIPCHK(c, hipMemcpyAsync(w->buf.p, b->arena.as<u8>() + at, want, hipMemcpyDeviceToHost, stream));
            HIPCHK(c, hipStreamSynchronize(stream));
            fetch_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tf).count();
            window_arrived(c, this, w->buf.p, want);
            w->start = at;
            w->len = want;
            w->pending = false;
            ++fetches;
            bytes += want;
            if (follows || want < len) {                                 // streaming (or a read longer than a window): the next range
                const int rc = prefetch(*nx, at + want);                 // sets out while this one is consumed
                if (rc) return rc;
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

extern "C" {

// what every read of a row begins with; *f: the row
static int read_row(mi_batch* b, uint64_t file_index, bool while_staging, const mi_batch::FileRec** f) {
    mi_ctx* c = b->ctx;
    if (!while_staging && (!b->staged || b->in_flight))
        return fail(c, MI_ERR_STATE, "mi_batch_read_file: the batch is not staged, or in flight");
    if (file_index >= b->files.size()) return fail(c, MI_ERR_INVALID, "mi_batch_read_file: no file %llu", (unsigned long long)file_index);
    *f = &b->files[file_index];
    return MI_OK;
}
static int read_file_impl(mi_batch* b, uint64_t file_index, uint64_t offset, void* dst, uint64_t len, bool while_staging) {
    if (!b || (!dst && len)) return MI_ERR_INVALID;
    if (b->group) return group_read_file(b, file_index, offset, dst, len, while_staging);
    mi_ctx* c = b->ctx;
    const mi_batch::FileRec* f = nullptr;
    const int rc = read_row(b, file_index, while_staging, &f);
    if (rc) return rc;
    if (f->part >= 0) return fail(c, MI_ERR_INVALID, "mi_batch_read_file: file %llu is a part", (unsigned long long)file_index);
    if (offset > f->size || len > f->size - offset)
        return fail(c, MI_ERR_INVALID, "mi_batch_read_file: [%llu, +%llu) is outside file %llu of %llu bytes", (unsigned long long)offset,
                    (unsigned long long)len, (unsigned long long)file_index, (unsigned long long)f->size);
    return b->readback.read(b, f->off + f->size, f->off + offset, dst, len, while_staging);
}
// (mi_internal.h) the row is a PART and `offset` a FILE offset inside the part's own range [begin, end): a split file of a batch group
int mi_batch_read_part(mi_batch* b, uint64_t file_index, uint64_t offset, void* dst, uint64_t len, int while_staging) {
    if (!b || (!dst && len)) return MI_ERR_INVALID;
    mi_ctx* c = b->ctx;
    const mi_batch::FileRec* f = nullptr;
    const int rc = read_row(b, file_index, while_staging, &f);
    if (rc) return rc;
    if (f->part < 0) return fail(c, MI_ERR_INVALID, "file %llu is not a part", (unsigned long long)file_index);
    const PartRec& pr = b->parts[f->part];
    if (offset < pr.begin || offset > pr.end || len > pr.end - offset)
        return fail(c, MI_ERR_INVALID, "mi_batch_read_file: [%llu, +%llu) is outside the part [%llu, %llu)", (unsigned long long)offset,
                    (unsigned long long)len, (unsigned long long)pr.begin, (unsigned long long)pr.end);
    return b->readback.read(b, f->off + f->size, f->off + (offset - f->origin), dst, len, while_staging);     // (the staged range begins at file offset `origin`)
}
int mi_batch_read_file(mi_batch* b, uint64_t file_index, uint64_t offset, void* dst, uint64_t len) {
    return read_file_impl(b, file_index, offset, dst, len, false);
}
int mi_batch_read_file_landed(mi_batch* b, uint64_t file_index, uint64_t offset, void* dst, uint64_t len) {   // (hidden: mi_local.h)
    return read_file_impl(b, file_index, offset, dst, len, true);
}

void mi_batch_read_stats(mi_batch* b, double* wait_s, double* fetch_s, uint64_t* fetches, uint64_t* bytes) {
    if (b && b->group) return group_read_stats(b, wait_s, fetch_s, fetches, bytes);
    const ReadBack none;
    (b ? b->readback : none).stats(wait_s, fetch_s, fetches, bytes);
}
// the layer writer's check (mi_layer.hip): the sums of chunk k (1 MiB of the FILE) of a row as they were taken where the bytes were
// read; *has = 0: the batch keeps none for this row.  A split file's chunk lies in the own range of exactly one part (parts begin
// on MiB boundaries of the file).
int mi_batch_chunk_sum(mi_batch* b, uint64_t file_index, uint64_t k, uint64_t* sum_a, uint64_t* sum_b, int* has) {
    if (!b || !has) return MI_ERR_INVALID;
    *has = 0;
    if (b->group) return group_chunk_sum(b, file_index, k, sum_a, sum_b, has);
    if (file_index >= b->files.size()) return MI_ERR_INVALID;
    const mi_batch::FileRec& f = b->files[file_index];
    if (!f.sums) return MI_OK;
    const u64 k0 = f.origin / mi_sum::kChunk;
    if (k < k0 || k - k0 >= mi_sum::chunks_of(f.origin % mi_sum::kChunk + f.size)) return MI_ERR_INVALID;
    *has = 1;
    if (sum_a) *sum_a = f.sums[k - k0].a.load(std::memory_order_relaxed);
    if (sum_b) *sum_b = f.sums[k - k0].b.load(std::memory_order_relaxed);
    return MI_OK;
}
// the read-back windows (two pinned 8 MiB buffers, a stream, two events) ahead of the first read: mi_memfs_reserve_device
int mi_batch_prepare_read(mi_batch* b) {
    if (!b) return MI_ERR_INVALID;
    if (b->group) return group_prepare_read(b);
    HIPCHK(b->ctx, hipSetDevice(b->ctx->device));
    return b->readback.prepare(b->ctx);
}
void mi_batch_drop_windows(mi_batch* b) {
    if (b && b->group) return group_drop_windows(b);
    if (b) b->readback.drop();
}
// A chunk that came back from HBM with other sums than it went with, twice: WHICH hop?  The chunk once more, by a plain copy
// into memory of this call's own (not the windows, not their stream): the same sums as at the source -- HBM holds the right
// bytes and the read-back windows delivered others; other sums -- the arena does not hold what the file had when it was read.
int mi_batch_explain_chunk(mi_batch* b, uint64_t file_index, uint64_t chunk, char* msg, uint64_t cap) {
    if (b && b->group) return group_explain_chunk(b, file_index, chunk, msg, cap);
    if (!b || !msg || !cap || file_index >= b->files.size()) return MI_ERR_INVALID;
    mi_ctx* c = b->ctx;
    const mi_batch::FileRec& f = b->files[file_index];
    const u64 off = chunk * mi_sum::kChunk;                             // in the FILE; the row's bytes begin at f.origin
    const u64 k0 = f.origin / mi_sum::kChunk;
    if (!f.sums || off < f.origin - f.origin % mi_sum::kChunk || off >= f.origin + f.size) return MI_ERR_INVALID;
    const u64 from = off > f.origin ? off : f.origin;                   // (a part's first chunk may begin before its staged bytes)
    const u64 len = std::min(off + mi_sum::kChunk, f.origin + f.size) - from;
    std::vector<u8> again(len);
    (void)hipSetDevice(c->device);
    const hipError_t e = hipMemcpy(again.data(), b->arena.as<u8>() + f.off + (from - f.origin), len, hipMemcpyDeviceToHost);
    u64 a = 0, bb = 0;
    if (e == hipSuccess) mi_sum::chunk_add(again.data(), (size_t)len, (size_t)(from - off), &a, &bb);
    const u64 wa = f.sums[chunk - k0].a.load(), wb = f.sums[chunk - k0].b.load();
    snprintf(msg, (size_t)cap, "arena [%llu, +%llu) (file %llu, bytes [%llu, +%llu)): sums where the bytes were read %016llx/%016llx; %s",
             (unsigned long long)(f.off + (from - f.origin)), (unsigned long long)len, (unsigned long long)file_index, (unsigned long long)from, (unsigned long long)len,
             (unsigned long long)wa, (unsigned long long)wb,
             e != hipSuccess ? "a third copy failed" :
             a == wa && bb == wb ? "a plain copy out of HBM has them: the arena holds the file's bytes, the hop HBM -> pinned read-back window delivered others, twice"
                                 : "a plain copy out of HBM has others too: the arena does not hold what the file held when it was read (the hop pinned slab -> HBM, or HBM itself)");
    return MI_OK;
}

}  // extern "C"
