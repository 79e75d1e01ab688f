// mi_group.hip -- one handle over n batches, one per ctx (one per GPU): mi_memfs_commit_layer_n's batch.
//
// A GROUP HEAD is an mi_batch without arena or stream whose `group` is set (mi_batch_group_begin): a handle behind which the
// file rows of a walk are spread over the member batches, each block / file going to the member with the fewest bytes so far.
// The walk and the commit see ONE batch: the mi_batch_* entry points of mi_api.hip hand a head to the function of this file
// that does the same for a group, and the group calls its members through those same entry points.  The head belongs to
// ctxs[0]: its errors are reported there, "gpu k of n: ..." naming the member.  Host code only.
#include "mi_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>

using namespace mi;

namespace mi {

// a file of MI_COMMIT_SPLIT_MIB (256) MiB and more is SPLIT over the members as parts (mi_batch_add_path_part: the parts protocol)
struct SplitPart { u32 member; u64 row, begin, end; };
struct Split { u64 size; std::vector<SplitPart> parts; };

struct Group {
    std::vector<mi_batch*> members;
    // group row g is row row_row[g] of members[row_member[g]] -- or, with row_member[g] == kGroupSplit, splits[row_row[g]]
    std::vector<u32> row_member;
    std::vector<u64> row_row;
    std::vector<u64> member_bytes;
    std::vector<Split> splits;
    u64 total_bytes = 0, n_chunks = 0;
    bool ran = false;
};

}  // namespace mi

mi_batch::mi_batch() = default;             // here: where Group is a complete type
mi_batch::~mi_batch() = default;

namespace {

constexpr u32 kGroupSplit = 0xFFFFFFFFu;             // row_member of a file that is split over the members as parts
constexpr u64 kGroupAtShift = 48, kGroupAtMask = (1ull << kGroupAtShift) - 1;       // a group's "arena offset": member << 48 | offset

int group_fail(mi_batch* h, size_t k, int rc) {
    return fail(h->ctx, rc, "gpu %zu of %zu: %s", k, h->group->members.size(), ctx_error(h->group->members[k]->ctx).c_str());
}
// call(member, k) on every member in turn; the first failure ends it, reported on the head's ctx with the member's name
template <typename F>
int each_member(mi_batch* h, F call) {
    for (size_t k = 0; k < h->group->members.size(); ++k) {
        const int rc = call(h->group->members[k], k);
        if (rc) return group_fail(h, k, rc);
    }
    return MI_OK;
}
size_t group_least_loaded(const Group& G) {
    size_t k = 0;
    for (size_t i = 1; i < G.members.size(); ++i) if (G.member_bytes[i] < G.member_bytes[k]) k = i;
    return k;
}

// Which member and row hold file offset `off` of group row g?  An ordinary row: that row, whatever `off`.  A split row (`split`
// set): the part whose own range [begin, end) holds `off` -- parts begin on MiB boundaries of the file, so a 1 MiB chunk lies in
// the own range of exactly one.  false: no row g, or no part of the split file holds `off`.
struct RowAt { u32 member = 0; u64 row = 0; const Split* split = nullptr; const SplitPart* part = nullptr; };
bool group_row_at(const Group& G, u64 g, u64 off, RowAt* at) {
    *at = RowAt{};
    if (g >= G.row_member.size()) return false;
    at->member = G.row_member[g];
    at->row = G.row_row[g];
    if (at->member != kGroupSplit) return true;
    at->split = &G.splits[at->row];
    for (const SplitPart& pt : at->split->parts)
        if (off >= pt.begin && off < pt.end) { at->part = &pt; at->member = pt.member; at->row = pt.row; return true; }
    return false;
}

// The parts of the group's split files agree on their boundary cuts (the parts protocol of include/makisu_mi.h, all owners in
// this process): every member that holds parts makes its cuts under an assumed entry; then, round by round, every part but a
// file's first is told its predecessor's last cut and the members re-select where that differed -- until no exit moved (one
// round on ordinary data, at most parts-per-file).
int group_resolve_parts(mi_batch* h) {
    Group& G = *h->group;
    const size_t nm = G.members.size();
    std::vector<char> holds(nm, 0);
    for (const Split& sp : G.splits) for (const SplitPart& pt : sp.parts) holds[pt.member] = 1;
    {
        std::vector<int> rcs(nm, MI_OK);
        std::vector<std::thread> th;
        for (size_t k = 0; k < nm; ++k) if (holds[k]) th.emplace_back([&, k] { rcs[k] = mi_batch_scan_cuts(G.members[k]); });
        for (auto& t : th) t.join();
        const int rc = each_member(h, [&](mi_batch*, size_t k) { return rcs[k]; });
        if (rc) return rc;
    }
    for (int round = 0; round < 70; ++round) {
        std::vector<std::vector<mi_part_state>> st(nm);
        int rc = each_member(h, [&](mi_batch* m, size_t k) {
            if (!holds[k]) return (int)MI_OK;
            uint64_t np = 0;
            mi_batch_parts(m, nullptr, 0, &np);
            st[k].resize(np ? np : 1);
            const int rc = mi_batch_parts(m, st[k].data(), np, &np);
            st[k].resize(np);
            return rc;
        });
        if (rc) return rc;
        auto state_of = [&](const SplitPart& pt) -> const mi_part_state* {
            for (const mi_part_state& x : st[pt.member]) if (x.file_index == pt.row) return &x;
            return nullptr;
        };
        bool redo = false;
        for (const Split& sp : G.splits)
            for (size_t i = 1; i < sp.parts.size(); ++i) {
                const mi_part_state *prev = state_of(sp.parts[i - 1]), *cur = state_of(sp.parts[i]);
                if (!prev || !cur) return fail(h->ctx, MI_ERR_STATE, "a split file's part is not among its member's parts");
                if (prev->exit != cur->entry) redo = true;
                if (prev->exit != cur->entry || !cur->entry_confirmed) {
                    rc = mi_batch_set_part_entry(G.members[sp.parts[i].member], sp.parts[i].row, prev->exit);
                    if (rc) return group_fail(h, sp.parts[i].member, rc);
                }
            }
        rc = each_member(h, [&](mi_batch* m, size_t k) { return holds[k] ? mi_batch_fix_cuts(m) : (int)MI_OK; });
        if (rc) return rc;
        if (!redo) return MI_OK;
    }
    return fail(h->ctx, MI_ERR_STATE, "the parts of a split file did not agree on their boundary cuts in 70 rounds");
}

}  // namespace

namespace mi {

void group_expect_host_bytes(mi_batch* h) { for (mi_batch* m : h->group->members) mi_batch_expect_host_bytes(m); }

int group_add_paths(mi_batch* h, u64 n, const char* const* paths, const u64* sizes, const u64* user_tags) {
    // each file to the member with the fewest bytes so far (the streaming form of longest-processing-time-first: the walk
    // hands files over as it finds them); a member's files keep the walk's order among themselves
    Group& G = *h->group;
    const size_t nm = G.members.size();
    std::vector<std::vector<const char*>> mp(nm);
    std::vector<std::vector<u64>> ms(nm), mt(nm);
    static const u64 split_min = [] {
        const char* e = getenv("MI_COMMIT_SPLIT_MIB");
        const long v = e && *e ? atol(e) : 256;
        return v <= 0 ? ~0ull : (u64)v << 20;
    }();
    auto flush = [&](mi_batch* m, size_t k) {                  // member k's pending files, in the walk's order
        const int rc = mp[k].empty() ? (int)MI_OK : mi_batch_add_paths(m, mp[k].size(), mp[k].data(), ms[k].data(), mt[k].data());
        mp[k].clear(); ms[k].clear(); mt[k].clear();
        return rc;
    };
    for (u64 i = 0; i < n; ++i) {
        if (sizes[i] >= split_min && sizes[i] >= 2 * mi_sum::kChunk) {
            // A file of 256 MiB and more is SPLIT: one part per member, at most -- each part to the member with
            // the fewest bytes so far, staged over that GPU's own link behind its halo (mi_batch_add_path_part).  Parts begin
            // on MiB boundaries of the file, so every 1 MiB chunk the tar writer checks lies in ONE part's own range.  The
            // parts' owners agree on the boundary cuts when the group runs (group_resolve_parts).
            u64 np = std::min<u64>(nm, sizes[i] / (split_min / 2 ? split_min / 2 : 1));
            if (np < 2) np = 2;
            const u64 step = (sizes[i] / np + mi_sum::kChunk - 1) / mi_sum::kChunk * mi_sum::kChunk;
            Split sp;
            sp.size = sizes[i];
            for (u64 begin = 0; begin < sizes[i]; begin += step) {
                const u64 end = std::min(begin + step, (u64)sizes[i]);
                const size_t k = group_least_loaded(G);
                // (the member's earlier pending files first: a part is added at once, its row must follow theirs)
                const int rc0 = flush(G.members[k], k);
                if (rc0) return group_fail(h, k, rc0);
                const u64 row = G.members[k]->files.size();
                const int rc = mi_batch_add_path_part(G.members[k], paths[i], sizes[i], begin, end, user_tags ? user_tags[i] : 0);
                if (rc) return group_fail(h, k, rc);
                G.member_bytes[k] += end - begin;
                sp.parts.push_back({(u32)k, row, begin, end});
            }
            G.row_member.push_back(kGroupSplit);
            G.row_row.push_back(G.splits.size());
            G.splits.push_back(std::move(sp));
            G.total_bytes += sizes[i];
            continue;
        }
        const size_t k = group_least_loaded(G);
        G.member_bytes[k] += sizes[i] + 4096;                 // (a file costs something even when it is empty: rows, a descriptor)
        G.row_member.push_back((u32)k);
        G.row_row.push_back(G.members[k]->files.size() + mp[k].size());
        mp[k].push_back(paths[i]);
        ms[k].push_back(sizes[i]);
        mt[k].push_back(user_tags ? user_tags[i] : 0);
        G.total_bytes += sizes[i];
    }
    return each_member(h, flush);
}

// the whole block -- a directory's small files -- to ONE member
int group_add_block(mi_batch* h, const void* src, u64 len, void (*release)(void*), void* release_arg, u64* at_out) {
    Group& G = *h->group;
    const size_t k = group_least_loaded(G);
    uint64_t at = 0;
    const int rc = mi_batch_add_block(G.members[k], src, len, release, release_arg, &at);
    if (rc) return group_fail(h, k, rc);
    G.member_bytes[k] += len;
    if (at_out) *at_out = ((u64)k << kGroupAtShift) | at;
    return MI_OK;
}

// rows of blocks that went to different members, in the walk's order
int group_add_placed(mi_batch* h, u64 n, const u64* arena_off, const u64* sizes, const u64* tags, const u64* sums) {
    Group& G = *h->group;
    const size_t nm = G.members.size();
    std::vector<std::vector<u64>> mo(nm), ms(nm), mt(nm), mq(nm);
    for (u64 i = 0; i < n; ++i) {
        const size_t k = (size_t)(arena_off[i] >> kGroupAtShift);
        if (k >= nm) return fail(h->ctx, MI_ERR_INVALID, "mi_batch_add_placed: no such member");
        G.row_member.push_back((u32)k);
        G.row_row.push_back(G.members[k]->files.size() + mo[k].size());
        mo[k].push_back(arena_off[i] & kGroupAtMask);
        ms[k].push_back(sizes[i]);
        mt[k].push_back(tags ? tags[i] : 0);
        if (sums) { mq[k].push_back(sums[2 * i]); mq[k].push_back(sums[2 * i + 1]); }
        G.total_bytes += sizes[i];
    }
    return each_member(h, [&](mi_batch* m, size_t k) {
        return mo[k].empty() ? (int)MI_OK : mi_batch_add_placed(m, mo[k].size(), mo[k].data(), ms[k].data(), mt[k].data(), sums ? mq[k].data() : nullptr);
    });
}

int group_keeps_sums(mi_batch* h) { return h->group->members[0]->keep_sums ? 1 : 0; }
void group_keep_sums(mi_batch* h, int on) {
    if (h->group->row_member.empty()) for (mi_batch* m : h->group->members) mi_batch_keep_sums(m, on);
}

// every member its share and a quarter (the split is by bytes, not exact)
int group_reserve(mi_batch* h, u64 more_files, u64 more_bytes, bool ahead) {
    const u64 nm = h->group->members.size();
    return each_member(h, [&](mi_batch* m, size_t) {
        return (ahead ? mi_batch_reserve_ahead : mi_batch_reserve)(m, more_files / nm + 1, more_bytes / nm + more_bytes / (4 * nm));
    });
}

// every member on a thread of its own: one GPU each
int group_run(mi_batch* h) {
    Group& G = *h->group;
    const size_t nm = G.members.size();
    if (!G.splits.empty()) {
        const int rc = group_resolve_parts(h);
        if (rc) return rc;
    }
    std::vector<int> rcs(nm, MI_OK);
    std::vector<std::thread> th;
    for (size_t k = 1; k < nm; ++k) th.emplace_back([&, k] { rcs[k] = mi_batch_run(G.members[k]); });
    rcs[0] = mi_batch_run(G.members[0]);
    for (auto& t : th) t.join();
    G.n_chunks = 0;
    const int rc = each_member(h, [&](mi_batch* m, size_t k) {
        if (!rcs[k]) G.n_chunks += m->n_chunks;
        return rcs[k];
    });
    if (rc) return rc;
    G.ran = true;
    return MI_OK;
}

int group_reset(mi_batch* h) {
    Group& G = *h->group;
    const int rc = each_member(h, [](mi_batch* m, size_t) { return mi_batch_reset(m); });
    if (rc) return rc;
    if (h->tree) { mi_batch_tree_free(h->tree); h->tree = nullptr; }
    G.row_member.clear();
    G.row_row.clear();
    G.splits.clear();
    G.member_bytes.assign(G.members.size(), 0);
    G.total_bytes = 0;
    G.n_chunks = 0;
    G.ran = false;
    return MI_OK;
}

int group_counts(mi_batch* h, u64* n_files, u64* n_chunks, u64* n_bytes) {
    if (n_files) *n_files = h->group->row_member.size();
    if (n_chunks) *n_chunks = h->group->n_chunks;
    if (n_bytes) *n_bytes = h->group->total_bytes;
    return MI_OK;
}

// the members' roots, put back into the walk's order
int group_roots(mi_batch* h, u8* out, u64 cap) {
    Group& G = *h->group;
    if (!G.ran) return fail(h->ctx, MI_ERR_STATE, "roots requested before mi_batch_run");
    const u64 nf = G.row_member.size();
    if (cap < nf) return fail(h->ctx, MI_ERR_CAPACITY, "root buffer holds %llu rows, need %llu", (unsigned long long)cap, (unsigned long long)nf);
    std::vector<std::vector<u8>> mr(G.members.size());
    int rc = each_member(h, [&](mi_batch* m, size_t k) {
        const u64 n = m->files.size();
        mr[k].resize(n * 32 + 32);
        return mi_batch_roots(m, mr[k].data(), n);
    });
    if (rc) return rc;
    for (u64 g = 0; g < nf; ++g) {
        if (G.row_member[g] != kGroupSplit) { memcpy(out + 32 * g, mr[G.row_member[g]].data() + 32 * G.row_row[g], 32); continue; }
        // a split file's root: mi_chunk_root_alg over its parts' chunk digests put end to end (include/makisu_mi.h, "parts")
        std::vector<u8> dg;
        for (const SplitPart& pt : G.splits[G.row_row[g]].parts) {
            const mi_file_result* fr = nullptr;
            const mi_chunk_result* cr = nullptr;
            uint64_t n1 = 0, n2 = 0;
            rc = mi_batch_files_view(G.members[pt.member], &fr, &n1);
            if (!rc) rc = mi_batch_chunks_view(G.members[pt.member], &cr, &n2);
            if (rc) return group_fail(h, pt.member, rc);
            const mi_file_result& f = fr[pt.row];
            for (u64 j = 0; j < f.n_chunks; ++j) { const u8* d = cr[f.first_chunk + j].sha256; dg.insert(dg.end(), d, d + 32); }
        }
        uint32_t alg = MI_DIGEST_SHA256;                              // (the members' ctxs agree: group_begin)
        (void)mi_ctx_chunk_digest(h->ctx, &alg);
        rc = mi_chunk_root_alg(alg, dg.data(), dg.size() / 32, out + 32 * g);
        if (rc) return fail(h->ctx, rc, "the root of a split file");
    }
    return MI_OK;
}

// from the GPU that holds the file -- a split file: from the GPUs that hold its parts
int group_read_file(mi_batch* h, u64 file_index, u64 offset, void* dst, u64 len, bool while_staging) {
    const Group& G = *h->group;
    RowAt at;
    if (!group_row_at(G, file_index, offset, &at) && !at.split)
        return fail(h->ctx, MI_ERR_INVALID, "mi_batch_read_file: no file %llu", (unsigned long long)file_index);
    if (!at.split) {
        const int rc = (while_staging ? mi_batch_read_file_landed : mi_batch_read_file)(G.members[at.member], at.row, offset, dst, len);
        return rc ? group_fail(h, at.member, rc) : MI_OK;
    }
    if (offset > at.split->size || len > at.split->size - offset)
        return fail(h->ctx, MI_ERR_INVALID, "mi_batch_read_file: outside split file %llu", (unsigned long long)file_index);
    u8* d = (u8*)dst;
    while (len && group_row_at(G, file_index, offset, &at)) {        // (the parts lie end to end: every offset below the size is in one)
        const u64 take = std::min(len, at.part->end - offset);
        const int rc = mi_batch_read_part(G.members[at.member], at.row, offset, d, take, while_staging);
        if (rc) return group_fail(h, at.member, rc);
        d += take;
        offset += take;
        len -= take;
    }
    return MI_OK;
}

void group_read_stats(mi_batch* h, double* wait_s, double* fetch_s, u64* fetches, u64* bytes) {
    double w = 0, f = 0;
    uint64_t nf = 0, nb = 0;
    for (mi_batch* m : h->group->members) { w += m->readback.wait_s; f += m->readback.fetch_s; nf += m->readback.fetches; nb += m->readback.bytes; }
    if (wait_s) *wait_s = w;
    if (fetch_s) *fetch_s = f;
    if (fetches) *fetches = nf;
    if (bytes) *bytes = nb;
}

int group_chunk_sum(mi_batch* h, u64 file_index, u64 k, u64* sum_a, u64* sum_b, int* has) {
    RowAt at;
    if (!group_row_at(*h->group, file_index, k * mi_sum::kChunk, &at)) return at.split && at.split->size == 0 ? MI_OK : MI_ERR_INVALID;
    return mi_batch_chunk_sum(h->group->members[at.member], at.row, k, sum_a, sum_b, has);
}

int group_prepare_read(mi_batch* h) { return each_member(h, [](mi_batch* m, size_t) { return mi_batch_prepare_read(m); }); }
void group_drop_windows(mi_batch* h) { for (mi_batch* m : h->group->members) mi_batch_drop_windows(m); }

int group_explain_chunk(mi_batch* h, u64 file_index, u64 chunk, char* msg, u64 cap) {
    RowAt at;
    if (!msg || cap < 16 || !group_row_at(*h->group, file_index, chunk * mi_sum::kChunk, &at)) return MI_ERR_INVALID;
    const int n = snprintf(msg, (size_t)cap, "gpu %u: ", at.member);
    return mi_batch_explain_chunk(h->group->members[at.member], at.row, chunk, msg + n, cap - (uint64_t)n);
}

int group_file_size(mi_batch* h, u64 file_index, u64* size) {
    RowAt at;
    if (!size || (!group_row_at(*h->group, file_index, 0, &at) && !at.split)) return MI_ERR_INVALID;
    if (at.split) { *size = at.split->size; return MI_OK; }
    return mi_batch_file_size(h->group->members[at.member], at.row, size);
}

int group_arena_info(mi_batch* h, u64* bytes, u64* pieces, u64* moves) {
    uint64_t tb = 0, tp = 0, tm = 0;
    for (mi_batch* m : h->group->members) { uint64_t x = 0, y = 0, z = 0; mi_batch_arena_info(m, &x, &y, &z); tb += x; tp += y; tm += z; }
    if (bytes) *bytes = tb;
    if (pieces) *pieces = tp;
    if (moves) *moves = tm;
    return MI_OK;
}

// what every member can count on: the smallest
int group_arena_room(mi_batch* h, u64* bytes) {
    *bytes = ~0ull;
    for (mi_batch* m : h->group->members) if (m->arena.bytes < *bytes) *bytes = m->arena.bytes;
    return MI_OK;
}

int group_free(mi_batch* h) {
    if (h->tree) { mi_batch_tree_free(h->tree); h->tree = nullptr; }
    for (mi_batch* m : h->group->members) mi_batch_free(m);
    --h->ctx->live_children;
    delete h;
    return MI_OK;
}

}  // namespace mi

extern "C" {

// The head belongs to ctxs[0]; it has no device state of its own.
int mi_batch_group_begin(mi_ctx* const* ctxs, uint32_t n, mi_batch** out) {
    if (!ctxs || n < 2 || n > 64 || !out) return MI_ERR_INVALID;
    for (uint32_t i = 0; i < n; ++i) {
        if (!ctxs[i]) return MI_ERR_INVALID;
        for (uint32_t j = 0; j < i; ++j) if (ctxs[j] == ctxs[i]) return fail(ctxs[0], MI_ERR_INVALID, "a batch group needs %u DIFFERENT ctxs", n);
    }
    for (uint32_t i = 1; i < n; ++i)                                  // one root per file, whichever member hashed it
        if ((ctxs[i]->cfg.flags ^ ctxs[0]->cfg.flags) & MI_FLAG_CHUNK_BLAKE2S)
            return fail(ctxs[0], MI_ERR_INVALID, "the ctxs of a batch group hash chunks with different algorithms (MI_FLAG_CHUNK_BLAKE2S)");
    mi_batch* h = new mi_batch();
    h->ctx = ctxs[0];
    h->group.reset(new Group());
    ++h->ctx->live_children;
    for (uint32_t i = 0; i < n; ++i) {
        mi_batch* m = nullptr;
        const int rc = mi_batch_begin(ctxs[i], 0, 0, &m);
        if (rc) {
            const std::string e = ctx_error(ctxs[i]);
            group_free(h);
            return fail(ctxs[0], rc, "gpu %u of %u: %s", i, n, e.c_str());
        }
        h->group->members.push_back(m);
    }
    h->group->member_bytes.assign(n, 0);
    *out = h;
    return MI_OK;
}
uint64_t mi_batch_group_splits(mi_batch* b) { return b && b->group ? b->group->splits.size() : 0; }
int mi_batch_group_members(mi_batch* b, mi_batch* const** members, const uint64_t** bytes, uint64_t* n) {   // (n = 0: not a group)
    if (!b || !n) return MI_ERR_INVALID;
    *n = b->group ? b->group->members.size() : 0;
    if (*n && members) *members = b->group->members.data();
    if (*n && bytes) *bytes = b->group->member_bytes.data();
    return MI_OK;
}

}  // extern "C"
