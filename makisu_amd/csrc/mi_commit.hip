// mi_commit.hip -- step.commitLayer in ONE call on the MemFS handle, mi_memfs_commit_layer / mi_memfs_commit_layer_n, on the
// host (no device code here) -- with a ctx THE SEAM of this library: the walk stages every file into one
// batch, the GPU cuts and hashes them, the diff runs with chunk roots (a path is in the layer if its header changed OR its
// content did), the layer tar is framed from the bytes in HBM; the scan runs on a thread of its own beside the diff and the
// writer (ScanJob), and with MI_MEMFS_TRUST_CTIME only files whose inode changed are read at all.  Beside it what belongs to
// a commit: the handle's batch and its one owner (mi_memfs_reserve_device / mi_memfs_release_device), the commit's stats,
// options and chunk index.  The handle and its tree: mi_copyfs.h; the scan's diff: mi_memfs.hip; the ops: mi_copyops.hip.
#include "mi_copyfs.h"

// ---- the commit's knobs: the environment is read here and nowhere else in this file ----------------------------------
// the first three once per process:
//   MI_COMMIT_PIPELINE=0        one phase after the other (default: the scan on a thread of its own, see Commit::start_scan)
//   MI_COMMIT_FORCE_WINDOWS=1   (tests) as if the tree / the sources did not fit the device
//   MI_COMMIT_VERIFY=0          (measurements) no sums at the source, no check in the layer writer
struct CommitKnobs { bool pipeline, force_windows; int verify; };
static const CommitKnobs& commit_knobs() {
    static const CommitKnobs k = [] {
        const char *p = getenv("MI_COMMIT_PIPELINE"), *w = getenv("MI_COMMIT_FORCE_WINDOWS"), *v = getenv("MI_COMMIT_VERIFY");
        return CommitKnobs{!(p && *p == '0'), w && *w == '1', !(v && *v == '0') ? 1 : 0};
    }();
    return k;
}
//   MI_COMMIT_WINDOW_MB         the window of a tree that is scanned in windows, read at every such commit (0 / unset: the
//                               arena's room decides); *given: the variable is set -- then the window may go below 64 MiB
static uint64_t commit_window_bytes(bool* given) {
    const char* e = getenv("MI_COMMIT_WINDOW_MB");
    *given = e != nullptr;
    return e ? (uint64_t)atol(e) << 20 : 0;
}

// ---- the handle's batch: ONE record of the ctxs it was made for, these two functions its only writers ------------------
// the commit's batch (its arena holds the last scanned tree's bytes) is given back; the next content-aware commit begins anew
// MI_MEMFS_CHUNK_PACK: a pack nobody took goes; until the next commit's pack a take says `why` with `rc`
static void memfs_pack_drop(mi_memfs* m, int rc, const std::string& why) {
    if (m->pack) mi_pack_free(m->pack);
    m->pack = nullptr;
    m->pack_rc = rc;
    m->pack_err = why;
}
// MI_MEMFS_CHUNK_ZPACK: the same for the compressed pack
static void memfs_zpack_drop(mi_memfs* m, int rc, const std::string& why) {
    if (m->zpack) mi_zpack_free(m->zpack);
    m->zpack = nullptr;
    m->zpack_rc = rc;
    m->zpack_err = why;
}
static int memfs_batch_drop(mi_memfs* m) {
    memfs_pack_drop(m, MI_ERR_STATE, "no commit since the device was released");      // (a pack is a child of the ctx, as the batch is)
    memfs_zpack_drop(m, MI_ERR_STATE, "no commit since the device was released");
    int rc = MI_OK;
    if (m->batch) rc = mi_batch_free(m->batch);
    m->batch = nullptr;
    m->batch_ctxs.clear();
    return rc;
}
// the handle's batch for these ctxs, empty: the one it has if it was made for the same ctxs (mi_batch_reset), else a new one
// in its place (files_hint: what a single ctx's batch is told to expect)
static int memfs_batch_for(mi_memfs* m, mi_ctx* const* ctxs, uint32_t n_ctx, uint64_t files_hint) {
    const std::vector<mi_ctx*> want(ctxs, ctxs + n_ctx);
    if (m->batch && m->batch_ctxs != want) (void)memfs_batch_drop(m);
    int rc;
    if (m->batch) rc = mi_batch_reset(m->batch);
    else {
        rc = n_ctx > 1 ? mi_batch_group_begin(ctxs, n_ctx, &m->batch) : mi_batch_begin(ctxs[0], files_hint, 0, &m->batch);
        m->batch_ctxs = want;
    }
    if (!rc) mi_batch_keep_sums(m->batch, commit_knobs().verify);                 // the tar is framed from HBM: held against what was read
    return rc;
}

// step.commitLayer (lib/builder/step/common.go:67-111) on the handle: the step's layer by scan (ctx.MustScan) or by its
// copy operations, through tarAndGzipDiffs' pipeline (the layer writer: tar framing, TarDigest, gzip leg, its digest and
// size), folded into the tree; nothing to do = *committed 0.  The walk of a scan happens here, with the handle's
// blacklist.  (MemFS.sync's one-second wait before either stays with the caller.)
//
// ctx == NULL: the reference's commit -- headers decide what changed (tario.IsSimilarHeader), the layer writer reads the
// changed files from disk.
// ctx != NULL: THE SEAM the GPU path exists for (mem_fs.go:315-341,487-503 + common.go:67-111 in one flow):
//     walk + stage   the root (must_scan) or the ops' sources are walked and every regular file they list is staged into
//                    ONE batch while the walk goes on (mi_batch_add_tree's way: small files read where they are listed,
//                    large ones by the reader threads) -- each file is opened and read ONCE;
//     scan           Gear CDC + SHA-256 per chunk + per-file chunk roots on the GPU (mi_batch_run);
//     diff           createLayerByScan / addToLayer with the roots: a path is in the layer if its header changed OR its
//                    content did (same size, same second, other bytes: invisible to the reference); unchanged files whose
//                    node had no root yet take theirs, so the next commit can tell;
//     write          the layer writer frames the tar; a regular file's bytes come from HBM -- the very bytes the root
//                    describes (mi_layer_add_batch_file) -- not from a second read of a file that may have moved on;
//     index          optionally (mi_memfs_set_index) the batch's chunk digests join the chunk index.
static double secs_since(const std::chrono::steady_clock::time_point& t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
static int memfs_commit_write(mi_memfs* m, mi_copy_layer* cl, uint64_t ne, const mi_layer_config* cfg, mi_layer_result* res,
                              mi_batch* batch, bool pipelined, mi_ctx* gzip_ctx) {
    std::vector<mi_tree_entry> ents(ne ? ne : 1);
    std::vector<const char*> srcs(ne ? ne : 1);
    int rc = mi_copy_layer_entries(cl, ents.data(), srcs.data(), ne);
    mi_layer* lw = nullptr;
    if (rc) m->err = "failed to generate diff layer: layer entries";
    if (!rc && (rc = mi_layer_begin(cfg, &lw))) m->err = "failed to generate diff layer: the layer writer refused its configuration";
    if (lw && pipelined) mi_layer_set_pipelined(lw, 1);        // a file's bytes are waited for where they have not landed yet
    // MI_MEMFS_GZIP_DEVICE: the gzip leg is coded on the first ctx's device (no effect where there is nothing to code)
    if (lw && gzip_ctx && cfg->gzip_level != MI_GZIP_OFF && cfg->gzip_level != 0 && (rc = mi_layer_set_gzip_ctx(lw, gzip_ctx)))
        m->err = std::string("failed to generate diff layer: the device gzip leg: ") + mi_layer_error(lw);
    for (uint64_t i = 0; i < ne && !rc; ++i) {
        const mi_copy::Node& nd = cl->nodes[i];
        if (ents[i].kind == 1 && ents[i].file_index >= 0) { ++m->last.n_layer_files; m->last.layer_file_bytes += ents[i].size; }
        if (batch && ents[i].kind == 1 && ents[i].file_index >= 0 && nd.batch_file >= 0 && nd.batch_gen == m->fs.commit_gen)
            rc = mi_layer_add_batch_file(lw, &ents[i], batch, (uint64_t)nd.batch_file);
        else
            rc = mi_layer_add(lw, &ents[i], ents[i].kind == 1 && srcs[i] && srcs[i][0] ? srcs[i] : nullptr);
        if (rc) m->err = std::string("failed to generate diff layer: write diffs: commit layer: ") + mi_layer_error(lw);
    }
    if (!rc) {
        rc = mi_layer_finish(lw, res);
        if (rc) m->err = std::string("failed to generate diff layer: ") + mi_layer_error(lw);
    }
    if (lw) {
        uint64_t o = 0, by = 0;
        mi_layer_io_counts(lw, &o, &by);
        m->last.files_opened += o;
        m->last.file_bytes_read += by;
        mi_layer_verify_counts(lw, &m->last.n_verified_files, &m->last.verified_bytes, &m->last.n_refetched);
        mi_layer_free(lw);
    }
    return rc;
}

// A tree that does not fit the device: the chunk roots of its regular files, computed in WINDOWS -- runs of files (walk order) the
// batch has room for; each window is staged, scanned and forgotten.  roots: 32 bytes per regular file, by the file's ordinal
// (a scanned tree: mi_tree_walk's numbering; COPY sources: numbered across the ops' walks).  The window: MI_COMMIT_WINDOW_MB, or
// half of what the batch's arena could be grown to before it failed, at least 64 MiB; a single file larger than the window is
// tried alone.
struct WindowFile { std::string path; uint64_t size, ordinal; };
static int commit_roots_by_windows(mi_memfs* m, mi_batch* b, const std::vector<WindowFile>& files, std::vector<uint8_t>* roots) {
    bool given = false;
    uint64_t window = commit_window_bytes(&given);
    if (!window) {
        uint64_t room = 0;
        mi_batch_arena_room(b, &room);
        window = room / 2;
    }
    if (window < (64ull << 20) && !given) window = 64ull << 20;
    roots->assign(files.size() * 32, 0);
    std::vector<const char*> cpaths;
    std::vector<uint64_t> sizes;
    auto run = [&](size_t lo, size_t hi) -> int {
        if (lo == hi) return MI_OK;
        cpaths.clear(); sizes.clear();
        for (size_t k = lo; k < hi; ++k) { cpaths.push_back(files[k].path.c_str()); sizes.push_back(files[k].size); }
        int rc = mi_batch_reset(b);
        if (!rc) rc = mi_batch_add_paths(b, hi - lo, cpaths.data(), sizes.data(), nullptr);
        if (!rc) rc = mi_batch_run(b);
        std::vector<uint8_t> r((hi - lo) * 32);
        if (!rc) rc = mi_batch_roots(b, r.data(), hi - lo);
        if (!rc) {
            uint64_t nc = 0;
            mi_batch_counts(b, nullptr, &nc, nullptr);
            m->last.n_chunks += nc;
            for (size_t k = lo; k < hi; ++k) memcpy(roots->data() + files[k].ordinal * 32, r.data() + (k - lo) * 32, 32);
            ++m->last.n_windows;
        }
        return rc;
    };
    size_t lo = 0;
    uint64_t held = 0;
    for (size_t i = 0; i < files.size(); ++i) {
        if (held && held + files[i].size > window) { const int rc = run(lo, i); if (rc) return rc; lo = i; held = 0; }
        held += files[i].size;
        m->last.n_scanned_files += 1;
        m->last.scanned_bytes += files[i].size;
    }
    return run(lo, files.size());
}

namespace {                                                                       // (this file's own types: no symbols leave it)
// the walk of a scanning commit, from its walk to its diff (given back before the tar is written)
struct ScanWalk {
    uint64_t n = 0;
    std::vector<mi_tree_entry> walked;                                            // n rows ...
    mi_tree* t = nullptr;                                                         // ... of the walk without a batch (owned), or
    const mi_walk::Tree* wt = nullptr;                                            // ... of the batch's own record / of `listing`
    mi_walk::Tree listing;                                                        // the walk of a tree that is scanned in windows
    ~ScanWalk() { if (t) mi_tree_free(t); }
};

// ONE commit, from the open batch to the handed-over layer: memfs_commit calls the stages in order.  Whichever way the commit is
// left, the scan thread is joined, fs.job cleared and every promised root settled (~Commit) before anything returns.
struct Commit {
    mi_memfs* const m;
    mi_copy::Fs& fs;
    mi_ctx* const* const ctxs;
    const uint32_t n_ctx;
    mi_ctx* const ctx;                                                            // ctxs[0]; NULL: the reference's commit
    const mi_copy_op* const ops;
    const uint64_t n_ops;
    const char* const how;
    const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
    const uint64_t opens0 = mi_io::content_opens.load(), bytes0 = mi_io::content_bytes.load();
    mi_batch* b = nullptr;                                                        // the handle's batch (ctx != NULL)
    uint64_t moves0 = 0;
    mi_copy::ScanJob job;
    bool piped = false;                                                           // job is running: fs.job points at it
    bool windowed = false;                                                        // what is scanned does not fit the device
    std::vector<uint8_t> roots;                                                   // the scan's, when they are there before the diff
    mi_copy_layer* cl = nullptr;
    uint64_t ne = 0;

    Commit(mi_memfs* m_, mi_ctx* const* ctxs_, uint32_t n_ctx_, bool must_scan, const mi_copy_op* ops_, uint64_t n_ops_)
        : m(m_), fs(m_->fs), ctxs(ctxs_), n_ctx(n_ctx_), ctx(n_ctx_ ? ctxs_[0] : nullptr), ops(ops_), n_ops(n_ops_),
          how(must_scan ? "create layer by scan: " : "create layer by copy ops: ") {
        fs.n_content_changed = fs.n_roots_learned = 0;
        fs.reserved_mark = 0;
        if (++fs.commit_gen == 0) fs.commit_gen = 1;
    }
    ~Commit() { settle_scan(nullptr); }

    int fail_with(int code, const std::string& what) {
        m->err = std::string("failed to generate diff layer: write diffs: ") + how + what;
        return code;
    }

    int open_batch() {
        if (!ctx) return MI_OK;
        const int rc = memfs_batch_for(m, ctxs, n_ctx, 0);
        if (rc) return fail_with(rc, std::string("gpu scan: ") + mi_last_error(ctx));
        b = m->batch;
        mi_batch_arena_info(b, nullptr, nullptr, &moves0);                        // (a batch that was kept: what it has moved so far)
        // (Until round 5 a first content scan of a tree the handle already knew reserved the arena here, once, for what the tree
        //  lists: an arena that grew in steps drained the reader threads and moved every time.  The arena no longer moves --
        //  mi_arena.hip: an address range mapped piece by piece behind the walk -- so there is nothing to prepare.)
        return MI_OK;
    }

    // PIPELINED (default; MI_COMMIT_PIPELINE=0: one phase after the other): the scan -- the end of staging, the kernels, the
    // roots' way back -- runs on a thread of its own (ScanJob) while this thread computes the layer and frames the tar from
    // the bytes that have landed.  The diff waits for the scan only where a root DECIDES (a file the tree holds with a root
    // and an unchanged header); an all-new layer, a first content scan, a COPY of new files never wait, and their commit
    // costs what the reference's costs: the serial TarDigest.  Roots that were only to be RECORDED are filled in at the end.
    int start_scan() {                                                            // scan what has been staged
        if (!b || windowed) return MI_OK;
        uint64_t nf = 0, nbytes = 0;
        mi_batch_counts(b, &nf, nullptr, &nbytes);
        m->last.n_scanned_files = nf;
        m->last.scanned_bytes = nbytes;
        if (!nf) return MI_OK;
        if (commit_knobs().pipeline) {
            job.start(b, nf);
            fs.job = &job;
            piped = true;
            return MI_OK;
        }
        const auto t0 = std::chrono::steady_clock::now();
        int r = mi_batch_run(b);
        if (!r) { roots.resize(nf * 32); r = mi_batch_roots(b, roots.data(), nf); }
        m->last.s_scan = secs_since(t0);
        if (!r) mi_batch_counts(b, nullptr, &m->last.n_chunks, nullptr);
        return r ? fail_with(r, std::string("gpu scan: ") + mi_last_error(ctx)) : MI_OK;
    }
    // the scan thread is joined and every promised root settled; layer_nodes: the layer's nodes take their roots too
    int settle_scan(std::vector<mi_copy::Node>* layer_nodes) {
        if (!piped) return MI_OK;
        const uint8_t* r = job.wait_roots();
        job.join();
        fs.job = nullptr;
        piped = false;
        fs.settle_pending(r, layer_nodes);
        m->last.s_scan = job.seconds;
        m->last.n_chunks = job.n_chunks;
        return job.rc;
    }

    // WHAT IS SCANNED DOES NOT FIT THE DEVICE: the roots are computed window by window -- walked once more, without a batch
    // (window_files: the scanned tree's listing / the ops planned again), the regular files through the batch in runs the
    // device has room for -- and the layer's files are read from disk by the writer: a second read for those, the price of
    // a tree larger than HBM.
    template <class Walked> int roots_in_windows(Walked& w) {
        windowed = true;
        (void)mi_batch_reset(b);
        std::vector<WindowFile> wf;
        int rc = window_files(w, &wf);
        if (rc) return rc;
        if ((rc = commit_roots_by_windows(m, b, wf, &roots)))
            return fail_with(rc, std::string("gpu scan (in windows): ") + mi_last_error(ctx));
        return MI_OK;
    }
    int window_files(ScanWalk& w, std::vector<WindowFile>* wf) {
        std::string werr;
        const int rc = mi_walk::scan_walk_listing(fs.root, m->blacklist, &w.listing, &werr);
        if (rc) return fail_with(rc, "walk " + fs.root + ": " + werr);
        w.n = w.listing.entries.size();
        w.walked.resize(w.n ? w.n : 1);
        for (uint64_t i = 0; i < w.n; ++i) {                                      // (mi_tree_entries' rows of the same record)
            const mi_walk::Entry& e = w.listing.entries[i];
            mi_tree_entry& o = w.walked[i];
            memset(&o, 0, sizeof o);
            o.relpath = e.relpath.c_str();
            o.link_target = e.has_link ? e.link.c_str() : nullptr;
            o.file_index = e.file_index; o.size = e.size; o.mtime_sec = e.mtime; o.mode = e.mode; o.kind = e.kind;
            o.uid = e.uid; o.gid = e.gid;
        }
        w.wt = &w.listing;                                                        // (the inode stamps: a window's files are hashed files)
        for (uint64_t i = 0; i < w.n; ++i)
            if (w.walked[i].kind == 1 && w.walked[i].file_index >= 0)
                wf->push_back({fs.root == "/" ? "/" + std::string(w.walked[i].relpath) : fs.root + "/" + w.walked[i].relpath,
                               w.walked[i].size, (uint64_t)w.walked[i].file_index});
        return MI_OK;
    }
    int window_files(CopyPlan& plan, std::vector<WindowFile>* wf) {               // the files numbered across the ops' walks
        plan = CopyPlan();
        copy_ops_plan(fs, ops, n_ops, nullptr, &plan);
        for (CopyOpPlan& op : plan.ops)
            for (CopySrcPlan& sp : op.srcs)
                for (mi_walk::Entry& we : sp.walked.entries)
                    if (we.kind == 1 && we.file_index >= 0) {
                        we.file_index = (int64_t)wf->size();
                        wf->push_back({we.relpath == "." ? sp.src : sp.src + "/" + we.relpath, we.size, (uint64_t)we.file_index});
                    }
        return MI_OK;
    }

    // ---- the layer of a scan: walk + stage, start the scan, diff
    int walk_root(ScanWalk& w) {
        std::vector<const char*> bl;
        for (const std::string& s : m->blacklist) bl.push_back(s.c_str());
        const auto t0 = std::chrono::steady_clock::now();
        int rc;
        if (b) {
            struct timespec now;
            clock_gettime(CLOCK_REALTIME, &now);
            fs.commit_started_ns = (int64_t)now.tv_sec * 1000000000ll + now.tv_nsec;
            if (fs.trust_ctime) {                                                 // files whose inode says "unchanged" are not read
                fs.reserved_mark = mi_copy::next_scan_mark();                     // (... and found held are marked by the readers)
                mi_walk::Tree* wtree = nullptr;
                std::string werr;
                struct Freeze { mi_memtree::Tree& t; Freeze(mi_memtree::Tree& x) : t(x) { t.frozen = true; } ~Freeze() { t.frozen = false; } } freeze(fs.t);   // (the readers look the tree up)
                mi_copy::Fs* const f = &fs;
                rc = mi_walk::scan_walk_batch_filtered(b, fs.root, m->blacklist,
                        [f, mark = fs.reserved_mark](const std::string& path, const struct stat& sb, const mi_walk::InodeStamp& st) {
                            return f->content_is_known(path, sb, st, mark);
                        },
                        &wtree, &werr);
                if (rc && rc != MI_ERR_NOMEM) { fs.reserved_mark = 0; return fail_with(rc, "walk " + fs.root + ": " + (werr.empty() ? mi_last_error(ctx) : werr)); }
                if (!rc) w.n = wtree->entries.size();
            } else if (m->went_windowed || commit_knobs().force_windows) {
                rc = MI_ERR_NOMEM;                                                // (it did not fit last time and everything is read again:
            } else {                                                              //  straight to the windows)
                rc = mi_batch_add_tree(b, fs.root.c_str(), fs.root.c_str(), bl.empty() ? nullptr : bl.data(), bl.size(), MI_TREE_SCAN, &w.n);
                if (rc && rc != MI_ERR_NOMEM) return fail_with(rc, "walk " + fs.root + ": " + mi_last_error(ctx));
            }
            if (rc == MI_ERR_NOMEM) {                                             // THE TREE DOES NOT FIT THE DEVICE
                m->went_windowed = true;
                fs.reserved_mark = 0;                                             // (another walk: another mark)
                if ((rc = roots_in_windows(w))) return rc;
                if (m->last.n_windows <= 1) m->went_windowed = false;             // (it has shrunk to one window's worth: one batch next time)
            } else {
                w.wt = (const mi_walk::Tree*)*mi_batch_tree_slot(b);
                w.walked.resize(w.n ? w.n : 1);
                rc = mi_batch_tree_entries(b, w.walked.data(), w.n);
            }
        } else {
            rc = mi_tree_walk(fs.root.c_str(), fs.root.c_str(), bl.empty() ? nullptr : bl.data(), bl.size(), MI_TREE_SCAN, &w.t, &w.n);
            if (rc) return fail_with(rc, "walk " + fs.root);
            w.walked.resize(w.n ? w.n : 1);
            rc = mi_tree_entries(w.t, w.walked.data(), w.n);
        }
        m->last.n_walked = w.n;
        m->last.s_walk_stage = secs_since(t0);
        return rc ? fail_with(rc, m->err) : MI_OK;
    }
    int diff_scan(ScanWalk& w) {
        const auto t1 = std::chrono::steady_clock::now();
        const int rc = memfs_scan(m, w.walked.data(), w.n, roots.empty() ? nullptr : roots.data(), 32, b != nullptr && !windowed, &cl, &ne, w.wt);
        m->last.s_diff = secs_since(t1);
        if (w.wt && w.wt->want_stamps && fs.trust_ctime)                          // files the walk did not read: their content is known
            for (size_t i = 0; i < w.wt->known.size() && i < w.n; ++i) m->last.n_content_trusted += w.wt->known[i] ? 1 : 0;
        return rc ? fail_with(rc, m->err) : MI_OK;
    }
    int layer_by_scan() {
        ScanWalk w;
        int rc = walk_root(w);
        if (!rc) rc = start_scan();
        if (!rc) rc = diff_scan(w);
        return rc;
    }

    // ---- the layer of COPY/ADD ops: plan (walk + stage), start the scan, apply (diff)
    int plan_ops(CopyPlan& plan) {
        fs.clear_layer();
        const auto t0 = std::chrono::steady_clock::now();
        const bool force_windows = b && commit_knobs().force_windows;
        if (!force_windows) copy_ops_plan(fs, ops, n_ops, b, &plan);
        if (b && (force_windows || plan.err_rc == MI_ERR_NOMEM))                  // THE SOURCES DO NOT FIT THE DEVICE
            if (const int rc = roots_in_windows(plan)) return rc;
        m->last.n_walked = plan.n_walked;
        m->last.s_walk_stage = secs_since(t0);
        return MI_OK;
    }
    int apply_ops(const CopyPlan& plan) {
        const auto t1 = std::chrono::steady_clock::now();
        std::string e;
        int rc = copy_ops_apply(fs, ops, plan, roots.empty() ? nullptr : roots.data(), &e);
        if (rc) {
            if (fs.rc) rc = memfs_fail(m); else { m->err = e; fs.clear_layer(); }
            return fail_with(rc, m->err);
        }
        cl = memfs_take_layer(m);
        ne = cl->nodes.size();
        m->last.s_diff = secs_since(t1);
        return MI_OK;
    }
    int layer_by_copy_ops() {
        CopyPlan plan;
        int rc = plan_ops(plan);
        // (a plan that stopped at a failure is applied up to it: the failure is the apply step's to raise, in its place.
        //  What was staged until then is scanned all the same -- the ops before the failing one are applied WITH roots.)
        if (!rc) rc = start_scan();
        if (!rc) rc = apply_ops(plan);
        return rc;
    }

    // ---- write, the scan's verdict, index, stats: a layer there is, whatever fails from here on
    int write_layer(const mi_layer_config* cfg, mi_layer_result* res) {
        m->last.n_layer_entries = ne;
        m->last.n_content_changed = fs.n_content_changed;
        m->last.n_roots_learned = fs.n_roots_learned;
        const auto t2 = std::chrono::steady_clock::now();
        const int rc = memfs_commit_write(m, cl, ne, cfg, res, windowed ? nullptr : b, piped, m->gzip_device && n_ctx ? ctxs[0] : nullptr);
        m->last.s_write = secs_since(t2);
        return rc;
    }
    // the scan's verdict: a file that vanished or shrank since the walk fails the commit here -- after the tree took the
    // layer, as a failing tar write does in the reference (AddLayerByScan updates the tree, then writes)
    int scan_verdict(int rc) {
        const bool was_piped = piped;
        const int src = settle_scan(&cl->nodes);
        if (src && !rc) { rc = src; m->err = "failed to generate diff layer: write diffs: " + std::string(how) + "gpu scan: " + job.err; }
        m->last.pipelined = was_piped ? 1 : 0;
        return rc;
    }
    int add_to_index() {
        int rc = MI_OK;
        if (b && m->index && m->last.n_scanned_files) {
            // the chunk index (keyvalue.Store seam): which of this commit's chunks no earlier commit held, and how many bytes they
            // are -- what a chunk-addressed store would have to take in for this layer.  A commit over several GPUs feeds the ONE
            // index batch by batch: the batch on the index's own GPU from device memory, the others' digests through the host.
            mi_batch* const* members = &b;
            uint64_t nm = 0;
            mi_batch_group_members(b, &members, nullptr, &nm);
            if (nm == 0) { members = &b; nm = 1; }
            for (uint64_t k = 0; k < nm && !rc; ++k) {
                mi_batch* mb = members[k];
                uint64_t nc = 0, nn = 0, nk = 0;
                mi_batch_counts(mb, nullptr, &nc, nullptr);
                std::vector<uint8_t> known(nc ? nc : 1);
                const mi_chunk_result* rows = nullptr;
                if (nc) rc = mi_batch_chunks_view(mb, &rows, &nc);
                if (!rc && mi_index_same_ctx(m->index, mb)) {
                    rc = mi_index_add_batch(m->index, mb, known.data(), nc, &nn, &nk);
                } else if (!rc) {
                    std::vector<uint8_t> dg(nc * 32 + 32);
                    for (uint64_t i = 0; i < nc; ++i) memcpy(dg.data() + 32 * i, rows[i].sha256, 32);
                    rc = mi_index_add_digests(m->index, dg.data(), nc, known.data(), &nn, &nk);
                }
                if (!rc) {
                    m->last.n_index_new += nn;
                    m->last.n_index_known += nk;
                    for (uint64_t i = 0; i < nc; ++i)
                        if (!known[i] && rows[i].dup_of < 0) m->last.index_new_bytes += rows[i].length;
                }
                if (!rc && (m->chunk_pack || m->chunk_zpack) && !windowed) pack_and_recipes(mb, rows, nc, known.data());     // (one ctx: one member)
            }
            if (rc) m->err = std::string("failed to generate diff layer: chunk index: ") + mi_last_error(ctx);
        } else if (b && m->chunk_pack && !windowed) {                             // nothing was scanned: a pack of nothing
            mi_pack* p = nullptr;
            const int prc = mi_pack_empty(ctx, &p);
            memfs_pack_drop(m, prc, prc ? "the empty pack of a commit that scanned nothing" : "");
            m->pack = p;
            cl->chunk_first.assign(cl->nodes.size() + 1, 0);
        }
        if (b && m->chunk_pack && windowed)
            memfs_pack_drop(m, MI_ERR_STATE, "the last commit's tree did not fit the device and was scanned in " + std::to_string(m->last.n_windows) +
                                             " windows: no batch holds its bytes, there is no pack (packs window by window are not built)");
        if (b && m->chunk_zpack && !windowed && !(m->index && m->last.n_scanned_files)) {      // nothing was scanned: a zpack of nothing
            mi_zpack* z = nullptr;
            void* d_blob = nullptr;
            mi_zpack_entry* h_rows = nullptr;
            const int zrc = mi_zpack_alloc(ctx, "mi_memfs_commit_layer", 0, 0, &z, &d_blob, &h_rows);
            if (!zrc) mi_zpack_set_result(z, 0, 0, 0, 1, 0, 0, 0);
            memfs_zpack_drop(m, zrc, zrc ? "the empty zpack of a commit that scanned nothing" : "");
            m->zpack = z;
            cl->chunk_first.assign(cl->nodes.size() + 1, 0);
        }
        if (b && m->chunk_zpack && windowed)
            memfs_zpack_drop(m, MI_ERR_STATE, "the last commit's tree did not fit the device and was scanned in " + std::to_string(m->last.n_windows) +
                                              " windows: no batch holds its bytes, there is no zpack (packs window by window are not built)");
        return rc;
    }
    // MI_MEMFS_CHUNK_PACK: the rows whose bytes index_new_bytes counts as ONE blob (mi_batch_pack_chunks with MI_PACK_VERIFY: the
    // batch still holds the tree's bytes), and every layer file's ordered chunks.  A pack that cannot be built does not fail the
    // commit -- the layer is written: mi_memfs_take_pack returns the error and the message.  MI_MEMFS_CHUNK_ZPACK: the same rows
    // coded straight from the arena (mi_batch_zpack_chunks with MI_ZPACK_VERIFY, and MI_ZPACK_LEVEL2 under MI_MEMFS_ZPACK_LEVEL2), the
    // same recipes.
    void pack_and_recipes(mi_batch* mb, const mi_chunk_result* rows, uint64_t nc, const uint8_t* known) {
        std::vector<uint8_t> select(nc ? nc : 1);
        for (uint64_t i = 0; i < nc; ++i) select[i] = !known[i] && rows[i].dup_of < 0;
        if (m->chunk_zpack) {
            mi_zpack* z = nullptr;
            const int zrc = mi_batch_zpack_chunks(mb, select.data(), nc, MI_ZPACK_VERIFY | (m->zpack_level2 ? MI_ZPACK_LEVEL2 : 0u), &z);
            memfs_zpack_drop(m, zrc, zrc ? std::string("chunk zpack: ") + mi_last_error(ctx) : std::string());
            m->zpack = z;
        } else {
            mi_pack* p = nullptr;
            const int prc = mi_batch_pack_chunks(mb, select.data(), nc, MI_PACK_VERIFY, &p);
            memfs_pack_drop(m, prc, prc ? std::string("chunk pack: ") + mi_last_error(ctx) : std::string());
            m->pack = p;
        }
        const mi_file_result* files = nullptr;
        uint64_t nf = 0;
        cl->chunk_first.assign(cl->nodes.size() + 1, 0);
        if (mi_batch_files_view(mb, &files, &nf)) return;
        for (size_t i = 0; i < cl->nodes.size(); ++i) {
            const mi_copy::Node& nd = cl->nodes[i];
            if (nd.batch_file >= 0 && nd.batch_gen == fs.commit_gen && (uint64_t)nd.batch_file < nf) {
                const mi_file_result& f = files[nd.batch_file];
                for (uint64_t k = f.first_chunk; k < f.first_chunk + f.n_chunks && k < nc; ++k) {
                    cl->chunk_digests.insert(cl->chunk_digests.end(), rows[k].sha256, rows[k].sha256 + 32);
                    cl->chunk_lengths.push_back(rows[k].length);
                }
            }
            cl->chunk_first[i + 1] = cl->chunk_lengths.size();
        }
    }
    void stats() {
        m->last.files_opened += mi_io::content_opens.load() - opens0;
        m->last.file_bytes_read += mi_io::content_bytes.load() - bytes0;
        m->last.s_total = secs_since(t_all);
        if (b) {
            uint64_t moves = 0;
            mi_batch_arena_info(b, &m->last.arena_bytes, &m->last.arena_pieces, &moves);
            m->last.arena_moves = moves - moves0;
            const uint64_t* loads = nullptr;
            uint64_t nm = 0;
            mi_batch_group_members(b, nullptr, &loads, &nm);
            m->last.n_ctxs = nm ? nm : 1;
            m->last.n_split_files = mi_batch_group_splits(b);
            m->last.ctx_bytes_max = m->last.ctx_bytes_min = nm ? loads[0] : m->last.scanned_bytes;
            for (uint64_t k = 1; k < nm; ++k) {
                if (loads[k] > m->last.ctx_bytes_max) m->last.ctx_bytes_max = loads[k];
                if (loads[k] < m->last.ctx_bytes_min) m->last.ctx_bytes_min = loads[k];
            }
        }
    }
    int hand_over(int rc, mi_copy_layer** layer_out, int* committed) {
        for (mi_copy::Node& nd : cl->nodes) nd.batch_file = -1;                   // (rows of a batch the caller does not hold)
        if (rc) { mi_copy_layer_free(cl); return rc; }
        *committed = 1;
        if (layer_out) *layer_out = cl; else mi_copy_layer_free(cl);
        return MI_OK;
    }
};

}  // namespace

// open the batch -> walk + stage (scan | copy ops) -> start the scan -> diff -> write -> settle the scan -> index -> stats
static int memfs_commit(mi_memfs* m, mi_ctx* const* ctxs, uint32_t n_ctx, int must_scan, const mi_copy_op* ops, uint64_t n_ops,
                        const mi_layer_config* cfg, mi_layer_result* res, mi_copy_layer** layer_out, int* committed) {
    if (!m || !cfg || !res || !committed || (n_ops && !ops)) return MI_ERR_INVALID;
    *committed = 0;
    if (layer_out) *layer_out = nullptr;
    memset(&m->last, 0, sizeof m->last);
    if (!must_scan && n_ops == 0) return MI_OK;                                   // "Nothing to do, return."
    // ONE chunk digest algorithm per handle: the ctxs agree among themselves, with the roots the tree holds and with the index --
    // roots of two hashes never compare equal, every file would read as changed.  Checked before anything is walked or changed.
    uint32_t alg = MI_DIGEST_SHA256;
    for (uint32_t k = 0; k < n_ctx; ++k) {
        uint32_t a = 0;
        if (mi_ctx_chunk_digest(ctxs[k], &a)) return MI_ERR_INVALID;
        if (k == 0) alg = a;
        else if (a != alg) { m->err = "failed to generate diff layer: the ctxs of one commit hash chunks with different algorithms (MI_FLAG_CHUNK_BLAKE2S)"; return MI_ERR_INVALID; }
    }
    if (n_ctx && m->root_alg >= 0 && (uint32_t)m->root_alg != alg) {
        m->err = "failed to generate diff layer: this handle's roots were computed with the other chunk digest algorithm (MI_FLAG_CHUNK_BLAKE2S): mi_memfs_reset first";
        return MI_ERR_STATE;
    }
    if (n_ctx && m->index) {
        uint32_t a = 0;
        if (mi_ctx_chunk_digest(mi_index_ctx(m->index), &a) || a != alg) {
            m->err = "failed to generate diff layer: chunk index: the index holds digests of the other chunk digest algorithm (MI_FLAG_CHUNK_BLAKE2S)";
            return MI_ERR_INVALID;
        }
    }
    if (!n_ctx && m->gzip_device && cfg && cfg->gzip_level != MI_GZIP_OFF && cfg->gzip_level != 0) {   // MI_MEMFS_GZIP_DEVICE: before anything is walked
        m->err = "failed to generate diff layer: MI_MEMFS_GZIP_DEVICE codes the gzip leg on a ctx's device: the commit has none (ctx == NULL)";
        return MI_ERR_STATE;
    }
    if (n_ctx && m->chunk_pack) {                                                 // MI_MEMFS_CHUNK_PACK: before anything is walked
        if (!m->index) { m->err = "failed to generate diff layer: chunk pack: MI_MEMFS_CHUNK_PACK packs the chunks the index did not know: set one first (mi_memfs_set_index)"; return MI_ERR_STATE; }
        if (n_ctx > 1) { m->err = "failed to generate diff layer: chunk pack: a pack over several GPUs' arenas is not built (MI_MEMFS_CHUNK_PACK with n_ctx > 1)"; return MI_ERR_INVALID; }
        memfs_pack_drop(m, MI_ERR_STATE, "the last commit made no pack");         // (an earlier commit's pack nobody took goes)
    }
    if (n_ctx && m->chunk_zpack) {                                                // MI_MEMFS_CHUNK_ZPACK: the same refusals
        if (!m->index) { m->err = "failed to generate diff layer: chunk zpack: MI_MEMFS_CHUNK_ZPACK packs the chunks the index did not know: set one first (mi_memfs_set_index)"; return MI_ERR_STATE; }
        if (n_ctx > 1) { m->err = "failed to generate diff layer: chunk zpack: a pack over several GPUs' arenas is not built (MI_MEMFS_CHUNK_ZPACK with n_ctx > 1)"; return MI_ERR_INVALID; }
        memfs_zpack_drop(m, MI_ERR_STATE, "the last commit made no zpack");       // (an earlier commit's zpack nobody took goes)
    }
    Commit c(m, ctxs, n_ctx, must_scan != 0, ops, n_ops);
    int rc = c.open_batch();
    if (!rc && n_ctx) m->root_alg = (int)alg;                                     // (from here on roots of this algorithm may land)
    if (!rc) rc = must_scan ? c.layer_by_scan() : c.layer_by_copy_ops();
    if (rc) return rc;                                                            // (no layer; ~Commit settles the scan)
    rc = c.write_layer(cfg, res);
    rc = c.scan_verdict(rc);
    if (!rc) rc = c.add_to_index();
    c.stats();
    return c.hand_over(rc, layer_out, committed);
}
extern "C" int mi_memfs_commit_layer(mi_memfs* m, mi_ctx* ctx, int must_scan, const mi_copy_op* ops, uint64_t n_ops,
                                     const mi_layer_config* cfg, mi_layer_result* res, mi_copy_layer** layer_out,
                                     int* committed) {
    return memfs_commit(m, ctx ? &ctx : nullptr, ctx ? 1 : 0, must_scan, ops, n_ops, cfg, res, layer_out, committed);
}
// THE COMMIT OVER SEVERAL GPUs (north_star: "file batches shard across the 8 GPUs of one node").  One ctx per
// GPU; what the walk hands over -- a directory's block of small files, a large file -- goes to the GPU with the fewest bytes so
// far (the streaming form of longest-processing-time-first: a walk does not know its files in advance); every GPU stages through
// its own reader threads and PCIe link, scans its share, and the committing thread gets the roots back in the walk's order; the
// tar writer reads each file from the GPU that holds it; the chunk index (on one of the ctxs) takes the other GPUs' digests
// through the host (32 bytes per chunk).  Everything else -- the diff, the pipelining, the sums, TRUST_CTIME, the windows of a
// tree that does not fit -- is the one-GPU commit's: behind the handle the n batches look like one (mi_batch_group_begin).
// n_ctx = 1 is mi_memfs_commit_layer, n_ctx = 0 the reference's commit.  A file of 256 MiB and more is split over the GPUs as parts
// (mi_group.hip: group_add_paths and group_resolve_parts).
// UNMEASURED on more than one physical GPU (no such box in this pool): tested with n ctxs on one device and on the HIP double.
extern "C" int mi_memfs_commit_layer_n(mi_memfs* m, mi_ctx* const* ctxs, uint32_t n_ctx, int must_scan, const mi_copy_op* ops,
                                       uint64_t n_ops, const mi_layer_config* cfg, mi_layer_result* res,
                                       mi_copy_layer** layer_out, int* committed) {
    if (n_ctx && !ctxs) return MI_ERR_INVALID;
    if (n_ctx > 64) return MI_ERR_INVALID;
    return memfs_commit(m, ctxs, n_ctx, must_scan, ops, n_ops, cfg, res, layer_out, committed);
}

extern "C" int mi_memfs_commit_stats(const mi_memfs* m, mi_commit_stats* out) {
    if (!m || !out) return MI_ERR_INVALID;
    *out = m->last;
    return MI_OK;
}
extern "C" int mi_memfs_set_options(mi_memfs* m, uint32_t options) {
    if (!m || (options & ~(MI_MEMFS_TRUST_CTIME | MI_MEMFS_CHUNK_PACK | MI_MEMFS_CHUNK_ZPACK | MI_MEMFS_ZPACK_LEVEL2 | MI_MEMFS_GZIP_DEVICE))) return MI_ERR_INVALID;
    if ((options & MI_MEMFS_CHUNK_PACK) && (options & MI_MEMFS_CHUNK_ZPACK)) {    // mi_pack_compress, or a decode, makes the other form
        m->err = "mi_memfs_set_options: MI_MEMFS_CHUNK_PACK and MI_MEMFS_CHUNK_ZPACK exclude each other: the commit does not do the work twice";
        return MI_ERR_INVALID;
    }
    m->fs.trust_ctime = (options & MI_MEMFS_TRUST_CTIME) != 0;
    m->chunk_pack = (options & MI_MEMFS_CHUNK_PACK) != 0;
    m->chunk_zpack = (options & MI_MEMFS_CHUNK_ZPACK) != 0;
    m->zpack_level2 = (options & MI_MEMFS_ZPACK_LEVEL2) != 0;            // (alone it changes nothing: there is no zpack to code)
    m->gzip_device = (options & MI_MEMFS_GZIP_DEVICE) != 0;
    return MI_OK;
}
extern "C" int mi_memfs_take_zpack(mi_memfs* m, mi_zpack** out) {
    if (!m || !out) return MI_ERR_INVALID;
    *out = nullptr;
    if (!m->zpack) {
        m->err = "mi_memfs_take_zpack: " + m->zpack_err;
        return m->zpack_rc ? m->zpack_rc : MI_ERR_STATE;
    }
    *out = m->zpack;
    m->zpack = nullptr;
    m->zpack_rc = MI_ERR_STATE;
    m->zpack_err = "no commit since the last mi_memfs_take_zpack";
    return MI_OK;
}
extern "C" int mi_memfs_take_pack(mi_memfs* m, mi_pack** out) {
    if (!m || !out) return MI_ERR_INVALID;
    *out = nullptr;
    if (!m->pack) {
        m->err = "mi_memfs_take_pack: " + m->pack_err;
        return m->pack_rc ? m->pack_rc : MI_ERR_STATE;
    }
    *out = m->pack;
    m->pack = nullptr;
    m->pack_rc = MI_ERR_STATE;
    m->pack_err = "no commit since the last mi_memfs_take_pack";
    return MI_OK;
}
extern "C" int mi_memfs_set_index(mi_memfs* m, mi_index* index) {
    if (!m) return MI_ERR_INVALID;
    m->index = index;
    return MI_OK;
}
// The handle's batch, made ahead of its first commit and sized for `bytes` of files in `files` files: fresh device memory costs
// up to 68 ms per GiB to allocate on some boxes (tools/first_use_probe.py) and the ctx's reader threads 55 ms to come up -- a host that knows what
// is coming (the base image it is pulling) pays that beside its own work instead of inside the first commit
extern "C" int mi_memfs_reserve_device(mi_memfs* m, mi_ctx* ctx, uint64_t files, uint64_t bytes) {
    if (!m || !ctx) return MI_ERR_INVALID;
    int rc = memfs_batch_for(m, &ctx, 1, files);                                  // (a commit's arena is the piecewise kind: a guess
                                                                                  //  that is too small costs nothing later)
    if (!rc) rc = mi_batch_reserve_ahead(m->batch, files, bytes);
    if (!rc) rc = mi_batch_prepare_read(m->batch);                                // (the tar writer's windows: 10 ms of pinned allocation)
    if (!rc) mi_batch_expect_host_bytes(m->batch);                                // (the reader threads set up behind the call)
    if (rc) m->err = std::string("reserve device memory: ") + mi_last_error(ctx);
    return rc;
}
extern "C" int mi_memfs_release_device(mi_memfs* m) {
    if (!m) return MI_ERR_INVALID;
    return memfs_batch_drop(m);
}
