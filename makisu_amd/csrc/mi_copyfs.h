// mi_copyfs.h -- what the files behind the MemFS handle share: the path-keyed tree with its layer (mi_copy::Fs: addToLayer,
// maybeAddToLayer, addAncestors, isUpdated, the whiteouts), a pipelined commit's scan thread (ScanJob), the layer a step
// hands over (mi_copy_layer), the handle itself (mi_memfs) and its few helpers, and the declarations of what crosses files.
// Header-only, no device code.  Users: mi_memfs.hip (the handle: merge, untar, scan), mi_copyops.hip (the COPY/ADD step:
// plan + apply), mi_commit.hip (mi_memfs_commit_layer).  Every function cites the Go it restates; the tree is mi_memtree.h.
#pragma once
#include "mi_memtree.h"
#include "../../include/makisu_mi_host.h"

#include <errno.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory_resource>
#include <mutex>
#include <new>
#include <thread>
#include <unordered_map>

// ---- MemFS.AddLayerByCopyOps: the layer a COPY / ADD step creates, on entry lists -----------------
// addToLayer + maybeAddToLayer(createWhiteout = false) + addAncestors + isUpdated + createHeader
// (lib/snapshot/mem_fs.go:276-289, 343-421, 440-503, 505-566; mem_layer.go:152-190) and
// CopyOperation's source resolution (copy_op.go, utils.go:249-327), restated on a path-keyed tree:
//   * a single non-directory source copies onto dst (or into dst + "/" + base when dst ends with "/");
//     otherwise dst is ensured to exist -- every EXISTING ancestor is carried into the layer, a
//     symlink on the way is followed (its target joined with the rest of the path, the reference's
//     own rule, depth-limited), missing directories are created with the last existing ancestor's
//     mode, the op's uid/gid and mtime = now -- and the sources' CONTENTS are copied below it;
//   * sources are resolved through symlinks inside src_root (a link leaving the root is an error)
//     and walked like every snapshot walk (".wh..wh." names, special files and mountpoints skipped;
//     no blacklist: the reference passes nil here);
//   * every walked path gets createHeader's header with the op's uid/gid and is added iff isUpdated
//     says so (tario.IsSimilarHeader against what the tree holds); adding a path first carries its
//     existing ancestors, then replaces the node: a directory keeps the old node's children, anything
//     else drops them.
// Result: the layer's entries in commit order (sorted by dst), each with the path its content is
// read from ("/" for directories the op created: memLayer.addHeader("", ...) -> AbsPath("")).  The caller's tree is not modified; to continue,
// apply the layer to it with mi_entries_apply_layer.
namespace mi_copy {

struct Node {
    mi_walk::Entry e;          // relpath = dst without the leading "/"
    std::string src;           // where the content is read from; what memFSNode.isOnDisk looks at
    bool has_root = false;     // chunk root of the content, when the caller scanned it (content-aware isUpdated)
    uint8_t root[32];
    int64_t batch_file = -1;   // a content-aware commit under way: the file's row in the commit's batch -- its bytes lie in HBM
    uint32_t batch_gen = 0;    // ... of WHICH commit (Fs::commit_gen): the tree keeps its nodes, a later commit that puts one back into
                               // its layer "as it is" (addAncestors over a path the tree holds as a file) must not take the old row
                               // for a row of its own batch -- it reads that file from its source path, as the reference does
    bool root_pending = false; // ... and its root is still being computed (a pipelined commit: ScanJob); root[] is not valid yet
};
// MI_MEMFS_TRUST_CTIME, per node whose root a commit of this handle computed: the inode as it was when the content was read, and
// when that was (CLOCK_REALTIME at the start of that commit's walk).  Beside the nodes (Fs::hashed, by node index), not in them:
// a tree merged from base layers and never scanned with a ctx pays nothing for it.
struct HashedAs { mi_walk::InodeStamp stamp; int64_t at_ns = 0; };
// a scan's mark ("this scan's walk lists the path", mi_memtree::Node::seen): never 0, never given twice
inline uint32_t next_scan_mark() {                                  // (inline: ONE counter for the library, whoever includes this)
    static std::atomic<uint32_t> g{0};
    uint32_t m = ++g;
    if (m == 0) m = ++g;
    return m;
}

// The GPU scan of a pipelined commit, on a thread of its own: mi_batch_run (the end of staging, the kernels) and the roots'
// way back, while the committing thread computes the layer and frames the tar from the bytes that have already landed.
// Whoever needs a root before the scan is through waits for it (Fs::root_now); everybody else is handed the roots at the end.
struct ScanJob {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    int rc = MI_OK;
    std::string err;
    std::vector<uint8_t> roots;
    uint64_t n_chunks = 0;
    double seconds = 0;
    void start(mi_batch* b, uint64_t n_files) {
        roots.resize(n_files * 32);
        th = std::thread([this, b, n_files] {
            const auto t0 = std::chrono::steady_clock::now();
            int r = mi_batch_run(b);
            if (!r) r = mi_batch_roots(b, roots.data(), n_files);
            uint64_t nc = 0;
            if (!r) mi_batch_counts(b, nullptr, &nc, nullptr);
            std::string e = r ? mi_last_error_of_batch(b) : "";          // (a locked copy: the committing thread may be failing too)
            {
                std::lock_guard<std::mutex> g(mu);
                rc = r;
                err = std::move(e);
                n_chunks = nc;
                seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                done = true;
            }
            cv.notify_all();
        });
    }
    const uint8_t* wait_roots() {                              // nullptr: the scan failed (rc, err)
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done; });
        return rc ? nullptr : roots.data();
    }
    void join() { if (th.joinable()) th.join(); }
    ~ScanJob() { join(); }
};
// memLayer.files: path -> header.  A merged base image puts a million keys in and throws them away when the merge is done
// (only their number is reported): from the C library's heap that is a million small allocations, a million frees, and --
// some unrelated allocation later -- a sweep over a million free fragments (measured: 0.3 s added to the next scan that
// has more than a handful of changes).  So keys and table live in a pool that grows in large blocks and is given back whole.
// A MERGE (UpdateFromTarReader) never looks at the map again: "Merged %d headers from tar to memfs" is all that is left of
// it.  In count-only mode the map is therefore a set of 128-bit fingerprints of its keys (two independent 64-bit hashes,
// open addressing, 16 bytes a key instead of ~130 with two allocations): the number of distinct keys, exact unless two
// of a layer's paths collide in 128 bits (10^7 keys: 10^-25).  At C4's ten million entries the full map was 1.3 GB of
// first-touched memory and a microsecond per header (profiles/r05_host_scale.txt).
struct KeyCounter {
    struct Fp { uint64_t a, b; };
    std::vector<Fp> tab;                                                            // a == 0 && b == 0: free
    size_t n = 0;
    static Fp fp(const char* p, size_t len) {
        uint64_t a = 0x9E3779B97F4A7C15ull ^ len, b = 0xC2B2AE3D27D4EB4Full + len;
        while (len >= 8) {
            uint64_t w;
            memcpy(&w, p, 8);
            a = (a ^ w) * 0xFF51AFD7ED558CCDull; a ^= a >> 32;
            b = (b + w) * 0xC4CEB9FE1A85EC53ull; b = (b << 29) | (b >> 35);
            p += 8; len -= 8;
        }
        uint64_t w = 0;
        memcpy(&w, p, len);
        a = (a ^ w) * 0xFF51AFD7ED558CCDull; a ^= a >> 33; a *= 0xC4CEB9FE1A85EC53ull; a ^= a >> 29;
        b = (b + w) * 0x9FB21C651E98DF25ull; b ^= b >> 31; b *= 0xFF51AFD7ED558CCDull; b ^= b >> 32;
        if (!(a | b)) a = 1;
        return {a, b};
    }
    void reserve(size_t keys) {
        size_t want = 16;
        while (want < keys * 2) want <<= 1;
        if (want > tab.size()) rehash(want);
    }
    void rehash(size_t cap) {
        std::vector<Fp> old;
        old.swap(tab);
        tab.assign(cap, Fp{0, 0});
        for (const Fp& f : old) if (f.a | f.b) place(f);
    }
    void place(const Fp& f) {
        size_t i = (size_t)f.a & (tab.size() - 1);
        while (tab[i].a | tab[i].b) i = (i + 1) & (tab.size() - 1);
        tab[i] = f;
    }
    void add(const char* p, size_t len) {
        if ((n + 1) * 2 > tab.size()) rehash(tab.empty() ? 1024 : tab.size() * 2);
        const Fp f = fp(p, len);
        size_t i = (size_t)f.a & (tab.size() - 1);
        for (; tab[i].a | tab[i].b; i = (i + 1) & (tab.size() - 1))
            if (tab[i].a == f.a && tab[i].b == f.b) return;
        tab[i] = f;
        ++n;
    }
    void clear() { std::vector<Fp>().swap(tab); n = 0; }
};

struct LayerMap {
    using Map = std::pmr::unordered_map<std::pmr::string, int64_t>;
    std::pmr::monotonic_buffer_resource pool;
    alignas(Map) unsigned char store[sizeof(Map)];
    Map* m;
    bool touched = false;
    bool count_only = false;                                                        // a merge under way: see KeyCounter
    KeyCounter counter;
    LayerMap() : m(new (store) Map(&pool)) {}
    ~LayerMap() { m->~Map(); }
    LayerMap(const LayerMap&) = delete;
    LayerMap& operator=(const LayerMap&) = delete;
    void set(const std::string& key, int64_t ref) {                                // l.files[key] = ...
        if (count_only) { counter.add(key.data(), key.size()); return; }
        touched = true;
        auto it = m->find(std::pmr::string(key.data(), key.size(), &scratch));
        scratch.release();
        if (it != m->end()) { it->second = ref; return; }
        auto at = m->emplace(std::piecewise_construct, std::forward_as_tuple(key.data(), key.size()), std::forward_as_tuple(ref)).first;
        seq.push_back(&*at);                                                       // (a table's elements do not move)
    }
    std::vector<const Map::value_type*> seq;                                       // the keys in the order they came
    size_t size() const { return count_only ? counter.n : m->size(); }
    void reserve(size_t n) { if (count_only) { counter.reserve(n); return; } touched = true; m->reserve(n); }
    void clear() {
        counter.clear();
        count_only = false;
        if (!touched) return;
        m->~Map();
        pool.release();
        m = new (store) Map(&pool);
        seq.clear();
        touched = false;
    }
private:
    unsigned char scratch_buf[512];
    std::pmr::monotonic_buffer_resource scratch{scratch_buf, sizeof scratch_buf};  // the lookup's key: never the pool's
};

struct Fs {
    mi_memtree::Tree t;                      // fs.tree; a node's ref indexes `nodes`
    std::vector<Node> nodes;
    LayerMap layer;                          // memLayer.files: keyed by dst -- by the DELETED path for a ".wh." name;
                                             // sorted when the layer is taken (rangeFiles, mem_layer.go:232-244)
    std::vector<Node> sorted_layer() const {                                        // sort.Strings on the keys: they came in
        const size_t n = layer.seq.size();                                          // walk order, which is nearly sorted
        std::vector<mi_walk::KeyRef> keys(n);
        std::vector<uint64_t> idx(n), tmp(n);
        for (size_t i = 0; i < n; ++i) {
            keys[i].p = layer.seq[i]->first.data();
            keys[i].len = (uint32_t)layer.seq[i]->first.size();
            idx[i] = i;
        }
        mi_walk::natural_merge_sort(idx.data(), tmp.data(), n, keys.data());
        std::vector<Node> out;
        out.reserve(n);
        for (size_t i = 0; i < n; ++i) out.push_back(nodes[layer.seq[idx[i]]->second]);
        return out;
    }
    std::string root;                      // fs.tree.src
    // the scan under way: "its walk lists this path".  Nodes the tree held when the scan began carry the answer as a
    // mark (Node::seen == scan_mark, set in one pass over the walk); for a node made DURING the scan the set of the walk's
    // paths is asked -- built the first time that happens, which a scan of an unchanged tree never sees
    uint32_t scan_mark = 0;                                          // 0 = no scan under way
    std::function<bool(const std::string&)> listed_by_walk;          // the fallback
    int64_t now = 0;
    std::string err;
    int rc = MI_OK;

    bool fail(int code, const std::string& m) { if (!rc) { rc = code; err = m; } return false; }
    int64_t keep(Node n) { nodes.push_back(std::move(n)); return (int64_t)nodes.size() - 1; }

    Fs() {
        t.on_add = [this](const std::string& dst, int64_t ref) {               // memLayer.addHeader (mem_layer.go:197-212)
            if (ref < 0) {                                                      // a parent the caller's list left out
                Node d;
                d.e.mode = (uint32_t)(S_IFDIR | 0755); d.e.kind = 0; d.e.relpath = dst.substr(1); d.e.mtime = now;
                d.src = "/";
                ref = keep(d);
                if (mi_memtree::Node* n = t.find(dst)) n->ref = ref;
            }
            const size_t cut = dst.find_last_of('/');
            if (dst.compare(cut == std::string::npos ? 0 : cut + 1, 4, ".wh.") == 0) {
                const std::string name = mi_walk::base_of(dst);
                const std::string dir = mi_walk::dir_of(dst);
                layer.set((dir == "/" ? "" : dir) + "/" + name.substr(4), ref);
            } else {
                layer.set(dst, ref);
            }
        };
        t.make_dir = [this](const std::string& dst, const mi_memtree::Node& last_ancestor, uint32_t uid, uint32_t gid) {
            Node d;                                                             // mem_fs.go:551-559
            d.e.mode = last_ancestor.ref >= 0 ? nodes[last_ancestor.ref].e.mode : (uint32_t)(S_IFDIR | 0755);
            d.e.kind = 0;
            d.e.relpath = dst.substr(1);
            d.e.mtime = now;
            d.e.uid = uid;
            d.e.gid = gid;
            d.src = "/";                       // l.addHeader("", curr, hdr): src = AbsPath("") -- isOnDisk says yes, always
            return keep(d);
        };
    }
    // addAncestors (mem_fs.go:505-566); returns the resolved dst
    // Entries arrive directory by directory, and addAncestors of a second path below the same parent repeats the first
    // one's work to the letter when nothing of the chain has changed in between: the same existing directories go
    // through addHeader again (layer[path] = the same header), nothing is created, nothing is cleared.  So the parent of
    // the last call is remembered -- while its chain held directories only (no symlink to follow, no file in the way),
    // the tree has not changed shape since (a leaf put below that parent keeps the memo: it is nobody's ancestor) and
    // the layer map has not been emptied -- and such a call returns at once (a merge of 10^6 entries: 3.4 -> 1.6 us each, with the kept parent node of mi_memtree.h).
    struct { bool valid = false; std::string parent; uint64_t gen = 0; } anc_memo;
    uint64_t n_anc_calls = 0, n_anc_memo = 0;                                   // MI_MEMFS_TIMING
    // content-aware isUpdated, counted per layer (mi_commit_stats): files whose header tario.IsSimilarHeader calls similar
    // and whose chunk roots differ; unchanged files whose node had no root yet and took the scan's
    uint64_t n_content_changed = 0, n_roots_learned = 0;
    const mi_walk::InodeStamp* stamp_for_next_keep = nullptr;                   // memfs_scan -> maybe_add: the new node's inode stamp
    std::vector<HashedAs> hashed;                                               // [node index]; shorter than `nodes`: no record beyond it
    void record_hashed(int64_t ref, const mi_walk::InodeStamp& st) {
        if ((size_t)ref >= hashed.size()) hashed.resize(nodes.size());
        hashed[(size_t)ref].stamp = st;
        hashed[(size_t)ref].at_ns = commit_started_ns;
    }
    const uint64_t id = [] { static std::atomic<uint64_t> n{0}; return ++n; }();    // (a handle's number: never given twice)
    uint32_t reserved_mark = 0;                                                 // the coming scan's mark, taken before its walk (0: none)
    uint32_t commit_gen = 0;                                                    // which mi_memfs_commit_layer call of this handle is under way (Node::batch_gen)
    bool trust_ctime = false;                                                   // mi_memfs_set_options(MI_MEMFS_TRUST_CTIME)
    int64_t commit_started_ns = 0;                                              // CLOCK_REALTIME when the commit under way began its walk
    // "is the content of the regular file at `disk_path` known?" -- asked by the walk's directory readers, several at a time,
    // while nothing changes the tree (the diff runs after the walk).  Known = the tree holds the path with a root that was
    // computed from THIS inode in THIS state: same device, inode, size, mtime and ctime to the nanosecond -- and the ctime lies
    // safely before the moment the content was read (a write in the same clock tick as the recorded ctime would leave no
    // trace: git's "racily clean" rule; MI_TRUST_CTIME_SLACK_MS, default 20, covers the kernel's coarse clock).
    // Returns mi_walk::kContentKnown, and with it kEntryHeld when the file's header is also what the node holds (tario.IsSimilarHeader
    // on a regular file: mode bits, owner, size, whole-second mtime) -- such an entry is nothing to the diff: the node is marked
    // "listed by this scan's walk" HERE (`mark`: the scan's mark, reserved before the walk), by the reader that stat'ed the file,
    // and memfs_scan passes it over.  A million unchanged files are then compared by sixteen readers beside their fstatat, not by
    // the committing thread after the walk.
    uint8_t content_is_known(const std::string& disk_path, const struct stat& sb, const mi_walk::InodeStamp& st, uint32_t mark) {
        const uint64_t size = (uint64_t)sb.st_size;
        static const int64_t slack_ns = [] { const char* e = getenv("MI_TRUST_CTIME_SLACK_MS"); return (int64_t)(e && *e ? atol(e) : 20) * 1000000ll; }();
        const size_t root_len = root == "/" ? 0 : root.size();
        if (disk_path.size() <= root_len || memcmp(disk_path.data(), root.data(), root_len) != 0) return 0;
        // A directory reader asks about ONE directory's files, in name order -- the order of the node's children map.  So the
        // directory's node and a position among its children are kept PER THREAD (the tree's own kept parent belongs to the
        // committing thread): the next file is the next child, or a few steps on -- not a walk from the root and a search among
        // thousands of siblings whose map nodes no cache holds (2.4 us per file, summed over the readers, before; the walk of a
        // million trusted files cost 0.12 s more than the plain walk).  Nothing changes the tree while the walk runs.
        using Kids = decltype(mi_memtree::Node::children);
        struct DirMemo { uint64_t fs_id = 0, gen = 0; uint32_t mark = 0; std::string dir; const mi_memtree::Node* node = nullptr; Kids::const_iterator at; };   // (mark: a memo never outlives the walk it was made in)
        static thread_local DirMemo memo;
        const size_t cut = disk_path.find_last_of('/');
        const mi_memtree::Node* nd = nullptr;
        if (cut != std::string::npos && cut >= root_len && cut + 1 < disk_path.size()) {
            const size_t dir_len = cut - root_len;                                // the directory below the root ("" = the root itself)
            if (!(memo.fs_id == id && memo.gen == t.gen && memo.mark == mark && memo.dir.size() == dir_len &&
                  memcmp(memo.dir.data(), disk_path.data() + root_len, dir_len) == 0)) {
                memo.dir.assign(disk_path, root_len, dir_len);
                memo.node = t.find_walk(memo.dir);                                // (find_walk keeps no cache: safe from many threads)
                memo.fs_id = id;
                memo.gen = t.gen;
                memo.mark = mark;
                if (memo.node) memo.at = memo.node->children.begin();
            }
            if (memo.node) {
                const std::string_view name(disk_path.data() + cut + 1, disk_path.size() - cut - 1);
                const Kids& kids = memo.node->children;
                int steps = 0;
                while (memo.at != kids.end() && steps < 8 && std::string_view(memo.at->first) < name) { ++memo.at; ++steps; }
                if (memo.at == kids.end() || std::string_view(memo.at->first) != name) memo.at = kids.lower_bound(name);
                if (memo.at != kids.end() && std::string_view(memo.at->first) == name) { nd = memo.at->second.get(); ++memo.at; }
            }
        } else {
            nd = t.find_walk(disk_path.substr(root_len));
        }
        if (!nd || nd->ref < 0) return 0;
        const Node& x = nodes[(size_t)nd->ref];
        if (x.e.kind != 1 || !x.has_root || x.root_pending || x.e.size != size || (size_t)nd->ref >= hashed.size()) return 0;
        const HashedAs& h = hashed[(size_t)nd->ref];
        // a file system that keeps whole seconds (ext3, FAT, some network mounts) shows as a ctime without a sub-second part:
        // its racy window is the second (two for FAT), not the kernel's clock tick
        const int64_t window_ns = st.ctime_ns % 1000000000ll == 0 ? std::max<int64_t>(slack_ns, 2000000000ll) : slack_ns;
        if (!h.at_ns || !(h.stamp == st)) return 0;                             // (with a clock that only moves forward the next line
        if (st.ctime_ns + window_ns >= h.at_ns) return 0;                       //  alone catches every later change: its ctime is
                                                                                 //  newer than our read.  The equality is what holds
                                                                                 //  when the clock was set back in between.)  Racily
                                                                                 //  clean: read it again
        // (counted after the walk, from its record: a shared counter here is a cache line sixteen directory readers fight over)
        if (mark && x.e.mtime == (int64_t)sb.st_mtime && x.e.uid == (uint32_t)sb.st_uid && x.e.gid == (uint32_t)sb.st_gid &&
            (x.e.mode & 07777u) == ((uint32_t)sb.st_mode & 07777u)) {
            const_cast<mi_memtree::Node*>(nd)->seen = mark;                      // (this reader's directory, this node: nobody else's)
            return mi_walk::kContentKnown | mi_walk::kEntryHeld;
        }
        return mi_walk::kContentKnown;
    }
    ScanJob* job = nullptr;                                                     // a pipelined commit's scan (else roots come ready)
    std::vector<int64_t> pending_refs;                                          // nodes whose root[] is filled in when it ends
    // the root a DECISION needs, now: waits for the scan when the node's root is still on its way (nullptr + rc: it failed)
    const uint8_t* root_now(Node& x) {
        if (!x.has_root) return nullptr;
        if (x.root_pending) {
            const uint8_t* r = job ? job->wait_roots() : nullptr;
            if (!r) { fail(MI_ERR_IO, "gpu scan: " + (job ? job->err : std::string("no scan under way"))); return nullptr; }
            memcpy(x.root, r + 32 * (uint64_t)x.batch_file, 32);
            x.root_pending = false;
        }
        return x.root;
    }
    // the scan is through (roots) or has failed (nullptr): every node that was promised a root gets it, or loses the promise
    void settle_pending(const uint8_t* roots, std::vector<Node>* layer_nodes) {
        auto settle = [&](Node& x) {
            if (!x.root_pending) return;
            x.root_pending = false;
            if (roots) memcpy(x.root, roots + 32 * (uint64_t)x.batch_file, 32);
            else x.has_root = false;
        };
        for (int64_t ref : pending_refs) settle(nodes[(size_t)ref]);
        pending_refs.clear();
        if (layer_nodes) for (Node& x : *layer_nodes) settle(x);
    }
    void clear_layer() { layer.clear(); anc_memo.valid = false; }
    // where dst splits into parent and name; npos = do not memo.  (dst is AbsPath's result in every caller -- the merge,
    // the scan, the copy ops: "/", then clean elements; so its parent IS the chain addAncestors walks.)
    static size_t parent_len(const std::string& dst) {
        const size_t cut = dst.find_last_of('/');
        return (dst.size() < 2 || dst[0] != '/' || cut + 1 >= dst.size()) ? std::string::npos : cut;
    }
    std::string add_ancestors(const std::string& dst, bool inclusive, uint32_t uid, uint32_t gid) {
        const size_t plen = inclusive ? std::string::npos : parent_len(dst);
        ++n_anc_calls;
        if (plen != std::string::npos && anc_memo.valid && anc_memo.gen == t.gen && anc_memo.parent.size() == plen &&
            memcmp(anc_memo.parent.data(), dst.data(), plen) == 0) {
            ++n_anc_memo;
            return dst;
        }
        anc_memo.valid = false;
        std::string resolved = dst;
        if (!t.add_ancestors(dst, inclusive, 0, uid, gid, &resolved)) { fail(MI_ERR_INVALID, "add ancestors of " + dst + ": " + t.err); return resolved; }
        if (plen != std::string::npos && t.chain_plain && !rc) {
            anc_memo.valid = true;
            anc_memo.parent.assign(dst, 0, plen);
            anc_memo.gen = t.gen;
        }
        return resolved;
    }
    // a leaf has been put at dst (not a whiteout): below the memo's parent that changes no chain
    void leaf_put(const std::string& dst, uint64_t gen_before) {
        if (!anc_memo.valid || anc_memo.gen != gen_before) { anc_memo.valid = false; return; }
        const size_t plen = parent_len(dst);
        if (plen != std::string::npos && anc_memo.parent.size() == plen && memcmp(anc_memo.parent.data(), dst.data(), plen) == 0)
            anc_memo.gen = t.gen;
        else
            anc_memo.valid = false;
    }
    // memLayer.addWhiteout (mem_layer.go:214-228) + whiteoutMemFile.updateMemFS
    bool add_whiteout(const std::string& p) {
        const std::string name = mi_walk::base_of(p);
        if (mi_walk::has_prefix(name, ".wh.")) return fail(MI_ERR_INVALID, "add whiteout to layer " + p + ": base name contains whiteout prefix: " + p);
        const std::string dir = mi_walk::dir_of(p);
        Node w;
        w.e.kind = 1;
        w.e.mode = 0;
        w.e.relpath = ((dir == "/" ? "" : dir) + "/.wh." + name).substr(1);
        layer.set(p, keep(w));
        if (!t.wipe(p)) return fail(MI_ERR_INVALID, "update memfs with whiteout " + p + ": " + t.err);
        return true;
    }
    // maybeAddToLayer(l, src, dst, hdr, createWhiteout) (mem_fs.go:440-483)
    void maybe_add(const std::string& src, const std::string& dst, Node n, bool create_whiteout = false) {
        if (rc) return;
        bool updated = true;
        mi_memtree::Node* cur = t.find(dst);                                      // isUpdated (:487-503)
        const bool had_node = cur != nullptr;
        if (cur && cur->ref >= 0) {
            mi_tree_entry a, b;
            auto fill = [](const Node& x, mi_tree_entry* o) {
                memset(o, 0, sizeof *o);
                o->relpath = x.e.relpath.empty() ? "" : x.e.relpath.c_str();
                o->link_target = x.e.has_link ? x.e.link.c_str() : nullptr;
                o->size = x.e.size; o->mtime_sec = x.e.mtime; o->mode = x.e.mode; o->kind = x.e.kind;
                o->uid = x.e.uid; o->gid = x.e.gid; o->file_index = -1;
            };
            fill(nodes[cur->ref], &a);
            fill(n, &b);
            int similar = 0;
            Node& o = nodes[cur->ref];
            // the roots decide only when BOTH sides carry one (mi_entry_similar ignores a single one): only then may the
            // decision have to wait for a scan that is still running
            const bool both = o.has_root && n.has_root && a.kind == 1 && b.kind == 1;
            const uint8_t* ra = both ? root_now(o) : nullptr;
            const uint8_t* rb = both ? root_now(n) : nullptr;
            if (rc) return;
            if (a.kind <= 3 && b.kind <= 3 && mi_entry_similar(&a, &b, 0, ra, rb, &similar) != MI_OK) {
                fail(MI_ERR_INVALID, "check header " + dst + ": unsupported type");
                return;
            }
            updated = !similar;
            if (similar && n.has_root && !o.has_root && n.e.kind == 1 && o.e.kind == 1) {   // the first content scan of an unchanged
                Node& held = nodes[cur->ref];                                                // file: its root is known from now on
                held.has_root = true;
                if (n.root_pending) { held.root_pending = true; held.batch_file = n.batch_file; held.batch_gen = commit_gen; pending_refs.push_back(cur->ref); }
                else memcpy(held.root, n.root, 32);
                ++n_roots_learned;
            } else if (!similar && o.has_root && n.has_root && a.kind == 1 && b.kind == 1) {
                int meta = 0;
                if (mi_entry_similar(&a, &b, 0, nullptr, nullptr, &meta) == MI_OK && meta) ++n_content_changed;
            }
        }
        if (updated && dst != "/") {
            add_ancestors(dst, false, 0, 0);
            if (rc) return;
            n.src = src;
            const uint8_t kind = n.e.kind;
            const std::string link = n.e.has_link ? n.e.link : std::string();
            const int64_t kref = keep(std::move(n));
            if (nodes[(size_t)kref].root_pending) pending_refs.push_back(kref);
            if (stamp_for_next_keep) { record_hashed(kref, *stamp_for_next_keep); stamp_for_next_keep = nullptr; }
            else if ((size_t)kref < hashed.size()) hashed[(size_t)kref] = HashedAs();
            // updateMemFS walks the tree part by part (mem_layer.go:57-80): every part before the last has to be a
            // node -- of any type.  A destination spelled THROUGH a symlink therefore works one level below the
            // link (the link node takes the child) and fails deeper ("missing intermediate directory"): what
            // addAncestors created lies on the link's TARGET, and its resolved path is only used by the createDst branch
            const uint64_t gen_before = t.gen;
            if (!t.add(dst, kref, kind, link)) {
                fail(MI_ERR_INVALID, "update memfs with file " + dst + ": " + t.err);
                return;
            }
            if (dst.compare(dst.find_last_of('/') + 1, 4, ".wh.") != 0) leaf_put(dst, gen_before);   // (a ".wh." name wipes)
        }
        if (create_whiteout && n.e.kind == 0 && had_node) whiteout_missing_children(dst);
    }
    // "Handle deletions.  Note: Only one whiteout file is needed for a deleted subtree." (:460-480): the children
    // the tree holds for this directory that are no longer on disk
    void whiteout_missing_children(const std::string& dst) {
        mi_memtree::Node* dir = t.find(dst);
        if (!dir) return;
        std::vector<std::string> gone;                                      // (wiping changes the map: collect first)
        const std::string stem = dst == "/" ? "/" : dst + "/";
        const size_t root_len = root == "/" ? 0 : root.size();
        for (auto& kv : dir->children) {
            const int64_t ref = kv.second->ref;
            static const std::string no_src;
            const std::string& child_src = ref >= 0 ? nodes[ref].src : no_src;   // (two lvalues: no copy per child)
            // memFSNode.isOnDisk (:49-57) is an lstat of the node's source.  When that source is the node's own place
            // under the root and the walk of THIS scan lists it, the walk has just lstat'ed it: no second one (the
            // reference pays it for every node of the tree on every scan)
            if (scan_mark && child_src.size() == root_len + stem.size() + kv.first.size() &&
                memcmp(child_src.data(), root.data(), root_len) == 0 &&
                memcmp(child_src.data() + root_len, stem.data(), stem.size()) == 0 &&
                memcmp(child_src.data() + root_len + stem.size(), kv.first.data(), kv.first.size()) == 0 &&
                (kv.second->seen == scan_mark || (listed_by_walk && listed_by_walk(stem + kv.first))))
                continue;
            const std::string child = stem + kv.first;
            struct stat st;
            if (lstat(child_src.c_str(), &st) == 0) continue;
            if (errno != ENOENT && errno != ENOTDIR) {
                fail(MI_ERR_IO, "check on disk " + child + ": lstat " + child_src + ": " + strerror(errno));
                return;
            }
            gone.push_back(child);
        }
        for (const std::string& child : gone) {
            if (!add_whiteout(child)) return;
            add_ancestors(child, false, 0, 0);
            if (rc) return;
        }
    }
    // isUpdated (:487-503) on a walk entry as it comes, before any node is built for it: true = the tree holds this path
    // with a header tario.IsSimilarHeader calls similar (and, when both sides carry one, the same content root) --
    // maybeAddToLayer then adds nothing.  The scan's common case: most of a tree does not change between two steps.
    // lazy_file >= 0: the file's root is row lazy_file of a scan that may still be running (content_root is NULL then)
    // stamp (optional): the file's inode as the walk saw it -- recorded with the root whenever THIS commit hashed the content
    // own_root: the walk did not read the file because its content is KNOWN to be what the tree holds (MI_MEMFS_TRUST_CTIME):
    // its root is the node's own
    bool holds_similar(const std::string& dst, const mi_tree_entry& e, const uint8_t* content_root, int64_t lazy_file = -1,
                       const mi_walk::InodeStamp* stamp = nullptr, bool own_root = false) {
        mi_memtree::Node* cur = t.find(dst);
        if (!cur || cur->ref < 0 || e.kind > 3) return false;
        Node& o = nodes[cur->ref];
        if (o.e.kind > 3) return false;
        // (own_root: the content IS what the node's root describes -- nothing to compare, and the node's root stays untouched
        //  in whatever cache line it lies)
        const bool same_content = own_root && o.has_root && !o.root_pending;
        mi_tree_entry a, b = e;
        memset(&a, 0, sizeof a);
        a.relpath = o.e.relpath.empty() ? "" : o.e.relpath.c_str();
        a.link_target = o.e.has_link ? o.e.link.c_str() : nullptr;
        a.size = o.e.size; a.mtime_sec = o.e.mtime; a.mode = o.e.mode; a.kind = o.e.kind;
        a.uid = o.e.uid; a.gid = o.e.gid; a.file_index = -1;
        b.relpath = dst.c_str() + 1;                                             // dst without its leading "/"
        b.file_index = -1;
        const bool file_has_root = content_root != nullptr || lazy_file >= 0;
        const uint8_t *ra = nullptr, *rb = nullptr;
        if (!same_content && o.has_root && file_has_root && a.kind == 1 && b.kind == 1) {   // both carry a root: it decides -- now
            ra = root_now(o);
            rb = content_root;
            if (!rb && !rc) {
                const uint8_t* r = job ? job->wait_roots() : nullptr;
                if (!r) fail(MI_ERR_IO, "gpu scan: " + (job ? job->err : std::string("no scan under way")));
                else rb = r + 32 * (uint64_t)lazy_file;
            }
            if (rc) return false;
        }
        int similar = 0;
        if (mi_entry_similar(&a, &b, 0, ra, rb, &similar) != MI_OK) return false;
        if (similar && file_has_root && !o.has_root && o.e.kind == 1 && b.kind == 1) {   // (as in maybe_add)
            o.has_root = true;
            if (content_root) memcpy(o.root, content_root, 32);
            else { o.root_pending = true; o.batch_file = lazy_file; o.batch_gen = commit_gen; pending_refs.push_back(cur->ref); }
            ++n_roots_learned;
        }                                                                                // (a content-only change is counted
        if (similar && stamp && file_has_root && o.has_root && b.kind == 1)              //  where it is added: maybe_add)
            record_hashed(cur->ref, *stamp);                                             // hashed now, in this state
        return similar != 0;
    }
};

// evalSymlinks (utils.go:249-327): resolves the symlinks of p inside root; a link that leaves the
// root is an error.  Returns the path relative to root ("/"-rooted).
inline bool eval_symlinks(const std::string& p, const std::string& root, std::string* out, std::string* err) {
    if (p.empty()) { *out = p; return true; }
    std::string cur = p;
    for (int walked = 0; walked <= 255;) {
        // resolve the first symlink found walking the components of cur
        const std::vector<std::string> parts = mi_memtree::Tree::parts(cur);
        std::string acc;
        bool replaced = false;
        for (size_t i = 0; i < parts.size(); ++i) {
            const std::string here = acc + "/" + parts[i];
            struct stat st;
            if (lstat((root + here).c_str(), &st) != 0) { *err = "walk link: lstat: " + here + ": " + strerror(errno); return false; }
            if (S_ISLNK(st.st_mode)) {
                std::vector<char> buf(4096);
                const ssize_t n = readlink((root + here).c_str(), buf.data(), buf.size() - 1);
                if (n < 0) { *err = "readlink " + here + ": " + strerror(errno); return false; }
                std::string target(buf.data(), (size_t)n);
                if (!target.empty() && target[0] == '/') {
                    if (!mi_walk::has_prefix(target, root)) {
                        *err = "link points outside of root: " + root + here + " -> " + target;
                        return false;
                    }
                    target = target.substr(root.size());
                    if (target.empty() || target[0] != '/') target = "/" + target;
                } else {
                    target = acc + "/" + target;                         // relative to the link's directory
                }
                for (size_t k = i + 1; k < parts.size(); ++k) target += "/" + parts[k];
                cur = mi_walk::clean_rooted(target);
                ++walked;
                replaced = true;
                break;
            }
            acc = here;
        }
        if (!replaced) { *out = mi_walk::abs_path(cur); return true; }
    }
    *err = "eval symlinks: too many links";
    return false;
}

}  // namespace mi_copy

struct mi_copy_layer {
    std::vector<mi_copy::Node> nodes;                       // commit order
    // MI_MEMFS_CHUNK_PACK / _ZPACK: the recipes -- entry i's ordered chunks are rows [chunk_first[i], chunk_first[i + 1]) of the two
    // arrays (32 bytes / one length per row); chunk_first is empty for a layer of a commit without the option
    std::vector<uint64_t> chunk_first;
    std::vector<uint8_t>  chunk_digests;
    std::vector<uint32_t> chunk_lengths;
};

// ---- MemFS as a handle: the reference's type (lib/snapshot/mem_fs.go:59-125) behind the ABI ---------------------------
// One tree for the life of a build, as in the reference: base layers are merged into it (UpdateFromTarReader), every
// step's layer is computed against it and folds into it (AddLayerByScan / AddLayerByCopyOps).  What the stateless calls
// above cannot keep between calls is kept here: the directories addAncestors created, and for every node the path its
// content came from (memFSNode.src -- what isOnDisk looks at: a copied file is "on disk" while its SOURCE is).
struct mi_memfs {
    mi_copy::Fs fs;
    std::vector<std::string> blacklist;
    std::string err;
    // the content-aware commit (mi_memfs_commit_layer with a ctx): ONE batch, kept between commits -- its arena and tables
    // are sized by the first commit and reused by the next (mi_batch_reset).  Assigned by memfs_batch_for / memfs_batch_drop
    // (mi_commit.hip) and by nobody else: the commit, mi_memfs_reserve_device and mi_memfs_release_device go through them
    mi_batch* batch = nullptr;
    std::vector<mi_ctx*> batch_ctxs;     // the ctxs it was made for: one, or several -- then one batch per ctx behind the one
                                         // handle (mi_memfs_commit_layer_n: a group)
    mi_index* index = nullptr;           // mi_memfs_set_index: every content-aware commit adds its batch's chunks
    int root_alg = -1;                   // MI_DIGEST_* of the roots the tree holds; -1: no content-aware commit since the handle was
                                         // made or reset (memfs_commit refuses a ctx of the other kind)
    mi_commit_stats last;                // of the last mi_memfs_commit_layer
    bool went_windowed = false;          // the scanned tree did not fit the device (the next full scan goes window by window at once)
    // MI_MEMFS_CHUNK_PACK: the pack of the last commit until mi_memfs_take_pack hands it over (mi_commit.hip: memfs_pack_drop /
    // Commit::pack_and_recipes are its only writers); pack_rc: what a take returns while there is none, pack_err: why
    bool chunk_pack = false;
    mi_pack* pack = nullptr;
    int pack_rc = MI_ERR_STATE;
    std::string pack_err = "no commit since the last mi_memfs_take_pack";
    // MI_MEMFS_CHUNK_ZPACK: the same for the compressed pack (mi_memfs_take_zpack); the two options exclude each other
    bool chunk_zpack = false;
    bool zpack_level2 = false;                   // MI_MEMFS_ZPACK_LEVEL2: the commit codes it with MI_ZPACK_LEVEL2
    bool gzip_device = false;                    // MI_MEMFS_GZIP_DEVICE: the layer writer's gzip leg is coded on the commit's first ctx
    mi_zpack* zpack = nullptr;
    int zpack_rc = MI_ERR_STATE;
    std::string zpack_err = "no commit since the last mi_memfs_take_zpack";
    mi_memfs() { memset(&last, 0, sizeof last); }
    ~mi_memfs() { if (pack) mi_pack_free(pack); if (zpack) mi_zpack_free(zpack); if (batch) mi_batch_free(batch); }
};

// MI_MEMFS_TIMING=1: one line per merge / scan on stderr
inline bool memfs_timing() {
    static const bool on = [] { const char* e = getenv("MI_MEMFS_TIMING"); return e && *e && *e != '0'; }();
    return on;
}
struct MemfsTimer {
    const char* what; mi_copy::Fs& fs; uint64_t n; uint64_t calls0, memo0;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    MemfsTimer(const char* w, mi_copy::Fs& f, uint64_t n_) : what(w), fs(f), n(n_), calls0(f.n_anc_calls), memo0(f.n_anc_memo) {}
    ~MemfsTimer() {
        if (!memfs_timing()) return;
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "mi_memfs %s: %llu entries in %.3f s (%.2f us each), addAncestors %llu calls, %llu answered by the memo, %zu nodes held\n",
                what, (unsigned long long)n, s, n ? s * 1e6 / (double)n : 0.0, (unsigned long long)(fs.n_anc_calls - calls0),
                (unsigned long long)(fs.n_anc_memo - memo0), fs.nodes.size());
    }
};
inline mi_copy_layer* memfs_take_layer(mi_memfs* m) {
    const auto t0 = std::chrono::steady_clock::now();
    mi_copy_layer* l = new mi_copy_layer();
    l->nodes = m->fs.sorted_layer();
    m->fs.clear_layer();
    if (memfs_timing())
        fprintf(stderr, "mi_memfs: a layer of %zu entries put in commit order and handed over in %.3f s\n", l->nodes.size(),
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return l;
}
inline int memfs_fail(mi_memfs* m) {
    m->err = m->fs.err;
    const int rc = m->fs.rc;
    m->fs.rc = MI_OK;                                                             // the handle stays usable, like the
    m->fs.err.clear();                                                            // reference's MemFS after an error
    m->fs.clear_layer();
    return rc;
}

// ---- what crosses files (hidden: not part of the ABI, mi_local.h) ------------------------------------------------------
// mi_copyops.hip -- addToLayer for each op in two steps, PLAN (what the ops read from the disk) and APPLY (the ops against the
// tree); the commit runs its batch between the two
struct CopySrcPlan { std::string src; mi_walk::Tree walked; };
struct CopyOpPlan {
    std::string src_root, dst;
    bool create_dst = true;
    std::vector<CopySrcPlan> srcs;
};
struct CopyPlan {
    std::vector<CopyOpPlan> ops;
    int err_rc = MI_OK;                 // the failure planning stopped at ...
    std::string err;
    bool err_before_dst = false;        // ... raised before the last planned op touches the tree / after its planned sources
    uint64_t n_walked = 0;
};
MI_LOCAL void copy_ops_plan(const mi_copy::Fs& fs, const mi_copy_op* ops, uint64_t n_ops, mi_batch* batch, CopyPlan* plan);
MI_LOCAL int  copy_ops_apply(mi_copy::Fs& fs, const mi_copy_op* ops, const CopyPlan& plan, const uint8_t* roots, std::string* err_out);
MI_LOCAL int  copy_ops_into(mi_copy::Fs& fs, const mi_copy_op* ops, uint64_t n_ops, std::string* err_out);
// mi_memfs.hip -- createLayerByScan on a walk of the root
MI_LOCAL int  memfs_scan(mi_memfs* m, const mi_tree_entry* walked, uint64_t n, const void* roots, uint64_t root_stride, bool from_batch,
                         mi_copy_layer** out, uint64_t* n_entries, const mi_walk::Tree* wt = nullptr);
