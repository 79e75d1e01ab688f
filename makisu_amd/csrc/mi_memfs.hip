// mi_memfs.hip -- the reference's MemFS as a handle, on the host (no device code here): the one implementation of the layer
// merge and of a step's layer (MemFS.addToLayer, in mi_copyfs.h): create, UpdateFromTarReader with and without untar
// (MemFS.untarOneItem + tario.ApplyHeader), AddLayerByScan, AddLayerByCopyOps (its ops: mi_copyops.hip), Reset, and what a
// caller reads back (the tree's entries and roots, a layer's entries).  step.commitLayer on the handle is mi_commit.hip.
// Every function cites the Go it restates; the tree they share is mi_memtree.h, the walks are mi_tree.hip's.
#include "mi_copyfs.h"

#include <fcntl.h>
#include <ftw.h>

#include <algorithm>
#include <unordered_set>

// ---- untar: MemFS.untarOneItem and tario.ApplyHeader (lib/snapshot/mem_fs.go:571-718, lib/tario/apply.go:23-47) --------
namespace mi_untar {

static int rm_cb(const char* p, const struct stat*, int, struct FTW*) { return remove(p); }
static bool remove_all(const std::string& p, std::string* err) {                 // os.RemoveAll
    struct stat st;
    if (lstat(p.c_str(), &st) != 0) {
        if (errno == ENOENT || errno == ENOTDIR) return true;
        *err = "lstat " + p + ": " + strerror(errno);
        return false;
    }
    if (!S_ISDIR(st.st_mode)) {
        if (unlink(p.c_str()) == 0 || errno == ENOENT) return true;
        *err = "unlinkat " + p + ": " + strerror(errno);
        return false;
    }
    if (nftw(p.c_str(), rm_cb, 64, FTW_DEPTH | FTW_PHYS) != 0) { *err = "unlinkat " + p + ": " + strerror(errno); return false; }
    return true;
}

// tario.ApplyHeader: owner, then permission bits (chmod after chown: setuid / setgid survive), then mtime; never on a
// symlink and never FOR a symlink header
static bool apply_header(const std::string& path, const mi_tree_entry& h, std::string* err) {
    struct stat st;
    if (lstat(path.c_str(), &st) != 0) { *err = "lstat " + path + ": " + strerror(errno); return false; }
    if (S_ISLNK(st.st_mode) || h.kind == 2) { *err = "update symlink instead of file: " + path; return false; }
    if (chown(path.c_str(), h.uid, h.gid) != 0) { *err = "chown " + path + ": " + strerror(errno); return false; }
    if (chmod(path.c_str(), h.mode & 07777) != 0) { *err = "chmod " + path + ": " + strerror(errno); return false; }
    struct timespec ts[2];
    ts[0].tv_sec = ts[1].tv_sec = (time_t)h.mtime_sec;
    ts[0].tv_nsec = ts[1].tv_nsec = 0;
    if (utimensat(AT_FDCWD, path.c_str(), ts, 0) != 0) { *err = "chtimes " + path + ": " + strerror(errno); return false; }
    return true;
}

static bool copy_range(int in_fd, uint64_t off, uint64_t len, int out_fd, std::string* err) {
    std::vector<char> buf(1 << 20);
    while (len) {
        const size_t want = len < buf.size() ? (size_t)len : buf.size();
        const ssize_t r = pread(in_fd, buf.data(), want, (off_t)off);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) { *err = r == 0 ? "unexpected EOF" : strerror(errno); return false; }
        size_t done = 0;
        while (done < (size_t)r) {
            const ssize_t w = write(out_fd, buf.data() + done, (size_t)r - done);
            if (w < 0 && errno == EINTR) continue;
            if (w < 0) { *err = strerror(errno); return false; }
            done += (size_t)w;
        }
        off += (uint64_t)r;
        len -= (uint64_t)r;
    }
    return true;
}

// untarOneItem(path, header, r): root = fs.tree.src; path = filepath.Join(root, hdr.Name); content of a regular file =
// [data_off, +size) of tar_fd
static bool one_item(const std::string& root, const std::string& path, const mi_tree_entry& h, int tar_fd, uint64_t data_off,
                     std::string* err) {
    const std::string base = mi_walk::base_of(path), dir = mi_walk::dir_of(path);
    std::string e;
    if (mi_walk::has_prefix(base, ".wh.")) {                                     // untarWhiteout
        if (!remove_all((dir == "/" ? "" : dir) + "/" + base.substr(4), &e)) { *err = "untar dir: untar whiteout: " + e; return false; }
        return true;
    }
    struct stat st;
    if (lstat(path.c_str(), &st) != 0) {
        if (errno != ENOENT && errno != ENOTDIR) { *err = "lstat " + path + ": " + strerror(errno); return false; }
    } else {
        // the header of what is there (tar.FileInfoHeader), link target trimmed of the root
        mi_tree_entry local;
        memset(&local, 0, sizeof local);
        std::string link;
        local.relpath = h.relpath && *h.relpath ? h.relpath : "x";              // (only "both names empty" matters to the predicate)
        local.mode = st.st_mode; local.mtime_sec = st.st_mtime; local.uid = st.st_uid; local.gid = st.st_gid;
        local.kind = S_ISDIR(st.st_mode) ? 0 : S_ISREG(st.st_mode) ? 1 : S_ISLNK(st.st_mode) ? 2 : 4;
        local.size = S_ISREG(st.st_mode) ? (uint64_t)st.st_size : 0;
        if (S_ISLNK(st.st_mode)) {
            std::vector<char> buf(4096);
            const ssize_t n = readlink(path.c_str(), buf.data(), buf.size() - 1);
            if (n < 0) { *err = "read link " + path + ": " + strerror(errno); return false; }
            link.assign(buf.data(), (size_t)n);
            if (!link.empty() && link[0] == '/') {
                if (!mi_walk::has_prefix(link, root)) { *err = "trim link " + link + ": failed to trim root prefix " + root + " from path " + link; return false; }
                link = mi_walk::abs_path(link.substr(root.size()));
            }
            local.link_target = link.c_str();
        }
        if (local.kind > 3) { *err = "compare headers " + path + ": unsupported type"; return false; }
        int similar = 0;
        mi_tree_entry hh = h;
        if (!hh.relpath || !*hh.relpath) hh.relpath = "x";
        if (mi_entry_similar(&local, &hh, 0, nullptr, nullptr, &similar) != MI_OK) { *err = "compare headers " + path + ": unsupported type"; return false; }
        if (similar) return true;                                                // "already on disk, nothing needs to be done"
        if (h.kind == 0 && S_ISDIR(st.st_mode)) {                                // existing directories are updated, not deleted
            if (!apply_header(path, h, &e)) { *err = "update fi " + path + ": " + e; return false; }
            return true;
        }
        if (!remove_all(path, &e)) { *err = "clear existing file " + path + ": " + e; return false; }
    }
    if (h.kind == 0) {
        if (mkdir(path.c_str(), h.mode & 07777) != 0) { *err = "untar dir: create dir " + path + ": " + strerror(errno); return false; }
        if (!apply_header(path, h, &e)) { *err = "untar dir: update fi " + path + ": " + e; return false; }
    } else if (h.kind == 2) {
        std::string target = h.link_target ? h.link_target : "";
        if (!target.empty() && target[0] == '/') target = mi_walk::abs_path(root + "/" + target);   // filepath.Join(root, target)
        if (symlink(target.c_str(), path.c_str()) != 0) { *err = "untar symlink: create symlink " + path + " => " + target + ": " + strerror(errno); return false; }
        if (lchown(path.c_str(), h.uid, h.gid) != 0) { *err = "untar symlink: lchown symlink: " + path; return false; }
    } else if (h.kind == 3) {
        const std::string target = mi_walk::abs_path(root + "/" + (h.link_target ? h.link_target : ""));
        if (link(target.c_str(), path.c_str()) != 0) { *err = "untar hard link: create link " + path + " => " + target + ": " + strerror(errno); return false; }
        if (!apply_header(path, h, &e)) { *err = "untar hard link: update hard link " + path + ": " + e; return false; }
    } else {
        const int fd = open(path.c_str(), O_CREAT | O_TRUNC | O_WRONLY | O_CLOEXEC, h.mode & 07777);
        if (fd < 0) { *err = "untar file: open file " + path + ": " + strerror(errno); return false; }
        const bool ok = h.size == 0 || (tar_fd >= 0 && copy_range(tar_fd, data_off, h.size, fd, &e));
        close(fd);
        if (!ok) { *err = "untar file: read from file " + path + ": " + (tar_fd < 0 ? "no archive to read from" : e); return false; }
        if (!apply_header(path, h, &e)) { *err = "untar file: update fi " + path + ": " + e; return false; }
    }
    return true;
}

}  // namespace mi_untar

extern "C" int mi_memfs_create(const char* root, const char* const* blacklist, uint64_t n_blacklist, int64_t now_sec,
                               mi_memfs** out) {
    if (!root || !out || (n_blacklist && !blacklist)) return MI_ERR_INVALID;
    struct stat st;
    if (lstat(root, &st) != 0) {
        mi_set_error(nullptr, (std::string("unable to stat root dir: ") + root).c_str());      // mi_last_error(NULL)
        return MI_ERR_IO;
    }
    mi_memfs* m = new mi_memfs();
    m->fs.root = mi_walk::abs_path(root);
    m->fs.now = now_sec;
    mi_copy::Node r;
    r.e.kind = 0;
    r.e.mode = st.st_mode; r.e.mtime = st.st_mtime; r.e.uid = st.st_uid; r.e.gid = st.st_gid;
    r.src = m->fs.root;
    m->fs.t.root.ref = m->fs.keep(r);
    for (uint64_t i = 0; i < n_blacklist; ++i) m->blacklist.push_back(blacklist[i] ? blacklist[i] : "");
    *out = m;
    return MI_OK;
}
extern "C" void mi_memfs_free(mi_memfs* m) { delete m; }
extern "C" const char* mi_memfs_error(const mi_memfs* m) { return m ? m->err.c_str() : ""; }
extern "C" int mi_memfs_set_clock(mi_memfs* m, int64_t now_sec) {
    if (!m) return MI_ERR_INVALID;
    m->fs.now = now_sec;
    return MI_OK;
}
extern "C" int mi_memfs_reset(mi_memfs* m) {                                      // MemFS.Reset (:127-130)
    if (!m) return MI_ERR_INVALID;
    m->fs.t.root.children.clear();
    m->fs.t.shape_reset();
    m->root_alg = -1;                                                             // (no roots left: a ctx of either algorithm may commit)
    return MI_OK;
}

// MemFS.UpdateFromTarReader (:165-255) on a layer's entries (mi_tar_entries); tar_fd >= 0: untar = true, a regular file's
// bytes are [data_offsets[j], +size) of that descriptor
static int memfs_update(mi_memfs* m, const mi_tree_entry* layer, uint64_t n_layer, int tar_fd, const uint64_t* data_offsets,
                        bool untar, uint64_t* n_merged) {
    mi_copy::Fs& fs = m->fs;
    MemfsTimer timer(untar ? "untar + merge" : "merge", fs, n_layer);
    fs.clear_layer();
    std::map<std::string, struct timespec> modtimes;                              // parent directories, to be put back
    std::string uerr;
    const mi_walk::MountTable& mt = mi_walk::mountpoints();
    if (!mt.error.empty()) { m->err = "check if mounted: " + mt.error; return MI_ERR_IO; }
    std::vector<std::string> bl;
    for (const std::string& b : m->blacklist) bl.push_back(mi_walk::abs_path(b));
    std::vector<std::string> below_mount;                                         // "<target>/": isMounted's prefixes
    for (const std::string& t : mt.targets) below_mount.push_back(t.back() == '/' ? t : t + "/");
    // "is this directory at or below a mountpoint" is asked once per directory, not per entry (entries come
    // directory by directory): an entry is mounted iff it IS a target or its directory lies at or below one
    std::string mdir;
    bool mdir_set = false, mdir_below = false;
    std::string on_disk_buf;
    auto skipped = [&](const mi_tree_entry& e, const std::string& p) {            // shouldSkip + IsMounted (:190-199)
        const size_t cut = p.find_last_of('/');
        if (p.compare(cut == std::string::npos ? 0 : cut + 1, 8, ".wh..wh.") == 0) return true;
        if (e.kind > 3) return true;
        if (fs.root == "/") on_disk_buf = p; else { on_disk_buf = fs.root; if (p != "/") on_disk_buf += p; }
        const std::string& on_disk = on_disk_buf;
        if (!bl.empty() && mi_walk::is_descendant_of_any_cleaned(on_disk, bl, bl)) return true;   // (bl: AbsPath'ed above, once)
        if (mt.targets.empty()) return false;
        if (mt.targets.count(on_disk)) return true;
        const size_t dcut = on_disk.find_last_of('/');
        if (dcut == std::string::npos) return false;
        if (!mdir_set || mdir.size() != dcut + 1 || memcmp(mdir.data(), on_disk.data(), dcut + 1) != 0) {
            mdir.assign(on_disk, 0, dcut + 1);                                   // the directory with its slash
            mdir_set = true;
            mdir_below = false;
            for (const std::string& t : below_mount)
                if (mi_walk::has_prefix(mdir, t)) { mdir_below = true; break; }
        }
        return mdir_below;
    };
    auto disk_path = [&](const std::string& p) { return fs.root == "/" ? p : fs.root + (p == "/" ? "" : p); };
    std::string src_buf;
    auto one = [&](const mi_tree_entry& e, const std::string& p, uint64_t j) {
        if (untar && !mi_untar::one_item(fs.root, disk_path(p), e, tar_fd, data_offsets ? data_offsets[j] : 0, &uerr)) {
            fs.fail(MI_ERR_IO, "untar one item " + disk_path(p) + ": " + uerr);
            return;
        }
        mi_copy::Node n;
        n.e.relpath = p == "/" ? "" : p.substr(1);
        n.e.kind = e.kind; n.e.mode = e.mode; n.e.mtime = e.mtime_sec; n.e.uid = e.uid; n.e.gid = e.gid; n.e.size = e.size;
        if (e.link_target) {
            n.e.has_link = true;                                                  // "Docker hard link names are all absolute,
            n.e.link = e.kind == 3 ? mi_walk::abs_path(e.link_target) : e.link_target;   //  but don't have a leading slash"
        }
        // src: the reference passes AbsPath(hdr.Name) (:225) -- the path the entry is untarred to when the root is "/",
        // as in every real build; under another root that is filepath.Join(root, name), and isOnDisk must look THERE
        if (fs.root == "/") src_buf = p; else { src_buf = fs.root; if (p != "/") src_buf += p; }
        fs.maybe_add(src_buf, p, std::move(n), false);
    };
    std::map<std::string, uint64_t> hardlinks;
    // (with room to spare: the first header a later step adds must not be the one that moves a million nodes)
    fs.nodes.reserve(fs.nodes.size() + n_layer + n_layer / 4 + 1024);
    fs.layer.count_only = true;                                                   // (nothing reads this layer: its size is reported)
    fs.layer.reserve(n_layer + n_layer / 8 + 16);                                 // (its entries: the layer's paths and their ancestors)
    std::string p;                                                                // one buffer for every header's path
    for (uint64_t j = 0; j < n_layer && !fs.rc; ++j) {
        mi_walk::abs_path_of_rel_into(layer[j].relpath ? layer[j].relpath : "", &p);
        if (skipped(layer[j], p)) continue;
        if (untar) {                                                              // "Record the modtime of the parent directory to
            const std::string parent = mi_walk::dir_of(disk_path(p));             //  reset it after we deal with all of the other files"
            if (!modtimes.count(parent)) {
                struct stat st;
                if (lstat(parent.c_str(), &st) != 0) {
                    fs.fail(MI_ERR_IO, "stat parent dir of " + disk_path(p) + ": " + strerror(errno));
                    break;
                }
                modtimes[parent] = st.st_mtim;
            }
        }
        if (layer[j].kind == 3) { hardlinks[p] = j; continue; }
        one(layer[j], p, j);
    }
    for (auto& kv : hardlinks) {
        if (fs.rc) break;
        one(layer[kv.second], kv.first, kv.second);
    }
    const bool untar_failed = fs.rc == MI_ERR_IO;
    if (fs.rc) { if (!untar_failed) fs.err = "add hdr from tar to layer: " + fs.err; return memfs_fail(m); }
    for (auto& kv : modtimes) {                                                   // "Reset the mod times on all of the directory we changed"
        struct timespec ts[2] = {kv.second, kv.second};
        if (utimensat(AT_FDCWD, kv.first.c_str(), ts, 0) != 0) {
            m->err = "chtimes on parent directory " + kv.first + ": " + strerror(errno);
            fs.clear_layer();
            return MI_ERR_IO;
        }
    }
    if (n_merged) *n_merged = fs.layer.size();                                    // "Merged %d headers from tar to memfs"
    fs.clear_layer();
    return MI_OK;
}

extern "C" int mi_memfs_update_from_entries(mi_memfs* m, const mi_tree_entry* layer, uint64_t n_layer,
                                            uint64_t* n_merged) {
    if (!m || (n_layer && !layer)) return MI_ERR_INVALID;
    return memfs_update(m, layer, n_layer, -1, nullptr, false, n_merged);
}

// UpdateFromTarReader with untar = true: the entries of a PLAIN tar (mi_tar_entries of tar_path with their data offsets;
// a gzip blob goes through mi_tar_inflate first) are written below the root as untarOneItem does -- whiteouts delete,
// what is already there and similar stays, a directory on a directory is updated in place, anything else is replaced;
// hard links last; the parents' mtimes are put back -- and merged into the tree
extern "C" int mi_memfs_untar(mi_memfs* m, const char* tar_path, const mi_tree_entry* layer, const uint64_t* data_offsets,
                              uint64_t n_layer, uint64_t* n_merged) {
    if (!m || !tar_path || (n_layer && (!layer || !data_offsets))) return MI_ERR_INVALID;
    const int fd = open(tar_path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) { m->err = std::string("open tar file ") + tar_path + ": " + strerror(errno); return MI_ERR_IO; }
    const int rc = memfs_update(m, layer, n_layer, fd, data_offsets, true, n_merged);
    close(fd);
    return rc;
}

// MemFS.createLayerByScan (:315-341) on a walk of the root (mi_tree_walk / mi_batch_add_tree with MI_TREE_SCAN,
// rel_base = root): every walked path through maybeAddToLayer with createWhiteout = true
// from_batch: the walk is a batch's (mi_batch_add_tree) -- an entry's file_index is its row there, and the layer's nodes keep it
// wt (optional): the walk's own record of the same entries (inode stamps, which files were not staged because their content is known)
int memfs_scan(mi_memfs* m, const mi_tree_entry* walked, uint64_t n, const void* roots, uint64_t root_stride, bool from_batch,
               mi_copy_layer** out, uint64_t* n_entries, const mi_walk::Tree* wt) {
    if (!m || (n && !walked) || !out) return MI_ERR_INVALID;
    mi_copy::Fs& fs = m->fs;
    MemfsTimer timer("scan", fs, n);
    fs.clear_layer();
    // pass 1: the nodes the tree holds for the walk's paths are marked "listed by this scan's walk"
    // (a reserved mark: the readers of THIS walk -- wt -- have marked the entries they found held with it)
    const uint32_t mark = wt && wt->want_stamps && fs.reserved_mark ? fs.reserved_mark : mi_copy::next_scan_mark();
    fs.reserved_mark = 0;
    std::string p;                                                              // one buffer for every path of the walk
    const bool have_flags = wt && wt->want_stamps;
    auto held_by_walk = [&](uint64_t i) { return have_flags && i < wt->known.size() && (wt->known[i] & mi_walk::kEntryHeld); };
    for (uint64_t i = 0; i < n; ++i) {
        if (held_by_walk(i)) continue;                                           // (marked where it was stat'ed)
        mi_walk::abs_path_of_rel_into(walked[i].relpath ? walked[i].relpath : "", &p);
        if (mi_memtree::Node* nd = fs.t.find(p)) nd->seen = mark;
    }
    std::unordered_set<std::string> on_walk;                                    // the fallback, built when first asked
    bool on_walk_built = false;
    fs.scan_mark = mark;
    fs.listed_by_walk = [&](const std::string& q) {
        if (!on_walk_built) {
            if (memfs_timing()) fprintf(stderr, "mi_memfs scan: the set of the walk's paths is built (asked about %s)\n", q.c_str());
            on_walk.reserve(n * 2);
            for (uint64_t i = 0; i < n; ++i) on_walk.insert(mi_walk::abs_path_of_rel(walked[i].relpath ? walked[i].relpath : ""));
            on_walk_built = true;
        }
        return on_walk.count(q) != 0;
    };
    struct Unset { mi_copy::Fs& f; ~Unset() { f.scan_mark = 0; f.listed_by_walk = nullptr; } } unset{fs};
    for (uint64_t i = 0; i < n && !fs.rc; ++i) {
        if (held_by_walk(i)) continue;                                           // a regular file, header and content as the tree holds them
        const mi_tree_entry& e = walked[i];
        mi_walk::abs_path_of_rel_into(e.relpath ? e.relpath : "", &p);
        const bool lazy = !roots && fs.job && from_batch && e.kind == 1 && e.file_index >= 0;   // (the scan may still be running)
        const uint8_t* content_root =
            roots && e.kind == 1 && e.file_index >= 0 ? (const uint8_t*)roots + (uint64_t)e.file_index * root_stride : nullptr;
        const bool have_wt = wt && wt->want_stamps && i < wt->stamps.size();
        const bool hashed_now = (from_batch || roots) && e.kind == 1 && e.file_index >= 0 && have_wt;   // (a batch's row, or a window's)
        const bool held = fs.holds_similar(p, e, content_root, lazy ? e.file_index : -1, hashed_now ? &wt->stamps[i] : nullptr,
                                           have_wt && wt->known[i]);       // (not read again: the content the tree knows)
        if (fs.rc) break;
        if (held) {                                                               // nothing to add; a directory's deletions
            if (e.kind == 0) fs.whiteout_missing_children(p);                     // are still looked for (maybe_add's tail)
            continue;
        }
        mi_copy::Node nd;
        nd.e.relpath = p == "/" ? "" : p.substr(1);
        nd.e.kind = e.kind; nd.e.mode = e.mode; nd.e.mtime = e.mtime_sec; nd.e.uid = e.uid; nd.e.gid = e.gid; nd.e.size = e.size;
        if (e.link_target) { nd.e.has_link = true; nd.e.link = e.link_target; }
        if (roots && e.kind == 1 && e.file_index >= 0) {
            nd.has_root = true;
            memcpy(nd.root, (const uint8_t*)roots + (uint64_t)e.file_index * root_stride, 32);
        }
        if (from_batch && e.kind == 1 && e.file_index >= 0) { nd.batch_file = e.file_index; nd.batch_gen = fs.commit_gen; }
        if (lazy) { nd.has_root = true; nd.root_pending = true; }
        fs.stamp_for_next_keep = hashed_now && nd.has_root ? &wt->stamps[i] : nullptr;   // (recorded with the node maybe_add keeps)
        const std::string src = fs.root == "/" ? p : fs.root + (p == "/" ? "" : p);
        fs.maybe_add(src, p, std::move(nd), true);
        fs.stamp_for_next_keep = nullptr;
    }
    if (fs.rc) { fs.err = "add to layer: " + fs.err; return memfs_fail(m); }
    mi_copy_layer* l = memfs_take_layer(m);
    if (n_entries) *n_entries = l->nodes.size();
    *out = l;
    return MI_OK;
}

extern "C" int mi_memfs_add_layer_by_scan(mi_memfs* m, const mi_tree_entry* walked, uint64_t n, const void* roots,
                                          uint64_t root_stride, mi_copy_layer** out, uint64_t* n_entries) {
    return memfs_scan(m, walked, n, roots, root_stride, false, out, n_entries);
}

// MemFS.AddLayerByCopyOps (:276-289): the ops against THIS tree, which they update
extern "C" int mi_memfs_add_layer_by_copy_ops(mi_memfs* m, const mi_copy_op* ops, uint64_t n_ops, mi_copy_layer** out,
                                              uint64_t* n_entries) {
    if (!m || (n_ops && !ops) || !out) return MI_ERR_INVALID;
    m->fs.clear_layer();
    std::string e;
    const int rc = copy_ops_into(m->fs, ops, n_ops, &e);
    if (rc) { if (m->fs.rc) return memfs_fail(m); m->err = e; m->fs.clear_layer(); return rc; }
    mi_copy_layer* l = memfs_take_layer(m);
    if (n_entries) *n_entries = l->nodes.size();
    *out = l;
    return MI_OK;
}

// the chunk root the tree holds for a path (absolute, below the root "/"): what the next isUpdated compares
extern "C" int mi_memfs_root_of(const mi_memfs* m, const char* path, uint8_t* root_out, int* has_root) {
    if (!m || !path || !has_root) return MI_ERR_INVALID;
    *has_root = 0;
    const mi_memtree::Node* nd = const_cast<mi_memtree::Tree&>(m->fs.t).find_walk(mi_walk::abs_path(path));
    if (!nd || nd->ref < 0) return MI_ERR_INVALID;
    const mi_copy::Node& n = m->fs.nodes[nd->ref];
    if (n.has_root) { *has_root = 1; if (root_out) memcpy(root_out, n.root, 32); }
    return MI_OK;
}
extern "C" int mi_copy_layer_roots(const mi_copy_layer* l, uint8_t* roots, uint8_t* has_root, uint64_t cap) {
    if (!l || (cap && (!roots || !has_root))) return MI_ERR_INVALID;
    if (cap < l->nodes.size()) return MI_ERR_CAPACITY;
    for (size_t i = 0; i < l->nodes.size(); ++i) {
        has_root[i] = l->nodes[i].has_root ? 1 : 0;
        if (l->nodes[i].has_root) memcpy(roots + i * 32, l->nodes[i].root, 32); else memset(roots + i * 32, 0, 32);
    }
    return MI_OK;
}

// the ordered chunks of layer entry `entry`: the recipe a chunk store rebuilds the file from (MI_MEMFS_CHUNK_PACK)
extern "C" int mi_copy_layer_chunks(const mi_copy_layer* l, uint64_t entry, uint8_t* digests, uint32_t* lengths, uint64_t cap, uint64_t* n) {
    if (!l || !n || entry >= l->nodes.size() || (cap && (!digests || !lengths))) return MI_ERR_INVALID;
    const uint64_t first = l->chunk_first.empty() ? 0 : l->chunk_first[entry];
    const uint64_t cnt = l->chunk_first.empty() ? 0 : l->chunk_first[entry + 1] - first;
    *n = cnt;
    if (cap == 0) return MI_OK;                                                   // sizing
    if (cap < cnt) return MI_ERR_CAPACITY;
    if (cnt) {
        memcpy(digests, l->chunk_digests.data() + 32 * first, 32 * cnt);
        memcpy(lengths, l->chunk_lengths.data() + first, 4 * cnt);
    }
    return MI_OK;
}

// the tree, sorted by path (directories made up by addAncestors included: they are nodes like any other)
extern "C" int mi_memfs_entries(const mi_memfs* m, mi_tree_entry* out, const char** src_paths, uint64_t cap, uint64_t* n_out) {
    if (!m || !n_out || (cap && !out)) return MI_ERR_INVALID;
    std::vector<std::pair<std::string, int64_t>> flat;
    std::function<void(const mi_memtree::Node&, const std::string&)> collect = [&](const mi_memtree::Node& n, const std::string& p) {
        for (auto& kv : n.children) {
            const std::string q = p + "/" + kv.first;
            if (kv.second->ref >= 0) flat.emplace_back(q, kv.second->ref);
            collect(*kv.second, q);
        }
    };
    collect(m->fs.t.root, "");
    std::sort(flat.begin(), flat.end());
    *n_out = flat.size();
    if (cap < flat.size()) return MI_ERR_CAPACITY;
    for (size_t i = 0; i < flat.size(); ++i) {
        const mi_copy::Node& n = m->fs.nodes[flat[i].second];
        memset(&out[i], 0, sizeof out[i]);
        out[i].relpath = n.e.relpath.c_str();
        out[i].link_target = n.e.has_link ? n.e.link.c_str() : nullptr;
        out[i].file_index = -1;
        out[i].size = n.e.size; out[i].mtime_sec = n.e.mtime; out[i].mode = n.e.mode; out[i].kind = n.e.kind;
        out[i].uid = n.e.uid; out[i].gid = n.e.gid;
        if (src_paths) src_paths[i] = n.src.c_str();
    }
    return MI_OK;
}

extern "C" int mi_copy_layer_entries(const mi_copy_layer* l, mi_tree_entry* out, const char** src_paths, uint64_t cap) {
    if (!l || (cap && !out)) return MI_ERR_INVALID;
    if (cap < l->nodes.size()) return MI_ERR_CAPACITY;
    int64_t n_regular = 0;
    for (size_t i = 0; i < l->nodes.size(); ++i) {
        const mi_copy::Node& n = l->nodes[i];
        memset(&out[i], 0, sizeof out[i]);
        out[i].relpath = n.e.relpath.c_str();
        out[i].link_target = n.e.has_link ? n.e.link.c_str() : nullptr;
        out[i].file_index = n.e.kind == 1 && !mi_walk::has_prefix(mi_walk::base_of(n.e.relpath), ".wh.") ? n_regular++ : -1;   // a whiteout has no content
        out[i].size = n.e.size;
        out[i].mtime_sec = n.e.mtime;
        out[i].mode = n.e.mode;
        out[i].kind = n.e.kind;
        out[i].uid = n.e.uid;
        out[i].gid = n.e.gid;
        if (src_paths) src_paths[i] = n.src.c_str();
    }
    return MI_OK;
}

extern "C" void mi_copy_layer_free(mi_copy_layer* l) { delete l; }
