// mi_copyops.hip -- a COPY/ADD step, on the host (no device code here):
//   * the caller's side of the step: --chown (utils.ResolveChown), source patterns (filepath.Match / Glob as
//     addCopyStep.resolveFromPaths uses them), NewCopyOperation's checks;
//   * MemFS.AddLayerByCopyOps' addToLayer as PLAN + APPLY on mi_copy::Fs (mi_copyfs.h) -- used by the handle (mi_memfs.hip) and,
//     with a batch between the two steps, by the commit (mi_commit.hip);
//   * CopyOperation.Execute over fileio.Copier, and MemFS.Checkpoint, which copies with the same Copier.
// Every function cites the Go it restates.
#include "mi_copyfs.h"

#include <dirent.h>
#include <fcntl.h>
#include <grp.h>
#include <pwd.h>

#include <algorithm>

// isDirFormat / checkCopyParams / resolveDestination (lib/snapshot/copy_op.go:149-180)
static bool copy_dst_is_dir_format(const std::string& dst) {
    return (!dst.empty() && dst.back() == '/') || dst == "." || dst == "..";
}
static std::string copy_check_params(uint64_t n_srcs, const char* work_dir, const std::string& dst) {
    if (n_srcs == 0) return "srcs cannot be empty";
    if (n_srcs > 1 && !copy_dst_is_dir_format(dst)) return "tarring multiple sources, destination must end with \"/\"";
    if ((dst.empty() || dst[0] != '/') && !(work_dir && work_dir[0] == '/'))
        return "dst is not absolute path, must specify absolute working directory";
    return "";
}

// ---- the caller's side of a COPY/ADD step: --chown and the source patterns ------------------------------------------
//
// utils.ResolveChown (lib/utils/utils.go:186-228): "<user>[:<group>]", each a number (strconv.Atoi: an optional sign and
// decimal digits) or a name looked up in the user / group database; no group = the uid; more than one ':' is an error.
static bool go_atoi(const std::string& t, long long* v) {
    size_t i = 0;
    if (!t.empty() && (t[0] == '+' || t[0] == '-')) i = 1;
    if (i == t.size()) return false;
    long long x = 0;
    for (size_t k = i; k < t.size(); ++k) {
        if (t[k] < '0' || t[k] > '9') return false;
        const int d = t[k] - '0';
        if (x > (9223372036854775807LL - d) / 10) return false;                  // beyond int64: Atoi reports a range error
        x = x * 10 + d;
    }
    *v = t[0] == '-' ? -x : x;
    return true;
}
extern "C" int mi_resolve_chown(const char* chown, int preserve_owner, int64_t* uid, int64_t* gid, char* err,
                                uint64_t err_cap) {
    auto put_err = [&](const std::string& m) { if (err && err_cap) snprintf(err, (size_t)err_cap, "%s", m.c_str()); };
    if (!uid || !gid) return MI_ERR_INVALID;
    *uid = *gid = 0;
    const std::string c = chown ? chown : "";
    if (!c.empty() && preserve_owner) { put_err("both chown and archive are true"); return MI_ERR_INVALID; }   // copy_op.go:52-55
    if (c.empty()) return MI_OK;
    std::vector<std::string> split(1);
    for (char ch : c) { if (ch == ':') split.emplace_back(); else split.back() += ch; }
    if (split.size() > 2) { put_err("resolve chown str: failed to split on ':'"); return MI_ERR_INVALID; }
    long long u = 0, g = 0;
    if (!go_atoi(split[0], &u)) {
        struct passwd pw, *res = nullptr;
        std::vector<char> buf(1 << 16);
        if (split[0].empty() || getpwnam_r(split[0].c_str(), &pw, buf.data(), buf.size(), &res) != 0 || !res) {
            put_err("resolve chown str: failed to look up user '" + split[0] + "'");
            return MI_ERR_INVALID;
        }
        u = (long long)pw.pw_uid;
    }
    if (split.size() == 1) { *uid = *gid = u; return MI_OK; }
    if (!go_atoi(split[1], &g)) {
        struct group gr, *res = nullptr;
        std::vector<char> buf(1 << 16);
        if (split[1].empty() || getgrnam_r(split[1].c_str(), &gr, buf.data(), buf.size(), &res) != 0 || !res) {
            put_err("resolve chown str: failed to look up group '" + split[0] + "'");   // (the reference names the USER here, :221)
            return MI_ERR_INVALID;
        }
        g = (long long)gr.gr_gid;
    }
    *uid = u; *gid = g;
    return MI_OK;
}

// path/filepath.Match and Glob as the Go 1.14 toolchain the reference builds with defines them (Makefile:34) --
// resolveFromPaths (lib/builder/step/add_copy_step.go:171-185) runs every source of a COPY/ADD through Glob:
//   '*' any run of non-'/' characters, '?' one non-'/' character, '[' ['^'] ranges ']' a character class (not empty;
//   lo '-' hi; characters are runes), '\\' escapes the next character; the whole name has to match.  A malformed
//   pattern is ErrBadPattern -- but only where matching GETS to the bad part (1.14 stops at the end of the name).
namespace mi_glob {

static size_t rune_at(const std::string& s, size_t i, uint32_t* r) {           // utf8.DecodeRuneInString
    const unsigned char c = (unsigned char)s[i];
    auto cont = [&](size_t k) { return i + k < s.size() && ((unsigned char)s[i + k] & 0xC0) == 0x80; };
    if (c < 0x80) { *r = c; return 1; }
    if (c >= 0xC2 && c <= 0xDF && cont(1)) { *r = ((c & 0x1Fu) << 6) | ((unsigned char)s[i + 1] & 0x3Fu); return 2; }
    if (c >= 0xE0 && c <= 0xEF && cont(1) && cont(2)) {
        const uint32_t v = ((c & 0x0Fu) << 12) | (((unsigned char)s[i + 1] & 0x3Fu) << 6) | ((unsigned char)s[i + 2] & 0x3Fu);
        if (v >= 0x800 && !(v >= 0xD800 && v <= 0xDFFF)) { *r = v; return 3; }
    }
    if (c >= 0xF0 && c <= 0xF4 && cont(1) && cont(2) && cont(3)) {
        const uint32_t v = ((c & 0x07u) << 18) | (((unsigned char)s[i + 1] & 0x3Fu) << 12) |
                           (((unsigned char)s[i + 2] & 0x3Fu) << 6) | ((unsigned char)s[i + 3] & 0x3Fu);
        if (v >= 0x10000 && v <= 0x10FFFF) { *r = v; return 4; }
    }
    *r = 0xFFFD;                                                                // RuneError, width 1
    return 1;
}

// getEsc: one possibly escaped character of a class; false = ErrBadPattern
static bool get_esc(const std::string& chunk, size_t* at, uint32_t* r) {
    size_t i = *at;
    if (i >= chunk.size() || chunk[i] == '-' || chunk[i] == ']') return false;
    if (chunk[i] == '\\') { if (++i >= chunk.size()) return false; }
    const size_t n = rune_at(chunk, i, r);
    bool ok = !(*r == 0xFFFD && n == 1);
    i += n;
    if (i >= chunk.size()) ok = false;
    *at = i;
    return ok;
}

// matchChunk: does chunk (no '*') match a prefix of s[from:]?  rest = where the match ends
static bool match_chunk(const std::string& chunk, const std::string& s, size_t from, size_t* rest, bool* bad) {
    size_t c = 0, i = from;
    while (c < chunk.size()) {
        if (i >= s.size()) return false;
        switch (chunk[c]) {
            case '[': {
                uint32_t r;
                i += rune_at(s, i, &r);
                if (++c >= chunk.size()) { *bad = true; return false; }
                const bool negated = chunk[c] == '^';
                if (negated) ++c;
                bool match = false;
                for (int nrange = 0;; ++nrange) {
                    if (c < chunk.size() && chunk[c] == ']' && nrange > 0) { ++c; break; }
                    uint32_t lo, hi;
                    if (!get_esc(chunk, &c, &lo)) { *bad = true; return false; }
                    hi = lo;
                    if (chunk[c] == '-') {
                        ++c;
                        if (!get_esc(chunk, &c, &hi)) { *bad = true; return false; }
                    }
                    if (lo <= r && r <= hi) match = true;
                }
                if (match == negated) return false;
                break;
            }
            case '?': {
                if (s[i] == '/') return false;
                uint32_t r;
                i += rune_at(s, i, &r);
                ++c;
                break;
            }
            case '\\':
                if (++c >= chunk.size()) { *bad = true; return false; }
                /* fallthrough */
            default:
                if (chunk[c] != s[i]) return false;
                ++i; ++c;
        }
    }
    *rest = i;
    return true;
}

static bool match(const std::string& pattern, const std::string& name, bool* bad) {
    size_t p = 0, n = 0;
    *bad = false;
    while (p < pattern.size()) {
        bool star = false;                                                      // scanChunk
        while (p < pattern.size() && pattern[p] == '*') { ++p; star = true; }
        bool inrange = false;
        size_t e = p;
        for (; e < pattern.size(); ++e) {
            const char ch = pattern[e];
            if (ch == '\\') { if (e + 1 < pattern.size()) ++e; }
            else if (ch == '[') inrange = true;
            else if (ch == ']') inrange = false;
            else if (ch == '*' && !inrange) break;
        }
        const std::string chunk = pattern.substr(p, e - p);
        p = e;
        if (star && chunk.empty()) return name.find('/', n) == std::string::npos;   // a trailing * takes the rest
        size_t t = 0;
        const bool ok = match_chunk(chunk, name, n, &t, bad);
        if (ok && (t == name.size() || p < pattern.size())) { n = t; continue; }
        if (*bad) return false;
        if (star) {
            bool advanced = false;
            for (size_t i = n; i < name.size() && name[i] != '/'; ++i) {
                if (match_chunk(chunk, name, i + 1, &t, bad)) {
                    if (p >= pattern.size() && t < name.size()) continue;       // last chunk: the name has to end here
                    n = t;
                    advanced = true;
                    break;
                }
                if (*bad) return false;
            }
            if (advanced) continue;
        }
        return false;
    }
    return n == name.size();
}

static bool has_meta(const std::string& s) { return s.find_first_of("*?[\\") != std::string::npos; }

// glob(dir, pattern, matches): the names of dir that match, sorted, joined to dir; I/O errors are ignored
static bool glob_dir(const std::string& dir, const std::string& pattern, std::vector<std::string>* out) {
    struct stat st;
    if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return true;
    DIR* d = opendir(dir.c_str());
    if (!d) return true;
    std::vector<std::string> names;
    while (struct dirent* de = readdir(d)) {
        const std::string n = de->d_name;
        if (n != "." && n != "..") names.push_back(n);
    }
    closedir(d);
    std::sort(names.begin(), names.end());
    for (const std::string& n : names) {
        bool bad = false;
        if (match(pattern, n, &bad)) {
            std::string j = dir == "." ? n : (dir.back() == '/' ? dir + n : dir + "/" + n);   // filepath.Join(dir, n)
            out->push_back(dir == "." ? j : (dir[0] == '/' ? mi_walk::clean_rooted(j) : mi_walk::clean_any(j)));
        }
        if (bad) return false;
    }
    return true;
}

static bool glob(const std::string& pattern, std::vector<std::string>* out) {   // false = ErrBadPattern
    bool bad = false;
    match(pattern, "", &bad);
    if (bad) return false;
    if (!has_meta(pattern)) {
        struct stat st;
        if (lstat(pattern.c_str(), &st) == 0) out->push_back(pattern);
        return true;
    }
    const size_t cut = pattern.find_last_of('/');                               // filepath.Split
    std::string dir = cut == std::string::npos ? "" : pattern.substr(0, cut + 1);
    const std::string file = cut == std::string::npos ? pattern : pattern.substr(cut + 1);
    if (dir.empty()) dir = ".";                                                 // cleanGlobPath
    else if (dir != "/") dir.pop_back();
    if (!has_meta(dir)) return glob_dir(dir, file, out);
    if (dir == pattern) return false;                                           // "Prevent infinite recursion"
    std::vector<std::string> dirs;
    if (!glob(dir, &dirs)) return false;
    for (const std::string& d : dirs)
        if (!glob_dir(d, file, out)) return false;
    return true;
}

}  // namespace mi_glob

extern "C" int mi_path_match(const char* pattern, const char* name, int* matched) {
    if (!pattern || !name || !matched) return MI_ERR_INVALID;
    bool bad = false;
    *matched = mi_glob::match(pattern, name, &bad) ? 1 : 0;
    return bad ? MI_ERR_INVALID : MI_OK;                                        // ErrBadPattern
}

// resolveFromPaths: every source joined to the context root and globbed; no match (or a bad pattern) = the joined
// path itself.  out = the resolved paths, NUL-terminated, back to back.
extern "C" int mi_context_sources(const char* context_root, const char* const* from_paths, uint64_t n_paths,
                                  char* out, uint64_t cap, uint64_t* n_out, uint64_t* bytes_out) {
    if (!context_root || (n_paths && !from_paths) || !n_out || !bytes_out || (cap && !out)) return MI_ERR_INVALID;
    std::string all;
    uint64_t n = 0;
    for (uint64_t i = 0; i < n_paths; ++i) {
        const std::string joined0 = std::string(context_root) + "/" + (from_paths[i] ? from_paths[i] : "");
        const std::string source = joined0[0] == '/' ? mi_walk::clean_rooted(joined0) : mi_walk::clean_any(joined0);
        std::vector<std::string> m;
        if (!mi_glob::glob(source, &m) || m.empty()) m.assign(1, source);
        for (const std::string& x : m) { all += x; all.push_back('\0'); ++n; }
    }
    *n_out = n;
    *bytes_out = all.size();
    if (cap < all.size()) return MI_ERR_CAPACITY;
    if (!all.empty()) memcpy(out, all.data(), all.size());
    return MI_OK;
}

extern "C" int mi_copy_op_resolve(uint64_t n_srcs, const char* work_dir, const char* dst, char* dst_out,
                                  uint64_t cap, char* err, uint64_t err_cap) {
    if (!dst || !dst_out) return MI_ERR_INVALID;
    const std::string d = dst;
    const std::string bad = copy_check_params(n_srcs, work_dir, d);
    if (!bad.empty()) {
        if (err && err_cap) snprintf(err, (size_t)err_cap, "check copy param: %s", bad.c_str());
        return MI_ERR_INVALID;
    }
    std::string r = d;
    if (d[0] != '/') {                                      // filepath.Join cleans; the trailing "/" is put back (the reference
                                                            // appends it even to a joined "/", giving "//": the same path once cleaned)
        r = mi_walk::abs_path(std::string(work_dir) + "/" + d);
        if (copy_dst_is_dir_format(d) && r.back() != '/') r += "/";
    }
    if (cap < r.size() + 1) return MI_ERR_CAPACITY;
    memcpy(dst_out, r.c_str(), r.size() + 1);
    return MI_OK;
}

// addToLayer (mem_fs.go:343-421) for each op, against fs.t, into fs.layer; fs.rc / fs.err carry what maybeAddToLayer
// refuses, *err_out everything else.
// In two steps.  PLAN: what the ops read from the DISK -- the parameter check, the stat of a single source, evalSymlinks,
// the walk of every source -- for all ops, in order, stopping at the first failure.  None of it depends on the tree, so
// it can run ahead; with a batch attached the walks stage every regular file on the GPU while they list it (an entry's
// file_index = its row).  APPLY: the ops against the tree, in order, each failure raised where the interleaved loop of the
// reference raises it (an op-2 source that does not exist fails after op 1 has been applied, not before).  Between the
// two, a content-aware commit runs the batch: the apply step then sees a chunk root for every regular file.
void copy_ops_plan(const mi_copy::Fs& fs, const mi_copy_op* ops, uint64_t n_ops, mi_batch* batch, CopyPlan* plan) {
    auto stop = [&](int rc, const std::string& m, bool before_dst) { plan->err_rc = rc; plan->err = m; plan->err_before_dst = before_dst; };
    for (uint64_t k = 0; k < n_ops; ++k) {
        const mi_copy_op& c = ops[k];
        plan->ops.emplace_back();
        CopyOpPlan& op = plan->ops.back();
        if (!c.src_root || !c.dst || (c.n_srcs && !c.srcs)) return stop(MI_ERR_INVALID, "", true);
        {   // what NewCopyOperation refuses (copy_op.go:48-50): the dst here is the resolved one, so it is absolute
            const std::string bad = copy_check_params(c.n_srcs, nullptr, c.dst);
            if (!bad.empty()) return stop(MI_ERR_INVALID, "check copy param: " + bad, true);
        }
        op.src_root = mi_walk::abs_path(c.src_root);
        op.dst = c.dst;
        if (c.n_srcs == 1) {
            struct stat st;
            const std::string s0 = op.src_root + mi_walk::abs_path(c.srcs[0] ? c.srcs[0] : "");
            if (stat(s0.c_str(), &st) != 0) return stop(MI_ERR_IO, "stat src " + s0 + ": " + strerror(errno), true);
            if (!S_ISDIR(st.st_mode)) op.create_dst = false;          // case 1: file onto file
        }
        for (uint64_t si = 0; si < c.n_srcs; ++si) {
            std::string rel, e2;
            if (!mi_copy::eval_symlinks(mi_walk::abs_path(c.srcs[si] ? c.srcs[si] : ""), op.src_root, &rel, &e2))
                return stop(MI_ERR_IO, "eval symlinks for " + std::string(c.srcs[si] ? c.srcs[si] : "") + ": " + e2, false);
            CopySrcPlan sp;
            sp.src = op.src_root == "/" ? rel : op.src_root + (rel == "/" ? "" : rel);
            std::string werr;                                           // shouldSkip with a nil blacklist; createHeader
            const int wrc = batch ? mi_walk::scan_walk_collect_batch(sp.src, fs.root, &sp.walked, &werr, batch)   // trims link targets
                                  : mi_walk::scan_walk_collect(sp.src, fs.root, &sp.walked, &werr);               // by the MEMFS root
            if (wrc) return stop(wrc, "copy src " + sp.src + ": " + werr, false);
            plan->n_walked += sp.walked.entries.size();
            op.srcs.push_back(std::move(sp));
        }
    }
}
// roots: 32 bytes per batch row (NULL: the reference's metadata-only isUpdated)
int copy_ops_apply(mi_copy::Fs& fs, const mi_copy_op* ops, const CopyPlan& plan, const uint8_t* roots, std::string* err_out) {
    auto put_err = [&](const std::string& m) { *err_out = m; };
    for (size_t k = 0; k < plan.ops.size() && !fs.rc; ++k) {
        const CopyOpPlan& op = plan.ops[k];
        const mi_copy_op& c = ops[k];
        const bool last = k + 1 == plan.ops.size();
        if (last && plan.err_rc && plan.err_before_dst) { put_err(plan.err); return plan.err_rc; }
        std::string dst = op.dst;
        if (op.create_dst) {
            std::string resolved = fs.add_ancestors(mi_walk::abs_path(dst), true, c.uid, c.gid);
            if (fs.rc) break;
            if (resolved.empty() || resolved.back() != '/') resolved += "/";
            dst = resolved;
        }
        const bool dst_is_dir = !dst.empty() && dst.back() == '/';
        for (size_t si = 0; si < op.srcs.size() && !fs.rc; ++si) {
            const std::string& src = op.srcs[si].src;
            for (const mi_walk::Entry& we : op.srcs[si].walked.entries) {
                const bool is_src = we.relpath == ".";
                std::string curr_dst;
                if (is_src) {
                    if (we.kind == 0) continue;                         // the directory itself: contents only
                    curr_dst = !dst_is_dir ? dst : mi_walk::clean_rooted(dst + "/" + mi_walk::base_of(src));
                } else {
                    curr_dst = mi_walk::clean_rooted(dst + "/" + we.relpath);
                }
                curr_dst = mi_walk::abs_path(curr_dst);
                mi_copy::Node n;
                n.e = we;
                n.e.relpath = curr_dst == "/" ? "" : curr_dst.substr(1);
                n.e.uid = c.uid;
                n.e.gid = c.gid;
                n.e.file_index = -1;
                if (roots && we.kind == 1 && we.file_index >= 0) {
                    n.batch_file = we.file_index;
                    n.batch_gen = fs.commit_gen;
                    n.has_root = true;
                    memcpy(n.root, roots + (uint64_t)we.file_index * 32, 32);
                } else if (fs.job && we.kind == 1 && we.file_index >= 0) {     // (a pipelined commit: the scan may still be running)
                    n.batch_file = we.file_index;
                    n.batch_gen = fs.commit_gen;
                    n.has_root = true;
                    n.root_pending = true;
                }
                const std::string curr_src = is_src ? src : src + "/" + we.relpath;
                fs.maybe_add(curr_src, curr_dst, n);
                if (fs.rc) break;
            }
        }
        if (!fs.rc && last && plan.err_rc) { put_err(plan.err); return plan.err_rc; }
    }
    if (fs.rc) { put_err(fs.err); return fs.rc; }
    return MI_OK;
}
int copy_ops_into(mi_copy::Fs& fs, const mi_copy_op* ops, uint64_t n_ops, std::string* err_out) {
    CopyPlan plan;
    copy_ops_plan(fs, ops, n_ops, nullptr, &plan);
    return copy_ops_apply(fs, ops, plan, nullptr, err_out);
}

// ---- CopyOperation.Execute: the on-disk copy of a COPY/ADD step with --modifyfs (lib/snapshot/copy_op.go:83-147) over
// fileio.Copier (lib/fileio/copy.go:31-394).  Owners: --chown -> the op's uid/gid for the destination directory if it
// has to be created and, always, for everything copied; from the context without --chown -> the same with 0:0; --from
// --archive -> a created destination directory gets the source's owner, everything copied keeps its own; --from alone ->
// owners as they are (a created destination directory: root).  Permission bits travel with the files; mtimes do not.
namespace mi_copyexec {

struct Owner { bool set = false; uint32_t uid = 0, gid = 0; bool overwrite = false; };
struct Copier {
    std::vector<std::string> blacklist;
    Owner dst_dir, children;
    std::string err;

    bool fail(const std::string& m) { err = m; return false; }
    bool blacklisted(const std::string& p) const { return mi_walk::is_descendant_of_any(p, blacklist); }

    bool mkdir_all(const std::string& dst) {                                     // Copier.mkdirAll (:336-393)
        if (dst.empty()) return fail("empty dst directory");
        const std::string abs = mi_walk::abs_path(dst);                          // callers pass absolute paths
        std::string cur;
        const std::vector<std::string> ps = mi_memtree::Tree::parts(abs);
        for (size_t k = 0; k + 1 < ps.size(); ++k) {
            cur += "/" + ps[k];
            struct stat st;
            if (lstat(cur.c_str(), &st) == 0) continue;
            if (errno != ENOENT) return fail("stat " + cur + ": " + strerror(errno));
            if (mkdir(cur.c_str(), 0755) != 0) return fail("mkdir " + cur + " with default mode 0755: " + strerror(errno));
            if (chown(cur.c_str(), 0, 0) != 0) return fail("chown " + cur + " with default owner (0:0): " + strerror(errno));
        }
        struct stat st;
        if (lstat(abs.c_str(), &st) != 0) {
            if (errno != ENOENT) return fail("stat " + abs + ": " + strerror(errno));
            if (mkdir(abs.c_str(), 0755) != 0) return fail("mkdir " + abs + " with default mode 0755: " + strerror(errno));
            const uint32_t u = dst_dir.set ? dst_dir.uid : 0, g = dst_dir.set ? dst_dir.gid : 0;
            if (chown(abs.c_str(), u, g) != 0) return fail("chown " + abs + ": " + strerror(errno));
        } else if (dst_dir.set && dst_dir.overwrite) {
            if (chown(abs.c_str(), dst_dir.uid, dst_dir.gid) != 0) return fail("chown " + abs + ": " + strerror(errno));
        }
        return true;
    }
    bool copy_symlink(const std::string& src, const std::string& dst) {          // :232-247
        struct stat st;
        if (lstat(dst.c_str(), &st) == 0 && remove(dst.c_str()) != 0)
            return fail("remove existing file " + dst + ": " + strerror(errno));
        std::vector<char> buf(4096);
        const ssize_t n = readlink(src.c_str(), buf.data(), buf.size() - 1);
        if (n < 0) return fail("read link " + src + ": " + strerror(errno));
        const std::string target(buf.data(), (size_t)n);
        if (symlink(target.c_str(), dst.c_str()) != 0)
            return fail("write link " + dst + " with content " + target + ": " + strerror(errno));
        return true;
    }
    bool copy_file(const std::string& src, const std::string& dst) {             // copyFile + copyRegularFile (:160-230)
        struct stat fi;
        if (lstat(src.c_str(), &fi) != 0) return fail("lstat " + src + ": " + strerror(errno));
        // (a blacklisted SOURCE FILE is only logged here -- the reference's else-if chain goes on to copy it; blacklisted
        // entries below a copied directory never get this far.  The same chain would also skip the special-file test for
        // it and open a blacklisted FIFO for reading; that one corner is not followed: a special file is never opened)
        if (!S_ISREG(fi.st_mode) && !S_ISDIR(fi.st_mode) && !S_ISLNK(fi.st_mode)) return true;
        if (S_ISLNK(fi.st_mode)) return copy_symlink(src, dst);                  // never chown'ed: that would hit the target
        struct stat dt;
        if (lstat(dst.c_str(), &dt) == 0) {
            if (chmod(dst.c_str(), 0777) != 0) return fail("chmod " + dst + ": " + strerror(errno));
        } else if (errno != ENOENT) {
            return fail("lstat " + dst + ": " + strerror(errno));
        }
        const int r = open(src.c_str(), O_RDONLY | O_CLOEXEC);
        if (r < 0) return fail("open " + dst + ": " + strerror(errno));
        const int w = open(dst.c_str(), O_WRONLY | O_CREAT | O_CLOEXEC, 0777);
        if (w < 0) { const int e = errno; close(r); return fail("create " + dst + ": " + strerror(e)); }
        bool ok = ftruncate(w, 0) == 0;
        std::string e = ok ? "" : std::string("truncate ") + dst + ": " + strerror(errno);
        std::vector<char> buf(1 << 20);
        while (ok) {
            const ssize_t n = read(r, buf.data(), buf.size());
            if (n < 0 && errno == EINTR) continue;
            if (n < 0) { ok = false; e = "copy " + src + " to " + dst + ": " + strerror(errno); break; }
            if (n == 0) break;
            for (ssize_t done = 0; done < n;) {
                const ssize_t k = write(w, buf.data() + done, (size_t)(n - done));
                if (k < 0 && errno == EINTR) continue;
                if (k < 0) { ok = false; e = "copy " + src + " to " + dst + ": " + strerror(errno); break; }
                done += k;
            }
        }
        close(r);
        close(w);
        if (!ok) return fail(e);
        const uint32_t u = children.set && children.overwrite ? children.uid : fi.st_uid;
        const uint32_t g = children.set && children.overwrite ? children.gid : fi.st_gid;
        if (chown(dst.c_str(), u, g) != 0) return fail("chown " + dst + ": " + strerror(errno));
        if (chmod(dst.c_str(), fi.st_mode & 07777) != 0) return fail("chmod " + dst + ": " + strerror(errno));   // after chown
        return true;
    }
    bool copy_dir(const std::string& src, const std::string& dst) {              // copyDir (:289-330): one directory, no contents
        struct stat si;
        if (lstat(src.c_str(), &si) != 0) return fail("lstat " + src + ": " + strerror(errno));
        if (!S_ISDIR(si.st_mode)) return fail("source " + src + " is not a directory");
        if (blacklisted(src)) return true;
        struct stat di;
        if (lstat(dst.c_str(), &di) != 0) {
            if (errno != ENOENT) return fail("lstat " + dst + ": " + strerror(errno));
            if (mkdir(dst.c_str(), si.st_mode & 07777) != 0) return fail("mkdir " + dst + ": " + strerror(errno));
        } else if (!S_ISDIR(di.st_mode)) {
            return fail("dst is not a directory");
        }
        if (chmod(dst.c_str(), si.st_mode & 07777) != 0) return fail("chmod " + dst + ": " + strerror(errno));
        const uint32_t u = children.set && children.overwrite ? children.uid : si.st_uid;
        const uint32_t g = children.set && children.overwrite ? children.gid : si.st_gid;
        if (chown(dst.c_str(), u, g) != 0) return fail("chown " + dst + ": " + strerror(errno));
        return true;
    }
    bool copy_dir_contents(const std::string& src, const std::string& dst, const std::string& orig_dst) {   // :252-285
        DIR* d = opendir(src.c_str());
        if (!d) return fail("read dir " + src + ": " + strerror(errno));
        std::vector<std::string> names;
        while (struct dirent* de = readdir(d)) {
            const std::string n = de->d_name;
            if (n != "." && n != "..") names.push_back(n);
        }
        closedir(d);
        std::sort(names.begin(), names.end());                                   // ioutil.ReadDir sorts by name
        for (const std::string& n : names) {
            const std::string cs = (src == "/" ? "" : src) + "/" + n, cd = (dst == "/" ? "" : dst) + "/" + n;
            if (blacklisted(cs) || cs == orig_dst) continue;                     // "Silently break infinite loop"
            struct stat st;
            if (lstat(cs.c_str(), &st) != 0) return fail("lstat " + cs + ": " + strerror(errno));
            if (S_ISDIR(st.st_mode)) {
                if (!copy_dir(cs, cd)) return fail("copy dir " + cs + " to " + cd + ": " + err);
                if (!copy_dir_contents(cs, cd, orig_dst)) return fail("copy dir contents " + cs + " to " + cd + ": " + err);
            } else if (!copy_file(cs, cd)) {
                return fail("copy file " + cs + " to " + cd + ": " + err);
            }
        }
        return true;
    }
    bool CopyFile(const std::string& src, const std::string& dst) {              // :122-130
        const std::string dir = mi_walk::dir_of(dst);
        if (!mkdir_all(dir)) return fail("mkdir all " + dir + ": " + err);
        return copy_file(src, dst);
    }
    bool CopyDir(const std::string& src, const std::string& dst) {               // :142-156
        if (blacklisted(src)) return true;
        if (!mkdir_all(dst)) return fail("mkdir all " + dst + ": " + err);
        return copy_dir_contents(src, dst, mi_walk::abs_path(dst));
    }
};

}  // namespace mi_copyexec

extern "C" int mi_copy_op_execute(const mi_copy_op* op, uint32_t flags, const char* const* blacklist, uint64_t n_blacklist,
                                  char* err, uint64_t err_cap) {
    auto put_err = [&](const std::string& m) { if (err && err_cap) snprintf(err, (size_t)err_cap, "%s", m.c_str()); };
    if (!op || !op->src_root || !op->dst || (op->n_srcs && !op->srcs) || (n_blacklist && !blacklist)) return MI_ERR_INVALID;
    const bool chown_given = flags & MI_COPY_CHOWN, internal = flags & MI_COPY_INTERNAL, archive = flags & MI_COPY_PRESERVE_OWNER;
    if (chown_given && archive) { put_err("both chown and archive are true"); return MI_ERR_INVALID; }
    const std::string src_root = mi_walk::abs_path(op->src_root);
    const std::string dst = op->dst;
    for (uint64_t si = 0; si < op->n_srcs; ++si) {
        std::string rel, e2;
        const std::string given = op->srcs[si] ? op->srcs[si] : "";
        if (!mi_copy::eval_symlinks(mi_walk::abs_path(given), src_root, &rel, &e2)) {
            put_err("eval symlinks for " + given + ": " + e2);
            return MI_ERR_IO;
        }
        const std::string src = src_root == "/" ? rel : src_root + (rel == "/" ? "" : rel);
        struct stat fi;
        if (lstat(src.c_str(), &fi) != 0) { put_err("lstat " + src + ": " + strerror(errno)); return MI_ERR_IO; }
        mi_copyexec::Copier c;
        if (!internal)                                                           // "there is no need to blacklist any path" for a
            for (uint64_t k = 0; k < n_blacklist; ++k) c.blacklist.push_back(blacklist[k] ? blacklist[k] : "");   // checkpointed stage
        if (chown_given) {
            c.dst_dir = {true, op->uid, op->gid, false};
            c.children = {true, op->uid, op->gid, true};
        } else if (!internal) {
            c.dst_dir = {true, 0, 0, false};
            c.children = {true, 0, 0, true};
        } else if (archive) {
            c.dst_dir = {true, fi.st_uid, fi.st_gid, false};
        }
        bool ok;
        std::string what;
        if (S_ISDIR(fi.st_mode)) {
            ok = c.CopyDir(src, dst);
            what = "copy dir " + src + " to dir " + dst;
        } else if (copy_dst_is_dir_format(dst)) {
            const std::string target = mi_walk::abs_path(dst + "/" + mi_walk::base_of(src));
            ok = c.CopyFile(src, target);
            what = "copy file " + src + " to dir " + target;
        } else {
            ok = c.CopyFile(src, dst);
            what = "copy file " + src + " to file " + dst;
        }
        if (!ok) { put_err(what + ": " + c.err); return MI_ERR_IO; }
    }
    return MI_OK;
}

// MemFS.Checkpoint (:132-185): the sources a later stage will COPY --from are moved aside, below new_root, with the
// layout they have below the root; a pattern is expanded like a COPY source, a directory's created target gets the
// source's owner, everything copied keeps its own
extern "C" int mi_memfs_checkpoint(mi_memfs* m, const char* new_root, const char* const* sources, uint64_t n_sources) {
    if (!m || !new_root || (n_sources && !sources)) return MI_ERR_INVALID;
    const std::string root = m->fs.root;
    for (uint64_t i = 0; i < n_sources; ++i) {
        const std::string given = sources[i] ? sources[i] : "";
        std::vector<std::string> matches;
        if (!mi_glob::glob(given, &matches) || matches.empty()) matches.assign(1, given);
        for (std::string src : matches) {
            if (src.empty() || src[0] != '/') src = mi_walk::abs_path(root + "/" + src);
            if (!mi_walk::has_prefix(src, root)) {
                m->err = "trim src " + src + ": failed to trim root prefix " + root + " from path " + src;
                return MI_ERR_INVALID;
            }
            const std::string dst = mi_walk::abs_path(std::string(new_root) + "/" + src.substr(root.size()));
            struct stat followed, fi;
            if (stat(src.c_str(), &followed) != 0) { m->err = "stat " + src + ": " + strerror(errno); return MI_ERR_IO; }
            if (lstat(src.c_str(), &fi) != 0) { m->err = "lstat " + src + ": " + strerror(errno); return MI_ERR_IO; }
            mi_copyexec::Copier c;
            c.blacklist = m->blacklist;
            c.dst_dir = {true, fi.st_uid, fi.st_gid, false};
            if (S_ISDIR(followed.st_mode)) {
                if (!c.CopyDir(src, dst)) { m->err = "copy dir " + src + ": " + c.err; return MI_ERR_IO; }
            } else if (!c.CopyFile(src, dst)) {
                m->err = "copy file " + src + ": " + c.err;
                return MI_ERR_IO;
            }
        }
    }
    return MI_OK;
}
