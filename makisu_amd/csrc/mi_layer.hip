// mi_layer.hip -- the layer writer: tar framing + the two serial layer digests, behind the C ABI.
// Host code only (no kernels): the opt-in device deflate leg is mi_deflate.hip's, driven through mi_local.h's mi_deflater_*.
//
// What it restates (reference = uber/makisu):
//   step.tarAndGzipDiffs        lib/builder/step/common.go:35-63   tar.Writer -> tee -> {tarDigester,
//                               gzip -> tee -> {file, gzipDigester}}
//   step.commitLayer            common.go:67-111                   the DigestPair it returns
//   memLayer.createHeader       lib/snapshot/mem_layer.go:152-190  Name = RelPath(dst), Uname/Gname "",
//                               directories get a trailing "/", symlinks carry their target
//   whiteoutMemFile.commit      mem_layer.go:127-132               header-only entry {Name: ".wh.<x>"}
//   tario.WriteEntry/WriteHeader lib/tario/write.go:28-68          leading "/" stripped, mtime truncated
//                               to seconds, then exactly h.Size bytes (io.CopyN) for regular files;
//                               dirs / links / symlinks header-only; anything else "unsupported type"
//   stream.ConcurrentMultiWriter lib/stream/multi_writer.go:35-66  every sink gets every block, sinks
//                               run concurrently, a block is handed on only when all took the last
//   tario.NewGzipWriter         lib/tario/gzip.go:26-48            level no / speed / size / default
// The header bytes themselves are Go's archive/tar (not under /root/reference): Writer.WriteHeader
// with Format unknown -> USTAR when every field fits (names up to 100 bytes or prefix/name split at a
// "/", octal numbers), else PAX (an "x" record file "PaxHeaders.0/<name>" with path / linkpath / uid /
// gid / size / mtime records, then the same header with what fits).  Restated from the Go 1.14
// sources.  PINNED since round 3 for the USTAR path: the Go-written layer tar among the reference's
// fixtures (testdata/files/busybox/393ccd5c.../layer.tar: 390 headers -- files, directories, hard
// links --, 1 308 672 bytes, SHA-256 4ac76077...) is reproduced byte for byte, header by header and
// as a whole stream (tests/test_host_layer.py, with MI_LAYER_MODE_WITH_TYPE: that tar's Mode fields
// carry the pre-Go-1.9 file-type bits).  Also pinned: the empty layer's digest (1024 zero bytes,
// lib/docker/image/const_darwin.go:18), read-back by python tarfile and GNU tar, agreement with the
// oracle's independent ustar header.  STILL UNPINNED (no Go toolchain, no Go-written sample): the
// PAX path (names over 100 bytes that do not split, non-ASCII names, ids over 2^21, sizes from 8 GiB).
// The gzip bytes are zlib's (the reference uses klauspost/pgzip, whose block splitting is its own):
// the gzip digest is a faithful DigestPair member for THIS writer, not comparable across writers.
#include "../../include/makisu_mi.h"
#include "host_sha256.h"
#include "host_blake2s.h"
#include "mi_local.h"             // mi_batch_file_size, mi_last_error_of_batch
#include "mi_filesum.h"           // the check of bytes that come back from HBM against the sums taken where they were read

#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <sched.h>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

typedef std::vector<uint8_t> Bytes;
typedef std::shared_ptr<const Bytes> Block;
const size_t kBlockBytes = 1u << 20;

// ---- one sink of the tee: its own thread, blocks in order ---------------------------------
class Sink {
public:
    virtual ~Sink() {}
    void start() { th_ = std::thread([this] { run(); }); }
    double idle_s = 0, full_s = 0;                 // MI_LAYER_TIMING: the sink waited for a block / the framer waited for the sink
    static constexpr size_t kDepth = 8;            // blocks a sink may be behind: one window of a batch's bytes (8 MiB) fits
    void push(const Block& b) {                    // blocks while the sink is kDepth blocks behind
        std::unique_lock<std::mutex> lk(mu_);
        if (q_.size() >= kDepth) {
            const auto t0 = std::chrono::steady_clock::now();
            cv_.wait(lk, [&] { return q_.size() < kDepth; });
            full_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        q_.push_back(b);
        cv_.notify_all();
    }
    void close() {
        {
            std::lock_guard<std::mutex> g(mu_);
            closed_ = true;
        }
        cv_.notify_all();
        if (th_.joinable()) th_.join();
    }
    std::string error() {                          // the sink thread may be setting it right now
        std::lock_guard<std::mutex> g(mu_);
        return err;
    }

protected:
    std::string err;                               // written by the sink thread only (under mu_)
    void set_error(const std::string& m) {
        std::lock_guard<std::mutex> g(mu_);
        if (err.empty()) err = m;
    }
    bool failed() {
        std::lock_guard<std::mutex> g(mu_);
        return !err.empty();
    }
    virtual void consume(const Block& b) = 0;
    virtual void finish() = 0;

private:
    void run() {
        for (;;) {
            Block b;
            {
                std::unique_lock<std::mutex> lk(mu_);
                if (!closed_ && q_.empty()) {
                    const auto t0 = std::chrono::steady_clock::now();
                    cv_.wait(lk, [&] { return closed_ || !q_.empty(); });
                    idle_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                }
                if (q_.empty()) break;
                b = q_.front();
            }
            if (!failed()) consume(b);
            {
                std::lock_guard<std::mutex> g(mu_);
                q_.pop_front();
            }
            cv_.notify_all();
        }
        if (!failed()) finish();
    }
    std::thread th_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Block> q_;
    bool closed_ = false;
};

bool write_all(int fd, const uint8_t* p, size_t n, std::string* err) {
    while (n) {
        const ssize_t w = write(fd, p, n);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) { *err = std::string("write layer blob: ") + strerror(errno); return false; }
        p += w;
        n -= (size_t)w;
    }
    return true;
}

class DigestSink : public Sink {                   // tarDigester (common.go:45)
public:
    uint8_t digest[32];
    uint64_t bytes = 0;
    int raw_fd = -1;                               // without a gzip leg the tar itself is the blob
protected:
    void consume(const Block& b) override {
        const uint8_t* p = b->data();
        const size_t n = b->size();
        sha_.update(p, n);
        bytes += n;
        std::string e;
        if (raw_fd >= 0 && !write_all(raw_fd, p, n, &e)) set_error(e);
    }
    void finish() override { sha_.final(digest); }
private:
    mi_host::Sha256 sha_;
};

// gzipper -> {tempGzipTar, gzipDigester} (common.go:44-52).  The reference compresses with pgzip
// (lib/tario/gzip.go:31-47): blocks deflated in parallel, one gzip member.  Same construction here
// (what pigz does): every 1 MiB block of the tar is deflated on its own by a pool thread as a raw
// stream closed with a sync flush -- it ends on a byte boundary and needs no dictionary --, the sink
// thread writes the pieces in order, then an empty final block and the trailer (CRC-32 of the blocks
// combined, length mod 2^32).  The bytes are this writer's (pgzip's differ: its own block size and
// deflate), so the gzip digest is valid for blobs written here -- as DESIGN.md says.
class GzipSink : public Sink {
public:
    uint8_t digest[32];
    uint64_t bytes = 0;
    int out_fd = -1;
    bool init(int level) {
        level_ = level;
        return true;
    }
    int level() const { return level_; }
    // the device leg (mi_layer_set_gzip_ctx, before the first block): the pool below is then never started
    void set_device(mi_ctx* ctx) { dev_ctx_ = ctx; }
    ~GzipSink() override { stop_pool(); if (dev_) mi_deflater_free(dev_); }
protected:
    // on the sink thread, at the first block (or at finish, for the header alone): the pool and the header -- or the device coder
    bool begin_leg() {
        if (begun_) return !failed();
        begun_ = true;
        if (dev_ctx_) {
            if (mi_deflater_create(dev_ctx_, mi_deflate_device_window(), &dev_) != MI_OK) { set_error("device gzip leg: no coder on the ctx's device"); return false; }
        } else {
            unsigned n = 0;
            if (const char* e = getenv("MI_GZIP_THREADS")) n = (unsigned)atoi(e);
            if (n == 0) {
                cpu_set_t set;
                n = sched_getaffinity(0, sizeof set, &set) == 0 ? (unsigned)CPU_COUNT(&set) : 1u;
                if (n > 16) n = 16;
            }
            if (n < 1) n = 1;
            if (n > 64) n = 64;
            window_ = 2 * n;
            for (unsigned i = 0; i < n; ++i) pool_.emplace_back([this] { work(); });
        }
        // gzip header as compress/gzip writes it: no name, no mtime, XFL by level, OS "unknown".  The device leg has ONE level,
        // whatever was asked for: XFL = 4
        const uint8_t hdr[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0,
                                 (uint8_t)(dev_ctx_ ? 4 : level_ == 9 ? 2 : level_ == 1 ? 4 : 0), 255};
        emit(hdr, sizeof hdr);
        return !failed();
    }
    static int device_emit(void* arg, const uint8_t* bytes, uint64_t n_out, uint32_t crc, uint64_t n_in) {
        GzipSink* g = (GzipSink*)arg;
        g->emit(bytes, (size_t)n_out);
        g->crc_ = g->total_in_ ? (uint32_t)crc32_combine(g->crc_, crc, (z_off_t)n_in) : crc;
        g->total_in_ += n_in;
        return g->failed() ? MI_ERR_IO : MI_OK;
    }
    void device_error(int rc) {                                     // never a fall-back to zlib inside a layer that has begun
        if (failed()) return;
        const char* m = mi_deflater_error(dev_);
        char buf[500];
        snprintf(buf, sizeof buf, "device gzip leg: %s (%d)", m && *m ? m : "no memory for a window", rc);
        set_error(buf);
    }
    bool device_push() {
        const int rc = mi_deflater_push(dev_, dev_fill_, device_emit, this);
        dev_fill_ = 0;
        if (rc) device_error(rc);
        return rc == MI_OK;
    }
    void device_consume(const Block& b) {                           // whole windows of the stream, whatever the blocks' sizes
        const uint8_t* p = b->data();
        size_t n = b->size();
        const uint64_t window = mi_deflater_window(dev_);
        while (n) {
            uint8_t* room = mi_deflater_room(dev_);
            if (!room) { device_error(MI_ERR_NOMEM); return; }
            const size_t take = (size_t)std::min<uint64_t>(n, window - dev_fill_);
            memcpy(room + dev_fill_, p, take);
            dev_fill_ += take; p += take; n -= take;
            if (dev_fill_ == window && !device_push()) return;
        }
    }
    void consume(const Block& b) override {
        if (b->empty()) return;
        if (!begin_leg()) return;
        if (dev_) { device_consume(b); return; }
        auto j = std::make_shared<Job>();
        j->in = b;
        {
            std::lock_guard<std::mutex> g(pm_);
            todo_.push_back(j);
        }
        pcv_.notify_one();
        inflight_.push_back(j);
        while (inflight_.size() >= window_) drain_one();
    }
    void finish() override {
        if (!begin_leg()) return;
        if (dev_) {
            if (dev_fill_ && !device_push()) return;
            const int rc = mi_deflater_flush(dev_, device_emit, this);
            if (rc) device_error(rc);
        }
        while (!inflight_.empty()) drain_one();
        stop_pool();
        if (failed()) return;
        const uint8_t last[2] = {0x03, 0x00};                     // empty final deflate block
        emit(last, 2);
        uint8_t tr[8];
        for (int i = 0; i < 4; ++i) { tr[i] = (uint8_t)(crc_ >> (8 * i)); tr[4 + i] = (uint8_t)(total_in_ >> (8 * i)); }
        emit(tr, 8);
        sha_.final(digest);
    }
private:
    struct Job {
        Block in;
        Bytes out;
        uint32_t crc = 0;
        bool ok = true, done = false;                             // guarded by pm_, announced on dcv_
    };
    void emit(const uint8_t* p, size_t n) {
        sha_.update(p, n);
        bytes += n;
        std::string e;
        if (out_fd >= 0 && !write_all(out_fd, p, n, &e)) set_error(e);
    }
    void drain_one() {
        std::shared_ptr<Job> j = inflight_.front();
        inflight_.pop_front();
        {
            std::unique_lock<std::mutex> lk(pm_);
            dcv_.wait(lk, [&] { return j->done; });
        }
        if (!j->ok) { set_error("deflate failed"); return; }
        if (failed()) return;
        emit(j->out.data(), j->out.size());
        crc_ = total_in_ ? (uint32_t)crc32_combine(crc_, j->crc, (z_off_t)j->in->size()) : j->crc;
        total_in_ += j->in->size();
    }
    void work() {
        z_stream z;
        memset(&z, 0, sizeof z);
        bool ready = deflateInit2(&z, level_, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK;
        // the probe of incompressible(): a second, fastest-level stream.  Not at level "no" (everything is stored anyway) and not
        // with MI_GZIP_PROBE=0 (A/B runs)
        z_stream zp;
        memset(&zp, 0, sizeof zp);
        bool probe_ready = level_ != 0 && probe_enabled() && deflateInit2(&zp, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK;
        for (;;) {
            std::shared_ptr<Job> j;
            {
                std::unique_lock<std::mutex> lk(pm_);
                pcv_.wait(lk, [&] { return stop_ || !todo_.empty(); });
                if (todo_.empty()) break;
                j = todo_.front();
                todo_.pop_front();
            }
            bool ok = ready;
            if (ok && probe_ready && incompressible(&zp, j->in->data(), j->in->size())) {
                store(j->in->data(), j->in->size(), &j->out);
                j->crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), j->in->data(), (uInt)j->in->size());
            } else if (ok) {
                deflateReset(&z);
                j->out.resize(deflateBound(&z, (uLong)j->in->size()) + 16);
                z.next_in = (Bytef*)j->in->data();
                z.avail_in = (uInt)j->in->size();
                z.next_out = j->out.data();
                z.avail_out = (uInt)j->out.size();
                const int rc = deflate(&z, Z_SYNC_FLUSH);         // whole block in one call: the bound holds
                ok = rc == Z_OK && z.avail_in == 0 && z.avail_out != 0;
                j->out.resize(j->out.size() - z.avail_out);
                j->crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), j->in->data(), (uInt)j->in->size());
            }
            {
                std::lock_guard<std::mutex> g(pm_);
                j->ok = ok;
                j->done = true;
            }
            dcv_.notify_all();
        }
        if (ready) deflateEnd(&z);
        if (probe_ready) deflateEnd(&zp);
    }
    // A block that will not compress is not worth the search for matches: zlib spends its LONGEST on such data (level 6: 14 MB/s
    // a thread on random bytes against 20-50 on binaries and text here), and a layer of jars, wheels, images or compressed blobs
    // is made of it.  Three 8 KiB samples -- the block's first, middle and last -- through the fastest level: when none of them
    // shrinks by 1/64 the block goes out as stored deflate blocks (byte-aligned like the sync-flushed ones: the member stays
    // one valid stream, its CRC and length cover the same bytes).  A repeat within deflate's 32 KiB window shows in an 8 KiB
    // sample or is at most 4 positions long; what the samples miss costs ratio, never correctness.  The reference's
    // compressor (pgzip over klauspost's deflate, lib/tario/gzip.go:46-48) skips incompressible input in the same spirit; its
    // bytes are its own either way (the gzip leg is unpinned).  Per block and from the bytes alone: the blob does
    // not depend on the number of threads.
    static bool probe_enabled() {
        static const bool on = [] { const char* v = getenv("MI_GZIP_PROBE"); return !(v && *v == '0'); }();
        return on;
    }
    static bool incompressible(z_stream* zp, const uint8_t* p, size_t n) {
        constexpr size_t kSample = 8192;
        if (n < 8 * kSample) return false;
        uint8_t out[kSample + 256];
        size_t in_total = 0, out_total = 0;
        const size_t at[3] = {0, (n / 2) & ~(size_t)4095, n - kSample};
        for (const size_t off : at) {
            if (deflateReset(zp) != Z_OK) return false;
            zp->next_in = (Bytef*)(p + off);
            zp->avail_in = (uInt)kSample;
            zp->next_out = out;
            zp->avail_out = (uInt)sizeof out;
            const int rc = deflate(zp, Z_SYNC_FLUSH);
            if (rc != Z_OK && rc != Z_BUF_ERROR) return false;
            if (zp->avail_in != 0) { out_total += kSample; in_total += kSample; continue; }   // did not even fit: no gain
            in_total += kSample;
            out_total += sizeof out - zp->avail_out;
        }
        return out_total + in_total / 64 >= in_total;
    }
    static void store(const uint8_t* p, size_t n, Bytes* out) {
        out->resize(n + 5 * (n / 65535 + 1));
        uint8_t* o = out->data();
        while (n) {
            const size_t take = n < 65535 ? n : 65535;
            *o++ = 0;                                              // BFINAL = 0, BTYPE = 00 (stored); the stream is byte-aligned here
            *o++ = (uint8_t)take; *o++ = (uint8_t)(take >> 8);
            *o++ = (uint8_t)~take; *o++ = (uint8_t)(~take >> 8);
            memcpy(o, p, take);
            o += take; p += take; n -= take;
        }
        out->resize((size_t)(o - out->data()));
    }
    void stop_pool() {
        {
            std::lock_guard<std::mutex> g(pm_);
            stop_ = true;
        }
        pcv_.notify_all();
        for (auto& t : pool_) if (t.joinable()) t.join();
        pool_.clear();
    }
    int level_ = Z_DEFAULT_COMPRESSION;
    bool begun_ = false;
    mi_ctx* dev_ctx_ = nullptr;
    mi_deflater* dev_ = nullptr;
    uint64_t dev_fill_ = 0;                                        // bytes in the device window being filled
    size_t window_ = 2;
    std::vector<std::thread> pool_;
    std::mutex pm_;
    std::condition_variable pcv_, dcv_;                            // work to do / a job done
    std::deque<std::shared_ptr<Job>> todo_, inflight_;
    bool stop_ = false;
    uint32_t crc_ = 0;
    uint64_t total_in_ = 0;
    mi_host::Sha256 sha_;
};

// ---- Go archive/tar header formatting -------------------------------------------------------
bool is_ascii(const std::string& s) {
    for (unsigned char ch : s) if (ch >= 0x80) return false;
    return true;
}
std::string to_ascii(const std::string& s) {       // archive/tar toASCII: non-ASCII bytes dropped
    if (is_ascii(s)) return s;
    std::string o;
    for (unsigned char ch : s) if (ch < 0x80) o.push_back((char)ch);
    return o;
}
bool fits_octal(int field, int64_t x) {            // fitsInOctal: field-1 digits
    const unsigned bits = (unsigned)(field - 1) * 3;
    return x >= 0 && (field >= 22 || x < ((int64_t)1 << bits));
}
void put_str(uint8_t* b, size_t n, const std::string& s) {      // formatter.formatString
    const size_t c = s.size() < n ? s.size() : n;
    memcpy(b, s.data(), c);
    if (s.size() < n) b[s.size()] = 0;
    // "Some buggy readers treat regular files with a trailing slash in the V7 path field as a directory even though the
    // full path recorded elsewhere (e.g., via PAX record) contains no trailing slash": a string cut at the field's end
    // right behind a "/" gets a NUL where its trailing slashes begin (that one byte only)
    if (s.size() > n && b[n - 1] == '/') {
        size_t k = n;
        while (k > 0 && s[k - 1] == '/') --k;
        b[k] = 0;
    }
}
void put_octal(uint8_t* b, int n, int64_t x) {     // formatter.formatOctal: zero-padded, NUL-terminated
    if (!fits_octal(n, x)) x = 0;                  // the PAX record carries the real value
    uint64_t v = (uint64_t)x;                      // (fits: at most n - 1 digits)
    for (int i = n - 2; i >= 0; --i) { b[i] = (uint8_t)('0' + (v & 7)); v >>= 3; }
    b[n - 1] = 0;
}
// splitUSTARPath: name = prefix + "/" + suffix with len(prefix) <= 155, len(suffix) <= 100
bool split_ustar(const std::string& name, std::string* prefix, std::string* suffix) {
    size_t length = name.size();
    if (length <= 100 || !is_ascii(name)) return false;
    if (length > 155 + 1) length = 155 + 1;
    else if (name[length - 1] == '/') --length;
    const size_t i = name.rfind('/', length ? length - 1 : 0);
    if (i == std::string::npos || i >= length) return false;
    const size_t nlen = name.size() - i - 1, plen = i;
    if (i == 0 || nlen > 100 || nlen == 0 || plen > 155) return false;
    *prefix = name.substr(0, i);
    *suffix = name.substr(i + 1);
    return true;
}
void set_checksum(uint8_t* blk) {                  // block.SetFormat: 6 octal digits, NUL, space
    memset(blk + 148, ' ', 8);
    unsigned sum = 0;
    for (int i = 0; i < 512; ++i) sum += blk[i];
    put_octal(blk + 148, 7, sum);
    blk[155] = ' ';
}
std::string pax_record(const std::string& k, const std::string& v) {   // formatPAXRecord
    size_t size = k.size() + v.size() + 3;
    size += std::to_string(size).size();
    std::string rec = std::to_string(size) + " " + k + "=" + v + "\n";
    if (rec.size() != size) rec = std::to_string(rec.size()) + " " + k + "=" + v + "\n";
    return rec;
}
// path.Clean (Go): single slashes, no "." elements, inner ".." elements eaten with the element before
// them, ".." directly under the root dropped, no trailing slash; "" -> "."
std::string path_clean(const std::string& p) {
    if (p.empty()) return ".";
    const bool rooted = p[0] == '/';
    std::vector<std::string> el;
    size_t i = 0;
    while (i < p.size()) {
        while (i < p.size() && p[i] == '/') ++i;
        size_t j = i;
        while (j < p.size() && p[j] != '/') ++j;
        if (j > i) {
            const std::string e = p.substr(i, j - i);
            if (e == ".") {
            } else if (e == "..") {
                if (!el.empty() && el.back() != "..") el.pop_back();
                else if (!rooted) el.push_back("..");
            } else {
                el.push_back(e);
            }
        }
        i = j;
    }
    std::string out = rooted ? "/" : "";
    for (size_t k = 0; k < el.size(); ++k) { if (k) out += "/"; out += el[k]; }
    return out.empty() ? "." : out;
}
// path.Join: the non-empty elements joined by "/" and cleaned; "" if there is none
std::string path_clean_join(const std::string& dir, const std::string& mid, const std::string& file) {
    std::string j;
    for (const std::string* e : {&dir, &mid, &file}) {
        if (e->empty()) continue;
        if (!j.empty()) j += "/";
        j += *e;
    }
    return j.empty() ? j : path_clean(j);
}

struct Hdr {
    std::string name, linkname;
    char typeflag = '0';
    int64_t mode = 0, uid = 0, gid = 0, size = 0, mtime = 0;
};

// Writer.WriteHeader with Format unknown: USTAR if everything fits, else PAX.  Appends the header
// block(s) to out.  False: neither format can carry the entry (a NUL in a name).
bool format_header(const Hdr& h, Bytes* out, std::string* err) {
    if (h.name.find('\0') != std::string::npos || h.linkname.find('\0') != std::string::npos) {
        *err = "archive/tar: header field contains NUL";
        return false;
    }
    std::vector<std::pair<std::string, std::string>> pax;
    bool ustar = true;
    std::string prefix, suffix;
    const bool long_name = h.name.size() > 100 || !is_ascii(h.name);
    const bool can_split = split_ustar(h.name, &prefix, &suffix);
    if (long_name) {
        if (!can_split) ustar = false;
        pax.push_back({"path", h.name});
    }
    if (h.linkname.size() > 100 || !is_ascii(h.linkname)) { ustar = false; pax.push_back({"linkpath", h.linkname}); }
    if (!fits_octal(8, h.uid)) { ustar = false; pax.push_back({"uid", std::to_string(h.uid)}); }
    if (!fits_octal(8, h.gid)) { ustar = false; pax.push_back({"gid", std::to_string(h.gid)}); }
    if (!fits_octal(12, h.size)) { ustar = false; pax.push_back({"size", std::to_string(h.size)}); }
    if (!fits_octal(12, h.mtime)) { ustar = false; pax.push_back({"mtime", std::to_string(h.mtime)}); }
    if (!fits_octal(8, h.mode)) { *err = "archive/tar: mode does not fit"; return false; }

    auto main_block = [&](const std::string& name, const std::string& linkname, const std::string& pfx) {
        uint8_t b[512];
        memset(b, 0, sizeof b);
        put_str(b + 0, 100, name);
        put_octal(b + 100, 8, h.mode);
        put_octal(b + 108, 8, h.uid);
        put_octal(b + 116, 8, h.gid);
        put_octal(b + 124, 12, h.size);
        put_octal(b + 136, 12, h.mtime);
        b[156] = (uint8_t)h.typeflag;
        put_str(b + 157, 100, linkname);
        memcpy(b + 257, "ustar\0" "00", 8);
        put_str(b + 265, 32, "");                  // Uname, Gname: cleared by createHeader
        put_str(b + 297, 32, "");
        put_octal(b + 329, 8, 0);                  // Devmajor / Devminor
        put_octal(b + 337, 8, 0);
        put_str(b + 345, 155, pfx);
        set_checksum(b);
        out->insert(out->end(), b, b + 512);
    };
    if (ustar) {
        if (can_split) main_block(suffix, h.linkname, prefix);
        else main_block(h.name, h.linkname, "");
        return true;
    }
    // PAX: the extended-header file first (writeRawFile: no uname/gname/dev fields at all)
    std::sort(pax.begin(), pax.end());
    std::string data;
    for (auto& kv : pax) data += pax_record(kv.first, kv.second);
    {
        // path.Split(realName): dir = up to and including the last "/", file = the rest
        const size_t slash = h.name.rfind('/');
        const std::string dir = slash == std::string::npos ? "" : h.name.substr(0, slash + 1);
        const std::string file = slash == std::string::npos ? h.name : h.name.substr(slash + 1);
        std::string xname = to_ascii(path_clean_join(dir, "PaxHeaders.0", file));
        if (xname.size() > 100) xname.resize(100);
        while (!xname.empty() && xname.back() == '/') xname.pop_back();
        uint8_t b[512];
        memset(b, 0, sizeof b);
        b[156] = 'x';
        put_str(b + 0, 100, xname);
        put_octal(b + 100, 8, 0);
        put_octal(b + 108, 8, 0);
        put_octal(b + 116, 8, 0);
        put_octal(b + 124, 12, (int64_t)data.size());
        put_octal(b + 136, 12, 0);
        memcpy(b + 257, "ustar\0" "00", 8);
        set_checksum(b);
        out->insert(out->end(), b, b + 512);
        out->insert(out->end(), data.begin(), data.end());
        out->insert(out->end(), (512 - data.size() % 512) % 512, 0);
    }
    main_block(to_ascii(h.name), to_ascii(h.linkname), "");
    return true;
}

// os.FileMode -> tar Mode: permission bits + setuid / setgid / sticky (FileInfoHeader)
int64_t tar_mode(uint32_t st_mode) { return (int64_t)(st_mode & 07777u); }

std::string trim_left_slashes(const char* s) {
    while (*s == '/') ++s;
    return std::string(s);
}

}  // namespace

struct mi_layer {
    std::string err;
    uint32_t flags = 0;                            // MI_LAYER_*
    DigestSink tar;
    std::unique_ptr<GzipSink> gz;
    std::shared_ptr<Bytes> cur;
    uint64_t n_entries = 0;
    uint64_t files_opened = 0, file_bytes_read = 0;    // what this writer read from disk itself (mi_layer_io_counts)
    bool pipelined = false;                            // batch files are read while the batch is still staged (mi_local.h)
    mi_batch* timed_batch = nullptr;                   // MI_LAYER_TIMING: the batch whose window this layer read through
    double read_s = 0;                                 // ... and the seconds the framer spent getting file bytes (either source)
    std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    bool finished = false, failed = false;
    bool gzip_ctx_set = false;

    int fail_soft(int code, const char* msg) { err = msg; return code; }    // a refused call: the layer goes on
    int fail(int code, const char* fmt, ...) {
        char buf[600];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        failed = true;
        return code;
    }
    // A chunk of a batch file that has not been held against its source sums yet must not reach the sinks (a SHA-256 stream
    // cannot be taken back): while `hold` is on, a block that fills up waits in `held` -- a chunk is at most one block long, so
    // at most one does -- and the chunk can be framed again from its first byte (rewind) after a second fetch from HBM.
    std::vector<std::shared_ptr<Bytes>> held;
    bool hold = false;
    uint64_t n_verified_files = 0, verified_bytes = 0, n_refetched = 0;
    struct Mark { size_t n_held, cur_size; };
    Mark mark() const { return Mark{held.size(), cur ? cur->size() : 0}; }
    void rewind(const Mark& m) {
        if (held.size() > m.n_held) { cur = held[m.n_held]; held.resize(m.n_held); }
        if (cur) cur->resize(m.cur_size);
    }
    void push_block(const std::shared_ptr<Bytes>& blk) {
        Block b = blk;
        tar.push(b);                               // the tee: both sinks see the same immutable block
        if (gz) gz->push(b);
    }
    void release_hold() {
        for (auto& blk : held) push_block(blk);
        held.clear();
        hold = false;
    }
    void flush_block() {
        if (!cur || cur->empty()) return;
        push_block(cur);
        cur.reset();
    }
    uint8_t* room(size_t* n) {                     // space in the current block (at most *n bytes)
        if (!cur) { cur = std::make_shared<Bytes>(); cur->reserve(kBlockBytes); }
        if (cur->size() == kBlockBytes) {
            if (hold) { held.push_back(cur); cur.reset(); } else flush_block();
            cur = std::make_shared<Bytes>();
            cur->reserve(kBlockBytes);
        }
        const size_t left = kBlockBytes - cur->size();
        if (*n > left) *n = left;
        const size_t at = cur->size();
        cur->resize(at + *n);
        return cur->data() + at;
    }
    void append(const uint8_t* p, size_t n) {
        while (n) {
            size_t take = n;
            uint8_t* dst = room(&take);
            if (p) { memcpy(dst, p, take); p += take; } else memset(dst, 0, take);
            n -= take;
        }
    }
    int sink_error() {
        // ConcurrentMultiWriter.Write (multi_writer.go:62-64): every failing sink's message, joined
        std::string e = tar.error();
        const std::string g = gz ? gz->error() : std::string();
        if (!g.empty()) e = e.empty() ? g : e + ", " + g;
        if (!e.empty()) return fail(MI_ERR_IO, "failed to write: %s", e.c_str());
        return MI_OK;
    }
};

extern "C" {

int mi_layer_config_default(mi_layer_config* cfg) {
    if (!cfg) return MI_ERR_INVALID;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->gzip_level = MI_GZIP_DEFAULT;
    cfg->out_fd = -1;
    return MI_OK;
}

int mi_layer_begin(const mi_layer_config* cfg, mi_layer** out) {
    if (!cfg || !out || cfg->struct_size != sizeof(mi_layer_config)) return MI_ERR_INVALID;
    if (cfg->gzip_level != MI_GZIP_OFF && (cfg->gzip_level < -1 || cfg->gzip_level > 9)) return MI_ERR_INVALID;
    if (cfg->flags & ~MI_LAYER_MODE_WITH_TYPE) return MI_ERR_INVALID;
    mi_layer* l = new mi_layer();
    l->flags = cfg->flags;
    if (cfg->gzip_level == MI_GZIP_OFF) {
        l->tar.raw_fd = cfg->out_fd;
    } else {
        l->gz.reset(new GzipSink());
        l->gz->out_fd = cfg->out_fd;
        if (!l->gz->init(cfg->gzip_level)) { delete l; return MI_ERR_NOMEM; }
        l->gz->start();
    }
    l->tar.start();
    *out = l;
    return MI_OK;
}

const char* mi_layer_error(mi_layer* l) { return l ? l->err.c_str() : "null layer"; }

// memLayer.addHeader (mem_layer.go:197-212): a path whose base name carries the whiteout prefix is filed as a
// whiteoutMemFile, whatever it is on disk -- committed as a zero header with only that name (newWhiteoutMemFile
// :97-101, commit :127-132), no content (TestAddHeader/Whiteout, mem_layer_test.go:123-148)
static bool whiteout_by_name(const std::string& rel_name, Hdr* z) {
    std::string p = rel_name;
    while (!p.empty() && p.back() == '/') p.pop_back();
    const size_t slash = p.rfind('/');
    if (p.compare(slash == std::string::npos ? 0 : slash + 1, 4, ".wh.") != 0) return false;
    *z = Hdr();
    z->name = p;
    z->typeflag = '0';                                          // TypeRegA promoted to TypeReg by WriteHeader
    return true;
}

static int add_header(mi_layer* l, const Hdr& h) {
    Bytes hb;
    std::string err;
    if (!format_header(h, &hb, &err)) return l->fail(MI_ERR_INVALID, "write header %s: %s", h.name.c_str(), err.c_str());
    l->append(hb.data(), hb.size());
    ++l->n_entries;
    return MI_OK;
}

// One entry: header, then -- a regular file -- exactly e->size bytes from ONE of two sources: the file at src_path
// (io.CopyN over os.Open, lib/tario/write.go:36-45), or file `batch_file` of a staged batch, i.e. the bytes the GPU scanned
// (mi_batch_read_file): what the content-aware commit uses, so that a file is read from disk once and the tar holds the
// very bytes its chunk root describes.
static int layer_add_entry(mi_layer* l, const mi_tree_entry* e, const char* src_path, mi_batch* batch, uint64_t batch_file) {
    if (!l || !e || !e->relpath) return MI_ERR_INVALID;
    if (l->finished || l->failed) return l->fail(MI_ERR_STATE, "layer is finished or failed");
    Hdr h;
    h.name = trim_left_slashes(e->relpath);                    // RelPath(dst) + WriteHeader's TrimLeft
    {
        Hdr z;
        if (whiteout_by_name(h.name, &z)) {
            int rc = add_header(l, z);
            return rc ? rc : l->sink_error();
        }
    }
    h.mode = (l->flags & MI_LAYER_MODE_WITH_TYPE) ? (int64_t)(e->mode & 0177777u) : tar_mode(e->mode);
    h.uid = e->uid;
    h.gid = e->gid;
    h.mtime = e->mtime_sec;                                     // already truncated to seconds
    switch (e->kind) {
        case 0:                                                 // directory: trailing "/" (mem_layer.go:166-170)
            h.typeflag = '5';
            if (h.name.empty() || h.name.back() != '/') h.name += "/";
            break;
        case 1: h.typeflag = '0'; h.size = (int64_t)e->size; break;
        case 2: h.typeflag = '2'; h.linkname = e->link_target ? e->link_target : ""; break;
        case 3: h.typeflag = '1'; h.linkname = e->link_target ? e->link_target : ""; break;
        default:
            return l->fail(MI_ERR_INVALID, "content commit %s: unsupported type %u", h.name.c_str(), (unsigned)e->kind);
    }
    int fd = -1;
    if (e->kind == 1 && !batch) {                               // open before the header, like os.Open failing first would
        if (!src_path) return l->fail(MI_ERR_INVALID, "content commit %s: no source path", h.name.c_str());
        fd = open(src_path, O_RDONLY | O_CLOEXEC);
        if (fd < 0) return l->fail(MI_ERR_IO, "open src file %s: %s", src_path, strerror(errno));
        ++l->files_opened;
    }
    int rc = add_header(l, h);
    if (rc) { if (fd >= 0) close(fd); return rc; }
    if (e->kind == 1) {
        uint64_t left = e->size, off = 0;                       // io.CopyN(w, f, h.Size): exactly Size bytes
        const auto t_read = std::chrono::steady_clock::now();
        double pushed0 = l->tar.full_s + (l->gz ? l->gz->full_s : 0);
        if (batch) l->timed_batch = batch;
        // A batch file is framed CHUNK BY CHUNK (1 MiB of the file, mi_filesum.h) when the batch kept the sums of its bytes as
        // they were read: the same sums over what came back from HBM; equal, or the chunk is framed again after a second
        // fetch, or the layer fails -- io.CopyN's "the bytes or an error" across two PCIe hops.
        bool want = false;
        static const bool verify_on = [] { const char* v = getenv("MI_COMMIT_VERIFY"); return !(v && *v == '0'); }();
        if (batch && verify_on && e->size) { int has = 0; if (mi_batch_chunk_sum(batch, batch_file, 0, nullptr, nullptr, &has) == MI_OK) want = has != 0; }
        while (left) {
            const uint64_t chunk_len = want ? std::min<uint64_t>(left, mi_sum::kChunk - off % mi_sum::kChunk) : left;
            for (int attempt = 0;; ++attempt) {
                const mi_layer::Mark m = l->mark();
                if (want) l->hold = true;
                uint64_t a = 0, b = 0, done = 0;
                while (done < chunk_len) {
                    size_t take = chunk_len - done > kBlockBytes ? kBlockBytes : (size_t)(chunk_len - done);
                    uint8_t* dst = l->room(&take);
                    if (batch) {
                        const int brc = l->pipelined ? mi_batch_read_file_landed(batch, batch_file, off + done, dst, take)
                                                     : mi_batch_read_file(batch, batch_file, off + done, dst, take);
                        if (brc) return l->fail(brc, "copy file %s to tar writer: staged file %llu: %s", h.name.c_str(),
                                                (unsigned long long)batch_file, mi_last_error_of_batch(batch));
                        if (want) mi_sum::chunk_add(dst, take, (size_t)((off + done) % mi_sum::kChunk), &a, &b);
                    } else {
                        size_t got = 0;
                        while (got < take) {
                            const ssize_t r = pread(fd, dst + got, take - got, (off_t)(off + done + got));
                            if (r < 0 && errno == EINTR) continue;
                            if (r <= 0) {
                                close(fd);
                                return l->fail(MI_ERR_IO, "copy file %s to tar writer: %s", src_path,
                                               r == 0 ? "unexpected EOF" : strerror(errno));
                            }
                            got += (size_t)r;
                        }
                        l->file_bytes_read += take;
                    }
                    done += take;
                }
                if (!want) break;
                const uint64_t k = off / mi_sum::kChunk;
                uint64_t wa = 0, wb = 0;
                int has = 0;
                if (mi_batch_chunk_sum(batch, batch_file, k, &wa, &wb, &has) != MI_OK || !has)
                    return l->fail(MI_ERR_STATE, "copy file %s to tar writer: the batch lost the sums of chunk %llu", h.name.c_str(), (unsigned long long)k);
                if (a == wa && b == wb) {
                    if (attempt) ++l->n_refetched;
                    l->release_hold();
                    break;
                }
                if (attempt == 0) {                                 // once more, from HBM (not from the window that delivered these)
                    l->rewind(m);
                    mi_batch_drop_windows(batch);
                    continue;
                }
                char why[700];
                why[0] = 0;
                (void)mi_batch_explain_chunk(batch, batch_file, k, why, sizeof why);
                return l->fail(MI_ERR_IO, "copy file %s to tar writer: the bytes that came back from HBM are not the bytes that were read from the file "
                               "(sums %016llx/%016llx, also after a second fetch): %s", h.name.c_str(), (unsigned long long)a, (unsigned long long)b, why);
            }
            off += chunk_len;
            left -= chunk_len;
        }
        if (want || (batch && verify_on && !e->size && mi_batch_keeps_sums(batch))) { ++l->n_verified_files; l->verified_bytes += e->size; }
        if (fd >= 0) close(fd);
        l->read_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_read).count() -
                     (l->tar.full_s + (l->gz ? l->gz->full_s : 0) - pushed0);
        l->append(nullptr, (size_t)((512 - e->size % 512) % 512));   // tar.Writer pads at the next header
    }
    return l->sink_error();
}

int mi_layer_add(mi_layer* l, const mi_tree_entry* e, const char* src_path) {
    return layer_add_entry(l, e, src_path, nullptr, 0);
}

int mi_layer_add_batch_file(mi_layer* l, const mi_tree_entry* e, mi_batch* batch, uint64_t file_index) {
    if (!batch) return MI_ERR_INVALID;
    if (l && e && e->kind == 1) {
        uint64_t nf = 0;
        mi_batch_counts(batch, &nf, nullptr, nullptr);
        uint64_t staged = 0;
        if (file_index >= nf || mi_batch_file_size(batch, file_index, &staged) != MI_OK)
            return l->fail(MI_ERR_INVALID, "content commit %s: the batch holds no file %llu", e->relpath ? e->relpath : "", (unsigned long long)file_index);
        if (staged != e->size)
            return l->fail(MI_ERR_INVALID, "content commit %s: the entry says %llu bytes, the staged file has %llu", e->relpath ? e->relpath : "",
                           (unsigned long long)e->size, (unsigned long long)staged);
    }
    return layer_add_entry(l, e, nullptr, batch, file_index);
}

int mi_layer_set_gzip_ctx(mi_layer* l, mi_ctx* ctx) {
    if (!l || !ctx) return MI_ERR_INVALID;
    if (!l->gz || l->gz->level() == 0) return l->fail_soft(MI_ERR_INVALID, "mi_layer_set_gzip_ctx: this layer has no gzip leg to code (MI_GZIP_OFF or level 0)");
    if (l->finished || l->failed || l->n_entries || l->cur || l->gzip_ctx_set)
        return l->fail_soft(MI_ERR_STATE, "mi_layer_set_gzip_ctx: after mi_layer_begin and before the first add, once");
    l->gzip_ctx_set = true;
    l->gz->set_device(ctx);
    return MI_OK;
}

void mi_layer_set_pipelined(mi_layer* l, int on) { if (l) l->pipelined = on != 0; }

void mi_layer_verify_counts(mi_layer* l, uint64_t* files, uint64_t* bytes, uint64_t* refetched) {   // (hidden: mi_local.h)
    if (files) *files = l ? l->n_verified_files : 0;
    if (bytes) *bytes = l ? l->verified_bytes : 0;
    if (refetched) *refetched = l ? l->n_refetched : 0;
}

int mi_layer_io_counts(mi_layer* l, uint64_t* files_opened, uint64_t* file_bytes_read) {
    if (!l) return MI_ERR_INVALID;
    if (files_opened) *files_opened = l->files_opened;
    if (file_bytes_read) *file_bytes_read = l->file_bytes_read;
    return MI_OK;
}

int mi_layer_add_whiteout(mi_layer* l, const char* deleted_path) {
    if (!l || !deleted_path) return MI_ERR_INVALID;
    if (l->finished || l->failed) return l->fail(MI_ERR_STATE, "layer is finished or failed");
    // memLayer.addWhiteout (mem_layer.go:213-228): <dir>/.wh.<base>, a zero header with only a Name
    std::string p = trim_left_slashes(deleted_path);
    while (!p.empty() && p.back() == '/') p.pop_back();
    const size_t slash = p.rfind('/');
    const std::string base = slash == std::string::npos ? p : p.substr(slash + 1);
    if (base.empty()) return l->fail(MI_ERR_INVALID, "whiteout of the root");
    if (base.compare(0, 4, ".wh.") == 0)
        return l->fail(MI_ERR_INVALID, "base name contains whiteout prefix: %s", deleted_path);
    Hdr h;
    h.name = (slash == std::string::npos ? "" : p.substr(0, slash + 1)) + ".wh." + base;
    h.typeflag = '0';                                           // TypeRegA promoted to TypeReg by WriteHeader
    int rc = add_header(l, h);
    return rc ? rc : l->sink_error();
}

int mi_layer_finish(mi_layer* l, mi_layer_result* out) {
    if (!l || !out) return MI_ERR_INVALID;
    if (l->finished) return l->fail(MI_ERR_STATE, "layer already finished");
    l->finished = true;
    if (!l->failed) l->append(nullptr, 1024);                   // tar.Writer.Close: two zero blocks
    l->flush_block();
    l->tar.close();
    if (l->gz) l->gz->close();
    if (l->failed) return MI_ERR_STATE;
    int rc = l->sink_error();
    if (rc) return rc;
    static const bool timing = [] { const char* e = getenv("MI_LAYER_TIMING"); return e && *e == '1'; }();
    if (timing) {
        double w = 0, f = 0;
        uint64_t nf = 0, nb = 0;
        mi_batch_read_stats(l->timed_batch, &w, &f, &nf, &nb);
        fprintf(stderr, "mi_layer: %llu tar bytes in %.3f s | framer: %.3f s getting file bytes (from HBM: %.3f s waiting for bytes to land, %.3f s in %llu window "
                "copies of %llu bytes -- the batch's totals), %.3f s held up by the tar sink%s | tar sink idle %.3f s\n",
                (unsigned long long)l->tar.bytes, std::chrono::duration<double>(std::chrono::steady_clock::now() - l->t_begin).count(), l->read_s, w, f,
                (unsigned long long)nf, (unsigned long long)nb, l->tar.full_s, l->gz ? " (+ gzip)" : "", l->tar.idle_s);
    }
    memset(out, 0, sizeof *out);
    memcpy(out->tar_sha256, l->tar.digest, 32);
    out->tar_bytes = l->tar.bytes;
    out->n_entries = l->n_entries;
    if (l->gz) {
        memcpy(out->gzip_sha256, l->gz->digest, 32);
        out->gzip_bytes = l->gz->bytes;
    }
    return MI_OK;
}

void mi_layer_free(mi_layer* l) {
    if (!l) return;
    if (!l->finished) {                                         // abandon: stop the sink threads
        l->tar.close();
        if (l->gz) l->gz->close();
    }
    delete l;
}

int mi_layer_header_bytes(const mi_tree_entry* e, uint32_t layer_flags, uint8_t* out, uint64_t cap, uint64_t* n) {
    if (!e || !e->relpath || !n || (layer_flags & ~MI_LAYER_MODE_WITH_TYPE)) return MI_ERR_INVALID;
    Hdr h;
    h.name = trim_left_slashes(e->relpath);
    h.mode = (layer_flags & MI_LAYER_MODE_WITH_TYPE) ? (int64_t)(e->mode & 0177777u) : tar_mode(e->mode);
    h.uid = e->uid;
    h.gid = e->gid;
    h.mtime = e->mtime_sec;
    Hdr z;
    if (e->kind <= 3 && whiteout_by_name(h.name, &z)) h = z;
    else if (e->kind == 0) { h.typeflag = '5'; if (h.name.empty() || h.name.back() != '/') h.name += "/"; }
    else if (e->kind == 1) { h.typeflag = '0'; h.size = (int64_t)e->size; }
    else if (e->kind == 2 || e->kind == 3) { h.typeflag = e->kind == 2 ? '2' : '1'; h.linkname = e->link_target ? e->link_target : ""; }
    else return MI_ERR_INVALID;
    Bytes hb;
    std::string err;
    if (!format_header(h, &hb, &err)) return MI_ERR_INVALID;
    *n = hb.size();
    if (cap < hb.size()) return MI_ERR_CAPACITY;
    if (out) memcpy(out, hb.data(), hb.size());
    return MI_OK;
}

// ---- cache entry codec (lib/cache/cache_manager.go:34-35, 239-252) ---------------------------
static const char kCachePrefix[] = "makisu_builder_cache_";
static const char kCacheEmpty[] = "MAKISU_CACHE_EMPTY";

int mi_cache_key(const char* cache_id, char* out, uint64_t cap) {
    if (!cache_id || !out) return MI_ERR_INVALID;
    const size_t need = sizeof kCachePrefix - 1 + strlen(cache_id) + 1;
    if (cap < need) return MI_ERR_CAPACITY;
    snprintf(out, (size_t)cap, "%s%s", kCachePrefix, cache_id);
    return MI_OK;
}

int mi_cache_create_entry(const uint8_t* tar_sha256, const uint8_t* gzip_sha256, char* out, uint64_t cap) {
    if (!out) return MI_ERR_INVALID;
    if (!tar_sha256 && !gzip_sha256) {                          // createEntry(nil): the step made no layer
        if (cap < sizeof kCacheEmpty) return MI_ERR_CAPACITY;
        memcpy(out, kCacheEmpty, sizeof kCacheEmpty);
        return MI_OK;
    }
    if (!tar_sha256 || !gzip_sha256) return MI_ERR_INVALID;
    if (cap < 130) return MI_ERR_CAPACITY;
    snprintf(out, 130, "%s,%s", mi::hex32(tar_sha256).c_str(), mi::hex32(gzip_sha256).c_str());
    return MI_OK;
}

static int unhex32(const char* s, uint8_t* out) {
    for (int i = 0; i < 32; ++i) {
        int v = 0;
        for (int k = 0; k < 2; ++k) {
            const char ch = s[2 * i + k];
            int d;
            if (ch >= '0' && ch <= '9') d = ch - '0';
            else if (ch >= 'a' && ch <= 'f') d = ch - 'a' + 10;
            else if (ch >= 'A' && ch <= 'F') d = ch - 'A' + 10;
            else return -1;
            v = v * 16 + d;
        }
        out[i] = (uint8_t)v;
    }
    return 0;
}

int mi_cache_parse_entry(const char* entry, int* is_empty, uint8_t* tar_sha256, uint8_t* gzip_sha256) {
    if (!entry || !is_empty || !tar_sha256 || !gzip_sha256) return MI_ERR_INVALID;
    *is_empty = 0;
    if (strcmp(entry, kCacheEmpty) == 0) { *is_empty = 1; return MI_OK; }   // PullCache returns (nil, nil)
    const char* comma = strchr(entry, ',');
    if (!comma) return MI_ERR_INVALID;                          // parseEntry: "parse redis entry"
    // SplitN(entry, ",", 2): both halves must be sha256 hex for the digests to mean anything
    if (comma - entry != 64 || strlen(comma + 1) != 64) return MI_ERR_INVALID;
    if (unhex32(entry, tar_sha256) || unhex32(comma + 1, gzip_sha256)) return MI_ERR_INVALID;
    return MI_OK;
}

int mi_cache_parse_entry_str(const char* entry, char* tar_digest, uint64_t tar_cap, char* gzip_digest,
                             uint64_t gzip_cap) {
    if (!entry || !tar_digest || !gzip_digest) return MI_ERR_INVALID;
    const char* comma = strchr(entry, ',');
    if (!comma) return MI_ERR_INVALID;                          // "parse redis entry: ..."
    const size_t a = (size_t)(comma - entry), b = strlen(comma + 1);
    if (tar_cap < a + 8 || gzip_cap < b + 8) return MI_ERR_CAPACITY;
    memcpy(tar_digest, "sha256:", 7);
    memcpy(tar_digest + 7, entry, a);
    tar_digest[7 + a] = 0;
    memcpy(gzip_digest, "sha256:", 7);
    memcpy(gzip_digest + 7, comma + 1, b + 1);
    return MI_OK;
}

// chunk_root of a digest list on the host: the definition the kernels implement (tables.hip root
// passes) -- one hash over the concatenation when n <= 64, else a fan-out-64 tree; the
// hash at every node is the ctx's chunk digest algorithm (MI_DIGEST_*).
// For a file whose chunk rows come from several batches (parts): concatenate the parts' digests in
// part order and call this; equals mi_file_result.chunk_root of the file scanned whole.
extern "C++" {
template <class Hash>
static void chunk_root_with(const uint8_t* digests, uint64_t n, uint8_t* root_out) {
    const uint64_t F = 64;
    std::vector<uint8_t> cur, next;
    const uint8_t* p = digests;
    while (n > F) {
        const uint64_t m = (n + F - 1) / F;
        next.resize(m * 32);
        for (uint64_t g = 0; g < m; ++g) {
            const uint64_t cnt = n - g * F < F ? n - g * F : F;
            Hash h;
            h.update(p + g * F * 32, cnt * 32);
            h.final(&next[g * 32]);
        }
        cur.swap(next);
        p = cur.data();
        n = m;
    }
    Hash h;
    h.update(p, n * 32);
    h.final(root_out);
}
}  // extern "C++"
int mi_chunk_root_alg(uint32_t alg, const uint8_t* digests, uint64_t n, uint8_t* root_out) {
    if ((!digests && n) || !root_out || alg > MI_DIGEST_BLAKE2S) return MI_ERR_INVALID;
    if (alg == MI_DIGEST_BLAKE2S) chunk_root_with<mi_host::Blake2s>(digests, n, root_out);
    else                          chunk_root_with<mi_host::Sha256>(digests, n, root_out);
    return MI_OK;
}
int mi_chunk_root(const uint8_t* digests, uint64_t n, uint8_t* root_out) {
    return mi_chunk_root_alg(MI_DIGEST_SHA256, digests, n, root_out);
}

}  // extern "C"
