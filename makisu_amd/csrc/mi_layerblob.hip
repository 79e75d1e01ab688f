// mi_layerblob.hip -- A PULLED LAYER BECOMES A BATCH: mi_batch_add_layer_blob and _path.  The blob goes up once; a
// gzip this library can inflate in parallel is inflated by mi_inflate.hip straight into the batch's arena (mi_inflater_run_device),
// anything else lands there as a plain tar; mi_tarscan.hip marks the header candidates where the tar lies, mi_tar.hip's parser
// follows the live chain through what came down (host_tarcache.h) and fetches the rest on demand; then, and only then, the
// batch changes: the regular members become its files where they lie.
//
// Order of work: checks, window.flush | the source from the first two bytes, the plan of a gzip blob with the blob's SHA-256
// taken while it goes up | the reservation behind what the arena holds | the bytes | the header pass and the listing | the batch.
#include "mi_internal.h"
#include "mi_inflate_local.h"
#include "mi_tarscan.h"
#include "host_sha256.h"

#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

using namespace mi;

namespace {

constexpr u64 kStage = 4ull << 20;                      // plain bytes go up in pieces of this, through two pinned buffers

void blob_sha_seen(void* arg, const uint8_t* bytes, uint64_t n) { ((mi_host::Sha256*)arg)->update(bytes, (size_t)n); }

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// a gzip blob the device cannot inflate in parallel: zlib, into host memory of the tar's size (members may be concatenated)
bool zlib_inflate(const u8* gz, u64 n, std::vector<u8>* tar) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 15 + 16) != Z_OK) return false;
    tar->resize(std::max<u64>(4 * n, 1u << 16));
    u64 in = 0, out = 0;
    bool ok = false;
    for (;;) {
        if (out == tar->size()) tar->resize(tar->size() * 2);
        if (z.avail_in == 0 && in < n) {
            const u64 take = std::min<u64>(n - in, 1u << 30);
            z.next_in = const_cast<Bytef*>(gz + in);
            z.avail_in = (uInt)take;
            in += take;
        }
        const u64 room = std::min<u64>(tar->size() - out, 1u << 30);
        z.next_out = tar->data() + out;
        z.avail_out = (uInt)room;
        const int rc = inflate(&z, Z_NO_FLUSH);
        out += room - z.avail_out;
        if (rc == Z_STREAM_END) {
            if (z.avail_in == 0 && in >= n) { ok = true; break; }
            if (inflateReset(&z) != Z_OK) break;
        } else if (rc != Z_OK && !(rc == Z_BUF_ERROR && z.avail_out == 0)) {
            break;                                      // corrupt, or the input ended inside the stream
        }
    }
    inflateEnd(&z);
    tar->resize(ok ? out : 0);
    return ok;
}

// src[0, n) to d_dst on the ctx stream through two pinned buffers; sha (may be NULL) sees every piece while it is under way
int upload_plain(mi_ctx* c, u8* d_dst, const u8* src, u64 n, mi_host::Sha256* sha) {
    PinBuf h[2];
    Event staged[2];
    StreamDrain drain{c->stream};                       // (goes first: buffers and events after it)
    const u64 piece = std::min(n, kStage);
    for (int k = 0; k < 2 && (k == 0 || n > kStage); ++k) {
        HIPCHK(c, h[k].ensure(piece));
        HIPCHK(c, staged[k].create(hipEventDisableTiming));
    }
    int k = 0;
    for (u64 at = 0; at < n; at += kStage, k ^= 1) {
        const u64 take = std::min(n - at, kStage);
        if (at >= 2 * kStage) HIPCHK(c, hipEventSynchronize(staged[k]));
        memcpy(h[k].p, src + at, take);
        HIPCHK(c, hipMemcpyAsync(d_dst + at, h[k].p, take, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(staged[k], c->stream));
        if (sha) sha->update(src + at, (size_t)take);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_OK;
}

struct Fetch { mi_ctx* c; const u8* d_tar; };
int fetch_from_device(void* arg, uint64_t off, void* dst, uint64_t n) {
    const Fetch* f = (const Fetch*)arg;
    if (hipMemcpyAsync(dst, f->d_tar + off, n, hipMemcpyDeviceToHost, f->c->stream) != hipSuccess) return MI_ERR_HIP;
    return hipStreamSynchronize(f->c->stream) == hipSuccess ? (int)MI_OK : (int)MI_ERR_HIP;
}

struct InflaterOwner { mi_inflater* d = nullptr; ~InflaterOwner() { mi_inflater_free(d); } };

// mi_batch_add_layer_blob's body; index (may be NULL): the blob's index of checkpoints, a hint; spec (may be NULL; no index
// then): the plan from speculative spans takes the index's place and route -- source 4
int add_layer_blob(mi_batch* b, const void* blob, uint64_t n, const u8* index, u64 index_bytes, uint64_t tag_base, mi_tar** listing,
                   uint8_t* blob_sha256, mi_layer_blob_info* info_out, const InfSpecAsk* spec = nullptr) {
    if (listing) *listing = nullptr;
    if (info_out) memset(info_out, 0, sizeof *info_out);
    if (!b || !blob) return MI_ERR_INVALID;
    mi_ctx* c = b->ctx;
    if (b->group) return fail(c, MI_ERR_INVALID, "mi_batch_add_layer_blob: a batch group has one arena per GPU; add the layer to one of its members");
    if (b->staged) return fail(c, MI_ERR_STATE, "batch already ran; begin a new batch");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = b->window.flush(b);                        // the inline window may hold bytes of earlier small adds
    if (rc) return rc;
    const u8* src = (const u8*)blob;
    const bool gzip = n >= 2 && src[0] == 0x1f && src[1] == 0x8b;
    u32 fell_back = 0;
    // with an index the way up may be gone twice: the spans straight into the arena, and -- the index refused, at the plan or by a span or
    // the trailer -- everything again as the unindexed call does it (nothing of the batch has changed by then)
    for (int with_index = gzip && (index || spec) ? 1 : 0; ; with_index = 0) {
    mi_layer_blob_info info = {};
    mi_host::Sha256 sha;
    InflaterOwner inf;
    std::vector<u8> host_tar;                           // source 2: the tar as zlib gave it
    src = (const u8*)blob;
    u64 T = n;
    auto t0 = std::chrono::steady_clock::now();
    if (gzip) {
        rc = mi_inflater_create(c, &inf.d);
        if (rc) return rc;
        rc = with_index && spec ? mi_inflater_plan_spec(inf.d, src, n, spec->piece_bytes, blob_sha256 ? blob_sha_seen : nullptr, &sha)
           : with_index         ? mi_inflater_plan_indexed(inf.d, src, n, index, index_bytes, blob_sha256 ? blob_sha_seen : nullptr, &sha)
                                : mi_inflater_plan(inf.d, src, n, blob_sha256 ? blob_sha_seen : nullptr, &sha);
        mi_inflater_info(inf.d, &info.inflate);
        if (with_index && spec && spec->spec_info) mi_inflater_spec_info(inf.d, spec->spec_info);
        if (rc) return fail(c, rc, "mi_batch_add_layer_blob: %s", mi_inflater_error(inf.d));
        if (with_index && info.inflate.verdict != MI_INFLATE_DONE) {
            fell_back = info.inflate.verdict == MI_INFLATE_INDEX_REFUSED ? 2 : 0;
            continue;
        }
        if (info.inflate.verdict == MI_INFLATE_DONE) {
            info.source = with_index ? (spec ? 4 : 3) : 1;
            T = info.inflate.out_bytes;
            info.ms_upload = std::max(0.0, ms_since(t0) - info.inflate.ms_size);
        } else {
            info.source = 2;
            info.inflate.fell_back = 1;
            mi_inflater_free(inf.d);                    // the member leaves the device: the tar needs the room
            inf.d = nullptr;
            if (!zlib_inflate(src, n, &host_tar)) return fail(c, MI_ERR_INVALID, "mi_batch_add_layer_blob: corrupt gzip stream");
            T = host_tar.size();
            src = host_tar.data();
            t0 = std::chrono::steady_clock::now();
        }
    }
    // room behind what the arena holds, as mi_batch_add_recipes asks for it; nothing of the batch changes yet
    const u64 at = (b->arena_used + kFileAlign - 1) / kFileAlign * kFileAlign;
    const u64 end_aligned = at + (T + kFileAlign - 1) / kFileAlign * kFileAlign;
    rc = mi_batch_arena_reserve(b, end_aligned);
    if (rc) return rc;
    rc = arena_wait_mapped(c, &b->arena, std::min<u64>(b->arena.bytes, end_aligned + 4096));   // a walk-fed arena is mapped piece by piece
    if (rc) return rc;
    u8* d_tar = b->arena.as<u8>() + at;
    if (info.source == 1 || info.source == 3 || info.source == 4) {
        rc = mi_inflater_run_device(inf.d, d_tar, nullptr);
        mi_inflater_info(inf.d, &info.inflate);
        if (rc == 1 && with_index) {                    // a verdict: what the spans wrote lies behind arena_used, where nothing counts
            fell_back = info.inflate.verdict == MI_INFLATE_INDEX_REFUSED ? 2 : 0;
            continue;
        }
        if (rc) return fail(c, rc, "mi_batch_add_layer_blob: %s", mi_inflater_error(inf.d));
    } else {
        rc = upload_plain(c, d_tar, src, T, info.source == 0 && blob_sha256 ? &sha : nullptr);
        if (rc) return rc;
        info.ms_upload = ms_since(t0);
    }
    // the header pass where the tar lies, and the listing through what came down
    t0 = std::chrono::steady_clock::now();
    TarScan scan;
    HIPCHK(c, tar_scan(d_tar, T, c->stream, &scan));
    Fetch fetch{c, d_tar};
    mi_tar* tar = nullptr;
    u64 counts[4] = {0, 0, 0, 0};
    char err[512] = "";
    rc = mi_tar_open_device(T, scan.blocks.data(), scan.kinds.data(), scan.dense.data(), scan.blocks.size(), fetch_from_device, &fetch, &tar, counts,
                            err, sizeof err);
    if (rc) return fail(c, rc, "mi_batch_add_layer_blob: %s", err);
    const u64 n_entries = counts[3];
    std::vector<mi_tree_entry> ents((size_t)n_entries);
    std::vector<u64> offs((size_t)n_entries);
    rc = mi_tar_entries(tar, ents.data(), offs.data(), n_entries);
    if (rc) { mi_tar_free(tar); return fail(c, rc, "mi_batch_add_layer_blob: mi_tar_entries failed"); }
    u64 n_files = 0, bytes = 0;
    for (u64 i = 0; i < n_entries; ++i) {
        if (ents[i].kind != 1) continue;
        if (ents[i].size > T || offs[i] > T - ents[i].size) {   // (the parser's has_range said so already)
            mi_tar_free(tar);
            return fail(c, MI_ERR_INVALID, "mi_batch_add_layer_blob: a member lies outside its archive");
        }
        ++n_files;
        bytes += ents[i].size;
    }
    info.ms_headers = ms_since(t0);
    // the bytes lie in the arena and the listing stands: now the batch changes
    info.tar_bytes = T;
    info.arena_at = at;
    info.first_file = b->files.size();
    info.n_files = n_files;
    info.n_entries = n_entries;
    info.n_marked = scan.blocks.size();
    info.n_live = counts[0];
    info.n_fetched = counts[1];
    info.fetched_bytes = counts[2];
    b->files.reserve(b->files.size() + n_files);
    for (u64 i = 0; i < n_entries; ++i)
        if (ents[i].kind == 1) b->files.push_back({at + offs[i], ents[i].size, tag_base + (u64)ents[i].file_index});
    b->arena_used = at + T;
    b->total_bytes += bytes;
    if (fell_back) info.inflate.fell_back = fell_back;
    if (blob_sha256) sha.final(blob_sha256);
    if (info_out) *info_out = info;
    if (listing) *listing = tar; else mi_tar_free(tar);
    return MI_OK;
    }
}

int add_layer_path(mi_batch* b, const char* blob_path, const u8* index, u64 index_bytes, uint64_t tag_base, mi_tar** listing, uint8_t* blob_sha256,
                   mi_layer_blob_info* info, const InfSpecAsk* spec = nullptr);

}  // namespace

extern "C" {

int mi_batch_add_layer_blob(mi_batch* b, const void* blob, uint64_t n, uint64_t tag_base, mi_tar** listing, uint8_t* blob_sha256,
                            mi_layer_blob_info* info_out) {
    return add_layer_blob(b, blob, n, nullptr, 0, tag_base, listing, blob_sha256, info_out);
}

int mi_batch_add_layer_blob_indexed(mi_batch* b, const void* blob, uint64_t n, const void* index, uint64_t index_bytes, uint64_t tag_base,
                                    mi_tar** listing, uint8_t* blob_sha256, mi_layer_blob_info* info_out) {
    if (!index) { if (listing) *listing = nullptr; if (info_out) memset(info_out, 0, sizeof *info_out); return MI_ERR_INVALID; }
    return add_layer_blob(b, blob, n, (const u8*)index, index_bytes, tag_base, listing, blob_sha256, info_out);
}

int mi_batch_add_layer_path_indexed(mi_batch* b, const char* blob_path, const void* index, uint64_t index_bytes, uint64_t tag_base, mi_tar** listing,
                                    uint8_t* blob_sha256, mi_layer_blob_info* info) {
    if (!index) { if (listing) *listing = nullptr; if (info) memset(info, 0, sizeof *info); return MI_ERR_INVALID; }
    return add_layer_path(b, blob_path, (const u8*)index, index_bytes, tag_base, listing, blob_sha256, info);
}

int mi_batch_add_layer_path(mi_batch* b, const char* blob_path, uint64_t tag_base, mi_tar** listing, uint8_t* blob_sha256,
                            mi_layer_blob_info* info) {
    return add_layer_path(b, blob_path, nullptr, 0, tag_base, listing, blob_sha256, info);
}

int mi_batch_add_layer_blob_spec(mi_batch* b, const void* blob, uint64_t n, uint64_t piece_bytes, uint64_t tag_base, mi_tar** listing,
                                 uint8_t* blob_sha256, mi_layer_blob_info* info_out, mi_inflate_spec_info* spec_info) {
    if (spec_info) memset(spec_info, 0, sizeof *spec_info);
    const InfSpecAsk ask = {piece_bytes, spec_info, nullptr, nullptr};
    return add_layer_blob(b, blob, n, nullptr, 0, tag_base, listing, blob_sha256, info_out, &ask);
}

int mi_batch_add_layer_path_spec(mi_batch* b, const char* blob_path, uint64_t piece_bytes, uint64_t tag_base, mi_tar** listing, uint8_t* blob_sha256,
                                 mi_layer_blob_info* info, mi_inflate_spec_info* spec_info) {
    if (spec_info) memset(spec_info, 0, sizeof *spec_info);
    const InfSpecAsk ask = {piece_bytes, spec_info, nullptr, nullptr};
    return add_layer_path(b, blob_path, nullptr, 0, tag_base, listing, blob_sha256, info, &ask);
}

}  // extern "C"

namespace {

int add_layer_path(mi_batch* b, const char* blob_path, const u8* index, u64 index_bytes, uint64_t tag_base, mi_tar** listing, uint8_t* blob_sha256,
                   mi_layer_blob_info* info, const InfSpecAsk* spec) {
    if (listing) *listing = nullptr;
    if (info) memset(info, 0, sizeof *info);
    if (!b || !blob_path) return MI_ERR_INVALID;
    mi_ctx* c = b->ctx;
    const int fd = open(blob_path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return fail(c, MI_ERR_IO, "mi_batch_add_layer_path: open %s: %s", blob_path, strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0) { const int e = errno; close(fd); return fail(c, MI_ERR_IO, "mi_batch_add_layer_path: stat %s: %s", blob_path, strerror(e)); }
    const u64 n = (u64)st.st_size;
    void* map = n ? mmap(nullptr, (size_t)n, PROT_READ, MAP_PRIVATE, fd, 0) : (void*)"";
    const int map_errno = errno;
    close(fd);
    if (map == MAP_FAILED) return fail(c, MI_ERR_IO, "mi_batch_add_layer_path: mmap %s: %s", blob_path, strerror(map_errno));
    const int rc = add_layer_blob(b, map, n, index, index_bytes, tag_base, listing, blob_sha256, info, spec);
    if (n) munmap(map, (size_t)n);
    return rc;
}

}  // namespace
