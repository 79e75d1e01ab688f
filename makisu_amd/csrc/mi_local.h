// mi_local.h -- the library's own cross-file helpers: C linkage (the translation units name them without sharing C++
// headers), HIDDEN visibility -- they are not part of the ABI and `nm -D libmakisu_mi.so` does not list them
// (tests/test_abi.py: the library exports what the two public headers declare and nothing else).
#pragma once
#include "../../include/makisu_mi.h"

#include <string>

#define MI_LOCAL __attribute__((visibility("hidden")))

namespace mi {
// 32 bytes as 64 lower-case hex digits: a digest in a message, the halves of a cache entry
inline std::string hex32(const uint8_t* d) {
    static const char* dig = "0123456789abcdef";
    std::string out(64, '0');
    for (int i = 0; i < 32; ++i) { out[2 * i] = dig[d[i] >> 4]; out[2 * i + 1] = dig[d[i] & 15]; }
    return out;
}
}  // namespace mi

extern "C" {
// mi_api.hip (what reads staged bytes back -- _read_file_landed, _read_stats, _chunk_sum, the windows, _explain_chunk: mi_readback.hip)
MI_LOCAL void        mi_set_error(mi_batch* b, const char* msg);     // b NULL: the message mi_last_error(NULL) returns
MI_LOCAL void**      mi_batch_tree_slot(mi_batch* b);                // the batch's walk record (mi_tree.hip owns its type)
MI_LOCAL int         mi_batch_file_size(mi_batch* b, uint64_t file_index, uint64_t* size);
MI_LOCAL const char* mi_last_error_of_batch(mi_batch* b);
// what the batch's arena holds now (bytes allocated): the room a window of an oversize tree can count on
MI_LOCAL int         mi_batch_arena_room(mi_batch* b, uint64_t* bytes);
// device memory behind the arena now, in how many pieces (1: one allocation), and how often its base address has changed
MI_LOCAL int         mi_batch_arena_info(mi_batch* b, uint64_t* bytes, uint64_t* pieces, uint64_t* moves);
// mi_batch_read_file for the pipelined commit: the batch is still being staged / scanned on another thread; the call waits
// until the bytes it is asked for have landed in HBM
MI_LOCAL int         mi_batch_read_file_landed(mi_batch* b, uint64_t file_index, uint64_t offset, void* dst, uint64_t len);
// MI_LAYER_TIMING: what the window behind mi_batch_read_file* did so far (seconds waiting for bytes to land, seconds in its copies)
MI_LOCAL void        mi_batch_read_stats(mi_batch* b, double* wait_s, double* fetch_s, uint64_t* fetches, uint64_t* bytes);
// mi_layer.hip: from now on mi_layer_add_batch_file reads through mi_batch_read_file_landed
MI_LOCAL void        mi_layer_set_pipelined(mi_layer* layer, int on);
// what the layer held against source sums so far: files, their bytes, chunks that were right only at the second fetch
MI_LOCAL void        mi_layer_verify_counts(mi_layer* layer, uint64_t* files, uint64_t* bytes, uint64_t* refetched);
// the walk's small files read in place: a block of host memory as one piece of the arena, and the table rows of files
// that lie in it; "host-fed bytes are on their way" (the reader threads set up behind the walk's first directories)
MI_LOCAL int  mi_batch_add_block(mi_batch* b, const void* src, uint64_t len, void (*release)(void*), void* release_arg,
                                 uint64_t* at_out);
MI_LOCAL int  mi_batch_add_placed(mi_batch* b, uint64_t n, const uint64_t* arena_off, const uint64_t* sizes,
                                  const uint64_t* tags, const uint64_t* sums);
// the end-to-end byte sums (mi_filesum.h): does the batch keep them (MI_FLAG_FILE_SUMS; a MemFS handle's batch always does --
// mi_batch_keep_sums, before its first file); the sums of chunk k (1 MiB of the file) of a row (*has = 0: none kept); forget what the
// read-back windows hold (the next read fetches again); which hop lost a chunk (a line for the error message)
MI_LOCAL int  mi_batch_keeps_sums(mi_batch* b);
MI_LOCAL void mi_batch_keep_sums(mi_batch* b, int on);
MI_LOCAL int  mi_batch_chunk_sum(mi_batch* b, uint64_t file_index, uint64_t chunk, uint64_t* sum_a, uint64_t* sum_b, int* has);
MI_LOCAL void mi_batch_drop_windows(mi_batch* b);
MI_LOCAL int  mi_batch_prepare_read(mi_batch* b);      // the read-back windows now, not at the tar writer's first read
MI_LOCAL int  mi_batch_explain_chunk(mi_batch* b, uint64_t file_index, uint64_t chunk, char* msg, uint64_t cap);
MI_LOCAL void mi_batch_expect_host_bytes(mi_batch* b);
// mi_deflate.hip -- the device deflate coder behind the layer writer's gzip leg and mi_deflate_buffer: windows of the stream, two
// in flight.  room: the pinned window to fill (NULL: no memory; the message is _error's); push: its first n bytes are coded --
// and the window pushed BEFORE it comes out through emit (the compressed bytes, their count, the window's CRC-32 and length);
// flush: what is still in flight comes out, in order.  One thread drives a deflater.  window: a multiple of 65 536
struct mi_deflater;
typedef int (*mi_deflate_emit_fn)(void* arg, const uint8_t* bytes, uint64_t n_out, uint32_t crc, uint64_t n_in);
MI_LOCAL int         mi_deflater_create(mi_ctx* ctx, uint64_t window_bytes, mi_deflater** out);
MI_LOCAL uint64_t    mi_deflater_window(const mi_deflater* d);
MI_LOCAL uint8_t*    mi_deflater_room(mi_deflater* d);
MI_LOCAL int         mi_deflater_push(mi_deflater* d, uint64_t n, mi_deflate_emit_fn emit, void* arg);
MI_LOCAL int         mi_deflater_flush(mi_deflater* d, mi_deflate_emit_fn emit, void* arg);
MI_LOCAL const char* mi_deflater_error(const mi_deflater* d);
MI_LOCAL void        mi_deflater_info(const mi_deflater* d, mi_deflate_info* out);
MI_LOCAL void        mi_deflater_free(mi_deflater* d);
MI_LOCAL uint64_t    mi_deflate_device_window(void);          // MI_GZIP_DEVICE_WINDOW_MB (1..1024), default 32
// mi_inflate.hip -- the device inflate behind mi_inflate_buffer and mi_tar_inflate_ctx.  plan: the member gz[0, n) goes
// up whole (`seen`, may be NULL, is told every piece of it in order while it is under way: the blob's digest), the candidates are
// marked, the size pass leaves its rows and the host walks the chain -- MI_OK with _info's verdict (DONE: out_bytes, n_rounds; NOT_PARALLEL:
// the segment and the rule), MI_ERR_INVALID for a corrupt member (the message is _error's).  run, after a plan that said DONE: the
// rounds come out through emit in order, two in flight, and the CRC-32 and ISIZE are held against the trailer at the end
// (MI_ERR_INVALID).  One thread drives an inflater; the ctx stays usable after any failure.  Window: MI_INFLATE_WINDOW_MB (1..1024), 64
struct mi_inflater;
typedef void (*mi_inflate_seen_fn)(void* arg, const uint8_t* bytes, uint64_t n);
typedef int (*mi_inflate_emit_fn)(void* arg, const uint8_t* bytes, uint64_t n);
MI_LOCAL int         mi_inflater_create(mi_ctx* ctx, mi_inflater** out);
MI_LOCAL int         mi_inflater_plan(mi_inflater* d, const uint8_t* gz, uint64_t n, mi_inflate_seen_fn seen, void* arg);
MI_LOCAL int         mi_inflater_run(mi_inflater* d, mi_inflate_emit_fn emit, void* arg);
MI_LOCAL const char* mi_inflater_error(const mi_inflater* d);
MI_LOCAL void        mi_inflater_info(const mi_inflater* d, mi_inflate_info* out);
MI_LOCAL void        mi_inflater_free(mi_inflater* d);
// run with a DEVICE destination: the member's inflation goes to d_dst[0, out_bytes) -- each round is decoded where it
// belongs there, its CRC-32 taken over that range, and only the CRC and the bad word come down; CRC and ISIZE are held against the
// trailer as in _run, with the same messages.  wait_for (may be NULL): the stream on which d_dst was made ready.  The bytes lie
// there when the call returns
typedef struct ihipStream_t* hipStream_t;
MI_LOCAL int         mi_inflater_run_device(mi_inflater* d, uint8_t* d_dst, hipStream_t wait_for);
// mi_inflate_index.hip -- the plan from an index of checkpoints instead of a size pass: the index is checked on the host,
// the member and the window area go up, the spans are cut into rounds.  MI_OK with _info's verdict: DONE; NOT_PARALLEL (a span larger
// than the window); MI_INFLATE_INDEX_REFUSED (the checker's number in info.reserved).  After DONE, _run and _run_device decode the spans;
// they return 1 -- not an error: _info's verdict is then INDEX_REFUSED (a span broke a rule -- info names it --, or the trailer does not
// hold) or NOT_PARALLEL (the last span ends before n - 8) and the caller inflates without the index
MI_LOCAL int         mi_inflater_plan_indexed(mi_inflater* d, const uint8_t* gz, uint64_t n, const uint8_t* index, uint64_t index_bytes,
                                              mi_inflate_seen_fn seen, void* arg);
// mi_inflate_spec.hip -- the plan from SPECULATIVE SPANS: no index is given, the span table and the window area are made on
// the device from the member alone (piece_bytes: 0 or 1 024 .. 16 777 216, else MI_ERR_INVALID).  MI_OK with _info's verdict: DONE (an
// indexed plan: _run and _run_device as above, a refusal there is INDEX_REFUSED); NOT_PARALLEL (a span beyond the window or the symbol
// cap, more members).  A broken rule on a live span is MI_ERR_INVALID naming the span, the rule and the bit.  _spec_info: the pieces,
// the candidates found, the live spans, the three passes' device times
MI_LOCAL int         mi_inflater_plan_spec(mi_inflater* d, const uint8_t* gz, uint64_t n, uint64_t piece_bytes, mi_inflate_seen_fn seen, void* arg);
MI_LOCAL void        mi_inflater_spec_info(const mi_inflater* d, mi_inflate_spec_info* out);
// mi_inflate.hip -- mi_tar_inflate_ctx's body; index (may be NULL): mi_tar_inflate_ctx_indexed's
MI_LOCAL int         mi_tar_inflate_ctx_with(mi_ctx* ctx, const char* blob_path, const uint8_t* index, uint64_t index_bytes, const char* tar_path_out,
                                             uint64_t* tar_bytes, uint8_t* tar_sha256, uint8_t* blob_sha256, mi_inflate_info* info, char* err,
                                             uint64_t err_cap);
// mi_tar.hip -- an mi_tar from a tar of tar_bytes that lies on the device: blocks / kinds / dense are what
// mi_tarscan.hip brought down (n_marked of them; host_tarcache.h), fetch copies tar[off, off + n) to dst for what the cache does
// not hold (MI_OK, or the listing fails with MI_ERR_IO).  The parser, its errors and its texts are mi_tar_open_ex's (err: the
// text without a path).  counts (may be NULL; four words): headers served from the cache as header candidates, fetches, fetched bytes, entries.
// mi_tar_entries and mi_tar_free work on *out as on any other
typedef int (*mi_tar_fetch_fn)(void* arg, uint64_t off, void* dst, uint64_t n);
MI_LOCAL int         mi_tar_open_device(uint64_t tar_bytes, const uint64_t* blocks, const uint8_t* kinds, const uint8_t* dense, uint64_t n_marked,
                                        mi_tar_fetch_fn fetch, void* fetch_arg, mi_tar** out, uint64_t* counts, char* err, uint64_t err_cap);
// mi_batch_reserve for a walk whose enumeration runs ahead of what it hands over (and for mi_memfs_reserve_device): the arena
// is the piecewise kind (mi_arena.hip) -- what is coming is known roughly and keeps growing
MI_LOCAL int  mi_batch_reserve_ahead(mi_batch* b, uint64_t more_files, uint64_t more_bytes);
// mi_group.hip -- one handle over n batches, one per ctx: what a walk hands over is spread by bytes, the commit sees one batch;
// the members and their loads (n = 0: not a group)
MI_LOCAL int  mi_batch_group_begin(mi_ctx* const* ctxs, uint32_t n, mi_batch** out);
MI_LOCAL uint64_t mi_batch_group_splits(mi_batch* b);      // files of the group that are split over its members as parts
MI_LOCAL int  mi_batch_group_members(mi_batch* b, mi_batch* const** members, const uint64_t** bytes, uint64_t* n);
// mi_api.hip -- job-wide marking of a rank's own rows, enqueued on the ctx stream; the first-occurrence count stays in
// ctx->dd_nuniq (device).  For mi_comm.hip
MI_LOCAL int  mi_dedup_mark_range_enqueue(mi_ctx* c, const void* d_digests, uint64_t n_total, uint64_t own_first,
                                          uint64_t own_n, void* d_dup_of_own);
// mi_index.hip: mi_index_add_batch for digests in host memory (a batch of another GPU than the index's)
MI_LOCAL int  mi_index_add_digests(mi_index* index, const void* digests, uint64_t n, uint8_t* known_out, uint64_t* n_new, uint64_t* n_known);
MI_LOCAL int  mi_index_same_ctx(mi_index* index, mi_batch* b);
MI_LOCAL mi_ctx* mi_index_ctx(mi_index* index);   /* whose algorithm its digests are of (mi_ctx_chunk_digest) */
// mi_tree.hip
MI_LOCAL void mi_batch_tree_free(void* tree);
// mi_pack.hip: a valid pack of nothing (a commit with the pack option that scanned no file has no batch that ran)
MI_LOCAL int  mi_pack_empty(mi_ctx* ctx, mi_pack** out);
// ... and the ctx a pack points at (mi_restore.hip: a set takes packs of its own ctx only)
MI_LOCAL mi_ctx* mi_pack_ctx(const mi_pack* p);
// mi_pack.hip, for mi_fetch.hip: a pack of n_entries (> 0) rows and a blob of blob_bytes whose contents the CALLER writes on the ctx
// stream -- *d_blob is device memory of the pack's own (exactly blob_bytes + the slack; does not fit: MI_ERR_NOMEM naming both
// sizes under `who`, no pack), *h_rows the n_entries rows mi_pack_entries hands out; mi_pack_free on any later failure.  Then what the
// caller found out about it (mi_pack_info's other fields)
MI_LOCAL int  mi_pack_alloc(mi_ctx* ctx, const char* who, uint64_t n_entries, uint64_t blob_bytes, uint64_t chunk_bytes, mi_pack** out,
                            void** d_blob, mi_pack_entry** h_rows);
MI_LOCAL void mi_pack_set_result(mi_pack* p, uint32_t verified, double ms_gather, double ms_verify);
// mi_restore.hip, for mi_fetch.hip: the set's ctx and its table as it is now (cap slots, a power of two; tags 8 bytes a slot, slots
// six words: digest 4 | the chunk's device address | its length).  MI_ERR_STATE under `who` with the first message for a set
// in its sticky failed state, MI_ERR_INVALID for NULL
MI_LOCAL int  mi_packset_table(const mi_packset* s, const char* who, mi_ctx** ctx, const uint64_t** tags, const uint64_t** slots,
                               uint64_t* cap);
// mi_restore.hip, for mi_zpack.hip: `bytes` of host memory up to d_dst through the set's two pinned windows (blocking; *ms: how
// long it took); and a PLAIN blob that lies on the device already -- blob: a mi::DevBuf of exactly blob_bytes + the slack, which
// the set takes over (NULL with n = 0); entries: on the host, structurally sound -- added as mi_packset_add_blob adds one behind
// its upload: MI_PACKSET_VERIFY, the table, the counters; until the insert begins every failure leaves the set as it was
MI_LOCAL int  mi_packset_upload(mi_packset* s, void* d_dst, const void* src, uint64_t bytes, double* ms);
MI_LOCAL int  mi_packset_adopt(mi_packset* s, const char* who, void* blob, uint64_t blob_bytes, const mi_pack_entry* entries, uint64_t n,
                               uint32_t flags, double ms_upload, uint64_t* first_bad);
// mi_zpack.hip, for mi_zset.hip.  The structural host check of a compressed add under `who` (MI_ERR_INVALID, *first_bad, the
// message of mi_packset_add_zblob).  The decoding half of such an add: the compressed blob lies on the device, the entries on
// the host, structurally sound, n > 0; plain_buf is a mi::DevBuf that receives the plain blob laid out as a pack's (exactly
// *plain_bytes + the slack), plain[n] its entries; *bad = the smallest entry that breaks a decoding rule or has a non-zero pad
// (~0: none) and *rule which one (mi_host::Lz4Rule) -- the caller words the refusal; ms_decode (may be NULL): the kernel's
// time.  Blocking on the ctx stream; the plain blob does not fit: MI_ERR_NOMEM naming both sizes under `who`
MI_LOCAL int  mi_zpack_structure(mi_ctx* ctx, const char* who, uint64_t blob_bytes, const mi_zpack_entry* entries, uint64_t n,
                                 uint64_t* first_bad);
MI_LOCAL int  mi_zpack_decode_plain(mi_ctx* ctx, const char* who, const void* d_zblob, const mi_zpack_entry* entries, uint64_t n,
                                    void* plain_buf, uint64_t* plain_bytes, mi_pack_entry* plain, uint64_t* bad, uint32_t* rule,
                                    double* ms_decode);
// a zpack of n_entries rows and a blob of blob_bytes whose contents the CALLER writes on the ctx stream (mi_pack_alloc's
// contract; n_entries = 0: the empty zpack, no blob), what the caller found out about it (ms_encode is 0: nothing was coded),
// and a zpack where it lies: its ctx, its blob on the device and its rows on the host
MI_LOCAL int  mi_zpack_alloc(mi_ctx* ctx, const char* who, uint64_t n_entries, uint64_t blob_bytes, mi_zpack** out, void** d_blob,
                             mi_zpack_entry** h_rows);
MI_LOCAL void mi_zpack_set_result(mi_zpack* z, uint64_t stored_bytes, uint64_t n_raw, uint64_t chunk_bytes, uint32_t verified,
                                  double ms_compact, double ms_verify, double ms_decode);
MI_LOCAL int  mi_zpack_device(const mi_zpack* z, mi_ctx** ctx, const void** d_blob, uint64_t* blob_bytes, const mi_zpack_entry** rows,
                              uint64_t* n);
// mi_zpack.hip, for mi_zbatch.hip (a zpack coded straight from a batch's arena): the decode kernel ENQUEUED on the ctx stream,
// nothing allocated, nothing waited for -- d_rows: the zpack's entries on the device, d_poff[k]: where entry k's plain bytes go
// in d_out (round16(length) bytes each are written), d_rule[k]: 0 or the rule that refuses it, *d_first_bad: atomicMin of the
// refused entries; and the coder's time, which mi_zpack_set_result leaves 0
MI_LOCAL int  mi_zpack_decode_enqueue(mi_ctx* ctx, const void* d_zblob, const uint64_t* d_rows, const uint64_t* d_poff, uint64_t n,
                                      void* d_out, uint32_t* d_rule, uint64_t* d_first_bad);
MI_LOCAL void mi_zpack_set_encode_ms(mi_zpack* z, double ms_encode);
// mi_zpack2.hip, for mi_zpack.hip and mi_zbatch.hip (MI_ZPACK_LEVEL2): the level-2 encode kernel ENQUEUED on the ctx stream in
// place of the caller's level-1 kernel, with that kernel's arguments -- d_base: the pack's blob or the batch's arena, d_rows[k]'s
// offset word the chunk's offset from it -- over `waves` workgroups of one wave
MI_LOCAL int  mi_zencode_l2_enqueue(mi_ctx* ctx, const void* d_base, uint64_t* d_rows, const uint64_t* d_woff, void* d_scratch, uint64_t n,
                                    uint32_t waves);
// mi_zset.hip, for mi_zbatch.hip (mi_zset_missing): the set's ctx -- MI_ERR_STATE under `who` with the first message for a set in
// its sticky failed state, MI_ERR_INVALID for NULL -- and zset_lookup_kernel ENQUEUED on the ctx stream over n digests on the
// device: d_src[r] / d_word[r] = where the set holds row r's stored span and its length | stored << 32 (0, 0: not held),
// d_len64[r] the set's length, *d_first_bad as the kernel states it (d_lengths may be NULL)
MI_LOCAL int  mi_zset_ctx(const mi_zset* s, const char* who, mi_ctx** ctx);
MI_LOCAL int  mi_zset_lookup_enqueue(const mi_zset* s, const uint8_t* d_digests, const uint32_t* d_lengths, uint64_t n, uint64_t* d_src,
                                     uint64_t* d_word, uint64_t* d_len64, uint64_t* d_first_bad);
// mi_api.hip, for mi_restore.hip: room in the batch's arena up to offset `end` (arena_reserve, as mi_batch_add_synthetic asks for
// it: what the arena holds stays, whichever kind it is)
MI_LOCAL int  mi_batch_arena_reserve(mi_batch* b, uint64_t end);
}
