/*
 * makisu_mi.h -- C ABI of libmakisu_mi.so, the MI355X (gfx950) layer-snapshot
 * content-scan and dedup engine for uber/makisu.
 *
 * The reference has no cgo/FFI today; this header is the
 * boundary a ~100-line cgo shim in lib/snapshot would bind (INTEGRATION.md shows
 * it).  Each entry point cites the reference seam it serves (paths relative to
 * the makisu tree).  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions (mirror Go's "wrap the error with context" style):
 *   - every function returns int: 0 = MI_OK, <0 = error code;
 *   - mi_last_error(ctx) returns a NUL-terminated message -- the calling thread's own copy, valid until
 *     that thread asks again -- so the shim can do fmt.Errorf("gpu scan: %s", C.GoString(..));
 *   - a ctx is not re-entrant but may be called from any OS thread (the engine
 *     calls hipSetDevice itself and keeps no thread-local state -- goroutines
 *     migrate between threads); several ctxs may run concurrently;
 *   - the engine never retains caller memory after a call returns (cgo pointer
 *     rule): mi_batch_add_bytes copies before returning;
 *   - no callbacks, no exceptions/longjmp across the boundary.
 *   - there is NO CPU fallback: if no gfx950 device is usable, mi_ctx_create
 *     fails with MI_ERR_NO_DEVICE.
 */
#ifndef MAKISU_MI_H
#define MAKISU_MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ABI_VERSION 6

/* ---- THREE KINDS OF EXPORT (round 6) ------------------------------------------------------------------------------------- *
 * Every prototype below carries one of three (empty) tags; tests/test_abi.py checks that each export has exactly one, and
 * tests/test_integration_shim.py that the cgo shim of INTEGRATION.md binds CORE calls only.
 *
 * MI_CORE   what a first cgo shim in lib/snapshot binds -- the seam as the reference has it (about thirty calls):
 *             ctx        mi_abi_version, mi_config_default, mi_ctx_create / _destroy, mi_last_error
 *             MemFS      mi_memfs_create / _free / _error / _set_clock / _reset / _update_from_entries / _entries / _root_of
 *             commit     mi_memfs_commit_layer (step.commitLayer in one call: walk, GPU scan, content-aware diff, tar from HBM,
 *                        DigestPair), mi_memfs_commit_layer_n (the same over several GPUs), mi_memfs_commit_stats, mi_memfs_set_options / _set_index / _reserve_device /
 *                        _release_device, mi_layer_config_default, mi_copy_layer_entries / _roots / _free
 *             cache      mi_cache_key / _create_entry / _parse_entry / _parse_entry_str   (cache.Manager's strings)
 *             index      mi_index_create / _free / _count / _export / _import               (keyvalue.Store seam)
 *             push       mi_sha256_many                                                     (image.Digester, batched)
 * MI_BLOCK  the building blocks the commit is made of, for a host that wants to arrange them itself (batches and their
 *           results, parts of large files, the RCCL exchange, tree walks, the tar reader and the layer writer, the stateless
 *           forms of the diff, the context checksum): everything INTEGRATION.md's later sections use.
 * MI_DIAG   measurement and diagnosis (stats, roofs, staging counters, wave records): no product flow depends on them.      */
#define MI_CORE
#define MI_BLOCK
#define MI_DIAG

enum {
    MI_OK = 0,
    MI_ERR_INVALID = -1,     /* bad argument / bad state                         */
    MI_ERR_NO_DEVICE = -2,   /* no usable gfx950 device (there is no CPU path)   */
    MI_ERR_HIP = -3,         /* a HIP runtime call failed (message has detail)   */
    MI_ERR_NOMEM = -4,       /* host or device allocation failed                 */
    MI_ERR_IO = -5,          /* open/pread of a path failed (mi_batch_add_path)  */
    MI_ERR_STATE = -6,       /* call out of order (e.g. results before run)      */
    MI_ERR_CAPACITY = -7     /* caller buffer too small                          */
};

/* mi_config.flags */
#define MI_FLAG_FILE_SHA256 0x1u  /* also compute SHA-256 of each whole file: what
                                     image.Digester.FromReader returns per file in
                                     `makisu push` (bin/makisu/cmd/push.go:207,230;
                                     lib/docker/image/digester.go:45-52).  One GPU lane per
                                     file -- 13.5 MB/s a lane, 1.77 TB/s when every lane has
                                     one -- EXCEPT files that would hold the pass up: a single
                                     SHA-256 stream is serial and belongs
                                     on a host core with SHA-NI (2.4 GB/s); such files are hashed
                                     by the library's reader threads out of HBM while the GPU
                                     takes the rest (csrc/mi_stage.hip route_long_strings: the
                                     length classes that make max(host time, GPU time) smallest;
                                     a 128 MiB file 0.06 s instead of 10 s).  Not a fallback: the
                                     same digests, each where it is computed fastest          */
#define MI_FLAG_FILE_CRC32  0x2u  /* also compute CRC32-IEEE of each whole file: the
                                     per-file term of checksumPathContents
                                     (lib/builder/step/add_copy_step.go:194-238)     */
#define MI_FLAG_NO_DEDUP    0x4u  /* skip in-batch duplicate marking                 */
#define MI_FLAG_PREFETCH_ROWS 0x8u /* mi_batch_wait also brings the result rows to the host
                                      (one packed copy, ~1 ms per 700 k chunks, while the
                                      other batch in flight keeps the GPU busy): the
                                      following mi_batch_chunks_view is a pointer.  The steps
                                      with the rows delivered run 0.5-2.2 % below the steps
                                      without (once 5.8 %: profiles/r05_with_rows_repeats.txt,
                                      `with_rows_on_host` in every bench line)             */
#define MI_FLAG_VERIFY_STAGING 0x10u /* host-fed batches check their own staged bytes: every
                                      span a reader thread (or the inline window) copies is
                                      summed on the host while it sits in the pinned slab and
                                      summed again on the GPU where it landed -- right after the
                                      copy and once more, every span of the batch, when staging
                                      ends (after any arena growth).  A span that differs is
                                      copied again from the slab; one that still differs, or
                                      differs at the end, fails the run with MI_ERR_IO naming
                                      the arena range, the reader thread and what the GPU holds
                                      there.  io.CopyN must deliver exactly the file's bytes
                                      (lib/tario/write.go:43-45).  New arena memory is filled
                                      with 0xA5 first, so a byte that never arrived does not
                                      read as a plausible zero.  Counters: mi_batch_stage_stats */
#define MI_FLAG_FILE_SUMS 0x20u     /* every host-fed file of a batch carries 128-bit sums of its
                                      bytes, per 1 MiB of the file, taken WHERE THE BYTES WERE READ
                                      (the reader thread's pinned slab right after its pread, the
                                      caller's buffer for mi_batch_add_bytes); mi_layer_add_batch_file
                                      takes the same sums over the bytes it is about to frame and
                                      accepts them only if equal: a chunk that differs is fetched from
                                      HBM once more, one that still differs fails the layer with
                                      MI_ERR_IO naming the file, the arena range and the hop (the
                                      bytes made two PCIe crossings; io.CopyN, lib/tario/write.go:
                                      43-45, hands over the bytes read() returned or an error).
                                      mi_memfs_commit_layer keeps these sums whatever the ctx's
                                      flags say (MI_COMMIT_VERIFY=0 in the environment: off, for
                                      measurements).  About 0.06 ns per byte on each side -- beside a
                                      2.45 GB/s SHA-256 stream.  The heavier MI_FLAG_VERIFY_STAGING
                                      checks every staged span on the GPU itself: a diagnosis tool */
#define MI_FLAG_CHUNK_BLAKE2S 0x40u /* chunk digests and chunk roots of this ctx are BLAKE2s-256 (RFC 7693:
                                      unkeyed, no salt, no personalisation, sequential mode; Python's
                                      hashlib.blake2s(b).digest(); the empty string is one all-zero block
                                      with t = 0 and the final flag) instead of SHA-256.  Both are keys of
                                      THIS engine -- dedup, the chunk index, "did this file's content
                                      change" -- and nothing Docker sees; what Docker sees stays SHA-256:
                                      MI_FLAG_FILE_SHA256, mi_sha256_many, the layer writer's TarDigest and
                                      gzip digest, the cache entry codec.  The chunk root is the same tree
                                      (mi_chunk_root_alg) with BLAKE2s-256 at every node.  Cut points, the
                                      rows, the dedup keys (a digest's first 8 bytes), the exchange do not
                                      change.  The algorithm BELONGS to whatever keeps digests or roots
                                      between batches: a chunk index, a MemFS handle, the ranks of an
                                      exchange, an exported index blob -- see each of them.  Fewer VALU
                                      instructions per block than SHA-256              */
/* a ctx's chunk digest algorithm (mi_ctx_chunk_digest, mi_chunk_root_alg) */
#define MI_DIGEST_SHA256  0u
#define MI_DIGEST_BLAKE2S 1u

typedef struct mi_ctx mi_ctx;
typedef struct mi_batch mi_batch;

/* Gear-CDC parameters + engine resources.  The reference has no CDC; the spec is
 * DESIGN.md "Gear-CDC spec".  Defaults (mi_config_default): seed 0x4D414B49,
 * mask_bits 13 (8 KiB mean gap), min 2 KiB, max 64 KiB. */
typedef struct {
    uint32_t struct_size;     /* sizeof(mi_config), for ABI evolution              */
    int32_t  device;          /* HIP device ordinal                                 */
    uint64_t gear_seed;       /* Gear table = first 256 outputs of splitmix64(seed) */
    uint32_t mask_bits;       /* 0..32: candidate iff top mask_bits bits of h == 0  */
    uint32_t min_size;        /* >= 64                                              */
    uint32_t max_size;        /* >= min_size, <= 2^30                               */
    uint32_t flags;           /* MI_FLAG_*                                          */
    uint64_t staging_bytes;   /* bytes per pinned staging slab (0 = 8 MiB)          */
    uint32_t n_streams;       /* reader threads for host-fed batches, one pinned slab
                                 and one copy stream each (0 = 8, at most 64)       */
    /* SHA-256 pass tuning, per ctx (0 = the engine's default).  The defaults
     * can also be moved for a whole process by MI_SHA_BLOCKS_PER_CU / MI_SHA_COOP_MIN_GIB /
     * MI_SHA_COOP_MIN_GIB_PIECES / MI_SHA_COOP_BLOCKS_PER_CU, read at mi_ctx_create; a non-zero field here wins.      */
    uint32_t sha_blocks_per_cu;      /* workgroups per CU of the hashing kernels (default 2, 1..8) */
    uint32_t sha_load_scheme;        /* MI_SHA_LOADS_*: how a lane fetches its next block      */
    uint32_t sha_coop_min_gib;       /* MI_SHA_LOADS_AUTO: arena footprint in GiB from which the
                                        quad-cooperative loads are used (default 9; on an arena
                                        mapped in pieces under 256 MiB -- every walk-fed batch's --
                                        from 1 GiB on: a quarter of the address translations)  */
    uint32_t sha_coop_blocks_per_cu; /* workgroups per CU with cooperative loads (default: 3 from
                                        24 GiB up, else sha_blocks_per_cu; 1..3)               */
    uint32_t sha_sched;              /* MI_SHA_SCHED_*: how the strings of a hashing launch are shared
                                        out among the waves of a SIMD (0 = default; this field was
                                        `reserved`, always 0, before ABI 3's round-3 library)     */
} mi_config;
/* sha_sched.  Default: the wave that arrives FIRST on a SIMD takes the longest quarter of the launch's
 * strings at issue priority, the other wave(s) the rest; whoever runs dry continues in the other range
 * (one string is a serial chain, and the older wave of a SIMD runs three times as fast).   */
#define MI_SHA_SCHED_FLAT      1u            /* one range, every wave equal (the scheme of rounds 1-2)      */
#define MI_SHA_SCHED_LONG_SHIFT(k) ((((k) & 15u) + 1u) << 8)   /* the long range = the first n >> k strings
                                                (k = 0..15; default 2)                                       */
#define MI_SHA_LOADS_AUTO 0u   /* by footprint (sha_coop_min_gib)                            */
#define MI_SHA_LOADS_LANE 1u   /* every lane loads its own block, byte-aligned               */
#define MI_SHA_LOADS_COOP 2u   /* the four lanes of a quad fetch one owner's block together  */

/* One result row per file, in the order files were added.  This is what a
 * content-aware MemFS.isUpdated (lib/snapshot/mem_fs.go:487-503) would compare
 * next to tario.IsSimilarHeader's metadata (lib/tario/compare.go:104-120).       */
typedef struct {
    uint64_t user_tag;         /* caller's tag from mi_batch_add_*                  */
    uint64_t size;             /* bytes                                             */
    uint64_t first_chunk;      /* index of the file's first row in the chunk table  */
    uint32_t n_chunks;
    uint32_t crc32;            /* CRC32-IEEE of the bytes (MI_FLAG_FILE_CRC32)      */
    uint8_t  chunk_root[32];   /* SHA-256 over the concatenated chunk digests       */
    uint8_t  file_sha256[32];  /* SHA-256 of the bytes (MI_FLAG_FILE_SHA256)        */
} mi_file_result;

/* One row per chunk, files in add order, chunks in file order.                    */
typedef struct {
    uint64_t file_index;       /* index into the file table                         */
    uint64_t offset;           /* byte offset inside the file                       */
    uint32_t length;           /* bytes (min_size..max_size except a file's last)   */
    uint32_t reserved;
    int64_t  dup_of;           /* smallest chunk index (global index after
                                  mi_dedup_mark_global) with the same digest, -1 if
                                  this row is the first occurrence                  */
    uint8_t  sha256[32];       /* what sha256.Sum256(chunk) gives in Go             */
} mi_chunk_result;

/* Per-ctx counters for roofline reporting.                          */
typedef struct {
    uint64_t bytes_in;         /* file bytes scanned by the last mi_batch_run       */
    uint64_t n_files;
    uint64_t n_chunks;
    uint64_t n_unique;         /* chunks with dup_of == -1 after the last dedup     */
    double   ms_h2d;           /* host->device staging (0 for device-resident)      */
    double   ms_cdc;           /* Gear marking + cut selection kernels              */
    double   ms_sort;          /* chunk-table compaction + length binning           */
    double   ms_sha_chunks;    /* SHA-256-per-chunk kernel (the dominant kernel)    */
    double   ms_sha_files;     /* chunk_root (+ whole-file SHA-256 / CRC32) kernels */
    double   ms_dedup;         /* duplicate marking                                 */
    double   ms_total;         /* first kernel start to last kernel end             */
} mi_stats;

/* Staging counters of one batch (MI_FLAG_VERIFY_STAGING; all zero without the flag except
 * spans / bytes).                                                                   */
typedef struct {
    uint64_t spans;            /* host->device copies issued (reader-thread runs + inline flushes) */
    uint64_t bytes;            /* bytes they carried                                       */
    uint64_t verified_spans;   /* spans summed on both sides right after their copy        */
    uint64_t mismatches;       /* ... whose sums differed                                  */
    uint64_t repaired;         /* ... and matched after one more copy from the slab        */
    uint64_t final_spans;      /* spans summed again when staging ended                    */
    uint64_t final_mismatches; /* ... that no longer matched (the run fails)               */
    double   ms_verify;        /* host time spent summing + waiting for the device sums    */
} mi_stage_stats;

/* ---- context ----------------------------------------------------------------- */
MI_CORE int  mi_abi_version(void);
/* Diagnostics: from now on every chunk-pass launch of this ctx runs the recording instantiation of the hashing kernel
 * and appends one record per wave to `path` (where it ran, when, how much it hashed: tools/sha_wave_stats.py reads it);
 * each such launch is followed by a stream synchronize -- never on a ctx whose time is measured.  NULL or "" turns it
 * off.  MI_SHA_WAVE_STATS=<file> in the environment of mi_ctx_create does the same for the new ctx.  The record is the
 * SHA-256 kernel's: on a ctx with MI_FLAG_CHUNK_BLAKE2S the call returns MI_ERR_INVALID (and the variable is ignored).   */
MI_DIAG int  mi_debug_sha_wave_stats(mi_ctx* ctx, const char* path);
/* MI_DIGEST_SHA256, or MI_DIGEST_BLAKE2S for a ctx created with MI_FLAG_CHUNK_BLAKE2S */
MI_BLOCK int mi_ctx_chunk_digest(mi_ctx* ctx, uint32_t* alg);
MI_CORE int  mi_config_default(mi_config* cfg);
MI_CORE int  mi_ctx_create(const mi_config* cfg, mi_ctx** out);
/* Batches and indexes hold a pointer to their ctx: free them first (mi_batch_free /
 * mi_index_free).  With live children the call changes nothing and returns MI_ERR_STATE (the
 * count is in the message) -- a finalizer that runs in the wrong order gets an error, not a
 * use-after-free.  NULL is MI_OK.                                                       */
MI_CORE int  mi_ctx_destroy(mi_ctx* ctx);
/* Optional: pays NOW what the ctx's first content-aware commit would pay otherwise -- the reader threads with their pinned
 * slabs and streams, the kernels' code objects (a four-file synthetic batch): 0.05-0.06 s of a first commit's 0.07 where a
 * later one takes 0.011 (tools/first_commit_probe.py, profiles/r06_first_commit_probe.txt).  Blocking; a host runs it beside its own start-up work (a goroutine)
 * and joins it before the ctx's next call.  Changes no result and no statistic.                                          */
MI_BLOCK int mi_ctx_warm(mi_ctx* ctx);
/* ctx may be NULL: returns the message of the last failed mi_ctx_create.           */
MI_CORE const char* mi_last_error(mi_ctx* ctx);
MI_DIAG int  mi_get_stats(mi_ctx* ctx, mi_stats* out);
/* device properties as measured by hipGetDeviceProperties: CUs, clock, HBM bytes   */
MI_DIAG int  mi_device_info(mi_ctx* ctx, int32_t* n_cu, int32_t* clock_mhz, uint64_t* hbm_bytes,
                    char* name, size_t name_cap);

/* The integer-VALU roof of SHA-256 on this device, measured now: every lane runs `blocks` 64-round
 * compressions over register data (the very function the hashing kernels inline; no memory traffic),
 * waves_per_simd waves on every SIMD; *bytes_per_second = 64 bytes per compression over the best of
 * three launches.  0 = defaults (8 waves, 512 blocks: ~10 ms).  bench.py quotes the SHA pass against
 * this number from the same run (SURVEY.md 8d "second roof that actually binds SHA-256").          */
MI_DIAG int  mi_sha_valu_roof(mi_ctx* ctx, uint32_t waves_per_simd, uint32_t blocks, double* bytes_per_second);
/* The same for BLAKE2s-256: the ten-round compression of the MI_FLAG_CHUNK_BLAKE2S kernels alone (any ctx may ask). */
MI_DIAG int  mi_blake2s_valu_roof(mi_ctx* ctx, uint32_t waves_per_simd, uint32_t blocks, double* bytes_per_second);

/* ---- batch: a set of files scanned in one pass --------------------------------- *
 * Serves the per-entry loop of MemFS.commitLayer -> contentMemFile.commit ->
 * tario.WriteEntry (lib/snapshot/mem_fs.go:424-433, mem_layer.go:83-88,
 * lib/tario/write.go:28-52): the shim registers each regular file it is about to
 * write to the layer tar; directories/links/whiteouts have no bytes and are not
 * added.  Order of results == order of adds (the caller adds in sorted-path order,
 * lib/snapshot/mem_layer.go:232-244).                                              */
MI_BLOCK int mi_batch_begin(mi_ctx* ctx, uint64_t n_files_hint, uint64_t bytes_hint, mi_batch** out);
/* The bytes have been consumed when the call returns (len may be 0): small buffers are copied
 * into the batch's own pinned window by the calling thread, buffers of 1 MiB and more by the
 * ctx's reader threads in parallel.  Two batches of one ctx may be filled at the same time.  */
MI_BLOCK int mi_batch_add_bytes(mi_batch* b, const void* data, uint64_t len, uint64_t user_tag);
/* The engine opens `path` and reads exactly `size` bytes (the size at stat time,
 * like io.CopyN(w, f, h.Size) at lib/tario/write.go:43-45).  Short files are an
 * error, extra appended bytes are ignored.  The open and the size check happen in this call;
 * the bytes are read by the ctx's reader threads (several files at once, consecutive small
 * files share one PCIe transfer), so a file that shrinks afterwards fails mi_batch_run /
 * mi_batch_submit with MI_ERR_IO.                                                    */
MI_BLOCK int mi_batch_add_path(mi_batch* b, const char* path, uint64_t size, uint64_t user_tag);
/* Bulk form for MANY files (a layer is mostly small ones): nothing is opened in this call, the reader
 * threads open, read and close the files themselves, several at a time.  The price of the deferred
 * open: a missing or short file does not fail this call but mi_batch_run / mi_batch_submit
 * (MI_ERR_IO naming the path).  user_tags may be NULL (tags 0).                              */
MI_BLOCK int mi_batch_add_paths(mi_batch* b, uint64_t n, const char* const* paths, const uint64_t* sizes,
                       const uint64_t* user_tags);
/* Room for what is known to come (more_files files of more_bytes bytes in total): the arena grows once, now.  Growing
 * under way is correct but costs -- the reader threads are drained first and what the arena holds is moved -- so a
 * caller that knows a layer's size (after its walk; mi_batch_begin's hints serve the same purpose for a fresh batch)
 * says so.  mi_batch_add_tree does it by itself: its enumeration runs ahead of the files it hands over.            */
MI_BLOCK int mi_batch_reserve(mi_batch* batch, uint64_t more_files, uint64_t more_bytes);
/* The same for a byte range of a file -- a member of an uncompressed layer tar, whose ranges
 * mi_tar_entries lists: the file's bytes are [offset, offset + size) of `path`.             */
MI_BLOCK int mi_batch_add_path_range(mi_batch* b, const char* path, uint64_t offset, uint64_t size,
                            uint64_t user_tag);
/* Device-generated synthetic files (bench / roofline runs):
 * file i has sizes[i] bytes of the counter-mode stream keyed by (seed,
 * content_ids[i]); equal content ids give byte-identical files.  content_ids may be
 * NULL (ids = running file index).  user_tag = content id.                         */
MI_BLOCK int mi_batch_add_synthetic(mi_batch* b, uint64_t n_files, const uint64_t* sizes,
                           const uint64_t* content_ids, uint64_t seed);
/* Blocking: stage -> Gear CDC -> SHA-256 per chunk -> per-file roots -> dedup.     */
MI_BLOCK int mi_batch_run(mi_batch* b);
/* Re-runs the device pipeline on data already resident from a previous run (bench
 * steps; no re-staging / re-generation).                                            */
MI_BLOCK int mi_batch_rerun(mi_batch* b);
/* Asynchronous form: mi_batch_submit stages the batch on first use and ENQUEUES the
 * whole pipeline on the batch's own HIP stream without any host synchronisation, then
 * returns; mi_batch_wait blocks until it has finished and publishes counts and stats.
 * Two batches may be in flight on one ctx: the Gear pass of one overlaps the SHA-256
 * pass of the other (they bind different units of the CU).  mi_batch_run ==
 * submit + wait.  A batch may be submitted again after its wait (same data).         */
MI_BLOCK int mi_batch_submit(mi_batch* b);
MI_BLOCK int mi_batch_wait(mi_batch* b);
MI_BLOCK int mi_batch_counts(mi_batch* b, uint64_t* n_files, uint64_t* n_chunks, uint64_t* n_bytes);
MI_BLOCK int mi_batch_files(mi_batch* b, mi_file_result* out, uint64_t cap);
MI_BLOCK int mi_batch_chunks(mi_batch* b, mi_chunk_result* out, uint64_t cap);
/* The same rows without the copy into caller memory: *rows points at the batch's own pinned host
 * buffer (packed on the device, one device-to-host copy), valid until the batch is submitted
 * again, marked globally, reset or freed.  What a cgo shim reads through unsafe.Slice.          */
MI_BLOCK int mi_batch_chunks_view(mi_batch* b, const mi_chunk_result** rows, uint64_t* n_chunks);
/* ... and the file rows the same way (they are packed on the device too and arrive with the same wait).                  */
MI_BLOCK int mi_batch_files_view(mi_batch* b, const mi_file_result** rows, uint64_t* n_files);
/* The per-file chunk roots alone, 32 bytes per file in add order (cap = rows `out` has room for): what a content-aware
 * MemFS.isUpdated compares (lib/snapshot/mem_fs.go:487-503) -- one copy of n_files x 32 bytes, none of the chunk rows.   */
MI_BLOCK int mi_batch_roots(mi_batch* b, uint8_t* out, uint64_t cap);
/* Bytes [offset, offset + len) of file `file_index` as they lie in HBM -- the bytes the scan saw -- through a pinned
 * window of the batch (a fetch brings neighbours along: files staged together are asked for together).  From the moment
 * the batch is staged (mi_batch_run / _submit + _wait / _scan_cuts returned) until it is reset or freed; not while in
 * flight; not for parts.  What the layer writer reads when a commit takes its files from the batch
 * (mi_layer_add_batch_file) instead of reading them from disk a second time (lib/tario/write.go:43-45 reads once).     */
MI_BLOCK int mi_batch_read_file(mi_batch* b, uint64_t file_index, uint64_t offset, void* dst, uint64_t len);
/* Device pointer to the batch's n_chunks x 32-byte digest array (valid until
 * mi_batch_free); what a rank contributes to the all-gather.        */
MI_BLOCK int mi_batch_device_digests(mi_batch* b, const void** d_digests, uint64_t* n_chunks);
/* Copies the batch's file bytes back to the host (tests; cap >= total bytes, files
 * concatenated in add order, no padding).                                           */
MI_DIAG int mi_batch_read_back(mi_batch* b, void* out, uint64_t cap);
/* Empties the batch (files, results, recorded walk) but keeps its device memory and pinned window
 * for the next set of files: the way to scan layer after layer without paying allocation -- and
 * the driver's clearing of fresh device memory, which slows the first host-to-device copies into
 * it -- every time.  Not while in flight.                                                  */
MI_BLOCK int mi_batch_reset(mi_batch* b);
MI_BLOCK int mi_batch_free(mi_batch* b);
/* Staging counters since mi_batch_begin / mi_batch_reset (MI_FLAG_VERIFY_STAGING).  A staging
 * failure (a missing, short or unreadable file, a failed copy, a span that does not verify) is
 * STICKY: every later mi_batch_run / _submit / _scan_cuts of the batch returns MI_ERR_IO with the
 * first failure's message until mi_batch_reset -- a failed batch never scans half-staged bytes.   */
MI_DIAG int mi_batch_stage_stats(mi_batch* b, mi_stage_stats* out);
/* What the first verification mismatch of the batch looked like -- arena range, reader thread, both
 * pairs of sums, how many bytes differed and what the GPU held there (zeros / the 0xA5 fill / other
 * data), whether a second copy repaired it; "" if every span verified.  Call it after staging has
 * ended (mi_batch_run / _submit / _scan_cuts returned): the reader threads write the note while they
 * stage.  The pointer is valid until the batch is reset or freed.                                */
MI_DIAG const char* mi_batch_stage_note(mi_batch* b);

/* ---- parts: ONE file split across batches / GPUs (files >= 256 MiB) ------------- *
 * No reference counterpart: the reference streams a file through one goroutine
 * (lib/tario/write.go:28-52).  A part is the byte range [begin, end) of a file; begin and end are
 * multiples of MI_PART_ALIGN (end may also be the file size).  The engine stages the part behind a
 * halo of max_size bytes (rounded up to MI_PART_ALIGN) so that the chunk straddling `begin` lies
 * inside the item; a part OWNS the chunks that END in (begin, end], wherever they begin.
 * The only thing the parts' owners exchange is 8 bytes per boundary -- the previous part's last cut:
 *     every owner:  mi_batch_scan_cuts(batch)          cuts under an assumed entry (the halo's own
 *                   mi_batch_parts(batch, ...)         selection: right unless it never re-synchronised)
 *     exchange exits; for every part but a file's first:
 *                   mi_batch_set_part_entry(batch, file_index, exit of the previous part)
 *                   mi_batch_fix_cuts(batch)           re-selects only where the entry differed
 *     repeat while some part's exit changed (at most parts-per-file rounds; one on ordinary data)
 *     then mi_batch_submit / mi_batch_run as usual.
 * Submitting a batch that holds a part with an unconfirmed entry is MI_ERR_STATE.
 * Results: mi_chunk_result.offset is the offset inside the WHOLE file; mi_file_result.size is
 * end - begin, chunk_root covers the part's own chunks only (the file's root: mi_chunk_root over
 * the parts' digests), file_sha256 / crc32 are zero.                                           */
#define MI_PART_ALIGN 262144u
typedef struct {
    uint64_t file_index;       /* the part's row in this batch's file table                       */
    uint64_t file_size, begin, end;
    uint64_t entry;            /* file offset of the cut the part's first chunk starts at          */
    uint64_t exit;             /* file offset of the part's last cut (<= end): the next part's entry */
    uint32_t entry_confirmed;  /* mi_batch_set_part_entry was called (always 1 for begin == 0)     */
    uint32_t cuts_current;     /* 0: the confirmed entry differs, mi_batch_fix_cuts is due         */
} mi_part_state;
MI_BLOCK int mi_batch_add_path_part(mi_batch* b, const char* path, uint64_t file_size, uint64_t begin,
                           uint64_t end, uint64_t user_tag);
/* the part of the synthetic file (seed, content_id) of file_size bytes: same bytes as the range
 * [begin, end) of what mi_batch_add_synthetic generates for that content id                     */
MI_BLOCK int mi_batch_add_synthetic_part(mi_batch* b, uint64_t file_size, uint64_t content_id, uint64_t seed,
                                uint64_t begin, uint64_t end);
/* The chunk root of a file from its chunk digests (n x 32 bytes, file order) on the host: SHA-256
 * over the concatenation when n <= 64, else the fan-out-64 tree the engine computes per file.  A
 * split file's root = mi_chunk_root over its parts' digests put end to end.                     */
MI_BLOCK int mi_chunk_root(const uint8_t* digests, uint64_t n, uint8_t* root_out);
/* The same tree with the hash of `alg` (MI_DIGEST_*) at every node: the chunk root of a ctx whose mi_ctx_chunk_digest
 * is alg.  alg = MI_DIGEST_SHA256 is mi_chunk_root; an unknown alg is MI_ERR_INVALID.                                */
MI_BLOCK int mi_chunk_root_alg(uint32_t alg, const uint8_t* digests, uint64_t n, uint8_t* root_out);
/* Blocking: stages the batch and runs Gear marking + cut selection only.                         */
MI_BLOCK int mi_batch_scan_cuts(mi_batch* b);
MI_BLOCK int mi_batch_parts(mi_batch* b, mi_part_state* out, uint64_t cap, uint64_t* n_parts);
MI_BLOCK int mi_batch_set_part_entry(mi_batch* b, uint64_t file_index, uint64_t entry);
/* Blocking: re-selects the parts whose confirmed entry differs from the one their cuts were made
 * with and refreshes their exits.                                                              */
MI_BLOCK int mi_batch_fix_cuts(mi_batch* b);

/* ---- cross-batch / cross-GPU dedup --------------------------------------------- *
 * Plugs in where the reference dedups layer blobs by digest
 * (lib/builder/step/common.go:88-91 LinkStoreFileFrom && !os.IsExist;
 * lib/cache/cache_manager.go:239-252 entry codec): here the unit is a chunk.
 * d_digests: device pointer to n x 32 bytes (e.g. the all-gathered digest set of
 * every rank).  d_dup_of: device pointer to n x int64, receives for every row the
 * smallest row index with an equal digest, or -1 for first occurrences.
 * n_unique (host, optional) receives the number of -1 rows.                        */
MI_BLOCK int mi_dedup_mark(mi_ctx* ctx, const void* d_digests, uint64_t n, void* d_dup_of,
                  uint64_t* n_unique);
/* The same marking for ONE rank of a multi-GPU job: d_digests holds the job-wide, rank-major
 * digest set (n_total rows, after the all-gather); only the rank's own rows
 * [own_first, own_first + own_n) are answered: d_dup_of_own[i] = smallest GLOBAL index with
 * the digest of row own_first + i, or -1.  Identical values to mi_dedup_mark over the whole
 * set, at a fraction of the work: own rows build the table, rows of earlier ranks probe it,
 * rows of later ranks cannot be a minimum and are not touched.  n_own_first = own rows that
 * are the job-wide first occurrence (their sum over ranks = the unique count).          */
MI_BLOCK int mi_dedup_mark_range(mi_ctx* ctx, const void* d_digests, uint64_t n_total, uint64_t own_first,
                        uint64_t own_n, void* d_dup_of_own, uint64_t* n_own_first);
/* Rewrites the batch's dup_of column from a global marking: row i of the batch is
 * global row first_global + i of d_dup_of_global (device, int64).                  */
MI_BLOCK int mi_batch_set_global_dedup(mi_batch* b, const void* d_dup_of_global, uint64_t first_global);
/* mi_dedup_mark_range for a batch's own chunks, written straight into its dup_of column (no
 * intermediate array, no copy): the batch's rows are rows [own_first, own_first + n_chunks) of
 * the job-wide set d_digests_all.                                                        */
MI_BLOCK int mi_batch_mark_global(mi_batch* b, const void* d_digests_all, uint64_t n_total,
                         uint64_t own_first, uint64_t* n_own_first);
/* Device pointer to the batch's dup_of column (n_chunks x int64; valid until mi_batch_free). */
MI_BLOCK int mi_batch_device_dup_of(mi_batch* b, const void** d_dup_of, uint64_t* n_chunks);

/* ---- the digest exchange inside the library: RCCL all-gather over xGMI ---------------- *
 * For hosts without torch (the Go shim).  RCCL is loaded at run time (dlopen), so these
 * fail with MI_ERR_NO_DEVICE where no librccl exists (MI_RCCL_LIB=<path> names another library with
 * the same nccl* entry points: tests/rccl_stub is one, for n ranks on a single GPU).  Multi-process: rank 0 obtains the
 * id, ships it to the peers, every rank calls mi_comm_init_rank.  Single process driving n
 * devices (one ctx each): mi_comm_init_all + mi_dedup_allgather_all.
 * mi_dedup_allgather: all-gathers the batches' digest arrays (counts first, then slabs
 * padded to the largest count), marks this rank's chunks against the gathered set
 * (mi_batch_mark_global) so the batch's dup_of holds GLOBAL row indices (rank-major), and
 * sums the ranks' first-occurrence counts into n_unique; collective: every rank must call
 * it.  Outputs are optional.
 * Every rank's digests must be of one algorithm (all ctxs with MI_FLAG_CHUNK_BLAKE2S, or none):
 * the _all forms check it (MI_ERR_INVALID); across processes it is the caller's to guarantee --
 * no collective is spent on it, and ranks that disagree simply find no duplicates of each other. */
#define MI_COMM_ID_BYTES 128
MI_BLOCK int mi_comm_unique_id(void* id_out /* MI_COMM_ID_BYTES */);
MI_BLOCK int mi_comm_init_rank(mi_ctx* ctx, int nranks, int rank, const void* id);
MI_BLOCK int mi_comm_init_all(mi_ctx** ctxs, int n);
MI_BLOCK int mi_comm_destroy(mi_ctx* ctx);
/* How many ranks the ctx's communicator spans (ncclCommCount); 0 without a communicator.  What a
 * scaling run records next to its number: a job that believes it ran on 8 GPUs can prove it.     */
MI_BLOCK int mi_comm_ranks(mi_ctx* ctx, int* n_ranks);
MI_BLOCK int mi_dedup_allgather(mi_batch* b, uint64_t* n_total, uint64_t* n_unique,
                       uint64_t* first_global);
MI_BLOCK int mi_dedup_allgather_all(mi_batch** batches, int n, uint64_t* n_total, uint64_t* n_unique);
/* The HASH-PARTITIONED form of the same exchange (SURVEY 8e's "optimisation"): same arguments, same results bit for bit,
 * two all-to-alls (grouped ncclSend / ncclRecv) instead of the all-gather.  Every digest has one OWNER rank, chosen by its
 * second 8 bytes; a rank sends each owner its share (32-byte digest + 4-byte row, split stably on the device), the owner
 * marks what it received -- n_total / n rows, each distinct digest of the job counted once -- and sends 8 bytes per row
 * back.  Per own row at 8 ranks: 38.5 bytes over xGMI instead of 224 received, and a table of 1/8 of the job's rows instead
 * of own rows probed by every earlier rank's.  At most 64 ranks; MI_ERR_NO_DEVICE if the collective library has no
 * ncclSend / ncclRecv.  The all-gather form stays the default of bench.py: the exchange is 3-4 % of a C4 step
 * (DESIGN.md 5), and this form has met only the double's ranks (tests/test_gpu_native_exchange.py), never 8 real ones. */
MI_BLOCK int mi_dedup_alltoall(mi_batch* b, uint64_t* n_total, uint64_t* n_unique, uint64_t* first_global);
MI_BLOCK int mi_dedup_alltoall_all(mi_batch** batches, int n, uint64_t* n_total, uint64_t* n_unique);
/* Device time of the ctx's LAST exchange, from HIP events on the ctx stream (what a scaling line
 * reports beside its rate): ms_gather = the slab all-gather (xGMI time), ms_marking = squeezing the padding
 * out + the job-wide marking of this rank's rows.  Both 0 before the first exchange with rows.  After the all-to-all
 * form: ms_gather = both all-to-alls, ms_marking = the split + the owner's marking and answers + the scatter.  */
MI_DIAG int mi_comm_exchange_ms(mi_ctx* ctx, double* ms_gather, double* ms_marking);

/* ---- COPY/ADD context checksum (addCopyStep.SetCacheID seam) ------------------------ *
 * Reproduces the ONE running CRC32-IEEE the reference feeds at plan time
 * (lib/builder/step/add_copy_step.go:102-122,153-238): `prefix` = seed + directive +
 * args (:104-105), then for every walked path, in filepath.Walk order: its relpath
 * (:211), and for a symlink its target (:221-227), for a regular file all of its bytes
 * (:230-236); directories contribute only their relpath (:216-218), special files are
 * skipped by the caller (:198-203).  File bytes are reduced on the GPU (the batch must
 * come from a ctx with MI_FLAG_FILE_CRC32 and have run); the strings are spliced in on
 * the host with crc(A||B) = crc(A)*x^(8|B|) + crc(B).  The shim prints the result with
 * fmt.Sprintf("%x", crc) (:119) -- unpadded hex -- to get the reference's cacheID.    */
typedef struct {
    const char* relpath;       /* filepath.Rel(ctx.ContextDir, path)                     */
    const char* link_target;   /* non-NULL for a symlink: os.Readlink(path)              */
    int64_t     file_index;    /* regular file: its index in the batch; otherwise -1     */
} mi_ctx_entry;
MI_BLOCK int mi_context_checksum(mi_batch* b, const void* prefix, uint64_t prefix_len,
                        const mi_ctx_entry* entries, uint64_t n, uint32_t* crc_out);

/* ---- host-side walks: which files reach the batch, in what order -------------------- *
 * C++ restatement of the two walks that feed the hot path (filepath.Walk order: lexical
 * per directory, a directory before its children, symlinks never followed):
 *   MI_TREE_CONTEXT  checksumPathContents' walk (lib/builder/step/add_copy_step.go:
 *                    153-169,194-238): only special files are skipped;
 *   MI_TREE_SCAN     the snapshot walk (lib/snapshot/utils.go:37-75): also skips
 *                    ".wh..wh."-prefixed names, blacklist descendants
 *                    (lib/pathutils/path.go:24-35) and mountpoints
 *                    (lib/mountutils/mountutils.go:54-93; the table is read once per
 *                    process from /proc/mounts, or from the file MI_MOUNTS_FILE names -- the
 *                    reference's tests swap mountInfo.mountsFile the same way; a malformed
 *                    table fails the walk with MI_ERR_IO); skipped directories are pruned.
 *                    As in memLayer.createHeader (lib/snapshot/mem_layer.go:171-185) an
 *                    ABSOLUTE symlink target loses the rel_base prefix (pathutils.TrimRoot,
 *                    path.go:63-68: plain string prefix, then AbsPath); a target outside
 *                    rel_base fails the walk with MI_ERR_INVALID, as it fails the scan there.
 * Every regular file is added to the batch (stat-time size, user_tag = entry index);
 * relpath = filepath.Rel(rel_base, path) (rel_base NULL = root).  May be called several
 * times (one per COPY source, add_copy_step.go:158-167); entries accumulate.          */
#define MI_TREE_CONTEXT 0u
#define MI_TREE_SCAN    1u
typedef struct {
    const char* relpath;       /* valid until mi_batch_free                              */
    const char* link_target;   /* symlinks only: os.Readlink (context walk) / root-trimmed (scan) */
    int64_t     file_index;    /* regular files: index in the batch, else -1             */
    uint64_t    size;
    int64_t     mtime_sec;     /* truncated to seconds like tario.WriteHeader (write.go:62) */
    uint32_t    mode;          /* st_mode                                                */
    uint8_t     kind;          /* 0 directory, 1 regular file, 2 symlink, 3 hard link
                                  (3 is never produced by the walks; callers that track
                                  inodes like the reference's snapshot may set it)       */
    uint32_t    uid, gid;
} mi_tree_entry;
/* Regular files reach the batch while the walk goes on.  Files up to 16 KiB (MI_WALK_INLINE_MAX_KIB) are read by the
 * walk's own directory readers where they are listed -- one block of host memory per directory, one piece of the arena
 * each; those threads work on a file-descriptor table of their own (unshare(CLONE_FILES); where that is refused, on
 * the shared one) -- and a file that cannot be opened, or has shrunk since its lstat, fails THIS call with MI_ERR_IO
 * naming it, at its place in walk order.  Larger files are handed over in bulk as paths (mi_batch_add_paths: the
 * reader threads open them); one of those that vanishes or shrinks fails mi_batch_run / mi_batch_submit.
 * MI_WALK_INLINE=0: every file as a path.  Where a file lies in the arena is independent of its index.            */
MI_BLOCK int mi_batch_add_tree(mi_batch* b, const char* root, const char* rel_base,
                      const char* const* blacklist, uint64_t n_blacklist, uint32_t mode,
                      uint64_t* n_entries);
MI_BLOCK int mi_batch_tree_entries(mi_batch* b, mi_tree_entry* out, uint64_t cap);
/* The same walk on its own -- no ctx, no GPU: lists what mi_batch_add_tree WOULD add and in
 * which order (file_index = running ordinal of the regular files).  Host logic only.      */
typedef struct mi_tree mi_tree;
MI_BLOCK int  mi_tree_walk(const char* root, const char* rel_base, const char* const* blacklist,
                  uint64_t n_blacklist, uint32_t mode, mi_tree** out, uint64_t* n_entries);
MI_BLOCK int  mi_tree_entries(const mi_tree* tree, mi_tree_entry* out, uint64_t cap);
MI_BLOCK void mi_tree_free(mi_tree* tree);
/* mi_context_checksum over the recorded walk (the batch must have run).                */
MI_BLOCK int mi_context_checksum_tree(mi_batch* b, const void* prefix, uint64_t prefix_len,
                             uint32_t* crc_out);

/* The order MemFS.commitLayer writes entries in (memLayer.rangeFiles, lib/snapshot/
 * mem_layer.go:232-244: sort.Strings over the absolute dst paths; a whiteout marker
 * ".wh.<name>" sorts under the path it deletes, addHeader :190-211) -- not the walk order
 * ("a-b" < "a/x").  order_out[k] = index of the k-th entry to commit; equal keys keep their input
 * order.  The input's sorted runs are merged (a walk's order is nearly this one: 0.13 us per entry);
 * from 131 072 entries on, blocks are sorted on up to 16 threads of the library's own
 * (MI_WALK_THREADS) that end with the call.  Host logic.                                    */
MI_BLOCK int mi_entries_commit_order(const mi_tree_entry* entries, uint64_t n, uint64_t* order_out);

/* "Did this path change?" -- tario.IsSimilarHeader (lib/tario/compare.go:24-117), the test
 * behind MemFS.isUpdated (lib/snapshot/mem_fs.go:487-503), on walk entries: two entries with
 * empty relpaths are similar; otherwise the kinds must match and symlinks compare their
 * targets; hard links mtime+target+uid+gid+mode; directories mtime+uid+gid+mode; regular
 * files mtime+uid+gid+size+mode (mtime at second resolution, skipped when ignore_time;
 * mode = permission, setuid/setgid/sticky bits).  Content-aware extension: when BOTH roots
 * are given (32-byte chunk_root of each file) regular files are similar only if the roots
 * are equal too -- the reference "ignores path and content" (compare.go:101-103) because it
 * has no cheap content identity; with NULL roots the answer is exactly the reference's.
 * Unknown kind -> MI_ERR_INVALID (the reference's "unsupported type" error).  Host logic.  */
MI_BLOCK int mi_entry_similar(const mi_tree_entry* a, const mi_tree_entry* b, int ignore_time,
                     const uint8_t* root_a, const uint8_t* root_b, int* similar);

/* ---- a layer tar as a source: entries and the byte range of every file, no extraction ---- *
 * MemFS.UpdateFromTarReader (lib/snapshot/mem_fs.go:165-255) fills the in-memory tree from the
 * headers of base / cached layers.  mi_tar_open reads the headers of an UNCOMPRESSED tar (ustar,
 * pax 'x' records, GNU long names / base-256 numbers -- what Go's archive/tar and docker
 * write) and lists them as mi_tree_entry rows: relpath = the cleaned header name ("." for the
 * root, no leading or trailing "/"), kind 0 directory / 1 regular / 2 symlink / 3 hard link /
 * 4 other (device, fifo, a pax GLOBAL header -- which archive/tar hands to its caller as a member
 * and applies to nobody), file_index = ordinal among the regular files.  What ends an archive and
 * what fails it follow archive/tar's reader, not POSIX (csrc/mi_tar.hip lists the rules): one zero
 * block + end of data is an end, a zero block + a header or a last block of 1..511 bytes is
 * MI_ERR_INVALID ("read header: ...", mem_fs.go:185), as are malformed numbers, pax records and
 * pax times.  data_offsets[i]
 * (optional) = where entry i's bytes start in the archive (regular files only): a file is one
 * contiguous range of the tar.  Whiteout markers (".wh.<name>") are listed as the entries they
 * are.  Strings live until mi_tar_free.  Host logic.                                        */
typedef struct mi_tar mi_tar;
MI_BLOCK int  mi_tar_open(const char* path, mi_tar** out, uint64_t* n_entries);
/* The same with the failure reason as text (err, err_cap; nothing is printed anywhere) and
 * *is_gzip = 1 when `path` is a gzip blob -- the form layers are stored and pulled in
 * (tario.NewGzipReader, lib/tario/gzip.go:50-53; lib/builder/build_node.go:133-148).  A gzip blob is
 * listed through a streaming inflate; its data offsets are offsets in the UNCOMPRESSED tar.   */
MI_BLOCK int  mi_tar_open_ex(const char* path, mi_tar** out, uint64_t* n_entries, int* is_gzip, char* err,
                    uint64_t err_cap);
/* gzip blob -> the uncompressed tar at tar_path_out (NULL = digests only), its size and SHA-256
 * (the layer's TarDigest / diffID) and, optionally, the blob's own SHA-256 (GzipDescriptor.Digest):
 * the reference's fixture pair 393ccd5c... / 4ac76077... (lib/utils/testutil/constants.go:28) is
 * the test.  Then mi_tar_open(tar_path_out) + mi_batch_add_path_range scan the members.  A plain
 * tar is copied through unchanged.  Host logic (zlib, SHA-NI).                                */
MI_BLOCK int  mi_tar_inflate(const char* blob_path, const char* tar_path_out, uint64_t* tar_bytes,
                    uint8_t* tar_sha256, uint8_t* blob_sha256, char* err, uint64_t err_cap);
MI_BLOCK int  mi_tar_entries(const mi_tar* tar, mi_tree_entry* out, uint64_t* data_offsets, uint64_t cap);
MI_BLOCK void mi_tar_free(mi_tar* tar);

/* The layer diff of a scan, on two walks -- what MemFS.createLayerByScan + maybeAddToLayer
 * (lib/snapshot/mem_fs.go:315-341, 440-480) decide against the in-memory tree:
 *   after_flags[i]      MI_DIFF_CHANGED  the path is new or mi_entry_similar says it changed
 *                                        (content-aware when both sides carry chunk roots);
 *                       MI_DIFF_ANCESTOR an unchanged directory carried along because something
 *                                        below it changed or was deleted (addAncestors);
 *                       MI_DIFF_SAME     not part of the layer.  The root ("." ) never is.
 *   before_whiteout[j]  1 = write a whiteout for this path: it is gone, and it is the top of
 *                       the deleted subtree under a parent that still is a directory
 *                       ("only one whiteout file is needed for a deleted subtree", :461).
 * A side's roots: 32-byte chunk roots indexed by entry.file_index with a byte stride (pass
 * &files[0].chunk_root and sizeof(mi_file_result)), or NULL for the reference's
 * metadata-only rule.  Host logic.                                                       */
#define MI_DIFF_SAME     0u
#define MI_DIFF_CHANGED  1u
#define MI_DIFF_ANCESTOR 2u
typedef struct {
    const mi_tree_entry* entries;
    uint64_t             n;
    const void*          roots;        /* may be NULL */
    uint64_t             root_stride;
    const char*          disk_root;    /* `after` side only, may be NULL: the directory that was walked.
                                          When given, a path missing from `after` is whited out only
                                          if it is really gone from disk (memFSNode.isOnDisk,
                                          mem_fs.go:49-57,466) -- a path the walk now SKIPS (a new
                                          mountpoint, a blacklisted directory) still exists and gets
                                          no whiteout.                                              */
} mi_snapshot_side;
MI_BLOCK int mi_snapshot_diff(const mi_snapshot_side* before, const mi_snapshot_side* after, int ignore_time,
                     uint8_t* after_flags, uint8_t* before_whiteout);

/* ---- the layer of a COPY / ADD step: MemFS.AddLayerByCopyOps on entry lists ---------------- *
 * addToLayer + maybeAddToLayer + addAncestors (lib/snapshot/mem_fs.go:276-289, 343-421, 440-566)
 * and CopyOperation's source handling (lib/snapshot/copy_op.go:29-100, utils.go:249-327):
 *   tree / tree_root  the merged view so far (entries with relpaths below tree_root, e.g. the
 *                     result of mi_memfs_entries) and the directory it describes;
 *   ops               one per COPY/ADD: srcs relative to src_root (symlinks inside src_root are
 *                     resolved, one leaving it is an error), dst absolute, "dir/" = copy INTO it;
 *                     a single non-directory source with a dst not ending in "/" copies onto dst;
 *   now_sec           mtime of the directories the step has to create.
 * The destination directory chain is ensured first (existing ancestors are carried into the layer,
 * symlinks on the way followed, missing directories created with the op's uid/gid), then every
 * walked source path (snapshot walk rules, no blacklist) gets its header with the op's uid/gid and
 * is added iff tario.IsSimilarHeader says it differs from what the tree holds.  A single FILE
 * source skips the first step, so its dst stays as spelled: right below a symlink it becomes a
 * child of the link's node (`COPY f /lib/f` with /lib -> usr/lib: the layer holds lib, lib/f, usr,
 * usr/lib), deeper it fails as in the reference ("missing intermediate directory").  No scan
 * whiteouts: a copy never deletes -- except by NAME: a source called ".wh.<x>" is a whiteout of its
 * sibling <x>, filed under that path (memLayer.addHeader, mem_layer.go:197-212).  Result: the layer's entries in commit order (mi_copy_layer_entries), each
 * with the path its bytes are read from ("/" for created directories, as in the reference) -- feed them to mi_layer_add
 * and the regular files to a batch.  The caller's tree is not modified.  Host logic.           */
typedef struct {
    const char*        src_root;
    const char* const* srcs;
    uint64_t           n_srcs;
    const char*        dst;
    uint32_t           uid, gid;
} mi_copy_op;
/* NewCopyOperation's parameter check and destination (lib/snapshot/copy_op.go:44-81, 149-180): no sources, several
 * sources with a dst that is not in directory format (trailing "/", "." or ".."), or a relative dst without an
 * absolute work_dir are MI_ERR_INVALID ("check copy param: ..."); otherwise dst_out = dst if absolute, else
 * filepath.Join(work_dir, dst) with a trailing "/" kept.  mi_memfs_add_layer_by_copy_ops applies the same check to the
 * (already resolved, hence absolute) dst of every op.  Host logic.                                                        */
MI_BLOCK int  mi_copy_op_resolve(uint64_t n_srcs, const char* work_dir, const char* dst, char* dst_out, uint64_t cap,
                        char* err, uint64_t err_cap);
typedef struct mi_copy_layer mi_copy_layer;
MI_CORE int  mi_copy_layer_entries(const mi_copy_layer* layer, mi_tree_entry* out, const char** src_paths,
                           uint64_t cap);
MI_CORE void mi_copy_layer_free(mi_copy_layer* layer);

/* ---- MemFS as a handle: the reference's type (lib/snapshot/mem_fs.go:59-125) ------------------------------------- *
 * One tree for the life of a build, nodes of the reference's shape (header + children + the path the content came
 * from).  This is the ONE implementation of the layer merge and of the copy-op layer behind this header (until ABI 3
 * there were stateless twins on entry lists, mi_entries_apply_layer and mi_snapshot_copy_ops; they could not name the
 * directories addAncestors creates and are gone).  The handle keeps what lies between a build's steps -- those
 * directories (nodes like any other, part of mi_memfs_entries) and memFSNode.src, which is what isOnDisk asks the
 * disk about (mem_fs.go:49-57: a file a COPY step added is "on disk" while its SOURCE exists, whether or not the step
 * modified the file system).  mi_snapshot_diff above stays as the stateless form of ONE question (the scan diff of two
 * walks), held against mi_memfs_add_layer_by_scan on generated trees.
 *   mi_memfs_create           NewMemFS(clk, root, blacklist): the root's header from lstat(root); now_sec = the clock
 *                             (mtime of created directories; mi_memfs_set_clock moves it).
 *   mi_memfs_update_from_entries  UpdateFromTarReader with untar = false on a layer's entries (mi_tar_entries): the
 *                             per-header filter (shouldSkip with the blacklist, IsMounted), hard links in a second
 *                             pass, *n_merged = "Merged %d headers from tar to memfs".  A merged node's source is
 *                             filepath.Join(root, name) -- the reference passes AbsPath(name), the same path under
 *                             the root "/" of every real build; under another root isOnDisk must look below it.
 *   mi_memfs_add_layer_by_scan    createLayerByScan on a walk of the root (mi_tree_walk / mi_batch_add_tree with
 *                             MI_TREE_SCAN, rel_base = root, the same blacklist): every walked path through
 *                             maybeAddToLayer with createWhiteout -- changed paths with their ancestors, one whiteout
 *                             per deleted subtree (if the child's src is really gone).  roots / root_stride: chunk roots
 *                             by file_index, kept in the tree -- for changed paths with their new node, for unchanged
 *                             files that had none as the root they have now -- so that the NEXT scan's isUpdated is
 *                             content-aware (NULL = the reference's metadata-only rule).  The handle does not know which
 *                             algorithm these roots were computed with: they must be of the one (mi_ctx_chunk_digest) that
 *                             later commits on this handle use, or every file reads as changed.  mi_memfs_commit_layer with
 *                             a ctx does walk, GPU scan, this call and the layer tar in one.
 *   mi_memfs_add_layer_by_copy_ops   AddLayerByCopyOps (mem_fs.go:276-289): addToLayer per mi_copy_op against this tree.
 * Both return the layer in commit order as an mi_copy_layer (mi_copy_layer_entries: headers + the path each entry's
 * bytes are read from; a whiteout is an entry named ".wh.<x>" without content) and fold it into the tree.  A failing
 * call returns the error code, mi_memfs_error() the reference's message, and leaves the handle usable.
 *   mi_memfs_entries          the tree in sorted-path order (src_paths may be NULL; cap 0 sizes).
 *   mi_memfs_reset            MemFS.Reset: the tree is emptied, the root stays.
 * A handle is not re-entrant (the reference serialises MemFS with one mutex); handles are independent.  Host logic. */
typedef struct mi_memfs mi_memfs;
typedef struct mi_index mi_index;         /* the chunk index, below */
MI_CORE int  mi_memfs_create(const char* root, const char* const* blacklist, uint64_t n_blacklist, int64_t now_sec,
                     mi_memfs** out);
MI_CORE void mi_memfs_free(mi_memfs* fs);
MI_CORE const char* mi_memfs_error(const mi_memfs* fs);
MI_CORE int  mi_memfs_set_clock(mi_memfs* fs, int64_t now_sec);
MI_CORE int  mi_memfs_reset(mi_memfs* fs);
MI_CORE int  mi_memfs_update_from_entries(mi_memfs* fs, const mi_tree_entry* layer, uint64_t n_layer, uint64_t* n_merged);
MI_BLOCK int  mi_memfs_add_layer_by_scan(mi_memfs* fs, const mi_tree_entry* walked, uint64_t n, const void* roots,
                                uint64_t root_stride, mi_copy_layer** out, uint64_t* n_entries);
MI_BLOCK int  mi_memfs_add_layer_by_copy_ops(mi_memfs* fs, const mi_copy_op* ops, uint64_t n_ops, mi_copy_layer** out,
                                    uint64_t* n_entries);
MI_CORE int  mi_memfs_entries(const mi_memfs* fs, mi_tree_entry* out, const char** src_paths, uint64_t cap, uint64_t* n_out);

/* ---- the layer writer: tar framing + the two serial layer digests (host threads) ---------- *
 * step.tarAndGzipDiffs + MemFS.commitLayer (lib/builder/step/common.go:35-111,
 * lib/snapshot/mem_fs.go:424-433) behind the ABI: the shim hands over the layer's entries in
 * commit order (mi_entries_commit_order) and gets the DigestPair's numbers back, while the GPU
 * scans the same files' content (an mi_batch fed with the same paths).  Pipeline, one thread
 * per stage, 1 MiB blocks, every sink sees every block (stream.ConcurrentMultiWriter,
 * lib/stream/multi_writer.go:35-66):
 *     framer --tee--> SHA-256 of the tar stream                      (tarDigester, common.go:45)
 *               '---> gzip (zlib) --> out_fd + SHA-256 of the blob   (gzipper/gzipDigester, :44-52)
 * Entries: memLayer.createHeader's rules (lib/snapshot/mem_layer.go:152-190: Name = dst without
 * the leading "/", directories with a trailing "/", Uname/Gname empty, symlink target as given --
 * mi_tree_walk already root-trims it) written the way tario.WriteEntry / WriteHeader do
 * (lib/tario/write.go:28-68: mtime in whole seconds; regular files followed by EXACTLY size bytes
 * read from src_path -- io.CopyN; a shorter file is MI_ERR_IO; directories, symlinks and hard
 * links header-only; any other kind MI_ERR_INVALID "unsupported type").  The header bytes follow
 * Go's archive/tar Writer (USTAR, PAX when a field does not fit); byte parity with Go is
 * UNPINNED here (no Go toolchain) -- see csrc/mi_layer.hip.  mi_layer_finish writes
 * tar.Writer.Close's 1024-byte trailer: an empty layer is 1024 zero bytes, digest 5f70bf18...
 * (lib/docker/image/const_darwin.go:18).  Not thread-safe per layer; layers are independent. */
#define MI_GZIP_OFF     (-2)   /* no gzip leg: out_fd receives the tar itself                    */
#define MI_GZIP_DEFAULT (-1)   /* "default"; 0 = "no", 1 = "speed", 9 = "size" (lib/tario/gzip.go:26-43) */
typedef struct mi_layer mi_layer;
typedef struct {
    uint32_t struct_size;
    int32_t  gzip_level;       /* MI_GZIP_OFF, MI_GZIP_DEFAULT or 0..9.  At every level but 0 a 1 MiB
                                  block that will not compress (three 8 KiB samples of it through
                                  level 1) is stored, not searched: one valid member either way    */
    int32_t  out_fd;           /* where the layer blob is written; -1 = digests only           */
    uint32_t flags;            /* MI_LAYER_*                                                    */
} mi_layer_config;
/* The header's Mode field keeps the file-type bits of the entry's st_mode (0100755, 040755,
 * 0120777): what tar.FileInfoHeader produced up to Go 1.8 (Mode |= c_ISREG / c_ISDIR / c_ISLNK) and
 * what the Go-written layer tars the reference holds as fixtures carry (testdata/files/busybox/
 * 393ccd5c.../layer.tar).  Without the flag: the Go >= 1.9 rule -- permission bits + setuid / setgid
 * / sticky only -- which is what createHeader (lib/snapshot/mem_layer.go:152-154) hands to the
 * writer under the reference's Go 1.14 toolchain.  Everything else in the header is the same, and
 * with the flag this writer reproduces that fixture byte for byte (tests/test_host_layer.py).     */
#define MI_LAYER_MODE_WITH_TYPE 0x1u
typedef struct {
    uint8_t  tar_sha256[32];   /* DigestPair.TarDigest      (common.go:97)                      */
    uint8_t  gzip_sha256[32];  /* GzipDescriptor.Digest     (:98-102); zero with MI_GZIP_OFF   */
    uint64_t tar_bytes;
    uint64_t gzip_bytes;       /* GzipDescriptor.Size                                           */
    uint64_t n_entries;
} mi_layer_result;
MI_CORE int  mi_layer_config_default(mi_layer_config* cfg);
MI_BLOCK int  mi_layer_begin(const mi_layer_config* cfg, mi_layer** out);
/* e->relpath = the entry's dst path; src_path = where a regular file's bytes are read from.  A dst whose
 * base name carries the whiteout prefix ".wh." is written as a whiteout -- a zero header with only that name,
 * no content -- whatever the entry is (memLayer.addHeader, lib/snapshot/mem_layer.go:197-212).                */
MI_BLOCK int  mi_layer_add(mi_layer* layer, const mi_tree_entry* e, const char* src_path);
/* The same entry with its content taken from a staged batch: the header as mi_layer_add writes it, then file
 * `file_index` of `batch` -- the bytes the GPU scanned, read back from HBM (mi_batch_read_file) -- instead of a second
 * read of the path.  The tar then holds exactly the bytes the file's chunk root describes, whatever has happened to the
 * file since it was staged; e->size must be the staged size (MI_ERR_INVALID otherwise).  Entries without content
 * (directories, links, whiteouts by name) are written as by mi_layer_add.                                              */
MI_BLOCK int  mi_layer_add_batch_file(mi_layer* layer, const mi_tree_entry* e, mi_batch* batch, uint64_t file_index);
/* What this writer read from disk itself so far: files it opened, bytes it read (mi_layer_add with a src_path).        */
MI_DIAG int  mi_layer_io_counts(mi_layer* layer, uint64_t* files_opened, uint64_t* file_bytes_read);
/* whiteoutMemFile.commit (mem_layer.go:101-132): a zero header named <dir>/.wh.<base>.          */
MI_BLOCK int  mi_layer_add_whiteout(mi_layer* layer, const char* deleted_path);
MI_BLOCK int  mi_layer_finish(mi_layer* layer, mi_layer_result* out);
MI_BLOCK const char* mi_layer_error(mi_layer* layer);
MI_BLOCK void mi_layer_free(mi_layer* layer);
/* THE DEVICE DEFLATE LEG (opt-in; csrc/mi_deflate_wave.h).  mi_layer_set_gzip_ctx, after mi_layer_begin and before
 * the first add (later: MI_ERR_STATE; with gzip_level MI_GZIP_OFF or 0: MI_ERR_INVALID, there is nothing to code): the gzip leg
 * of this layer is coded on ctx's device instead of by zlib's pool threads, which are then not started.  The sink collects whole
 * 1 MiB blocks of the tar into a window (MI_GZIP_DEVICE_WINDOW_MB, 1..1024, default 32), two windows in flight on streams of the
 * leg's own, and writes the pieces in order, with SHA-256 and `write` as the host leg does; then 03 00, the combined CRC-32 and
 * the length.  The ten header bytes are the host leg's with XFL = 4.  THERE IS ONE DEVICE LEVEL: gzip_level 1..9 or default does
 * not change the device leg's bytes.  A device error is the layer's error (mi_layer_error) and fails mi_layer_finish; a layer that
 * has begun never falls back to zlib.  The ctx must outlive the layer.  The tar, TarDigest and everything else are unchanged;
 * gzip_sha256 and gzip_bytes describe the blob written, as ever (the gzip bytes are this writer's own).
 *
 * FORMAT.  The member's deflate stream is the PIECES' stored forms end to end, then the writer's 03 00.  Piece k is tar bytes
 * [k * 65536, (k + 1) * 65536), the last one shorter; no match reaches before a piece's first byte, so the blob is a pure
 * function of the tar stream, whatever window, thread count or GPU produced it.  A piece is stored as (D) one dynamic-Huffman
 * block (BFINAL 0, BTYPE 2) followed by an empty stored block -- three zero bits, zero bits to the byte boundary, 00 00 FF FF, what
 * Z_SYNC_FLUSH writes: the piece ends on a byte boundary -- or as (S) stored blocks of at most 65 535 bytes (a full piece: 65 535
 * and 1).  (D) is kept only where it is smaller than (S).  No fixed-Huffman blocks, no BFINAL in a piece.  The parse, the split of
 * long matches, the length-limited COMPLETE codes and the header's run rule are stated in csrc/mi_deflate_wave.h and restated by the
 * model the tests hold the bytes against (tests/deflate_cases.py).
 *
 * mi_deflate_buffer is the coder alone, host bytes in, host bytes out: the pieces' stored forms of src[0, n) end to end in dst, no
 * gzip header and no final block -- zlib.decompressobj(-15).decompress(out + b"\x03\x00") gives src back.  *crc32 (may be NULL):
 * the CRC-32 of src, computed on the device; info (may be NULL): the pieces by form, the bytes, the device time of the windows.
 * n == 0 gives 0 bytes.  cap below mi_deflate_bound(n) is MI_ERR_CAPACITY, a NULL ctx, dst, out_bytes or src (with n > 0)
 * MI_ERR_INVALID.  Any failure leaves dst unspecified and the ctx usable.  The bytes cross PCIe through pinned windows on streams
 * of the call's own (MI_GZIP_DEVICE_WINDOW_MB as above).                                                                       */
typedef struct { uint64_t n_pieces, n_dynamic, n_stored, in_bytes, out_bytes; double ms_device; } mi_deflate_info;
MI_BLOCK uint64_t mi_deflate_bound(uint64_t n);   /* what dst must hold for any n bytes */
MI_BLOCK int  mi_deflate_buffer(mi_ctx* ctx, const void* src, uint64_t n, void* dst, uint64_t cap, uint64_t* out_bytes, uint32_t* crc32,
                                mi_deflate_info* info);
MI_BLOCK int  mi_layer_set_gzip_ctx(mi_layer* layer, mi_ctx* ctx);
/* THE DEVICE INFLATE (opt-in; csrc/mi_inflate_wave.h, csrc/host_inflate.h): the way back.  mi_tar_inflate and
 * mi_tar_open_ex are what they were.  One whole gzip member is inflated on ctx's device WITHOUT AN INDEX: both of this library's
 * writers end a run of deflate blocks with an empty stored block (00 00 FF FF on a byte boundary: the host leg every 1 MiB block, the
 * device leg every dynamic 65 536-byte piece) and start the next run without history, so the positions behind those four bytes are
 * found bytewise and a wave decodes from each.
 *
 * FORMAT RULE.  A CANDIDATE is a byte offset p with gz[p - 4, p) == 00 00 FF FF and p <= n - 8, or the first byte behind the gzip
 * header (parsed on the host with FEXTRA / FNAME / FCOMMENT / FHCRC; a wrong magic, a method other than 8, a reserved flag bit, a
 * wrong header CRC or a header that does not end: MI_ERR_INVALID).  The SEGMENT from a candidate is decoded -- stored, fixed and
 * dynamic blocks -- until an empty stored block with BFINAL 0 has been read (it ends at the byte behind it, a candidate), a block with
 * BFINAL 1 has been read (END) or a rule of csrc/host_inflate.h's InflateRule is broken (they are zlib's, and a distance that
 * reaches before the SEGMENT's first byte).  The LIVE CHAIN runs from the header's end along the segments' ends to END, which must
 * lie at n - 8; candidates that are not on it are dead and ignored.  The live segments are decoded a second time to their final
 * offsets, in rounds whose output fits a window (MI_INFLATE_WINDOW_MB, 1..1024, default 64: the output of a round AND the most one
 * segment may inflate to), two rounds in flight on streams of the call's own; the CRC-32 of every round is taken on the device,
 * combined on the host and held against the trailer with ISIZE (mod 2^32).
 *
 * VERDICTS.  MI_INFLATE_DONE: the output is the member's inflation, CRC and ISIZE checked.  MI_INFLATE_NOT_PARALLEL (returned as
 * MI_OK): nothing is delivered and the caller inflates serially -- a live segment reaches before its own start (pgzip's and pigz's
 * blocks carry the previous block's dictionary; this cannot be told from corruption, zlib decides), a live segment inflates to
 * more than a window, or END lies before n - 8 (more members, trailing bytes); info names the segment (at_in, at_out: its input
 * and output offsets) and the rule.  Any other broken rule on a LIVE segment, or a CRC / ISIZE mismatch, is MI_ERR_INVALID;
 * mi_last_error names the segment's input offset, its output offset and the rule; the ctx stays usable.
 *
 * mi_inflate_buffer: gz[0, n) in host memory in, its inflation in dst.  The total is known after the size pass: cap too small is
 * MI_ERR_CAPACITY with *out_bytes = the size needed (cap == 0 with dst == NULL asks for it); on NOT_PARALLEL *out_bytes is 0.  A
 * NULL ctx, gz or out_bytes, or a NULL dst with cap > 0: MI_ERR_INVALID.  The member lies whole on the device for the call; a failed
 * allocation is MI_ERR_NOMEM.  info (may be NULL): the bytes, candidates, live segments, rounds, the verdict, the device time of
 * the size pass (with the marking) and of the write passes.  Any failure leaves dst unspecified.
 *
 * mi_tar_inflate_ctx: mi_tar_inflate's contract and results through the device.  The blob is hashed (blob_sha256) while it goes
 * up; the rounds come down in order into the SHA-256 stream (tar_sha256) and the output file (tar_path_out NULL: digests only).  A
 * plain tar is copied through as mi_tar_inflate does.  On NOT_PARALLEL the call runs mi_tar_inflate itself and sets
 * info->fell_back = 1; the output file is not created before the verdict is known.  A corrupt blob is MI_ERR_INVALID with
 * "<blob_path>: corrupt gzip stream ..." in err, and no output file is left behind.                                            */
#define MI_INFLATE_DONE 0
#define MI_INFLATE_NOT_PARALLEL 1
typedef struct { uint64_t in_bytes, out_bytes, n_candidates, n_segments, n_rounds, at_in, at_out;
                 uint32_t verdict, rule, fell_back, reserved; double ms_size, ms_write; } mi_inflate_info;
MI_BLOCK int  mi_inflate_buffer(mi_ctx* ctx, const void* gz, uint64_t n, void* dst, uint64_t cap, uint64_t* out_bytes, mi_inflate_info* info);
MI_BLOCK int  mi_tar_inflate_ctx(mi_ctx* ctx, const char* blob_path, const char* tar_path_out, uint64_t* tar_bytes, uint8_t* tar_sha256,
                                 uint8_t* blob_sha256, mi_inflate_info* info, char* err, uint64_t err_cap);
/* ANY GZIP MEMBER FROM AN INDEX OF CHECKPOINTS (opt-in; csrc/host_inflate_index.h, csrc/mi_inflate_index.hip).  The
 * calls above pay off on blobs this library's device leg wrote.  For every other gzip -- a base image from a registry, a cache layer
 * the reference wrote through pgzip, the host leg's blob -- the missing piece is the classic one (zran, rapidgzip): an index of
 * CHECKPOINTS, each a deflate block boundary with its bit offset in the member, its output offset and the (up to) 32 KiB of output in
 * front of it.  It is built once, by zlib, when the blob is pulled for the first time (zlib inflates serially then anyway; with
 * tar_sha256 the same pass gives the TarDigest) and is kept beside the blob.  With it every SPAN between two checkpoints is
 * independent: one wave a span decodes straight to the span's final offset, no size pass, no marker, any encoder's output.
 *
 * THE INDEX, little-endian, a pure function of (member, spacing): 64 bytes "MIGZIX01" | u64 member bytes | u64 out_bytes | u32 CRC-32 |
 * u32 ISIZE | u64 gzip header length | u64 n_points | u64 spacing | u64 windows_bytes; n_points rows u64 in_bit | u64 out_at | u64 win_at
 * | u32 win_bytes = min(32 768, out_at) | u32 0; the windows, each padded with zeros to 16.  Point 0 is the stream's start; after every
 * non-final block that ends with at least `spacing` bytes of output since the last point there is a new one (spacing 0: 262 144; a
 * point at which the output is already complete is dropped).  Only a single member that ends at n - 8 is indexed.
 *
 * mi_inflate_index_build (host only): gz[0, n) -> *index (malloc'ed: mi_inflate_index_free), *index_bytes.  CRC-32 and ISIZE are
 * checked; tar_sha256 (may be NULL): the SHA-256 of the inflation.  MI_ERR_INVALID with the reason in err: no gzip header, a corrupt
 * stream, a second member, trailing bytes, a wrong CRC-32 or ISIZE.  mi_inflate_index_check (host only): 0, or the number of the first
 * reason an UNTRUSTED index is refused (mi_inflate_index_refusal: its text) -- 1 magic, 2 sizes, 3 point 0, 4 in_bit not ascending,
 * 5 out_at not ascending, 6 in_bit behind the stream, 7 out_at behind the output, 8 win_bytes, 9 a window out of bounds, unaligned or
 * overlapping, 10 (gz given) another member's: n, header length, CRC-32 or ISIZE differ.
 *
 * VERDICTS of the indexed calls, all returned as MI_OK: MI_INFLATE_DONE; MI_INFLATE_NOT_PARALLEL (a span larger than the window
 * MI_INFLATE_WINDOW_MB, or the last span's stream ends before n - 8); MI_INFLATE_INDEX_REFUSED: the checker refused the index
 * (info.reserved: its number), a span broke a rule (rule 12: it does not end where the index says; info: the span's at_in = in_bit / 8,
 * at_out and the rule), or CRC-32 / ISIZE do not hold (rule 0).  A stale index cannot be told from a corrupt blob, so the index is
 * only ever a hint: it never produces MI_ERR_INVALID and never delivers bytes that fail the trailer.
 *
 * mi_inflate_buffer_indexed: mi_inflate_buffer with the index.  The total is the index's: MI_ERR_CAPACITY (with *out_bytes = the size
 * needed) comes before any device work; *out_bytes is 0 unless the verdict is DONE (dst is then unspecified).
 * mi_tar_inflate_ctx_indexed: mi_tar_inflate_ctx with the index; on INDEX_REFUSED or NOT_PARALLEL any partial output is removed and
 * mi_tar_inflate runs -- zlib decides whether the blob is corrupt --, info->fell_back = 2 when the index was refused, 1 otherwise.   */
#define MI_INFLATE_INDEX_REFUSED 2
typedef struct { uint64_t n_points, n_blocks, out_bytes, windows_bytes, spacing; double ms_build; } mi_inflate_index_info;
MI_BLOCK int  mi_inflate_index_build(const void* gz, uint64_t n, uint64_t spacing, void** index, uint64_t* index_bytes,
                                     mi_inflate_index_info* info, uint8_t* tar_sha256, char* err, uint64_t err_cap);
MI_BLOCK void mi_inflate_index_free(void* index);
MI_BLOCK int  mi_inflate_index_check(const void* index, uint64_t index_bytes, const void* gz, uint64_t n);
MI_BLOCK const char* mi_inflate_index_refusal(int refusal);
MI_BLOCK int  mi_inflate_buffer_indexed(mi_ctx* ctx, const void* gz, uint64_t n, const void* index, uint64_t index_bytes, void* dst, uint64_t cap,
                                        uint64_t* out_bytes, mi_inflate_info* info);
MI_BLOCK int  mi_tar_inflate_ctx_indexed(mi_ctx* ctx, const char* blob_path, const void* index, uint64_t index_bytes, const char* tar_path_out,
                                         uint64_t* tar_bytes, uint8_t* tar_sha256, uint8_t* blob_sha256, mi_inflate_info* info, char* err,
                                         uint64_t err_cap);
/* A GZIP MEMBER NOBODY INDEXED: SPECULATIVE SPANS (opt-in; csrc/mi_inflate_spec.hip, csrc/host_inflate_spec.h).  The
 * first pull of a foreign gzip has no index yet.  These calls make the indexed inflate's span table and window area on the device from
 * the member alone (pugz's and rapidgzip's technique): the deflate stream behind the header is cut into PIECES of piece_bytes member
 * bytes (0: 65 536; otherwise 1 024 .. 16 777 216, else MI_ERR_INVALID; doubled until there are at most 16 384 pieces -- the value used
 * is reported); a finder takes for every piece the smallest bit at which a non-final dynamic block header parses (piece 0: the
 * stream's start); a speculative pass decodes from every such CANDIDATE without the 32 KiB in front of it, into a ring of markers,
 * until the next block header that begins at a candidate; the host walks the chain of these spans from the stream's start; a window
 * pass resolves the markers in chain order.  From there the spans are decoded as an index's are, held to their ends, and the member's
 * CRC-32 and ISIZE decide.  One route serves every gzip; the marker route of the unindexed calls is not tried first.
 *
 * VERDICTS (returned as MI_OK): MI_INFLATE_DONE; MI_INFLATE_NOT_PARALLEL -- a span larger than the window MI_INFLATE_WINDOW_MB (rule
 * 11), a span of more than 32 x piece_bytes literals and matches that reaches no candidate (rule 13: a stream of fixed blocks; stored
 * bytes do not count), or a stream that ends before n - 8 (more members); MI_INFLATE_INDEX_REFUSED -- the write pass refused a span
 * (rule 10: a match reaches before the member's first byte) or the trailer does not hold (rule 0): nothing is delivered and zlib
 * decides.  A rule broken on a span of the chain in the speculative pass is MI_ERR_INVALID; mi_last_error names the span, the rule
 * and the bit.
 *
 * mi_inflate_buffer_spec: mi_inflate_buffer this way.  The total is known after the plan: MI_ERR_CAPACITY (with *out_bytes = the size
 * needed) comes before the write pass.  index / index_bytes (both NULL, or both given): with the verdict DONE they receive a MIGZIX01
 * index of the spans -- the points as planned, the windows as the device made them, the spacing field = the piece_bytes used -- that
 * passes mi_inflate_index_check and drives every indexed call; free it with mi_inflate_index_free.  It is NOT what
 * mi_inflate_index_build gives for any spacing: its points are the candidates the chain passed.
 * mi_tar_inflate_ctx_spec: mi_tar_inflate_ctx this way; on NOT_PARALLEL or INDEX_REFUSED any partial output is removed and
 * mi_tar_inflate runs (info->fell_back 1 or 2).  A plain tar is copied through.
 * mi_inflate_spec_info: the piece used, the pieces, the pieces with a candidate, the spans on the chain (before spans without output
 * are merged into the one in front), the rings' bytes, and the device times of the finder, the speculative pass and the window pass. */
typedef struct { uint64_t piece_bytes, n_pieces, n_found, n_live, ring_bytes; double ms_find, ms_speculate, ms_windows; } mi_inflate_spec_info;
MI_BLOCK int  mi_inflate_buffer_spec(mi_ctx* ctx, const void* gz, uint64_t n, uint64_t piece_bytes, void* dst, uint64_t cap, uint64_t* out_bytes,
                                     mi_inflate_info* info, mi_inflate_spec_info* spec_info, void** index, uint64_t* index_bytes);
MI_BLOCK int  mi_tar_inflate_ctx_spec(mi_ctx* ctx, const char* blob_path, uint64_t piece_bytes, const char* tar_path_out, uint64_t* tar_bytes,
                                      uint8_t* tar_sha256, uint8_t* blob_sha256, mi_inflate_info* info, mi_inflate_spec_info* spec_info,
                                      void** index, uint64_t* index_bytes, char* err, uint64_t err_cap);
/* A PULLED LAYER BECOMES A BATCH (csrc/mi_layerblob.hip, csrc/mi_tarscan.hip, csrc/host_tarcache.h).  The
 * reference fills its tree from a base or cached layer by reading the tar (MemFS.UpdateFromTarPath, lib/snapshot/mem_fs.go:139-161:
 * open, tario.NewGzipReader when the blob is gzip, UpdateFromTarReader).  Everything behind this library's scan takes a batch
 * (mi_index_add_batch, mi_batch_pack_chunks, mi_batch_zpack_chunks, mi_zset_missing, the roots, the dedup marks); this call fills
 * one from a layer blob in one way up: the blob -- this library's device-leg gzip, its host-leg gzip, a foreign gzip or a plain tar
 * -- is uploaded once, inflated on the device STRAIGHT INTO THE BATCH'S ARENA, and its regular members become the batch's files
 * where they lie: the tar does not come down, no tar file is written, nothing is staged twice, no member is copied on the device.
 * The host needs only the tar's headers: the device marks every 512-byte block for which the parser's checksum rule holds (a meta
 * header -- x, g, L, K -- takes the next two blocks with it), the marked blocks come down, and mi_tar_open_ex's own parser follows
 * the live chain through them; what the cache does not hold (the end marker, a meta body beyond 1 024 bytes, a block on the chain
 * the device did not mark -- which the parser then refuses) is fetched on demand, and counted.
 *
 * source: 0 a plain tar (uploaded as it is), 1 gzip inflated on the device (the plan said MI_INFLATE_DONE; the member's CRC-32 and
 * ISIZE are checked on the device), 2 a gzip that is not parallel (MI_INFLATE_NOT_PARALLEL: zlib inflates it into host memory of
 * the tar's size, which then goes up as a plain tar).  Every regular member (kind 1, empty ones included) becomes, in listing
 * order, the file {arena_at + data_offset, size, tag_base + file_index}; its batch index is first_file + file_index.  arena_at is a
 * multiple of 256 and data offsets are multiples of 512, so every member starts on the boundary every other add gives a file.
 * *listing (may be NULL) receives the archive's mi_tar (mi_tar_entries; data offsets are offsets in the tar; mi_tar_free).
 * blob_sha256 (may be NULL): the blob's own SHA-256, taken while it goes up.  NO TarDigest comes out of this call, on purpose: it
 * is the serial SHA-256 stream this path exists to avoid -- a cache hit knows the pair from its entry (mi_cache_parse_entry), and
 * a caller who wants the diffID computed keeps mi_tar_inflate_ctx.  Files from a layer carry no end-to-end byte sums (they never
 * crossed PCIe as files); to everything behind the add they are ordinary files.  The call returns when the device work is done.
 *
 * info (may be NULL): the tar's size, where it lies, the files and entries, the blocks the device marked (n_marked), the headers
 * the listing consumed from them (n_live), the on-demand fetches and their bytes, the source, the host's time for the way up
 * (ms_upload; a gzip blob: the plan's time less its device time) and for the header pass with the listing (ms_headers), and the
 * inflater's own info.
 *
 * On ANY failure the batch's files, bytes, arena offset and usability are what they were (the arena may have grown).  NULL b or
 * blob: MI_ERR_INVALID; a batch that ran: MI_ERR_STATE; a batch group: MI_ERR_INVALID; a corrupt gzip: MI_ERR_INVALID with the
 * inflater's message; a tar error: MI_ERR_INVALID with mi_tar_open_ex's text for the same archive -- all in mi_last_error.
 * _path maps the file and calls _blob.  One GPU; the blob (gzip) and the tar both lie in device memory for the call. */
typedef struct { uint64_t tar_bytes, arena_at, first_file, n_files, n_entries,
                 n_marked, n_live, n_fetched, fetched_bytes;
                 uint32_t source, reserved;      /* 0 plain tar, 1 gzip inflated on the device, 2 gzip through zlib */
                 double ms_upload, ms_headers; mi_inflate_info inflate; } mi_layer_blob_info;
MI_BLOCK int mi_batch_add_layer_blob(mi_batch* b, const void* blob, uint64_t n, uint64_t tag_base,
                                     mi_tar** listing, uint8_t* blob_sha256, mi_layer_blob_info* info);
MI_BLOCK int mi_batch_add_layer_path(mi_batch* b, const char* blob_path, uint64_t tag_base,
                                     mi_tar** listing, uint8_t* blob_sha256, mi_layer_blob_info* info);
/* ... with the blob's index of checkpoints (mi_inflate_index_build): a gzip blob whose index carries through is decoded
 * span by span straight into the arena -- source 3.  The index is a hint: when it is refused (or a span is larger than the window) the
 * batch is as it was and the call proceeds exactly as the unindexed one does, with info->inflate.fell_back = 2 (refused) and the
 * source the unindexed call gives.  A plain tar ignores the index. */
MI_BLOCK int mi_batch_add_layer_blob_indexed(mi_batch* b, const void* blob, uint64_t n, const void* index, uint64_t index_bytes,
                                             uint64_t tag_base, mi_tar** listing, uint8_t* blob_sha256, mi_layer_blob_info* info);
MI_BLOCK int mi_batch_add_layer_path_indexed(mi_batch* b, const char* blob_path, const void* index, uint64_t index_bytes,
                                             uint64_t tag_base, mi_tar** listing, uint8_t* blob_sha256, mi_layer_blob_info* info);
/* ... and with no index at all: the speculative plan takes the index's place and route -- source 4.  On NOT_PARALLEL or
 * INDEX_REFUSED the batch is as it was and the call proceeds exactly as the unindexed one does (info->inflate.fell_back = 2: refused). */
MI_BLOCK int mi_batch_add_layer_blob_spec(mi_batch* b, const void* blob, uint64_t n, uint64_t piece_bytes, uint64_t tag_base, mi_tar** listing,
                                          uint8_t* blob_sha256, mi_layer_blob_info* info, mi_inflate_spec_info* spec_info);
MI_BLOCK int mi_batch_add_layer_path_spec(mi_batch* b, const char* blob_path, uint64_t piece_bytes, uint64_t tag_base, mi_tar** listing,
                                          uint8_t* blob_sha256, mi_layer_blob_info* info, mi_inflate_spec_info* spec_info);
/* step.commitLayer (lib/builder/step/common.go:67-111) in one call on a MemFS handle: the step's layer by scan
 * (must_scan: the root is walked here, with the handle's blacklist) or by its copy operations, written through the layer
 * writer configured by cfg (tarAndGzipDiffs: tar framing, TarDigest, the gzip leg with its digest and size), folded into
 * the tree.  Neither a scan nor ops: "Nothing to do" -- *committed = 0, res untouched.  layer_out (may be NULL): the
 * layer's entries and source paths (mi_copy_layer_entries) and chunk roots (mi_copy_layer_roots); free with
 * mi_copy_layer_free.  Errors carry the reference's chain in mi_memfs_error ("failed to generate diff layer: write
 * diffs: ...").  MemFS.sync's one-second wait stays with the caller.
 *
 * ctx == NULL: the reference's commit, byte for byte -- tario.IsSimilarHeader decides what changed
 * (lib/tario/compare.go:24-120), the writer reads the changed files from disk (lib/tario/write.go:28-52).  Host logic.
 *
 * ctx != NULL: the CONTENT-AWARE commit -- the seam this library exists for (lib/snapshot/mem_fs.go:315-341,440-503 +
 * lib/builder/step/common.go:67-111 as one flow):
 *   1. the root (must_scan) or the ops' sources are walked and every regular file listed is staged into one batch of
 *      `ctx` while the walk goes on: each file is opened once and read once;
 *   2. the GPU cuts and hashes them (Gear CDC, SHA-256 per chunk, one chunk root per file);
 *   3. createLayerByScan / addToLayer run with the roots: a path is in the layer if its header changed (the reference's
 *      rule) OR its content did -- a same-size edit within the same second, invisible to the reference, is caught.  A
 *      file the tree holds without a root (merged from a base layer, committed with ctx == NULL) and whose header is
 *      unchanged takes the root it has now; from the next commit on its content is watched;
 *   4. the layer writer frames the tar; file content comes from HBM (mi_layer_add_batch_file): the tar holds the bytes
 *      the stored root describes, even if the file was written to after it was staged;
 *   5. with an index set (mi_memfs_set_index) the batch's chunk digests are added to it (mi_index_add_batch).
 * The roots a handle holds were computed with ONE chunk digest algorithm (mi_ctx_chunk_digest of the ctx that committed
 * them).  A commit with a ctx of the other algorithm would compare roots of different hashes and call every file changed:
 * it fails with MI_ERR_STATE before anything is walked or changed.  mi_memfs_commit_layer_n with ctxs that disagree among
 * themselves is MI_ERR_INVALID.  A handle on which no commit with a ctx has begun its scan takes either; a commit that fails
 * after that point may already have stored roots, so it fixes the algorithm as a successful one does.  mi_memfs_reset forgets
 * the tree and with it the algorithm.  Roots handed in from outside (mi_memfs_add_layer_by_scan's `roots`) are not tracked:
 * they must be of the algorithm that later commits on the handle use.
 * Steps 2-4 overlap: the scan runs on a thread of the library's own while the committing thread computes the layer and
 * frames the tar from the bytes that have landed; the diff waits for the scan only where a root DECIDES (a file the tree
 * holds with a root and an unchanged header).  A file that vanishes or shrinks between the walk and its staging therefore
 * fails the commit AFTER the tree took the layer -- as a failing tar write does in the reference (MemFS.AddLayerByScan
 * updates the tree, then writes; lib/snapshot/mem_fs.go:260-274).  MI_COMMIT_PIPELINE=0: one step after the other.
 * The handle keeps the batch (device memory sized by the largest commit so far) for its next commit; it belongs to
 * `ctx`: free the handle, or call mi_memfs_release_device, before mi_ctx_destroy.  A scanned tree larger than the device's
 * free memory is not refused: its roots are computed in windows (runs of files the device has room for; MI_COMMIT_WINDOW_MB)
 * and the writer reads the layer's files from disk -- a second read for those, mi_commit_stats.n_windows says so; copy ops
 * whose sources do not fit go the same way (planned again without a batch).  mi_memfs_commit_stats: what the last
 * commit did.                                                                                                            */
typedef struct {
    uint64_t n_walked;           /* paths the walk(s) listed                                                    */
    uint64_t n_scanned_files;    /* regular files staged and scanned on the GPU (0 with ctx == NULL)            */
    uint64_t scanned_bytes;
    uint64_t n_chunks;
    uint64_t n_layer_entries;    /* headers in the layer                                                        */
    uint64_t n_layer_files;      /* ... of them regular files with content                                      */
    uint64_t layer_file_bytes;
    uint64_t n_content_changed;  /* files IsSimilarHeader calls similar whose chunk roots differ: in the layer  */
    uint64_t n_roots_learned;    /* unchanged files that had no root in the tree and have one now               */
    uint64_t n_content_trusted;  /* MI_MEMFS_TRUST_CTIME: files that were not read again (their inode is as it was)  */
    uint64_t n_index_new, n_index_known;   /* mi_index_add_batch's counts (index set)                           */
    uint64_t index_new_bytes;    /* ... and the bytes of the chunks no earlier commit held: what a chunk-addressed
                                    store would have to take in for this commit                                 */
    uint64_t files_opened;       /* file descriptors whose content was read, by every thread of the library ... */
    uint64_t file_bytes_read;    /* ... and the bytes read from them, during this commit (process-wide counters:
                                    a commit running beside another one counts both)                            */
    uint64_t pipelined;          /* 1: the scan ran beside the diff and the tar writer (its time is not in the sum) */
    uint64_t n_windows;          /* 0 normally; k: the tree did not fit the device and was scanned in k windows (the
                                    layer's files were then read from disk by the writer: a second read for those)   */
    double   s_walk_stage;       /* walk (+ staging, which goes on behind it)                                   */
    double   s_scan;             /* end of staging + the GPU passes + the roots' way back (pipelined: on a thread
                                    of its own, overlapping s_diff and s_write)                                 */
    double   s_diff;             /* createLayerByScan / addToLayer + commit order                               */
    double   s_write;            /* tar framing, digests, gzip leg                                              */
    double   s_total;
    uint64_t n_verified_files;   /* layer files whose framed bytes were held against the sums taken where they were read
                                    (MI_FLAG_FILE_SUMS: every file the writer took out of HBM) ...                   */
    uint64_t verified_bytes;     /* ... and their bytes                                                          */
    uint64_t n_refetched;        /* 1 MiB chunks that differed and were right at the second fetch from HBM (a commit
                                    with a chunk that differs twice fails)                                         */
    uint64_t arena_bytes;        /* device memory behind the handle's arena after this commit ...                */
    uint64_t arena_pieces;       /* ... in how many pieces (the arena of a commit is an address range mapped piece by
                                    piece behind the walk: csrc/mi_arena.hip) ...                                  */
    uint64_t arena_moves;        /* ... and how often its base address changed during this commit -- each time the reader
                                    threads were drained and, until round 5, the arena copied.  0, unless the tree
                                    outgrew the address range (four times the first estimate, 32 GiB at least)      */
    uint64_t n_ctxs;             /* GPUs the commit ran on (mi_memfs_commit_layer_n; 1 otherwise, 0 with ctx == NULL) ... */
    uint64_t ctx_bytes_max, ctx_bytes_min;   /* ... and the bytes the fullest and the emptiest of them were handed        */
    uint64_t n_split_files;      /* files of 256 MiB and more (MI_COMMIT_SPLIT_MIB) that were split over the GPUs as parts     */
} mi_commit_stats;
MI_CORE int  mi_memfs_commit_layer(mi_memfs* fs, mi_ctx* ctx, int must_scan, const mi_copy_op* ops, uint64_t n_ops,
                           const mi_layer_config* cfg, mi_layer_result* res, mi_copy_layer** layer_out, int* committed);
/* The same commit over n_ctx GPUs of one node, one ctx each (north_star: "file batches shard across the 8 GPUs"): what the walk
 * hands over goes to the GPU with the fewest bytes so far, every GPU stages through its own reader threads and PCIe link and scans
 * its share; roots come back in the walk's order, the tar writer reads each file from the GPU that holds it, the chunk index (on
 * any one of the ctxs) takes the other GPUs' digests through the host.  Layer, roots and DigestPair are those of the one-GPU
 * commit, byte for byte.  n_ctx = 1: mi_memfs_commit_layer; n_ctx = 0: the reference's commit.  A handle keeps its batches
 * between commits as long as it is called with the same ctxs.  A file of 256 MiB and more (MI_COMMIT_SPLIT_MIB) is split over the
 * GPUs as parts (the parts protocol below: a halo of 256 KiB per boundary is read twice, the file is opened once per part); its root
 * is mi_chunk_root over the parts' digests, its bytes are checked chunk by chunk like everybody's.  UNMEASURED on more than one
 * physical GPU (tested with n ctxs on one device, and on the HIP double): mi_commit_stats.n_ctxs / ctx_bytes_max / _min.        */
MI_CORE int  mi_memfs_commit_layer_n(mi_memfs* fs, mi_ctx* const* ctxs, uint32_t n_ctx, int must_scan, const mi_copy_op* ops,
                             uint64_t n_ops, const mi_layer_config* cfg, mi_layer_result* res, mi_copy_layer** layer_out,
                             int* committed);
MI_CORE int  mi_memfs_commit_stats(const mi_memfs* fs, mi_commit_stats* out);
/* Options of a handle's content-aware commits (default: none).
 * MI_MEMFS_TRUST_CTIME: a scan commit does not read a regular file again whose inode is what it was when the tree's root for
 * it was computed -- same device, inode number, size, mtime and ctime, to the nanosecond.  ctime is the kernel's own record
 * of the last change of an inode and cannot be set from user space (utimes sets it to "now"), so the same-size same-SECOND
 * rewrite the reference misses still changes it.  What git calls "racily clean" is handled as git does: a file whose ctime is
 * not safely older than the moment its content was read (MI_TRUST_CTIME_SLACK_MS, default 20: the kernel's timestamps tick
 * every 1-4 ms; two seconds for a ctime without a sub-second part -- a file system that keeps whole seconds) is read again.
 * With the option a commit that changed nothing costs a walk and a diff (the reference's price) instead of a read of the
 * whole tree; the layer, the roots and the DigestPair are the same unless the kernel's timestamps lie (a clock set back
 * between a write and the next one to the same file).  Scan commits only.                                               */
#define MI_MEMFS_TRUST_CTIME 0x1u
/* MI_MEMFS_CHUNK_PACK: a content-aware scan or copy commit on ONE ctx, with an index set, also packs exactly the rows whose
 * bytes index_new_bytes counts (known[i] == 0 and dup_of < 0) -- mi_batch_pack_chunks with MI_PACK_VERIFY, after the index took
 * the batch, while the handle's batch still holds the tree's bytes -- and keeps every layer file's ordered chunks (its recipe:
 * mi_copy_layer_chunks).  mi_memfs_take_pack hands the pack over.  With the option and no index the commit fails with
 * MI_ERR_STATE, with mi_memfs_commit_layer_n and n_ctx > 1 with MI_ERR_INVALID, both before anything is walked.  A commit in
 * windows (n_windows > 0) succeeds as before and has no pack (take: MI_ERR_STATE); a pack that cannot be built (MI_ERR_NOMEM) does
 * not fail the commit -- the layer is written -- and the take returns the error.  Without the option nothing changes.       */
#define MI_MEMFS_CHUNK_PACK 0x2u
/* MI_MEMFS_CHUNK_ZPACK: MI_MEMFS_CHUNK_PACK in every respect but the product -- the same rows (known[i] == 0 and dup_of < 0), the
 * same recipes (mi_copy_layer_chunks works under either option), the same refusals (no index: MI_ERR_STATE; n_ctx > 1:
 * MI_ERR_INVALID; both before anything is walked), a commit in windows succeeds and has no zpack (take: MI_ERR_STATE with the
 * reason), a zpack that cannot be built does not fail the commit -- but the chunks are coded straight from the batch's arena into a
 * COMPRESSED pack (mi_batch_zpack_chunks with MI_ZPACK_VERIFY, while the handle's batch still holds the tree's bytes), which
 * mi_memfs_take_zpack hands over: byte for byte what mi_memfs_take_pack followed by mi_pack_compress gives.  Setting BOTH options
 * is MI_ERR_INVALID from mi_memfs_set_options: mi_pack_compress, or a decode, makes the other form; the commit does not do the
 * work twice.                                                                                                              */
#define MI_MEMFS_CHUNK_ZPACK 0x4u
/* MI_MEMFS_ZPACK_LEVEL2: beside MI_MEMFS_CHUNK_ZPACK (alone it changes nothing), the commit's zpack is coded at level 2
 * (mi_batch_zpack_chunks with MI_ZPACK_VERIFY | MI_ZPACK_LEVEL2): mi_memfs_take_zpack is then byte for byte what
 * mi_memfs_take_pack followed by mi_pack_compress(MI_ZPACK_LEVEL2) gives.  The layer, the recipes and the index are the same. */
#define MI_MEMFS_ZPACK_LEVEL2 0x10u
/* MI_MEMFS_GZIP_DEVICE: a commit with a ctx codes its layer's gzip leg on that ctx's device (mi_layer_set_gzip_ctx; with
 * mi_memfs_commit_layer_n on ctxs[0]'s).  With ctx == NULL the commit fails with MI_ERR_STATE before anything is walked.  At
 * MI_GZIP_OFF or level 0 the option has no effect.  A commit in windows takes it like any other.  The layer, TarDigest, roots,
 * index, packs and recipes are unchanged by the option: only gzip_sha256 and gzip_bytes differ.                                */
#define MI_MEMFS_GZIP_DEVICE 0x40u   /* (0x8 and 0x20 stay refused) */
MI_CORE int  mi_memfs_set_options(mi_memfs* fs, uint32_t options);
/* From now on every content-aware commit of this handle adds its batch to `index` (NULL: stop).  The index must belong
 * to the ctx the commits run on and outlive them; the handle does not own it.                                          */
MI_CORE int  mi_memfs_set_index(mi_memfs* fs, mi_index* index);
/* The handle's batch ahead of its first content-aware commit, with room for `files` files of `bytes` bytes in total: a
 * ctx's first use costs (the reader threads: 40-55 ms; device memory: by the byte on some boxes, 47-68 ms per
 * GiB at every allocation) -- a host that knows what is coming, e.g. the size of the base image it is pulling, pays them beside its own work.
 * Optional.                                                                                                              */
MI_CORE int  mi_memfs_reserve_device(mi_memfs* fs, mi_ctx* ctx, uint64_t files, uint64_t bytes);
/* Gives back the batch a content-aware commit left with the handle (its arena holds the scanned tree's bytes).          */
MI_CORE int  mi_memfs_release_device(mi_memfs* fs);
/* The chunk root the tree holds for `path` ("/"-rooted, relative to the handle's root): *has_root = 0 when the path was
 * never scanned; MI_ERR_INVALID when the tree does not hold the path.                                                  */
MI_CORE int  mi_memfs_root_of(const mi_memfs* fs, const char* path, uint8_t* root_out, int* has_root);
/* The chunk roots of a layer's entries, in mi_copy_layer_entries' order: roots = n x 32 bytes, has_root = n flags
 * (regular files of a content-aware commit carry one; everything else zeros).                                          */
MI_CORE int  mi_copy_layer_roots(const mi_copy_layer* layer, uint8_t* roots, uint8_t* has_root, uint64_t cap);
/* The header block(s) mi_layer_add would write for `e` (512 bytes, or 1536+ with a PAX record) in
 * a layer begun with `layer_flags` (MI_LAYER_*).                                                 */
MI_BLOCK int  mi_layer_header_bytes(const mi_tree_entry* e, uint32_t layer_flags, uint8_t* out, uint64_t cap, uint64_t* n);

/* ---- cache entry codec (cache.Manager seam, lib/cache/cache_manager.go:34-35,239-252) -------- *
 * key   = "makisu_builder_cache_" + cacheID;
 * entry = "<tarHex>,<gzipHex>" (createEntry), or "MAKISU_CACHE_EMPTY" for a step that produced no
 *         layer (pass NULL, NULL); parse is parseEntry + PullCache's empty-entry case: *is_empty
 *         = 1 means "cached, and there is no layer"; an entry without "," is MI_ERR_INVALID
 *         (the reference wraps it as ErrorLayerNotFound).                                      */
MI_CORE int mi_cache_key(const char* cache_id, char* out, uint64_t cap);
MI_CORE int mi_cache_create_entry(const uint8_t* tar_sha256, const uint8_t* gzip_sha256, char* out, uint64_t cap);
MI_CORE int mi_cache_parse_entry(const char* entry, int* is_empty, uint8_t* tar_sha256, uint8_t* gzip_sha256);
/* parseEntry to the letter (cache_manager.go:239-245): the two halves around the FIRST comma, each
 * behind "sha256:", whatever they contain -- the reference does not validate them (the strict form
 * above needs two 64-digit hex halves because it hands out raw digests).  MI_ERR_INVALID without a
 * comma, MI_ERR_CAPACITY if a half does not fit.                                                 */
MI_CORE int mi_cache_parse_entry_str(const char* entry, char* tar_digest, uint64_t tar_cap, char* gzip_digest,
                             uint64_t gzip_cap);

/* ---- standalone digests (image.Digester seam) ---------------------------------- *
 * n independent byte strings -> n SHA-256 digests: the batched form of
 * image.NewDigester().FromBytes / FromReader (lib/docker/image/digester.go:45-60;
 * `makisu push`: bin/makisu/cmd/push.go:207,230).  data: host pointer, string i =
 * data[offsets[i] .. offsets[i]+lens[i]).  out: n x 32 bytes.
 * Many short strings (manifests, configs, small files): one GPU lane each.  Long ones -- a
 * `docker save` layer tar -- on host threads with SHA-NI, one stream per thread, straight from
 * `data`, beside the GPU's launch: one lane does 13.5 MB/s, one core 2.4 GB/s, and a
 * Merkle-Damgard stream cannot be split ("must stay on a CPU core").
 * route_long_strings (csrc/mi_stage.hip) sends the length classes to the host that make
 * max(host time, GPU time) smallest: eight 128 MiB blobs take 0.06-0.12 s on eight cores
 * instead of 10 s on eight lanes; 100 000 x 64 KiB stay on the GPU.  MI_SHA_HOST_THREADS
 * (default: the cores the process may use, at most 16); MI_SHA_LONG_ON_GPU=1 keeps every
 * string on a lane (tests).                                                                */
MI_CORE int mi_sha256_many(mi_ctx* ctx, const void* data, const uint64_t* offsets,
                   const uint64_t* lens, uint64_t n, uint8_t* out);

/* ---- chunk index: dedup across batches (keyvalue.Store seam) -------------------- *
 * A device-resident set of chunk digests that outlives a batch.  The reference
 * remembers earlier work as content-addressed layers (IsExist + CAS link,
 * lib/builder/step/common.go:88-91) and as cacheID -> "tarHex,gzipHex" strings
 * behind keyvalue.Store (lib/cache/keyvalue/store.go:22-26, written at
 * lib/cache/cache_manager.go:239-252); this is the chunk-granular analogue:
 * "which chunks of this layer did an earlier layer already hold?".
 *
 * mi_index_add_batch: for every chunk of a batch that has run, known[i] = 1 if its
 * digest was in the index BEFORE the call (an in-batch repeat of a new digest stays
 * 0 - dup_of already says so), then the new digests are added.  known may be NULL.
 * mi_index_export / mi_index_import move the set as a flat blob of 32-byte digests
 * (order unspecified) so the shim can keep it behind keyvalue.Store.Put/Get.
 *
 * An index holds digests of ONE algorithm, its ctx's (mi_ctx_chunk_digest): it takes
 * batches of its own ctx only, and a commit whose ctxs hash with the other algorithm
 * fails with MI_ERR_INVALID before it starts (mi_memfs_set_index).  The blob of
 * mi_index_export is raw digests and says nothing about their algorithm: the caller
 * keeps the algorithm with the blob and imports it into an index of the same kind --
 * SHA-256 and BLAKE2s digests of the same chunk never compare equal, so a mixed-up
 * index silently knows nothing.                                                    */
MI_CORE int  mi_index_create(mi_ctx* ctx, uint64_t capacity_hint, mi_index** out);
MI_CORE void mi_index_free(mi_index* index);
MI_CORE int  mi_index_count(mi_index* index, uint64_t* n_digests);
MI_BLOCK int  mi_index_add_batch(mi_index* index, mi_batch* b, uint8_t* known, uint64_t cap,
                        uint64_t* n_new, uint64_t* n_known);
MI_CORE int  mi_index_export(mi_index* index, void* out_digests, uint64_t cap_digests);
MI_CORE int  mi_index_import(mi_index* index, const void* digests, uint64_t n, uint64_t* n_new);

/* ---- chunk packs: a batch's selected chunks as ONE blob, gathered on the device ---------------------- *
 * mi_index_add_batch says which chunks of a layer no earlier layer held, mi_commit_stats.index_new_bytes counts their
 * bytes; a pack DELIVERS them: what a chunk-addressed store behind keyvalue.Store (lib/cache/keyvalue/store.go:22-26) takes
 * in for a layer, next to the files' recipes (their ordered chunk digests: mi_batch_chunks).  The reference has no
 * counterpart: its unit is the layer blob (lib/builder/step/common.go:88-91).
 *   mi_batch_pack_chunks  select: n_select flags in host memory, n_select = the batch's chunk count; NULL = every row.  Rows
 *                         with a non-zero flag go in, in ascending row order -- duplicates too if the caller selects them.
 *                         Entry k begins at the sum of the lengths before it, each rounded up to 16; the pad bytes behind a
 *                         chunk are zero: the blob is a pure function of the rows and their bytes.  The batch must have run
 *                         and not be in flight (MI_ERR_STATE); a group head (mi_memfs_commit_layer_n's batch) and a wrong
 *                         n_select are MI_ERR_INVALID; part rows are rows like any other; an empty selection is a valid pack
 *                         of 0 entries.  The blob lives in device memory of its own: if it does not fit, MI_ERR_NOMEM naming
 *                         both sizes, nothing else has changed, and the caller may pack in several calls with partial
 *                         selections.  A pack points at its ctx (free it before mi_ctx_destroy, which refuses while one
 *                         lives) but not at its batch: it survives mi_batch_reset and mi_batch_free.
 *                         MI_PACK_VERIFY: the blob's entries are hashed again on the device (the ctx's algorithm) and held
 *                         against the batch's digests; one differing row fails the call with MI_ERR_IO naming the row, its
 *                         arena offset and its blob offset, and no pack is returned.
 *   mi_pack_entries       the entries in blob order (cap = rows `out` has room for).
 *   mi_pack_read          bytes [offset, offset + len) of the blob through two pinned windows of the pack's own (8 MiB each:
 *                         a reader that streams finds the next window on its way); outside the blob: MI_ERR_INVALID.
 *   mi_pack_device        the blob where it lies (valid until mi_pack_free); NULL for an empty pack.
 *   mi_pack_check         host logic, no ctx, no GPU -- what the pulling side runs before it trusts a pack: the entries lie
 *                         inside the blob on 16-byte offsets, ascending, without overlap; the pad bytes are zero; every chunk
 *                         hashes to its digest under alg (MI_DIGEST_*).  MI_OK, or MI_ERR_INVALID with *first_bad = the
 *                         first entry that fails (an unknown alg: MI_ERR_INVALID).                                    */
#define MI_PACK_VERIFY 0x1u
typedef struct mi_pack mi_pack;
typedef struct {               /* 56 bytes */
    uint8_t  digest[32];       /* the row's chunk digest (the ctx's algorithm) */
    uint64_t offset;           /* where the chunk begins in the blob: a multiple of 16 */
    uint64_t chunk_index;      /* the row in the batch's chunk table */
    uint32_t length;           /* bytes */
    uint32_t reserved;         /* 0 */
} mi_pack_entry;
typedef struct {
    uint64_t n_entries, blob_bytes, chunk_bytes;   /* blob_bytes = sum of lengths rounded up to 16 */
    uint32_t alg;              /* MI_DIGEST_* of the ctx that made it */
    uint32_t verified;         /* 1: the blob was hashed again on the device and every digest agreed */
    double   ms_gather, ms_verify;
} mi_pack_info;
MI_BLOCK int  mi_batch_pack_chunks(mi_batch* b, const uint8_t* select, uint64_t n_select, uint32_t flags, mi_pack** out);
MI_BLOCK int  mi_pack_get_info(const mi_pack* p, mi_pack_info* out);
MI_BLOCK int  mi_pack_entries(const mi_pack* p, mi_pack_entry* out, uint64_t cap);
MI_BLOCK int  mi_pack_read(mi_pack* p, uint64_t offset, void* dst, uint64_t len);
MI_BLOCK int  mi_pack_device(const mi_pack* p, const void** d_blob, uint64_t* blob_bytes);
MI_BLOCK void mi_pack_free(mi_pack* p);
MI_BLOCK int  mi_pack_check(const void* blob, uint64_t blob_bytes, const mi_pack_entry* entries, uint64_t n,
                   uint32_t alg, uint64_t* first_bad);
/* the pack of the handle's last commit (MI_MEMFS_CHUNK_PACK); the caller owns it (mi_pack_free).  MI_ERR_STATE with no commit
 * since the last take, and after a commit in windows; the pack's own error if it could not be built (mi_memfs_error says why) */
MI_BLOCK int mi_memfs_take_pack(mi_memfs* fs, mi_pack** out);
/* the ordered chunks of layer entry `entry` (mi_copy_layer_entries' order): digests n x 32 bytes, lengths n x u32;
   cap 0 sizes; regular files of a commit made with the option, *n = 0 for everything else */
MI_BLOCK int mi_copy_layer_chunks(const mi_copy_layer* layer, uint64_t entry, uint8_t* digests, uint32_t* lengths,
                                  uint64_t cap, uint64_t* n);

/* ---- the consuming side: files of a batch rebuilt on the device from packs and recipes ---------------------- *
 * A host that pulled packs (blob + entries) and recipes (mi_copy_layer_chunks' digests and lengths) from its chunk store puts
 * the layer's bytes back into a batch without the files ever existing on its disk: the batch is then an ordinary batch --
 * mi_batch_run gives the recipes' own rows and roots (same CDC parameters), mi_batch_read_file and mi_layer_add_batch_file
 * give the bytes and the layer tar with its TarDigest, mi_batch_pack_chunks packs again.
 *   mi_packset_create     a PACK SET: packs resident on the ctx's device, addressed by digest through a device hash table
 *                         (open addressing, the tag a digest's first 8 bytes; entries_hint sizes it, 0 is fine: it is
 *                         rebuilt at twice the size when it passes half full).  A child of its ctx: free it before
 *                         mi_ctx_destroy, which refuses while one lives.
 *   mi_packset_add_blob   a pack from host memory.  ALWAYS, on the host, before a byte is uploaded: the entries lie inside
 *                         the blob on 16-byte offsets, ascending, without overlap (offset + length rounded up to 16 <=
 *                         blob_bytes, without 64-bit wrap), n < 2^32 -- the structural half of mi_pack_check; a violation is
 *                         MI_ERR_INVALID with *first_bad = the entry (first_bad may be NULL), the set unchanged.  The blob goes
 *                         up through two pinned windows of the set's own into device memory of its own (does not fit:
 *                         MI_ERR_NOMEM naming both sizes, the set unchanged).  MI_PACKSET_VERIFY: the other half -- the pad
 *                         bytes are zero and every entry hashes to its digest under the ctx's algorithm, hashed on the device
 *                         by the ctx's own hashing kernel; MI_ERR_INVALID with *first_bad = the entry mi_pack_check names for
 *                         the same input, the set unchanged.  A digest the set holds already is kept once (the same pack
 *                         twice, another pack, several entries of one pack).  The same digest with ANOTHER LENGTH -- only
 *                         unverified input can hold one -- fails the add with MI_ERR_INVALID and the set is unusable from
 *                         then on: every later call with it is MI_ERR_STATE with that first message (sticky, like a staging
 *                         failure; mi_packset_free is what remains).
 *   mi_packset_add_pack   the same for a pack of the SAME ctx where it lies (mi_batch_pack_chunks, mi_memfs_take_pack): a
 *                         device-to-device copy; the pack stays the caller's.
 *   mi_batch_add_recipes  n_files files from their recipes: file i has n_chunks[i] rows, `digests` (32 bytes a row) and
 *                         `lengths` hold all files' rows end to end, a file's size is the sum of its lengths, 0 rows are an
 *                         empty file; user_tags may be NULL (tags 0).  The files are placed as mi_batch_add_synthetic places
 *                         them and may be mixed with host-fed files in any order.  BLOCKING: every row is looked up in the
 *                         set's table, the files are assembled in the arena by one destination-driven kernel, and the call
 *                         returns when the bytes lie there -- the set may be freed at once, the batch keeps no pointer to it.
 *                         MI_ERR_INVALID: a digest the set does not hold (the message names the file, the row within it and
 *                         the digest), a digest held with another length than the row states, a row of length 0, more than
 *                         2^32 - 1 rows, a set of another ctx, a group head; the smallest bad row is the one named.
 *                         MI_ERR_STATE: a batch that was staged already.  MI_RECIPE_VERIFY: the assembled ranges are hashed
 *                         where they lie (the ctx's hashing kernel) and held against the recipes' digests -- the end-to-end
 *                         check, whatever the set believed about its packs; a row that differs is MI_ERR_IO naming file, row,
 *                         arena offset and source address.  ANY failure leaves the batch as it was before the call.  Restored
 *                         rows carry no source sums (like synthetic rows): MI_RECIPE_VERIFY is their check.                */
#define MI_PACKSET_VERIFY 0x1u
#define MI_RECIPE_VERIFY  0x1u
typedef struct mi_packset mi_packset;
typedef struct {
    uint64_t n_packs, n_entries, n_digests /* distinct */, blob_bytes;
    uint32_t alg /* MI_DIGEST_* of the ctx */, reserved;
    double   ms_upload, ms_verify, ms_insert;      /* of the last add */
} mi_packset_info;
typedef struct {
    uint64_t n_files, n_rows, bytes;
    uint64_t n_joined_units;     /* 16-byte destination units assembled from more than one row (counted by the kernel) */
    double   ms_resolve, ms_assemble, ms_verify;
} mi_recipe_stats;
MI_BLOCK int  mi_packset_create(mi_ctx* ctx, uint64_t entries_hint, mi_packset** out);
MI_BLOCK int  mi_packset_add_blob(mi_packset* s, const void* blob, uint64_t blob_bytes, const mi_pack_entry* entries,
                                  uint64_t n, uint32_t flags, uint64_t* first_bad);
MI_BLOCK int  mi_packset_add_pack(mi_packset* s, const mi_pack* p, uint32_t flags);
MI_BLOCK int  mi_packset_get_info(const mi_packset* s, mi_packset_info* out);
MI_BLOCK void mi_packset_free(mi_packset* s);
MI_BLOCK int  mi_batch_add_recipes(mi_batch* b, const mi_packset* set, uint64_t n_files, const uint64_t* n_chunks,
                                   const uint8_t* digests, const uint32_t* lengths, const uint64_t* user_tags,
                                   uint32_t flags, mi_recipe_stats* stats_out);

/* ---- fetch only what is missing: a pack set asked by digest, and cut by digest into a new pack ------------------- *
 * What connects the two sides at chunk granularity.  The puller asks its own set which chunks of a layer's recipes it lacks
 * (the want list), the server cuts exactly those out of whatever packs hold them (one mi_pack), the puller adds that pack
 * (mi_packset_add_blob with MI_PACKSET_VERIFY) and assembles the layer (mi_batch_add_recipes) as before.  mi_packset_pack over a
 * store's live digests is also its compaction: live digests -> a pack -> a new set -> free the old one.  Both calls block on
 * the ctx stream, leave the set unchanged, take fewer than 2^32 rows (more: MI_ERR_INVALID) and answer MI_ERR_STATE with the
 * first message for a set in its sticky failed state.
 *   mi_packset_missing    digests: n x 32 bytes of host memory (a layer's recipes end to end); lengths: n x u32 or NULL.
 *                         held (optional, n bytes): 1 where the set holds the row's digest.  want_rows (cap = the rows it has
 *                         room for): the rows at which a digest the set lacks occurs for the FIRST time, ascending -- every
 *                         distinct missing digest once; the caller has digest and length at each row.  cap < n_want: nothing
 *                         is written to want_rows and the call is MI_ERR_CAPACITY with held and *info filled; cap = 0 with
 *                         want_rows = NULL is the sizing call and MI_OK.  With lengths: a row of length 0 is MI_ERR_INVALID;
 *                         a digest the set holds with another length than the row states is MI_ERR_INVALID naming the
 *                         smallest such row, its digest and both lengths (mi_batch_add_recipes' words); repeats of a MISSING
 *                         digest are not compared with each other -- nothing is known about it yet.  n = 0: MI_OK, *info zero.
 *   mi_packset_pack       an ordinary mi_pack of every distinct requested digest once, in order of first occurrence: entry k
 *                         = {digest, offset, chunk_index = the request row of the first occurrence, length = the SET'S,
 *                         reserved 0}, the blob laid out as mi_batch_pack_chunks lays it out -- entry k at the sum of the
 *                         lengths before it, each rounded up to 16, the pad bytes ZERO whatever the source blob held behind
 *                         the chunk (a set built without MI_PACKSET_VERIFY may hold non-zero pads): a pure function of the
 *                         request and the chunks' bytes, whichever pack held a chunk.  Everything that takes a pack takes
 *                         this one (mi_pack_get_info with alg = the ctx's, _entries, _read, _device, mi_packset_add_pack,
 *                         _free; mi_pack_check on the host).  The pack owns a COPY: it survives mi_packset_free; it is a
 *                         child of the set's ctx (mi_ctx_destroy refuses while it lives).  MI_ERR_INVALID: a digest the
 *                         set does not hold (or holds with 0 bytes: a pack has no entry for that), and with lengths a
 *                         stated length of 0 or another one than the set's -- *first_bad (may be NULL) = the smallest such
 *                         row, the message gives row and digest.  A blob that does not fit: MI_ERR_NOMEM naming both sizes,
 *                         nothing has changed, the caller splits the request.  n = 0: the empty pack.
 *                         MI_SUBPACK_VERIFY: the new blob's entries are hashed on the device (the ctx's algorithm) and held
 *                         against the REQUESTED digests; an entry that differs is MI_ERR_IO naming the request row (also in
 *                         *first_bad), the source address and the blob offset, and no pack is returned -- what catches a set
 *                         fed from an unverified, damaged blob.  mi_pack_info.verified, ms_gather and ms_verify as for a
 *                         batch's pack.                                                                                  */
#define MI_SUBPACK_VERIFY 0x1u
typedef struct {               /* 56 bytes */
    uint64_t n_rows, n_distinct;   /* request rows; distinct digests among them */
    uint64_t n_held, n_want;       /* distinct digests the set holds / lacks: n_held + n_want == n_distinct */
    uint64_t held_bytes;           /* sum of the SET's lengths over the held distinct digests */
    uint64_t want_bytes;           /* sum of the request's stated lengths over the want rows (0 when lengths == NULL) */
    double   ms_resolve;           /* device time of the call, HIP events on the ctx stream */
} mi_want_info;
MI_BLOCK int  mi_packset_missing(const mi_packset* s, const uint8_t* digests, const uint32_t* lengths, uint64_t n,
                                 uint8_t* held, uint64_t* want_rows, uint64_t cap, mi_want_info* info);
MI_BLOCK int  mi_packset_pack(const mi_packset* s, const uint8_t* digests, const uint32_t* lengths, uint64_t n,
                              uint32_t flags, mi_pack** out, uint64_t* first_bad);

/* ---- compressed packs ("zpacks"): every chunk coded on its own as one LZ4 block, on the device ------------------- *
 * What a chunk store keeps at rest and sends over the wire instead of plain bytes: take_pack -> mi_pack_compress -> store; the
 * puller hands blob and entries to mi_packset_add_zblob and goes on as before -- a set holds PLAIN chunks, whatever fed it.
 * FORMAT.  mi_zpack_entry is mi_pack_entry with `stored` where `reserved` was.  offset is a multiple of 16, entry k begins
 * at the sum of the stored sizes before it, each rounded up to 16, the pad bytes are zero, length is never 0.  stored ==
 * length: the chunk's bytes as they are.  stored < length: ONE STANDARD LZ4 BLOCK (token, literal-length extension bytes,
 * literals, a 2-byte little-endian offset in 1..65535, match-length extension bytes; the last sequence is literals only, the
 * last 5 bytes are literals, no match starts within the last 12 bytes) that any LZ4 library expands.  The coder keeps the block
 * only when it is smaller than length - (length >> 4); chunks under 13 bytes are always raw.  Blob and entries are a pure
 * function of the input pack and the LEVEL: no timing, no hardware write order, no device shows in them.
 * LEVELS.  The coder has two parses for the one format.  Level 1 (flags without MI_ZPACK_LEVEL2): the minimal parse, every byte
 * as before there were levels.  MI_ZPACK_LEVEL2: a denser parse (two hash tables, the longest of the step's matches, backward
 * extension, every position of a match remembered) that stores fewer bytes over a corpus -- NOT for every chunk: a single
 * chunk may store a few bytes more at level 2 than at level 1 -- and takes twice the LDS per wave.  The flag is taken by the calls
 * that CODE: mi_pack_compress and mi_batch_zpack_chunks, alone or with MI_ZPACK_VERIFY.  Nothing that reads, moves or decodes a
 * stored form takes it or needs it: mi_zpack_check, mi_packset_add_z*, mi_zset_add_z*, mi_zset_zpack, mi_zset_missing,
 * mi_zset_prune and mi_batch_add_zrecipes treat a block of either level alike.
 * THE ENTROPY STAGE (MI_ZPACK_ENTROPY, beside either level).  A stored span with stored < length whose FIRST BYTE IS 0x00 is an
 * entropy form, "form H" -- no LZ4 block begins with a token without literals: a match at output position 0 has no source:
 *     byte 0 0x00 | byte 1 kind | byte 2 S - 1 (0..63) | byte 3 0 | bytes 4..7 the inner length, u32 little-endian |
 *     128 bytes: 256 code lengths of 4 bits, symbol 2k in the low nibble of byte k, 0 = absent, 1..11 |
 *     S stream sizes, u16 little-endian | the streams
 * kind 1: the inner bytes are ONE STANDARD LZ4 BLOCK of the chunk, as above (0 < inner length < length); kind 2: they are the
 * chunk's plain bytes (inner length == length).  Stream s holds the symbols s, s + S, s + 2S, ... of the inner bytes in a
 * canonical Huffman code assigned by (length, symbol) ascending, packed as deflate packs: LSB first, codes bit-reversed, the
 * last byte of a stream padded with zero bits.  Form H is made only for chunks of at most 65 536 bytes, always with S = 32, and
 * kept only where it is smaller than the form under it (the level's LZ4 block, or the raw chunk) by more than a sixteenth of
 * that form; the code lengths are a stated function of the byte counts (tests/zentropy_cases.py): the stored form stays a pure
 * function of the chunk, the level and the stage.  Everything that MOVES stored spans (mi_zset_zpack, mi_zset_prune,
 * mi_zset_missing, the gathers) is untouched.  Everything that DECODES accepts form H with 1..64 streams: mi_zpack_check,
 * mi_packset_add_z*, MI_ZSET_VERIFY, MI_ZPACK_VERIFY and mi_batch_add_zrecipes unwrap it first (one classify launch where no
 * form H is; else one scratch for the inner forms -- it does not fit: MI_ERR_NOMEM naming its size, nothing changed).  The
 * unwrap trusts nothing; its refusals continue the decoder's numbering: 8 the header (kind, reserved byte, stream count, inner
 * length, a span shorter than header, table and sizes, a chunk above 65 536 bytes), 9 the code (a length above 11, no symbol,
 * an over-subscribed code; an incomplete one is legal), 10 stream sizes that do not sum to the rest of the span, 11 a stream
 * that ends early, meets an unassigned code, has a whole byte left over or a pad bit set; then the inner block's own rules.
 * A library from before the stage refuses such a span cleanly (its decoder fails the 0x00 token's offset).  mi_zset_recode takes
 * the flag beside the level and MI_ZSET_RECODE_VERIFY: its rule is unchanged (a stored form is replaced only where the candidate
 * is strictly smaller; a second call changes nothing), the candidate is the level's form with the stage over it, and with or
 * without the flag it decodes the form H a set already holds.  mi_batch_zpack_chunks and the commit's zpack options refuse the
 * flag: the commit's critical path codes at level 1, a store densifies at rest.
 *   mi_pack_compress      any pack (mi_batch_pack_chunks, mi_memfs_take_pack, mi_packset_pack), which stays the caller's and is
 *                         not changed.  Blocking, on the ctx stream.  The zpack is a child of the pack's ctx (mi_ctx_destroy
 *                         refuses while one lives).  0 entries: a zpack of 0 entries.  The coder's scratch (worst-case spans)
 *                         or the blob does not fit: MI_ERR_NOMEM naming both sizes, nothing has changed.  MI_ZPACK_VERIFY: the
 *                         new blob is decoded again on the device, hashed by the ctx's own hashing kernel and held against
 *                         the entries' digests; an entry that differs is MI_ERR_IO naming the entry, its offset and its
 *                         digest, and no zpack is returned.
 *   mi_zpack_entries, _read, _free   as their mi_pack_* namesakes (mi_zpack_read: two pinned windows of the zpack's own).
 *   mi_packset_add_zblob  a zpack from host memory into an ordinary set.  ALWAYS, on the host, before a byte is uploaded:
 *                         offsets on the 16-byte grid, ascending, without overlap, offset + stored rounded up to 16 <=
 *                         blob_bytes (no 64-bit wrap), 0 < stored <= length, n < 2^32; a violation is MI_ERR_INVALID with
 *                         *first_bad (may be NULL) = the entry, the set unchanged.  The blob goes up through the set's
 *                         windows and is decoded on the device into a plain blob laid out as a pack's.  The decoder trusts
 *                         nothing: an offset of 0 or beyond the bytes produced so far, a literal run or a length extension
 *                         that leaves the stored span, output that passes or falls short of `length`, stored bytes left over,
 *                         a non-zero pad byte each fail the entry; the smallest failing entry is named (MI_ERR_INVALID,
 *                         *first_bad, the message says which rule), the set unchanged.  Then as mi_packset_add_blob behind its
 *                         upload: MI_PACKSET_VERIFY hashes the PLAIN entries -- whatever the stream claimed, an entry that does
 *                         not hash to its digest never enters a verified set.
 *   mi_packset_add_zpack  the same for a zpack of the SAME ctx, decoded where it lies; the zpack stays the caller's.
 *   mi_zpack_check        host logic, no ctx, no GPU -- what a puller runs before it trusts a zpack: the structure as above,
 *                         zero pads, and every entry decodes under the device's rules to `length` bytes that hash to its
 *                         digest under alg.  MI_OK, or MI_ERR_INVALID with *first_bad = the entry the device path names for
 *                         the same input (structure first, then the first entry that does not decode, then the first that
 *                         does not hash).                                                                                */
#define MI_ZPACK_VERIFY 0x1u
#define MI_ZPACK_LEVEL2 0x4u   /* mi_pack_compress, mi_batch_zpack_chunks: the denser parse (LEVELS above) */
#define MI_ZPACK_ENTROPY 0x20u /* mi_pack_compress, mi_zset_recode: the entropy stage over the level's forms (THE ENTROPY STAGE above) */
typedef struct mi_zpack mi_zpack;
typedef struct {               /* 56 bytes: mi_pack_entry's layout */
    uint8_t  digest[32];       /* of the chunk's PLAIN bytes (the ctx's algorithm) */
    uint64_t offset;           /* where the stored form begins in the blob: a multiple of 16 */
    uint64_t chunk_index;      /* as in the pack the zpack was made from */
    uint32_t length;           /* the chunk's bytes, never 0 */
    uint32_t stored;           /* bytes in the blob: == length raw, < length one LZ4 block or, first byte 0x00, form H */
} mi_zpack_entry;
typedef struct {               /* 80 bytes */
    uint64_t n_entries, blob_bytes, chunk_bytes;   /* blob_bytes = sum of stored sizes rounded up to 16 */
    uint64_t stored_bytes;     /* sum of the stored sizes */
    uint64_t n_raw;            /* entries stored as they are */
    uint32_t alg;              /* MI_DIGEST_* of the ctx that made it */
    uint32_t verified;         /* 1: decoded again on the device and every digest agreed */
    double   ms_encode, ms_compact, ms_verify;     /* HIP events on the ctx stream */
    double   ms_decode;        /* the part of ms_verify that is the decode kernel over the whole blob */
} mi_zpack_info;
MI_BLOCK int  mi_pack_compress(const mi_pack* p, uint32_t flags, mi_zpack** out);
MI_BLOCK int  mi_zpack_get_info(const mi_zpack* z, mi_zpack_info* out);
MI_BLOCK int  mi_zpack_entries(const mi_zpack* z, mi_zpack_entry* out, uint64_t cap);
MI_BLOCK int  mi_zpack_read(mi_zpack* z, uint64_t offset, void* dst, uint64_t len);
MI_BLOCK void mi_zpack_free(mi_zpack* z);
MI_BLOCK int  mi_packset_add_zblob(mi_packset* s, const void* blob, uint64_t blob_bytes, const mi_zpack_entry* entries,
                                   uint64_t n, uint32_t flags, uint64_t* first_bad);
MI_BLOCK int  mi_packset_add_zpack(mi_packset* s, const mi_zpack* z, uint32_t flags);
MI_BLOCK int  mi_zpack_check(const void* blob, uint64_t blob_bytes, const mi_zpack_entry* entries, uint64_t n,
                             uint32_t alg, uint64_t* first_bad);
/* the census of a zpack's (a compressed pack set's) stored forms, counted on the device from every span's first bytes: [0] raw,
 * [1] one LZ4 block, [2] form H over an LZ4 block, [3] form H over the plain bytes.  Nothing is decoded: a span an unverified set
 * holds that begins like form H counts by its kind byte alone, 1 under [2] and ANY other value under [3].  Blocking, on the ctx
 * stream.  The info structs do not change */
typedef struct {               /* 64 bytes */
    uint64_t n[4];             /* entries (digests) of each form */
    uint64_t stored[4];        /* the sum of their stored sizes */
} mi_zforms;
MI_BLOCK int  mi_zpack_count_forms(const mi_zpack* z, mi_zforms* out);

/* ---- compressed pack sets: zpacks resident AS STORED, cut by digest and restored without recoding ------------------ *
 * A chunk's stored form is a pure function of its bytes and the level (every chunk is coded on its own), so a store server
 * answers a want list by MOVING stored spans -- no decode, no parse -- and the result is byte for byte what mi_packset_pack
 * followed by mi_pack_compress AT THE LEVEL THE SPANS WERE CODED AT gives; a puller decodes every recipe row straight to its
 * place in the arena, no plain blob in between.  A set that meets the same digest at two levels keeps the first form, under the
 * rule below; mi_zset_zpack, mi_zset_missing, mi_zset_prune and mi_batch_add_zrecipes take no level flag: they move or decode
 * stored forms, whoever coded them.
 *   mi_zset_create        a COMPRESSED PACK SET: a device hash table as mi_packset_create makes one (open addressing, the tag a
 *                         digest's first 8 bytes, entries_hint sizes it, rebuilt at twice the size when it passes half full); a
 *                         slot holds the digest, the device address of the stored span and length | stored << 32.  A child of
 *                         its ctx: free it before mi_ctx_destroy, which refuses while one lives.
 *   mi_zset_add_zblob     a zpack from host memory.  ALWAYS first, on the host: mi_packset_add_zblob's structural check, with
 *                         its message and its *first_bad.  The blob goes up through two pinned windows of the set's own into
 *                         device memory of its own (does not fit: MI_ERR_NOMEM naming both sizes, the set unchanged) and stays
 *                         AS STORED.  A digest the set holds already is kept once, the first form wins; the same digest with
 *                         another `length` fails the add with MI_ERR_INVALID and the set is unusable from then on (sticky:
 *                         every later call is MI_ERR_STATE with that first message).  Without MI_ZSET_VERIFY no stream is
 *                         decoded: what an unverified set costs is paid by its readers (below).  MI_ZSET_VERIFY: the blob is
 *                         decoded on the device into a scratch laid out as a plain pack, hashed by the ctx's own hashing kernel
 *                         and held against the entries; the scratch is freed before the call returns.  An entry that breaks a
 *                         decoding rule, has a non-zero pad byte or does not hash to its digest is MI_ERR_INVALID with
 *                         *first_bad = the entry mi_zpack_check names for the same input, the set unchanged.
 *   mi_zset_add_zpack     the same for a zpack of the SAME ctx (a device-to-device copy); the zpack stays the caller's.
 *   mi_zset_zpack         mi_packset_pack for stored forms: an ordinary mi_zpack of every distinct requested digest once, in
 *                         order of first occurrence; entry k = {digest, offset, chunk_index = the request row of the first
 *                         occurrence, length, stored} as the set holds them, entry k at the sum of the stored sizes before it,
 *                         each rounded up to 16, the pad bytes ZERO whatever the source held.  Everything that takes a zpack
 *                         takes it (mi_zpack_get_info, _entries, _read, _free, mi_packset_add_zpack, mi_zset_add_zpack); it
 *                         owns a COPY and survives mi_zset_free.  mi_zpack_info: ms_encode is 0 (nothing is coded), ms_compact
 *                         the device time of lookup, scan and gather.  MI_ERR_INVALID with *first_bad (may be NULL) = the
 *                         smallest such row, the message giving row and digest: a digest the set lacks, a stated length of 0,
 *                         a stated length other than the set's.  Fewer than 2^32 rows; n = 0: the empty zpack.  A blob that
 *                         does not fit: MI_ERR_NOMEM naming both sizes, nothing has changed.  MI_ZPACK_VERIFY: the new blob is
 *                         decoded and hashed as mi_pack_compress does it; an entry that does not decode or does not hash to
 *                         the REQUESTED digest is MI_ERR_IO naming the request row (also in *first_bad), the entry's offset
 *                         and the digest, and no zpack is returned.
 *   mi_batch_add_zrecipes mi_batch_add_recipes from a compressed set, with its arguments, its placement, its errors and its
 *                         stats (n_joined_units is 0, ms_assemble the one kernel's time): every row is decoded -- a raw row
 *                         copied -- by one wave DIRECTLY to its byte position in the arena.  New: a row whose stored form does
 *                         not decode under mi_zpack_check's rules (a non-zero pad byte among them) is MI_ERR_INVALID naming
 *                         file, row within the file, digest and the rule; the smallest bad row is the one named.
 *                         MI_RECIPE_VERIFY hashes the assembled ranges where they lie.  ANY failure leaves the batch as it was. */
#define MI_ZSET_VERIFY 0x1u
typedef struct mi_zset mi_zset;
typedef struct {               /* 80 bytes */
    uint64_t n_packs, n_entries, n_digests /* distinct */;
    uint64_t blob_bytes;       /* stored spans held, each rounded up to 16: summed over the entries of every added zpack */
    uint64_t stored_bytes;     /* sum of stored over the distinct digests */
    uint64_t chunk_bytes;      /* sum of length over the distinct digests */
    uint32_t alg /* MI_DIGEST_* of the ctx */, reserved;
    double   ms_upload, ms_verify, ms_insert;      /* of the last add */
} mi_zset_info;
MI_BLOCK int  mi_zset_create(mi_ctx* ctx, uint64_t entries_hint, mi_zset** out);
MI_BLOCK int  mi_zset_add_zblob(mi_zset* s, const void* blob, uint64_t blob_bytes, const mi_zpack_entry* entries,
                                uint64_t n, uint32_t flags, uint64_t* first_bad);
MI_BLOCK int  mi_zset_add_zpack(mi_zset* s, const mi_zpack* z, uint32_t flags);
MI_BLOCK int  mi_zset_get_info(const mi_zset* s, mi_zset_info* out);
MI_BLOCK int  mi_zset_count_forms(const mi_zset* s, mi_zforms* out);   /* mi_zpack_count_forms for what the set holds now */
MI_BLOCK void mi_zset_free(mi_zset* s);
MI_BLOCK int  mi_zset_zpack(const mi_zset* s, const uint8_t* digests, const uint32_t* lengths, uint64_t n,
                            uint32_t flags, mi_zpack** out, uint64_t* first_bad);
MI_BLOCK int  mi_batch_add_zrecipes(mi_batch* b, const mi_zset* set, uint64_t n_files, const uint64_t* n_chunks,
                                    const uint8_t* digests, const uint32_t* lengths, const uint64_t* user_tags,
                                    uint32_t flags, mi_recipe_stats* stats_out);

/* ---- a compressed set cut for a reader that knows less than the set ------------------------------------------------ *
 * A set that was densified at rest holds form H almost everywhere, and mi_zset_zpack moves form H verbatim.  These two cuts take
 * the same request and follow mi_zset_zpack's contract word for word -- host digests and optional lengths, fewer than 2^32
 * rows, every distinct digest once in order of first occurrence, chunk_index = the request row of the first occurrence, n = 0:
 * the empty result; MI_ERR_INVALID with *first_bad and mi_zset_zpack's message words for a digest the set lacks, a stated length
 * of 0 or another one than the set's; MI_ERR_STATE with the first message for a sticky set; a blob that does not fit:
 * MI_ERR_NOMEM naming both sizes; the result owns a copy, survives mi_zset_free and is a child of the ctx; blocking, on the ctx
 * stream -- except where stated here.  THE SET NEVER CHANGES: mi_zset_get_info, _get_usage, _entries and _count_forms answer
 * the same before and after, on success and on every failure.  Neither call builds a plain set, a table or an intermediate zpack.
 *   mi_zset_zpack_unwrapped  THE CUT WITHOUT FORM H, for a reader built before the entropy stage.  An entry whose stored form in
 *                         the set is form H carries its INNER form: kind 1, the LZ4 block, stored = the inner length; kind 2,
 *                         the chunk's plain bytes, stored == length, a raw entry.  Every other entry is moved verbatim.  Entry k
 *                         lies at the sum of the NEW stored sizes before it, each rounded up to 16, the pads zero; the info
 *                         carries stored_bytes, n_raw and chunk_bytes of the new blob, ms_encode is 0, ms_compact the device
 *                         time of lookup, sizing, scan, unwrap and gather.  The stage wraps a chunk's FINISHED stored form, so
 *                         for forms the coders made the result is byte for byte, blob and entries, what mi_zset_zpack gives
 *                         from a set that was fed the same chunks coded at the same level WITHOUT MI_ZPACK_ENTROPY.  A
 *                         requested form H row that does not unwrap (rules 8..11, and 7 for the pad behind its span) is
 *                         MI_ERR_INVALID naming the request row, the digest and the rule, the smallest such row in *first_bad,
 *                         and no zpack is returned; the inner LZ4 block is MOVED, not decoded, and rows that are moved verbatim
 *                         are not looked at, as in mi_zset_zpack.  MI_ZPACK_VERIFY (the only flag) decodes and hashes the new
 *                         blob against the requested digests as mi_zset_zpack does, with its MI_ERR_IO message.  A request
 *                         that meets no form H is byte for byte mi_zset_zpack's answer; where form H is met, each such row is
 *                         unwrapped by one wave straight to its place in the new blob -- the inner length stands in the form's
 *                         header, so sizes and offsets come first and there is no scratch of inner forms.
 *   mi_zset_pack          THE PLAIN CUT, for a reader that knows no compression: mi_packset_pack's contract word for word over
 *                         a compressed set, an ordinary mi_pack -- length is the set's, entry k at the sum of the lengths
 *                         before it, each rounded up to 16, the pads zero, reserved 0; everything that takes a pack takes it --
 *                         byte for byte, blob and entries, what mi_packset_pack gives from a plain set fed the same zpacks.  One
 *                         launch, one wave an entry, decoded straight to its place: a raw row is copied, an LZ4 row decoded,
 *                         form H over raw unwrapped into the pack, form H over LZ4 unwrapped into a per-call scratch and decoded
 *                         from there by the same wave.  The scratch holds the inner lengths of the requested kind-1 rows only
 *                         (each rounded up to 64); if it does not fit: MI_ERR_NOMEM naming its size, nothing has changed.  A row
 *                         that does not decode under mi_zpack_check's rules (1..11, the non-zero pad among them) is
 *                         MI_ERR_INVALID naming the request row, the digest and the rule, the smallest bad row in *first_bad;
 *                         on one row an unwrap rule (8..11) comes before the inner block's (1..6) before the pad's (7).
 *                         MI_SUBPACK_VERIFY (the only flag) hashes the new blob with the ctx's algorithm against the requested
 *                         digests: MI_ERR_IO as in mi_packset_pack. */
MI_BLOCK int  mi_zset_zpack_unwrapped(const mi_zset* s, const uint8_t* digests, const uint32_t* lengths, uint64_t n,
                                      uint32_t flags /* MI_ZPACK_VERIFY only */, mi_zpack** out, uint64_t* first_bad);
MI_BLOCK int  mi_zset_pack(const mi_zset* s, const uint8_t* digests, const uint32_t* lengths, uint64_t n,
                           uint32_t flags /* MI_SUBPACK_VERIFY only */, mi_pack** out, uint64_t* first_bad);

/* ---- zpacks straight from the arena; a compressed set asked what it lacks ------------------------------------------ *
 * The producing side without the plain detour: the chunks of a batch are coded WHERE THEY LIE, so a commit hands a zpack over
 * without the plain blob, its gather and its hashing pass; and the pulling side asks the compressed set it keeps.  With both,
 * the compressed line needs no plain pack anywhere: commit -> zpack -> mi_zset_add_* -> mi_zset_zpack (the want list's cut) ->
 * mi_zset_missing / mi_batch_add_zrecipes on the puller.
 *   mi_batch_zpack_chunks mi_batch_pack_chunks' arguments and state rules, word for word: select: n_select flags in host memory,
 *                         n_select = the batch's chunk count, NULL = every row, non-zero bytes count as set; a wrong n_select,
 *                         a group head or unknown flags: MI_ERR_INVALID; a batch that has not run or is in flight:
 *                         MI_ERR_STATE; 2^32 or more entries: MI_ERR_INVALID; an empty selection: a zpack of 0 entries.  The
 *                         result is an ORDINARY mi_zpack, byte for byte (blob and entries) what mi_batch_pack_chunks +
 *                         mi_pack_compress gives for the same selection: chunk_index is the batch row; a child of the batch's
 *                         ctx that survives mi_batch_reset and mi_batch_free; everything that takes a zpack takes it.  Blocking,
 *                         on the ctx stream; the batch is not changed.  The call needs the coder's scratch (the sum of the
 *                         worst-case spans: the selected bytes + 0.4 % + up to 31 bytes a chunk) and the blob; if either does
 *                         not fit: MI_ERR_NOMEM naming the size and what the device has free, nothing has changed, the caller
 *                         splits the selection.  MI_ZPACK_LEVEL2: the denser parse, and then what mi_pack_compress gives
 *                         WITH THAT FLAG.  MI_ZPACK_VERIFY (the only other flag): the new blob is decoded again on the device
 *                         into the scratch, hashed by the ctx's own hashing kernel and held against THE BATCH'S digest table at
 *                         chunk_index -- one decode and one hashing pass vouch for both hops, arena -> stored form -> plain
 *                         again; an entry that differs or does not decode is MI_ERR_IO naming the entry, the chunk row, the
 *                         arena offset, the blob offset and the digest, and no zpack is returned.  mi_zpack_info: ms_encode the
 *                         coder's time, ms_compact plan + layout + gather, ms_verify / ms_decode as for mi_pack_compress.
 *   mi_memfs_take_zpack   the zpack of the handle's last commit (MI_MEMFS_CHUNK_ZPACK); the caller owns it (mi_zpack_free).
 *                         MI_ERR_STATE with no commit since the last take, and after a commit in windows; the zpack's own
 *                         error if it could not be built (mi_memfs_error says why).  A zpack nobody took is freed by the next
 *                         commit.
 *   mi_zset_missing       mi_packset_missing's contract, word for word, over a compressed set: held (optional, n bytes): 1
 *                         where the set holds the row's digest; want_rows (cap rows of room): the rows at which a digest the
 *                         set lacks occurs for the FIRST time, ascending; cap < n_want: nothing is written to want_rows and the
 *                         call is MI_ERR_CAPACITY with held and *info filled; cap = 0 with want_rows = NULL is the sizing call
 *                         and MI_OK.  With lengths: a row of length 0 is MI_ERR_INVALID; a digest the set holds with another
 *                         length than the row states is MI_ERR_INVALID naming the smallest such row, its digest and both
 *                         lengths.  held_bytes is the sum of the set's PLAIN lengths.  A set in its sticky failed state:
 *                         MI_ERR_STATE with the first message; fewer than 2^32 rows; n = 0: MI_OK, *info zero.  Blocking, on
 *                         the ctx stream; the set is not changed.                                                        */
MI_BLOCK int  mi_batch_zpack_chunks(mi_batch* b, const uint8_t* select, uint64_t n_select, uint32_t flags, mi_zpack** out);
MI_BLOCK int  mi_memfs_take_zpack(mi_memfs* fs, mi_zpack** out);
MI_BLOCK int  mi_zset_missing(const mi_zset* s, const uint8_t* digests, const uint32_t* lengths, uint64_t n,
                              uint8_t* held, uint64_t* want_rows, uint64_t cap, mi_want_info* info);

/* ---- pruning a compressed set in place ---------------------------------------------------------------------------- *
 * A set drops digests and gives device memory back without being cut into a new set: what a mark-and-sweep collector (the
 * digests that STAY) or an eviction list (the digests that GO) needs.  For every digest still held the set answers
 * mi_zset_zpack, mi_zset_missing and mi_batch_add_zrecipes exactly as before; a dropped digest is one that was never added.
 *   mi_zset_prune         digests: n x 32 bytes of host memory, n < 2^32, repeats allowed; a digest the set does not hold is
 *                         no error, its rows are counted in n_unknown.  flags: exactly one of MI_ZSET_PRUNE_KEEP (everything
 *                         else goes; n = 0 empties the set) and MI_ZSET_PRUNE_DROP (everything else stays; n = 0 changes
 *                         nothing); both, neither, an unknown flag or min_live_permille > 1000: MI_ERR_INVALID.  A BLOB is one
 *                         added zpack's bytes or an earlier prune's compaction blob; its live bytes are the sum of
 *                         round16(stored) over the surviving digests the set holds IN it (an entry that lost to "the first
 *                         form wins" was never live).  A blob with no live bytes is freed.  A blob with
 *                         live * 1000 < min_live_permille * its bytes as added is COMPACTED: its survivors are moved into ONE
 *                         new blob shared by all such blobs of the call, then it is freed; 0 never moves anything.  Moves are
 *                         VERBATIM: whole 16-byte units, round16(stored) bytes a span, the pad as it was (an unverified set's
 *                         non-zero pad stays what mi_batch_add_zrecipes refuses); stored form, length and stored size never
 *                         change.  The table is REBUILT for the survivors (a power of two, at least 1 024 slots, at most half
 *                         full): it shrinks.  mi_zset_info afterwards: n_digests, stored_bytes, chunk_bytes describe what is
 *                         held; n_packs, n_entries, blob_bytes stay sums over the zpacks that were added (residency:
 *                         mi_zset_get_usage).  Nothing to drop: the set is untouched, *info (may be NULL) still filled.  The
 *                         new table, the new blob and all scratch are allocated before anything changes and the old table
 *                         and blobs go only when the new table is complete: a failure leaves the set as it was.  A compaction
 *                         blob that does not fit is not an error: dead blobs still go, n_blobs_sparse_kept says how many
 *                         stayed; a table or scratch that does not fit: MI_ERR_NOMEM naming the size and what the device has
 *                         free.  A set in its sticky failed state: MI_ERR_STATE with the first message.  Zpacks cut and
 *                         batches restored earlier own their bytes and are not affected.  Blocking, on the ctx stream.
 *   mi_zset_get_usage     what is resident: blobs and the device bytes allocated for them, the live bytes, the table.
 *   mi_zset_entries       what the set holds, in no stated order: digests (32 bytes each), lengths, stored sizes -- any of the
 *                         three may be NULL; *n = how many there are; cap = 0 is the sizing call; 0 < cap < *n: MI_ERR_INVALID. */
#define MI_ZSET_PRUNE_KEEP 0x1u   /* digests = what stays; everything else goes */
#define MI_ZSET_PRUNE_DROP 0x2u   /* digests = what goes; everything else stays  (exactly one of the two) */
typedef struct {               /* 112 bytes */
    uint64_t n_rows, n_unknown;              /* request rows; rows whose digest the set did not hold (repeats counted per row) */
    uint64_t n_dropped, dropped_stored_bytes, dropped_chunk_bytes;   /* distinct digests removed, and their stored / length sums */
    uint64_t n_blobs_freed, freed_bytes;     /* blobs given back (wholly dead, or compacted away) and their ALLOCATED bytes */
    uint64_t n_blobs_compacted, moved_bytes; /* blobs whose survivors were moved; sum of round16(stored) moved */
    uint64_t n_blobs_sparse_kept;            /* blobs under the threshold that stayed because the new blob did not fit */
    uint64_t peak_extra_bytes;               /* device bytes this call allocated before it freed anything (new table + new blob + scratch), from the sizes */
    double   ms_mark, ms_move, ms_rebuild;   /* HIP events on the ctx stream */
} mi_prune_info;
typedef struct {               /* 40 bytes */
    uint64_t n_blobs, resident_bytes;        /* blobs held and the device bytes allocated for them */
    uint64_t live_bytes;                     /* sum of round16(stored) over the held digests */
    uint64_t table_slots, table_bytes;
} mi_zset_usage;
MI_BLOCK int  mi_zset_prune(mi_zset* s, const uint8_t* digests, uint64_t n, uint32_t flags, uint32_t min_live_permille,
                            mi_prune_info* info);
MI_BLOCK int  mi_zset_get_usage(const mi_zset* s, mi_zset_usage* out);
MI_BLOCK int  mi_zset_entries(const mi_zset* s, uint8_t* digests, uint32_t* lengths, uint32_t* stored, uint64_t cap,
                              uint64_t* n);

/* ---- recoding a compressed set in place ---------------------------------------------------------------------------- *
 * A commit codes at level 1 (level 2's encode is too slow for its critical path); a store densifies AT REST.  A resident set
 * codes every chunk it holds again at a requested level and replaces a stored form only where the new one is STRICTLY SMALLER:
 * no chunk ever grows, whatever the level does to it.  No plain pack set, no second set, no second table in the caller's hands.
 *   mi_zset_recode        flags: the level as the coders take it -- MI_ZPACK_LEVEL2, or absent = level 1 -- and optionally
 *                         MI_ZSET_RECODE_VERIFY and MI_ZPACK_ENTROPY (the candidate is then the level's form with the entropy
 *                         stage over it, "compressed packs" above); any other bit, or s = NULL: MI_ERR_INVALID.  THE RULE: for every digest the
 *                         set holds, `plain` is what its stored form decodes to (a raw form is its own bytes); the CANDIDATE
 *                         is exactly what the coder of the level stores for `plain` -- the LZ4 block if it is smaller than
 *                         length - (length >> 4), else raw; chunks under 13 bytes are always raw; the stored form is replaced
 *                         if and only if the candidate's size < stored, otherwise the entry keeps its bytes verbatim.  A
 *                         chunk's new form is a pure function of its current stored form and the level: a second call at the
 *                         same level changes nothing; `length` and the digest never change; a set of raw entries holds
 *                         afterwards, byte for byte, mi_pack_compress's forms at that level.  BLOBS: a blob with at least one
 *                         replaced entry is REWRITTEN -- every entry the table holds in it goes to ONE new blob shared by the
 *                         call, replaced entries in their new form with ZERO pads, the others verbatim (whole 16-byte units,
 *                         round16(stored) bytes a span, the pad as it was, as in mi_zset_prune) -- and then freed, with
 *                         whatever dead spans it carried.  A blob with no replaced entry is not touched: no span moves, no
 *                         address changes.  The order inside the new blob is the table's slot order, as in a prune's
 *                         compaction; no caller may depend on it.  The table is REBUILT through the set's own insert (a power
 *                         of two, at least 1 024 slots, at most half full) and swapped; the old table is never written.
 *                         Nothing to replace: the set is untouched -- no new blob, no new table -- and the call is MI_OK with
 *                         *info (may be NULL) filled.  mi_zset_info afterwards: stored_bytes describes what is held;
 *                         n_packs, n_entries and blob_bytes stay sums over what was added, as after a prune (residency and
 *                         live bytes: mi_zset_get_usage).  ROUNDS: scratch_bytes bounds one round's scratch -- the plain
 *                         bytes decoded (round16(length) of every coded entry; a raw one is coded where it lies) plus the
 *                         worst-case coded spans (length + length / 255 + 16, rounded up to 16) of its entries; 0 = 256 MiB; a
 *                         single chunk that needs more gets a round of its own with scratch of its size; the result does
 *                         not depend on scratch_bytes, n_rounds says how many ran.  The new forms wait in staging memory of
 *                         exactly their size (one piece a round) until the new blob is written.  UNDECODABLE ENTRIES: an
 *                         unverified set may hold a form that breaks a rule of mi_zpack_check (a non-zero pad byte among
 *                         them).  Without VERIFY that is no error: the entry is counted in n_undecodable and kept verbatim
 *                         -- moved verbatim if its blob is rewritten -- and readers refuse it exactly as before.  The decoder
 *                         is the bounds-safe one of every reader; neither it nor the coder reads or writes outside the span
 *                         and the scratch it was given.  MI_ZSET_RECODE_VERIFY: (a) every held entry's `plain` is hashed by
 *                         the ctx's own hashing kernel (SHA-256 or BLAKE2s, as the ctx is) and held against its digest; if
 *                         any entry does not decode or does not hash, the call is MI_ERR_IO, the message gives the count and
 *                         one such digest in hex, and the set is unchanged; (b) before the swap every replaced form is
 *                         decoded again FROM THE NEW BLOB and hashed against its digest; a difference is MI_ERR_IO saying so,
 *                         the set unchanged.  With VERIFY and nothing to replace the call is a scrub of the whole set.
 *                         Everything is allocated before anything changes: scratch, staging, new blob or table that does not
 *                         fit is MI_ERR_NOMEM naming the size and what the device has free, the set unchanged.  A set in its
 *                         sticky failed state: MI_ERR_STATE with the first message.  An empty set: MI_OK, *info zero.  Zpacks
 *                         cut and batches restored earlier own their bytes and are not affected.  Blocking, on the ctx
 *                         stream.  One GPU; a plain mi_packset has no counterpart.                                          */
#define MI_ZSET_RECODE_VERIFY 0x1u
typedef struct {               /* 152 bytes */
    uint64_t n_digests;                       /* held when the call began */
    uint64_t n_recoded, n_raw_recoded;        /* forms replaced; of them, those that were raw */
    uint64_t n_undecodable;                   /* stored forms that break a decoding rule: left as they are */
    uint64_t stored_before, stored_after;     /* sums of stored over the held digests */
    uint64_t live_before, live_after;         /* sums of round16(stored) */
    uint64_t n_blobs_rewritten, n_blobs_freed, freed_bytes, new_blob_bytes;   /* freed_bytes: ALLOCATED bytes given back */
    uint64_t n_rounds;
    uint64_t peak_extra_bytes;                /* as mi_prune_info's: device bytes this call allocated before it freed anything, from the sizes */
    double   ms_decode, ms_encode, ms_move, ms_rebuild, ms_verify;   /* HIP events on the ctx stream; ms_move: choose, stage, plan, gather */
} mi_recode_info;
MI_BLOCK int  mi_zset_recode(mi_zset* s, uint32_t flags, uint64_t scratch_bytes, mi_recode_info* info);

/* ---- ageing a compressed set ---------------------------------------------------------------------------------------- *
 * A store behind keyvalue.Store expires by age.  A set can know when each chunk was last used: a 32-bit STAMP per digest on
 * the device, a clock (the set's EPOCH) the caller advances, and "everything older than epoch E goes" through mi_zset_prune's
 * sweep, compaction and rebuild.  No timestamp table on the host, no digest list uploaded: touch, census, expire and
 * mi_index_retain_zset make a whole collection cycle.  What an epoch means (hours, builds, ...) is the caller's.  OFF UNTIL
 * ASKED FOR: until mi_zset_set_epoch is called nothing is allocated or launched for it, and every other call allocates,
 * answers and counts as before.  INVARIANT while ageing is on: every held digest has exactly one stamp, stamp <= epoch; the
 * stamp follows the digest through every table rebuild (growth inside an add, mi_zset_prune, mi_zset_recode, mi_zset_expire),
 * and those calls count the new table's stamp array (4 bytes a slot) in their peak_extra_bytes.  READERS DO NOT TOUCH:
 * mi_zset_zpack, both plainer cuts, mi_zset_missing and mi_batch_add_zrecipes take a const set; the caller touches with the
 * digests it passed to them.  Stamps are not kept across mi_zset_free (mi_zset_stamps over mi_zset_entries is what a caller
 * saves).  All calls block, run on the ctx stream, and answer MI_ERR_STATE with the first message for a set in its sticky failed
 * state.  One GPU; a plain mi_packset has no counterpart.  Measured once (profiles/chunk_zage.txt): on 10^6
 * digests an expiry that drops half is 1.68 ms a call against 2.30 ms for mi_zset_prune(DROP) fed the digests as a list.
 *   mi_zset_set_epoch     the first call turns ageing on: the stamp array (4 bytes x table slots) is allocated and everything
 *                         held is stamped `epoch`; if it does not fit: MI_ERR_NOMEM naming the size and what the device has
 *                         free, the set unchanged and ageing still off.  Later calls advance the clock: an epoch below the
 *                         set's is MI_ERR_INVALID, the same epoch changes nothing.  0xFFFFFFFF is reserved: MI_ERR_INVALID.
 *   mi_zset_get_epoch     *ageing = 1 once ageing is on, *epoch = the clock, *stamp_bytes = the device bytes allocated for the
 *                         stamps (0 while ageing is off); any of the three may be NULL.
 *   mi_zset_touch         digests: n x 32 bytes of host memory, n < 2^32, repeats allowed (NULL with n > 0, or more rows:
 *                         MI_ERR_INVALID; n = 0: MI_OK).  A held digest's stamp becomes the set's epoch; a digest the set lacks
 *                         is no error.  n_unknown counts the ROWS not held (repeats counted per row, as mi_prune_info does),
 *                         n_refreshed the DISTINCT digests whose stamp was older than the epoch before the call.  Nothing but
 *                         stamps changes.  Ageing off: MI_ERR_STATE saying so.
 *   adds                  while ageing is on every digest an add brings gets the current epoch, whether it is new or already
 *                         held: the first form still wins, but a re-add is a use.
 *   mi_zset_stamps        stamps[r] = the stamp of row r's digest, 0xFFFFFFFF where the set does not hold it.  Read-only.
 *                         Ageing off: MI_ERR_STATE.
 *   mi_zset_age_census    bounds: 1 to 255 strictly ascending values (anything else: MI_ERR_INVALID); bins: n_bounds + 1 entries.
 *                         Bin i takes the held digests with bounds[i-1] <= stamp < bounds[i]; bin 0 begins at stamp 0, the last
 *                         bin is open above.  live_bytes is the sum of round16(stored), as mi_zset_get_usage counts it: with
 *                         bounds = {E}, bin 0 is what mi_zset_expire(E) will drop -- how a store with a byte budget picks E.
 *                         Read-only.  Ageing off: MI_ERR_STATE.
 *   mi_zset_expire        drops every held digest whose stamp is below min_epoch; no list is involved.  For everything else
 *                         mi_zset_prune's contract with MI_ZSET_PRUNE_DROP, word for word: dead blobs are freed, blobs under
 *                         min_live_permille are compacted verbatim into one new blob in slot order, the table is rebuilt and
 *                         swapped, everything is allocated before anything changes (whatever fails, the set is as it was), a
 *                         compaction blob that does not fit is not an error (n_blobs_sparse_kept), nothing to drop leaves the
 *                         set untouched with *info (may be NULL) filled.  n_rows = n_unknown = 0.  Survivors keep their
 *                         stamps.  peak_extra_bytes: what mi_zset_prune allocates for the same drop with an empty request,
 *                         plus the new stamp array when the table is rebuilt.  min_epoch above the set's epoch is
 *                         MI_ERR_INVALID -- it would empty the set on a clock mistake, and MI_ZSET_PRUNE_KEEP with n = 0 is how
 *                         one empties a set; min_live_permille > 1000: MI_ERR_INVALID; ageing off: MI_ERR_STATE.               */
typedef struct {               /* 32 bytes */
    uint64_t n_rows, n_unknown;              /* request rows; rows whose digest the set did not hold (repeats counted per row) */
    uint64_t n_refreshed;                    /* distinct digests whose stamp was older than the epoch */
    double   ms_touch;                       /* HIP events on the ctx stream */
} mi_touch_info;
typedef struct {               /* 32 bytes */
    uint64_t n_digests, stored_bytes;        /* held digests whose stamp lies in the bin, and the sum of their stored sizes */
    uint64_t live_bytes, chunk_bytes;        /* sums of round16(stored) and of the lengths */
} mi_zage_bin;
MI_BLOCK int  mi_zset_set_epoch(mi_zset* s, uint32_t epoch);
MI_BLOCK int  mi_zset_get_epoch(const mi_zset* s, uint32_t* ageing, uint32_t* epoch, uint64_t* stamp_bytes);
MI_BLOCK int  mi_zset_touch(mi_zset* s, const uint8_t* digests, uint64_t n, mi_touch_info* info);
MI_BLOCK int  mi_zset_stamps(const mi_zset* s, const uint8_t* digests, uint64_t n, uint32_t* stamps);
MI_BLOCK int  mi_zset_age_census(const mi_zset* s, const uint32_t* bounds, uint32_t n_bounds, mi_zage_bin* bins);
MI_BLOCK int  mi_zset_expire(mi_zset* s, uint32_t min_epoch, uint32_t min_live_permille, mi_prune_info* info);

/* ---- the chunk index: asking without adding, forgetting ------------------------------------------------------------ *
 * The index's half of garbage collection.  A store that prunes its set (mi_zset_prune) hands the same list to the index, or a
 * builder's index would go on calling a dropped chunk "known", the commit would leave it out of its pack, and the layer's
 * recipe would name a digest no store holds.  A dropped digest is one that was never added: the next mi_index_add_batch or
 * mi_index_import reports it new and takes it again.
 *   mi_index_query        digests: n x 32 bytes of host memory, n < 2^32 (more, or NULL with n > 0: MI_ERR_INVALID).  held[i] =
 *                         1 if the index holds row i's digest -- every row is answered by the table alone, repeats each get
 *                         the answer; *n_held = the rows held; either may be NULL.  READ-ONLY: the count, the table's size and
 *                         the export are the same before and after; the table never grows.
 *   mi_index_query_batch  the same over the device-resident digests of a batch that has run (nothing is uploaded): held[i] for
 *                         every chunk row -- what a second mi_index_add_batch of an unchanged index would report as known; an
 *                         in-batch repeat of a digest the index lacks is 0.  mi_index_add_batch's rules: a batch of another
 *                         ctx: MI_ERR_INVALID; one that has not run: MI_ERR_STATE; held given and cap < n_chunks:
 *                         MI_ERR_CAPACITY.
 *   mi_index_prune        mi_zset_prune's argument rules: digests n x 32 bytes of host memory, n < 2^32, repeats allowed; a
 *                         digest the index does not hold is no error, its rows are counted in n_unknown, and a prune never
 *                         adds it.  flags: exactly one of MI_INDEX_PRUNE_KEEP (everything else goes; n = 0 empties the index)
 *                         and MI_INDEX_PRUNE_DROP (everything else stays; n = 0 changes nothing); both, neither or an unknown
 *                         bit: MI_ERR_INVALID.  The table is REBUILT for the survivors (a power of two, at least 1 024 slots,
 *                         at most half full): it shrinks.  Nothing to drop: the table is not touched (rebuilt = 0), *info (may
 *                         be NULL) still filled.  The old table is never written; the new one, the survivors' records and all
 *                         scratch are allocated before the launch they serve, and the tables are swapped only when the new
 *                         one is complete and its count checked: whatever fails, the index is as it was (what does not fit:
 *                         MI_ERR_NOMEM naming the size and what the device has free).  Blocking, on the ctx stream.
 *   mi_index_retain_zset  keeps exactly the digests the set holds; no list crosses the host (n_rows = n_unknown = 0).  The
 *                         index and the set belong to the same ctx, otherwise MI_ERR_INVALID; a set in its sticky failed
 *                         state: MI_ERR_STATE with the first message, the index unchanged.                                     */
MI_BLOCK int  mi_index_query(mi_index* index, const uint8_t* digests, uint64_t n, uint8_t* held, uint64_t* n_held);
MI_BLOCK int  mi_index_query_batch(mi_index* index, mi_batch* b, uint8_t* held, uint64_t cap, uint64_t* n_held);
#define MI_INDEX_PRUNE_KEEP 0x1u  /* digests = what stays; everything else goes */
#define MI_INDEX_PRUNE_DROP 0x2u  /* digests = what goes; everything else stays  (exactly one of the two) */
typedef struct {               /* 88 bytes */
    uint64_t n_rows, n_unknown;              /* request rows; rows whose digest the index did not hold (repeats counted per row) */
    uint64_t n_before, n_dropped, n_after;   /* distinct digests held before, removed, held after */
    uint64_t slots_before, slots_after;
    uint64_t rebuilt;                        /* 0: nothing was dropped, the table was not touched */
    uint64_t peak_extra_bytes;               /* device bytes the call allocated before it freed anything, from the sizes */
    double   ms_mark, ms_rebuild;            /* HIP events on the ctx stream */
} mi_index_prune_info;
MI_BLOCK int  mi_index_prune(mi_index* index, const uint8_t* digests, uint64_t n, uint32_t flags, mi_index_prune_info* info);
MI_BLOCK int  mi_index_retain_zset(mi_index* index, const mi_zset* set, mi_index_prune_info* info);

#ifdef __cplusplus
}
#endif
#endif /* MAKISU_MI_H */
