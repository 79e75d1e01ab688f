"""makisu_amd -- MI355X (gfx950) layer-snapshot content scan + dedup engine.

Thin ctypes binding over the C ABI (include/makisu_mi.h, libmakisu_mi.so).  It is
the stand-in for the cgo shim a Makisu maintainer would add and
what tests/ and bench.py drive.  No CPU fallback: without the built HIP library
or without a gfx950 device every entry point raises.  Nothing here imports
oracle/.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import build as _build

__all__ = ["Engine", "Batch", "Config", "MiError", "load_library", "FILE_DTYPE", "CHUNK_DTYPE",
           "FLAG_FILE_SHA256", "FLAG_FILE_CRC32", "FLAG_NO_DEDUP", "FLAG_PREFETCH_ROWS", "FLAG_VERIFY_STAGING", "FLAG_FILE_SUMS",
           "FLAG_CHUNK_BLAKE2S", "DIGEST_SHA256", "DIGEST_BLAKE2S", "chunk_root",
           "SHA_LOADS_AUTO", "SHA_LOADS_LANE", "SHA_LOADS_COOP", "Digest", "digest_hex",
           "Pack", "PackEntry", "PackInfo", "PACK_ENTRY_DTYPE", "PACK_VERIFY", "pack_check",
           "PackSet", "PackSetInfo", "RecipeStats", "PACKSET_VERIFY", "RECIPE_VERIFY", "WantInfo", "SUBPACK_VERIFY",
           "ZPack", "ZPackEntry", "ZPackInfo", "ZPACK_ENTRY_DTYPE", "ZPACK_VERIFY", "zpack_check",
           "ZSet", "ZSetInfo", "ZSET_VERIFY", "MEMFS_CHUNK_ZPACK", "ZPACK_LEVEL2", "MEMFS_ZPACK_LEVEL2", "ZPACK_ENTROPY", "ZForms",
           "PruneInfo", "ZSetUsage", "ZSET_PRUNE_KEEP", "ZSET_PRUNE_DROP", "RecodeInfo", "ZSET_RECODE_VERIFY", "TouchInfo", "AgeBin", "STAMP_NONE",
           "IndexPruneInfo", "INDEX_PRUNE_KEEP", "INDEX_PRUNE_DROP"]

FLAG_FILE_SHA256 = 0x1
FLAG_FILE_CRC32 = 0x2
FLAG_NO_DEDUP = 0x4
FLAG_PREFETCH_ROWS = 0x8
FLAG_VERIFY_STAGING = 0x10
FLAG_FILE_SUMS = 0x20
FLAG_CHUNK_BLAKE2S = 0x40                # chunk digests and chunk roots are BLAKE2s-256 (hashlib.blake2s) instead of SHA-256
DIGEST_SHA256, DIGEST_BLAKE2S = 0, 1     # Engine.chunk_digest, chunk_root(alg=)
SHA_LOADS_AUTO, SHA_LOADS_LANE, SHA_LOADS_COOP = 0, 1, 2
SHA_SCHED_FLAT = 1                       # mi_config.sha_sched: one range, every wave equal


def sha_sched_long_shift(k):
    """MI_SHA_SCHED_LONG_SHIFT(k): the long range of a hashing launch = its first n >> k strings."""
    return ((k & 15) + 1) << 8

ERR_NAMES = {0: "MI_OK", -1: "MI_ERR_INVALID", -2: "MI_ERR_NO_DEVICE", -3: "MI_ERR_HIP",
             -4: "MI_ERR_NOMEM", -5: "MI_ERR_IO", -6: "MI_ERR_STATE", -7: "MI_ERR_CAPACITY"}


class MiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERR_NAMES.get(code, code), msg))
        self.code = code


class Config(C.Structure):
    """mi_config (include/makisu_mi.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("gear_seed", C.c_uint64),
                ("mask_bits", C.c_uint32), ("min_size", C.c_uint32), ("max_size", C.c_uint32),
                ("flags", C.c_uint32), ("staging_bytes", C.c_uint64), ("n_streams", C.c_uint32),
                ("sha_blocks_per_cu", C.c_uint32), ("sha_load_scheme", C.c_uint32),
                ("sha_coop_min_gib", C.c_uint32), ("sha_coop_blocks_per_cu", C.c_uint32),
                ("sha_sched", C.c_uint32)]


class _FileResult(C.Structure):
    _fields_ = [("user_tag", C.c_uint64), ("size", C.c_uint64), ("first_chunk", C.c_uint64),
                ("n_chunks", C.c_uint32), ("crc32", C.c_uint32), ("chunk_root", C.c_uint8 * 32),
                ("file_sha256", C.c_uint8 * 32)]


class _ChunkResult(C.Structure):
    _fields_ = [("file_index", C.c_uint64), ("offset", C.c_uint64), ("length", C.c_uint32),
                ("reserved", C.c_uint32), ("dup_of", C.c_int64), ("sha256", C.c_uint8 * 32)]


class CtxEntry(C.Structure):
    """mi_ctx_entry: one walked path of a COPY/ADD source tree."""
    _fields_ = [("relpath", C.c_char_p), ("link_target", C.c_char_p), ("file_index", C.c_int64)]


class TreeEntry(C.Structure):
    """mi_tree_entry: one path recorded by mi_batch_add_tree."""
    _fields_ = [("relpath", C.c_char_p), ("link_target", C.c_char_p), ("file_index", C.c_int64),
                ("size", C.c_uint64), ("mtime_sec", C.c_int64), ("mode", C.c_uint32),
                ("kind", C.c_uint8), ("uid", C.c_uint32), ("gid", C.c_uint32)]


TREE_CONTEXT, TREE_SCAN = 0, 1


class SnapshotSide(C.Structure):
    """mi_snapshot_side: one walk (+ optional chunk roots by file_index) for mi_snapshot_diff."""
    _fields_ = [("entries", C.POINTER(TreeEntry)), ("n", C.c_uint64), ("roots", C.c_void_p),
                ("root_stride", C.c_uint64), ("disk_root", C.c_char_p)]


DIFF_SAME, DIFF_CHANGED, DIFF_ANCESTOR = 0, 1, 2


class CopyOp(C.Structure):
    """mi_copy_op."""
    _fields_ = [("src_root", C.c_char_p), ("srcs", C.POINTER(C.c_char_p)), ("n_srcs", C.c_uint64),
                ("dst", C.c_char_p), ("uid", C.c_uint32), ("gid", C.c_uint32)]


class LayerConfig(C.Structure):
    """mi_layer_config."""
    _fields_ = [("struct_size", C.c_uint32), ("gzip_level", C.c_int32), ("out_fd", C.c_int32),
                ("flags", C.c_uint32)]


LAYER_MODE_WITH_TYPE = 0x1
MEMFS_TRUST_CTIME = 0x1
MEMFS_CHUNK_PACK = 0x2                   # a commit also packs the chunks its index did not know (MemFS.take_pack) and keeps the recipes
MEMFS_CHUNK_ZPACK = 0x4                  # ... codes them straight from the arena into a compressed pack instead (MemFS.take_zpack)
MEMFS_ZPACK_LEVEL2 = 0x10                # ... at level 2 (beside MEMFS_CHUNK_ZPACK)
MEMFS_GZIP_DEVICE = 0x40                 # a commit with an Engine codes its layer's gzip leg on the device (Layer.set_gzip_engine)
PACK_VERIFY = 0x1                        # mi_batch_pack_chunks: hash the blob again on the device


class PackEntry(C.Structure):
    """mi_pack_entry: one chunk of a pack."""
    _fields_ = [("digest", C.c_uint8 * 32), ("offset", C.c_uint64), ("chunk_index", C.c_uint64),
                ("length", C.c_uint32), ("reserved", C.c_uint32)]


class PackInfo(C.Structure):
    """mi_pack_info."""
    _fields_ = [("n_entries", C.c_uint64), ("blob_bytes", C.c_uint64), ("chunk_bytes", C.c_uint64),
                ("alg", C.c_uint32), ("verified", C.c_uint32), ("ms_gather", C.c_double), ("ms_verify", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


PACKSET_VERIFY = 0x1                     # mi_packset_add_*: pad bytes and digests checked on the device before the set takes the pack
RECIPE_VERIFY = 0x1                      # mi_batch_add_recipes: the assembled rows hashed where they lie, held against the recipes


class PackSetInfo(C.Structure):
    """mi_packset_info."""
    _fields_ = [("n_packs", C.c_uint64), ("n_entries", C.c_uint64), ("n_digests", C.c_uint64), ("blob_bytes", C.c_uint64),
                ("alg", C.c_uint32), ("reserved", C.c_uint32), ("ms_upload", C.c_double), ("ms_verify", C.c_double),
                ("ms_insert", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RecipeStats(C.Structure):
    """mi_recipe_stats."""
    _fields_ = [("n_files", C.c_uint64), ("n_rows", C.c_uint64), ("bytes", C.c_uint64), ("n_joined_units", C.c_uint64),
                ("ms_resolve", C.c_double), ("ms_assemble", C.c_double), ("ms_verify", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


SUBPACK_VERIFY = 0x1                     # mi_packset_pack: the new blob hashed on the device, held against the requested digests


class WantInfo(C.Structure):
    """mi_want_info."""
    _fields_ = [("n_rows", C.c_uint64), ("n_distinct", C.c_uint64), ("n_held", C.c_uint64), ("n_want", C.c_uint64),
                ("held_bytes", C.c_uint64), ("want_bytes", C.c_uint64), ("ms_resolve", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


ZPACK_VERIFY = 0x1                       # mi_pack_compress: the new blob decoded and hashed again on the device
ZPACK_LEVEL2 = 0x4                       # mi_pack_compress, mi_batch_zpack_chunks: the denser parse, the same block format
ZPACK_ENTROPY = 0x20                     # mi_pack_compress: the entropy stage over the level's forms (form H where it is smaller)


class ZPackEntry(C.Structure):
    """mi_zpack_entry: one chunk of a compressed pack (stored == length: raw; stored < length: one LZ4 block)."""
    _fields_ = [("digest", C.c_uint8 * 32), ("offset", C.c_uint64), ("chunk_index", C.c_uint64),
                ("length", C.c_uint32), ("stored", C.c_uint32)]


class ZPackInfo(C.Structure):
    """mi_zpack_info."""
    _fields_ = [("n_entries", C.c_uint64), ("blob_bytes", C.c_uint64), ("chunk_bytes", C.c_uint64), ("stored_bytes", C.c_uint64),
                ("n_raw", C.c_uint64), ("alg", C.c_uint32), ("verified", C.c_uint32), ("ms_encode", C.c_double),
                ("ms_compact", C.c_double), ("ms_verify", C.c_double), ("ms_decode", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


ZSET_VERIFY = 0x1                        # mi_zset_add_*: the blob decoded into a scratch and hashed on the device before the set takes it


class ZForms(C.Structure):
    """mi_zforms: entries and stored bytes per form -- [0] raw, [1] one LZ4 block, [2] form H over an LZ4 block, [3] form H over
    the plain bytes."""
    _fields_ = [("n", C.c_uint64 * 4), ("stored", C.c_uint64 * 4)]
    NAMES = ("raw", "lz4", "h_lz4", "h_raw")

    def as_dict(self):
        return dict((name, (int(self.n[i]), int(self.stored[i]))) for i, name in enumerate(self.NAMES))


class ZSetInfo(C.Structure):
    """mi_zset_info."""
    _fields_ = [("n_packs", C.c_uint64), ("n_entries", C.c_uint64), ("n_digests", C.c_uint64), ("blob_bytes", C.c_uint64),
                ("stored_bytes", C.c_uint64), ("chunk_bytes", C.c_uint64), ("alg", C.c_uint32), ("reserved", C.c_uint32),
                ("ms_upload", C.c_double), ("ms_verify", C.c_double), ("ms_insert", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


ZSET_PRUNE_KEEP = 0x1                    # mi_zset_prune: the digests are what stays
ZSET_PRUNE_DROP = 0x2                    # ... what goes (exactly one of the two)


class PruneInfo(C.Structure):
    """mi_prune_info."""
    _fields_ = [(n, C.c_uint64) for n in ("n_rows", "n_unknown", "n_dropped", "dropped_stored_bytes", "dropped_chunk_bytes", "n_blobs_freed",
                                          "freed_bytes", "n_blobs_compacted", "moved_bytes", "n_blobs_sparse_kept", "peak_extra_bytes")] + \
               [(n, C.c_double) for n in ("ms_mark", "ms_move", "ms_rebuild")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ZSetUsage(C.Structure):
    """mi_zset_usage."""
    _fields_ = [(n, C.c_uint64) for n in ("n_blobs", "resident_bytes", "live_bytes", "table_slots", "table_bytes")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


ZSET_RECODE_VERIFY = 0x1                 # mi_zset_recode: hash what every entry decodes to, before and after (beside ZPACK_LEVEL2)


class RecodeInfo(C.Structure):
    """mi_recode_info."""
    _fields_ = [(n, C.c_uint64) for n in ("n_digests", "n_recoded", "n_raw_recoded", "n_undecodable", "stored_before", "stored_after",
                                          "live_before", "live_after", "n_blobs_rewritten", "n_blobs_freed", "freed_bytes", "new_blob_bytes",
                                          "n_rounds", "peak_extra_bytes")] + \
               [(n, C.c_double) for n in ("ms_decode", "ms_encode", "ms_move", "ms_rebuild", "ms_verify")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


STAMP_NONE = 0xFFFFFFFF                  # mi_zset_stamps: the set does not hold the digest; as an epoch: reserved


class TouchInfo(C.Structure):
    """mi_touch_info."""
    _fields_ = [(n, C.c_uint64) for n in ("n_rows", "n_unknown", "n_refreshed")] + [("ms_touch", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class AgeBin(C.Structure):
    """mi_zage_bin."""
    _fields_ = [(n, C.c_uint64) for n in ("n_digests", "stored_bytes", "live_bytes", "chunk_bytes")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


INDEX_PRUNE_KEEP = 0x1                   # mi_index_prune: the digests are what stays
INDEX_PRUNE_DROP = 0x2                   # ... what goes (exactly one of the two)


class IndexPruneInfo(C.Structure):
    """mi_index_prune_info."""
    _fields_ = [(n, C.c_uint64) for n in ("n_rows", "n_unknown", "n_before", "n_dropped", "n_after", "slots_before", "slots_after",
                                          "rebuilt", "peak_extra_bytes")] + \
               [(n, C.c_double) for n in ("ms_mark", "ms_rebuild")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class LayerResult(C.Structure):
    """mi_layer_result: the numbers of step.commitLayer's DigestPair."""
    _fields_ = [("tar_sha256", C.c_uint8 * 32), ("gzip_sha256", C.c_uint8 * 32), ("tar_bytes", C.c_uint64),
                ("gzip_bytes", C.c_uint64), ("n_entries", C.c_uint64)]


GZIP_OFF, GZIP_DEFAULT = -2, -1
# tario.SetCompressionLevel's names (lib/tario/gzip.go:28-43; the `--compression` flag of bin/makisu/cmd/build.go) -> the
# gzip_level of mi_layer_config: "no" is a gzip member of stored blocks (pgzip.NoCompression), not MI_GZIP_OFF
COMPRESSION_LEVELS = {"no": 0, "speed": 1, "size": 9, "default": GZIP_DEFAULT}


def _zpack_level_flag(level):
    """the zpack coder's level (1: every byte as ever, 2: MI_ZPACK_LEVEL2) as a flag of the calls that code"""
    if level not in (1, 2):
        raise ValueError("a zpack is coded at level 1 or 2, not %r" % (level,))
    return ZPACK_LEVEL2 if level == 2 else 0


def compression_level(name):
    """tario.SetCompressionLevel (lib/tario/gzip.go:36-43): the level for a name, `invalid compression level <name>` otherwise."""
    try:
        return COMPRESSION_LEVELS[name]
    except (KeyError, TypeError):
        raise ValueError("invalid compression level %s" % (name,)) from None


class CommitStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_walked", "n_scanned_files", "scanned_bytes", "n_chunks", "n_layer_entries",
                                          "n_layer_files", "layer_file_bytes", "n_content_changed", "n_roots_learned", "n_content_trusted",
                                          "n_index_new", "n_index_known", "index_new_bytes", "files_opened", "file_bytes_read", "pipelined", "n_windows")] + \
               [(n, C.c_double) for n in ("s_walk_stage", "s_scan", "s_diff", "s_write", "s_total")] + \
               [(n, C.c_uint64) for n in ("n_verified_files", "verified_bytes", "n_refetched", "arena_bytes", "arena_pieces", "arena_moves",
                                          "n_ctxs", "ctx_bytes_max", "ctx_bytes_min", "n_split_files")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PartState(C.Structure):
    """mi_part_state: one part of a split file (include/makisu_mi.h "parts")."""
    _fields_ = [("file_index", C.c_uint64), ("file_size", C.c_uint64), ("begin", C.c_uint64),
                ("end", C.c_uint64), ("entry", C.c_uint64), ("exit", C.c_uint64),
                ("entry_confirmed", C.c_uint32), ("cuts_current", C.c_uint32)]


PART_ALIGN = 262144


class Stats(C.Structure):
    _fields_ = [("bytes_in", C.c_uint64), ("n_files", C.c_uint64), ("n_chunks", C.c_uint64),
                ("n_unique", C.c_uint64), ("ms_h2d", C.c_double), ("ms_cdc", C.c_double),
                ("ms_sort", C.c_double), ("ms_sha_chunks", C.c_double),
                ("ms_sha_files", C.c_double), ("ms_dedup", C.c_double), ("ms_total", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class StageStats(C.Structure):
    """mi_stage_stats."""
    _fields_ = [("spans", C.c_uint64), ("bytes", C.c_uint64), ("verified_spans", C.c_uint64),
                ("mismatches", C.c_uint64), ("repaired", C.c_uint64), ("final_spans", C.c_uint64),
                ("final_mismatches", C.c_uint64), ("ms_verify", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _np_dtype(struct):
    names, fmts, offs = [], [], []
    for name, ctype in struct._fields_:
        names.append(name)
        offs.append(getattr(struct, name).offset)
        if issubclass(ctype, C.Array):
            fmts.append(("u1", ctype._length_))
        else:
            fmts.append(np.dtype(ctype))
    return np.dtype({"names": names, "formats": fmts, "offsets": offs,
                     "itemsize": C.sizeof(struct)})


FILE_DTYPE = _np_dtype(_FileResult)
CHUNK_DTYPE = _np_dtype(_ChunkResult)
PACK_ENTRY_DTYPE = _np_dtype(PackEntry)
ZPACK_ENTRY_DTYPE = _np_dtype(ZPackEntry)

_lib = None


class DeflateInfo(C.Structure):
    _fields_ = [("n_pieces", C.c_uint64), ("n_dynamic", C.c_uint64), ("n_stored", C.c_uint64), ("in_bytes", C.c_uint64),
                ("out_bytes", C.c_uint64), ("ms_device", C.c_double)]


class InflateInfo(C.Structure):
    _fields_ = [("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("n_candidates", C.c_uint64), ("n_segments", C.c_uint64),
                ("n_rounds", C.c_uint64), ("at_in", C.c_uint64), ("at_out", C.c_uint64), ("verdict", C.c_uint32), ("rule", C.c_uint32),
                ("fell_back", C.c_uint32), ("reserved", C.c_uint32), ("ms_size", C.c_double), ("ms_write", C.c_double)]


INFLATE_DONE, INFLATE_NOT_PARALLEL = 0, 1
INFLATE_INDEX_REFUSED = 2
INFLATE_INDEX_SPACING = 262144


class InflateIndexInfo(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("n_blocks", C.c_uint64), ("out_bytes", C.c_uint64), ("windows_bytes", C.c_uint64),
                ("spacing", C.c_uint64), ("ms_build", C.c_double)]


class InflateSpecInfo(C.Structure):
    _fields_ = [("piece_bytes", C.c_uint64), ("n_pieces", C.c_uint64), ("n_found", C.c_uint64), ("n_live", C.c_uint64),
                ("ring_bytes", C.c_uint64), ("ms_find", C.c_double), ("ms_speculate", C.c_double), ("ms_windows", C.c_double)]


INFLATE_SPEC_PIECE = 65536


class LayerBlobInfo(C.Structure):
    _fields_ = [("tar_bytes", C.c_uint64), ("arena_at", C.c_uint64), ("first_file", C.c_uint64), ("n_files", C.c_uint64),
                ("n_entries", C.c_uint64), ("n_marked", C.c_uint64), ("n_live", C.c_uint64), ("n_fetched", C.c_uint64),
                ("fetched_bytes", C.c_uint64), ("source", C.c_uint32), ("reserved", C.c_uint32), ("ms_upload", C.c_double),
                ("ms_headers", C.c_double), ("inflate", InflateInfo)]


LAYER_SOURCE_TAR, LAYER_SOURCE_DEVICE_GZIP, LAYER_SOURCE_ZLIB = 0, 1, 2
LAYER_SOURCE_INDEXED_GZIP = 3
LAYER_SOURCE_SPEC_GZIP = 4


def _inflate_info_dict(info):
    return dict((f, getattr(info, f)) for f, _ in InflateInfo._fields_ if f != "reserved")


def _spec_info_dict(spec):
    return dict((f, getattr(spec, f)) for f, _ in InflateSpecInfo._fields_)


def _indexed_info_dict(info):
    d = _inflate_info_dict(info)
    d["index_refusal"] = info.reserved                  # the checker's number when it refused the index, else 0
    return d


def load_library(rebuild=False):
    """Loads (building first if stale) makisu_amd/libmakisu_mi.so.  Raises if it is missing."""
    global _lib
    if _lib is not None and not rebuild:
        return _lib
    path = os.environ.get("MAKISU_MI_LIB") or _build.LIB    # another build of the library (same-box A/B runs)
    if path == _build.LIB and (rebuild or (_build.needs_build() and os.path.exists(_build.HIPCC))):
        _build.build(force=rebuild)
    if not os.path.exists(path):
        raise MiError(-2, "libmakisu_mi.so is not built (run `python -m makisu_amd.build`); "
                          "there is no CPU fallback")
    L = C.CDLL(path)
    vp, u64, u64p = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)
    sigs = {
        "mi_abi_version": ([], C.c_int),
        "mi_ctx_warm": ([vp], C.c_int),
        "mi_debug_sha_wave_stats": ([vp, C.c_char_p], C.c_int),
        "mi_config_default": ([C.POINTER(Config)], C.c_int),
        "mi_ctx_create": ([C.POINTER(Config), C.POINTER(vp)], C.c_int),
        "mi_ctx_destroy": ([vp], C.c_int),
        "mi_last_error": ([vp], C.c_char_p),
        "mi_get_stats": ([vp, C.POINTER(Stats)], C.c_int),
        "mi_device_info": ([vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), u64p, C.c_char_p,
                            C.c_size_t], C.c_int),
        "mi_sha_valu_roof": ([vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)], C.c_int),
        "mi_blake2s_valu_roof": ([vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)], C.c_int),
        "mi_ctx_chunk_digest": ([vp, C.POINTER(C.c_uint32)], C.c_int),
        "mi_batch_begin": ([vp, u64, u64, C.POINTER(vp)], C.c_int),
        "mi_batch_add_bytes": ([vp, vp, u64, u64], C.c_int),
        "mi_batch_add_path": ([vp, C.c_char_p, u64, u64], C.c_int),
        "mi_batch_reserve": ([vp, u64, u64], C.c_int),
        "mi_batch_add_path_range": ([vp, C.c_char_p, u64, u64, u64], C.c_int),
        "mi_batch_add_paths": ([vp, u64, C.POINTER(C.c_char_p), u64p, u64p], C.c_int),
        "mi_batch_add_synthetic": ([vp, u64, u64p, u64p, u64], C.c_int),
        "mi_batch_add_path_part": ([vp, C.c_char_p, u64, u64, u64, u64], C.c_int),
        "mi_batch_add_synthetic_part": ([vp, u64, u64, u64, u64, u64], C.c_int),
        "mi_chunk_root": ([vp, u64, vp], C.c_int),
        "mi_chunk_root_alg": ([C.c_uint32, vp, u64, vp], C.c_int),
        "mi_batch_scan_cuts": ([vp], C.c_int),
        "mi_batch_parts": ([vp, C.POINTER(PartState), u64, u64p], C.c_int),
        "mi_batch_set_part_entry": ([vp, u64, u64], C.c_int),
        "mi_batch_fix_cuts": ([vp], C.c_int),
        "mi_batch_run": ([vp], C.c_int),
        "mi_batch_rerun": ([vp], C.c_int),
        "mi_batch_submit": ([vp], C.c_int),
        "mi_batch_wait": ([vp], C.c_int),
        "mi_batch_counts": ([vp, u64p, u64p, u64p], C.c_int),
        "mi_batch_files": ([vp, vp, u64], C.c_int),
        "mi_batch_chunks": ([vp, vp, u64], C.c_int),
        "mi_batch_chunks_view": ([vp, C.POINTER(vp), u64p], C.c_int),
        "mi_batch_files_view": ([vp, C.POINTER(vp), u64p], C.c_int),
        "mi_batch_device_digests": ([vp, C.POINTER(vp), u64p], C.c_int),
        "mi_batch_read_back": ([vp, vp, u64], C.c_int),
        "mi_batch_reset": ([vp], C.c_int),
        "mi_batch_stage_stats": ([vp, C.POINTER(StageStats)], C.c_int),
        "mi_batch_stage_note": ([vp], C.c_char_p),
        "mi_batch_free": ([vp], C.c_int),
        "mi_dedup_mark": ([vp, vp, u64, vp, u64p], C.c_int),
        "mi_batch_set_global_dedup": ([vp, vp, u64], C.c_int),
        "mi_dedup_mark_range": ([vp, vp, u64, u64, u64, vp, u64p], C.c_int),
        "mi_batch_mark_global": ([vp, vp, u64, u64, u64p], C.c_int),
        "mi_batch_device_dup_of": ([vp, C.POINTER(vp), u64p], C.c_int),
        "mi_sha256_many": ([vp, vp, u64p, u64p, u64, vp], C.c_int),
        "mi_context_checksum": ([vp, vp, u64, C.POINTER(CtxEntry), u64, C.POINTER(C.c_uint32)],
                                C.c_int),
        "mi_batch_add_tree": ([vp, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), u64, C.c_uint32,
                               u64p], C.c_int),
        "mi_batch_tree_entries": ([vp, C.POINTER(TreeEntry), u64], C.c_int),
        "mi_context_checksum_tree": ([vp, vp, u64, C.POINTER(C.c_uint32)], C.c_int),
        "mi_tree_walk": ([C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), u64, C.c_uint32,
                          C.POINTER(vp), u64p], C.c_int),
        "mi_tree_entries": ([vp, C.POINTER(TreeEntry), u64], C.c_int),
        "mi_tree_free": ([vp], None),
        "mi_entries_commit_order": ([C.POINTER(TreeEntry), u64, u64p], C.c_int),
        "mi_snapshot_diff": ([C.POINTER(SnapshotSide), C.POINTER(SnapshotSide), C.c_int, vp, vp], C.c_int),
        "mi_tar_open": ([C.c_char_p, C.POINTER(vp), u64p], C.c_int),
        "mi_tar_open_ex": ([C.c_char_p, C.POINTER(vp), u64p, C.POINTER(C.c_int), C.c_char_p, u64], C.c_int),
        "mi_tar_inflate": ([C.c_char_p, C.c_char_p, u64p, vp, vp, C.c_char_p, u64], C.c_int),
        "mi_tar_entries": ([vp, C.POINTER(TreeEntry), u64p, u64], C.c_int),
        "mi_tar_free": ([vp], None),
        "mi_entry_similar": ([C.POINTER(TreeEntry), C.POINTER(TreeEntry), C.c_int, vp, vp,
                              C.POINTER(C.c_int)], C.c_int),
        "mi_copy_op_resolve": ([u64, C.c_char_p, C.c_char_p, C.c_char_p, u64, C.c_char_p, u64], C.c_int),
        "mi_resolve_chown": ([C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, u64], C.c_int),
        "mi_path_match": ([C.c_char_p, C.c_char_p, C.POINTER(C.c_int)], C.c_int),
        "mi_context_sources": ([C.c_char_p, C.POINTER(C.c_char_p), u64, C.c_char_p, u64, u64p, u64p], C.c_int),
        "mi_memfs_create": ([C.c_char_p, C.POINTER(C.c_char_p), u64, C.c_int64, C.POINTER(vp)], C.c_int),
        "mi_memfs_free": ([vp], None),
        "mi_memfs_error": ([vp], C.c_char_p),
        "mi_memfs_set_clock": ([vp, C.c_int64], C.c_int),
        "mi_memfs_reset": ([vp], C.c_int),
        "mi_memfs_update_from_entries": ([vp, C.POINTER(TreeEntry), u64, u64p], C.c_int),
        "mi_memfs_untar": ([vp, C.c_char_p, C.POINTER(TreeEntry), u64p, u64, u64p], C.c_int),
        "mi_memfs_add_layer_by_scan": ([vp, C.POINTER(TreeEntry), u64, vp, u64, C.POINTER(vp), u64p], C.c_int),
        "mi_memfs_add_layer_by_copy_ops": ([vp, C.POINTER(CopyOp), u64, C.POINTER(vp), u64p], C.c_int),
        "mi_memfs_entries": ([vp, C.POINTER(TreeEntry), C.POINTER(C.c_char_p), u64, u64p], C.c_int),
        "mi_memfs_checkpoint": ([vp, C.c_char_p, C.POINTER(C.c_char_p), u64], C.c_int),
        "mi_memfs_commit_layer": ([vp, vp, C.c_int, C.POINTER(CopyOp), u64, C.POINTER(LayerConfig), C.POINTER(LayerResult),
                                   C.POINTER(vp), C.POINTER(C.c_int)], C.c_int),
        "mi_memfs_commit_layer_n": ([vp, C.POINTER(vp), C.c_uint32, C.c_int, C.POINTER(CopyOp), u64, C.POINTER(LayerConfig),
                                     C.POINTER(LayerResult), C.POINTER(vp), C.POINTER(C.c_int)], C.c_int),
        "mi_memfs_commit_stats": ([vp, C.POINTER(CommitStats)], C.c_int),
        "mi_memfs_set_index": ([vp, vp], C.c_int),
        "mi_memfs_set_options": ([vp, C.c_uint32], C.c_int),
        "mi_memfs_release_device": ([vp], C.c_int),
        "mi_memfs_reserve_device": ([vp, vp, u64, u64], C.c_int),
        "mi_memfs_root_of": ([vp, C.c_char_p, vp, C.POINTER(C.c_int)], C.c_int),
        "mi_copy_layer_roots": ([vp, vp, vp, u64], C.c_int),
        "mi_batch_roots": ([vp, vp, u64], C.c_int),
        "mi_batch_read_file": ([vp, u64, u64, vp, u64], C.c_int),
        "mi_layer_add_batch_file": ([vp, C.POINTER(TreeEntry), vp, u64], C.c_int),
        "mi_layer_io_counts": ([vp, u64p, u64p], C.c_int),
        "mi_copy_op_execute": ([C.POINTER(CopyOp), C.c_uint32, C.POINTER(C.c_char_p), u64, C.c_char_p, u64], C.c_int),
        "mi_copy_layer_entries": ([vp, C.POINTER(TreeEntry), C.POINTER(C.c_char_p), u64], C.c_int),
        "mi_copy_layer_free": ([vp], None),
        "mi_layer_config_default": ([C.POINTER(LayerConfig)], C.c_int),
        "mi_layer_begin": ([C.POINTER(LayerConfig), C.POINTER(vp)], C.c_int),
        "mi_layer_add": ([vp, C.POINTER(TreeEntry), C.c_char_p], C.c_int),
        "mi_layer_add_whiteout": ([vp, C.c_char_p], C.c_int),
        "mi_layer_finish": ([vp, C.POINTER(LayerResult)], C.c_int),
        "mi_layer_error": ([vp], C.c_char_p),
        "mi_layer_free": ([vp], None),
        "mi_layer_set_gzip_ctx": ([vp, vp], C.c_int),
        "mi_deflate_bound": ([u64], u64),
        "mi_deflate_buffer": ([vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(C.c_uint32), C.POINTER(DeflateInfo)], C.c_int),
        "mi_inflate_buffer": ([vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(InflateInfo)], C.c_int),
        "mi_tar_inflate_ctx": ([vp, C.c_char_p, C.c_char_p, u64p, vp, vp, C.POINTER(InflateInfo), C.c_char_p, u64], C.c_int),
        "mi_batch_add_layer_blob": ([vp, vp, u64, u64, C.POINTER(vp), vp, C.POINTER(LayerBlobInfo)], C.c_int),
        "mi_batch_add_layer_path": ([vp, C.c_char_p, u64, C.POINTER(vp), vp, C.POINTER(LayerBlobInfo)], C.c_int),
        "mi_inflate_index_build": ([vp, u64, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(InflateIndexInfo), vp, C.c_char_p, u64], C.c_int),
        "mi_inflate_index_free": ([vp], None),
        "mi_inflate_index_check": ([vp, u64, vp, u64], C.c_int),
        "mi_inflate_index_refusal": ([C.c_int], C.c_char_p),
        "mi_inflate_buffer_indexed": ([vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(InflateInfo)], C.c_int),
        "mi_tar_inflate_ctx_indexed": ([vp, C.c_char_p, vp, u64, C.c_char_p, u64p, vp, vp, C.POINTER(InflateInfo), C.c_char_p, u64], C.c_int),
        "mi_inflate_buffer_spec": ([vp, vp, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(InflateInfo), C.POINTER(InflateSpecInfo), C.POINTER(vp),
                                    C.POINTER(u64)], C.c_int),
        "mi_tar_inflate_ctx_spec": ([vp, C.c_char_p, u64, C.c_char_p, u64p, vp, vp, C.POINTER(InflateInfo), C.POINTER(InflateSpecInfo), C.POINTER(vp),
                                     C.POINTER(u64), C.c_char_p, u64], C.c_int),
        "mi_batch_add_layer_blob_spec": ([vp, vp, u64, u64, u64, C.POINTER(vp), vp, C.POINTER(LayerBlobInfo), C.POINTER(InflateSpecInfo)], C.c_int),
        "mi_batch_add_layer_path_spec": ([vp, C.c_char_p, u64, u64, C.POINTER(vp), vp, C.POINTER(LayerBlobInfo), C.POINTER(InflateSpecInfo)], C.c_int),
        "mi_batch_add_layer_blob_indexed": ([vp, vp, u64, vp, u64, u64, C.POINTER(vp), vp, C.POINTER(LayerBlobInfo)], C.c_int),
        "mi_batch_add_layer_path_indexed": ([vp, C.c_char_p, vp, u64, u64, C.POINTER(vp), vp, C.POINTER(LayerBlobInfo)], C.c_int),
        "mi_layer_header_bytes": ([C.POINTER(TreeEntry), C.c_uint32, vp, u64, u64p], C.c_int),
        "mi_cache_parse_entry_str": ([C.c_char_p, C.c_char_p, u64, C.c_char_p, u64], C.c_int),
        "mi_cache_key": ([C.c_char_p, C.c_char_p, u64], C.c_int),
        "mi_cache_create_entry": ([vp, vp, C.c_char_p, u64], C.c_int),
        "mi_cache_parse_entry": ([C.c_char_p, C.POINTER(C.c_int), vp, vp], C.c_int),
        "mi_comm_unique_id": ([vp], C.c_int),
        "mi_comm_init_rank": ([vp, C.c_int, C.c_int, vp], C.c_int),
        "mi_comm_init_all": ([C.POINTER(vp), C.c_int], C.c_int),
        "mi_comm_destroy": ([vp], C.c_int),
        "mi_comm_ranks": ([vp, C.POINTER(C.c_int)], C.c_int),
        "mi_comm_exchange_ms": ([vp, C.POINTER(C.c_double), C.POINTER(C.c_double)], C.c_int),
        "mi_dedup_allgather": ([vp, u64p, u64p, u64p], C.c_int),
        "mi_dedup_allgather_all": ([C.POINTER(vp), C.c_int, u64p, u64p], C.c_int),
        "mi_dedup_alltoall": ([vp, u64p, u64p, u64p], C.c_int),
        "mi_dedup_alltoall_all": ([C.POINTER(vp), C.c_int, u64p, u64p], C.c_int),
        "mi_index_create": ([vp, u64, C.POINTER(vp)], C.c_int),
        "mi_index_free": ([vp], None),
        "mi_index_count": ([vp, u64p], C.c_int),
        "mi_index_add_batch": ([vp, vp, vp, u64, u64p, u64p], C.c_int),
        "mi_index_export": ([vp, vp, u64], C.c_int),
        "mi_index_import": ([vp, vp, u64, u64p], C.c_int),
        "mi_batch_pack_chunks": ([vp, vp, u64, C.c_uint32, C.POINTER(vp)], C.c_int),
        "mi_pack_get_info": ([vp, C.POINTER(PackInfo)], C.c_int),
        "mi_pack_entries": ([vp, vp, u64], C.c_int),
        "mi_pack_read": ([vp, u64, vp, u64], C.c_int),
        "mi_pack_device": ([vp, C.POINTER(vp), u64p], C.c_int),
        "mi_pack_free": ([vp], None),
        "mi_pack_check": ([vp, u64, vp, u64, C.c_uint32, u64p], C.c_int),
        "mi_memfs_take_pack": ([vp, C.POINTER(vp)], C.c_int),
        "mi_copy_layer_chunks": ([vp, u64, vp, vp, u64, u64p], C.c_int),
        "mi_packset_create": ([vp, u64, C.POINTER(vp)], C.c_int),
        "mi_packset_add_blob": ([vp, vp, u64, vp, u64, C.c_uint32, u64p], C.c_int),
        "mi_packset_add_pack": ([vp, vp, C.c_uint32], C.c_int),
        "mi_packset_get_info": ([vp, C.POINTER(PackSetInfo)], C.c_int),
        "mi_packset_free": ([vp], None),
        "mi_batch_add_recipes": ([vp, vp, u64, vp, vp, vp, vp, C.c_uint32, C.POINTER(RecipeStats)], C.c_int),
        "mi_packset_missing": ([vp, vp, vp, u64, vp, vp, u64, C.POINTER(WantInfo)], C.c_int),
        "mi_packset_pack": ([vp, vp, vp, u64, C.c_uint32, C.POINTER(vp), u64p], C.c_int),
        "mi_pack_compress": ([vp, C.c_uint32, C.POINTER(vp)], C.c_int),
        "mi_zpack_get_info": ([vp, C.POINTER(ZPackInfo)], C.c_int),
        "mi_zpack_entries": ([vp, vp, u64], C.c_int),
        "mi_zpack_read": ([vp, u64, vp, u64], C.c_int),
        "mi_zpack_free": ([vp], None),
        "mi_packset_add_zblob": ([vp, vp, u64, vp, u64, C.c_uint32, u64p], C.c_int),
        "mi_packset_add_zpack": ([vp, vp, C.c_uint32], C.c_int),
        "mi_zpack_check": ([vp, u64, vp, u64, C.c_uint32, u64p], C.c_int),
        "mi_zset_create": ([vp, u64, C.POINTER(vp)], C.c_int),
        "mi_zset_add_zblob": ([vp, vp, u64, vp, u64, C.c_uint32, u64p], C.c_int),
        "mi_zset_add_zpack": ([vp, vp, C.c_uint32], C.c_int),
        "mi_zset_get_info": ([vp, C.POINTER(ZSetInfo)], C.c_int),
        "mi_zset_count_forms": ([vp, C.POINTER(ZForms)], C.c_int),
        "mi_zpack_count_forms": ([vp, C.POINTER(ZForms)], C.c_int),
        "mi_zset_free": ([vp], None),
        "mi_zset_zpack": ([vp, vp, vp, u64, C.c_uint32, C.POINTER(vp), u64p], C.c_int),
        "mi_zset_zpack_unwrapped": ([vp, vp, vp, u64, C.c_uint32, C.POINTER(vp), u64p], C.c_int),
        "mi_zset_pack": ([vp, vp, vp, u64, C.c_uint32, C.POINTER(vp), u64p], C.c_int),
        "mi_batch_add_zrecipes": ([vp, vp, u64, vp, vp, vp, vp, C.c_uint32, C.POINTER(RecipeStats)], C.c_int),
        "mi_batch_zpack_chunks": ([vp, vp, u64, C.c_uint32, C.POINTER(vp)], C.c_int),
        "mi_memfs_take_zpack": ([vp, C.POINTER(vp)], C.c_int),
        "mi_zset_missing": ([vp, vp, vp, u64, vp, vp, u64, C.POINTER(WantInfo)], C.c_int),
        "mi_zset_prune": ([vp, vp, u64, C.c_uint32, C.c_uint32, C.POINTER(PruneInfo)], C.c_int),
        "mi_zset_recode": ([vp, C.c_uint32, u64, C.POINTER(RecodeInfo)], C.c_int),
        "mi_zset_get_usage": ([vp, C.POINTER(ZSetUsage)], C.c_int),
        "mi_zset_entries": ([vp, vp, vp, vp, u64, u64p], C.c_int),
        "mi_zset_set_epoch": ([vp, C.c_uint32], C.c_int),
        "mi_zset_get_epoch": ([vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u64p], C.c_int),
        "mi_zset_touch": ([vp, vp, u64, C.POINTER(TouchInfo)], C.c_int),
        "mi_zset_stamps": ([vp, vp, u64, vp], C.c_int),
        "mi_zset_age_census": ([vp, vp, C.c_uint32, vp], C.c_int),
        "mi_zset_expire": ([vp, C.c_uint32, C.c_uint32, C.POINTER(PruneInfo)], C.c_int),
        "mi_index_query": ([vp, vp, u64, vp, u64p], C.c_int),
        "mi_index_query_batch": ([vp, vp, vp, u64, u64p], C.c_int),
        "mi_index_prune": ([vp, vp, u64, C.c_uint32, C.POINTER(IndexPruneInfo)], C.c_int),
        "mi_index_retain_zset": ([vp, vp, C.POINTER(IndexPruneInfo)], C.c_int),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(L, name)          # AttributeError here = header/library drift
        fn.argtypes = args
        fn.restype = res
    L._mi_symbols = tuple(sigs)
    _lib = L
    return L


def digest_hex(raw32):
    return bytes(bytearray(raw32)).hex()


class Digest(str):
    """"sha256:<hex>" -- mirrors image.Digest (lib/docker/image/digest.go:26-50)."""

    @classmethod
    def from_raw(cls, raw32):
        return cls("sha256:" + digest_hex(raw32))

    def hex(self):                      # Digest.Hex()
        return self[self.index(":") + 1:]


KIND_DIR, KIND_FILE, KIND_SYMLINK, KIND_HARDLINK = 0, 1, 2, 3


def entry_similar(a, b, ignore_time=False, root_a=None, root_b=None):
    """tario.IsSimilarHeader on two entry dicts (keys: relpath, link_target, size, mtime_sec, mode,
    kind, uid, gid; missing keys = 0/None), optionally content-aware through 32-byte chunk roots."""
    def make(d):
        e = TreeEntry()
        e.relpath = os.fsencode(d.get("relpath", "x"))
        lt = d.get("link_target")
        e.link_target = os.fsencode(lt) if lt is not None else None
        e.file_index = d.get("file_index", -1)
        for k in ("size", "mtime_sec", "mode", "kind", "uid", "gid"):
            setattr(e, k, d.get(k, 0))
        return e
    ea, eb, out = make(a), make(b), C.c_int()
    ra = (C.c_uint8 * 32).from_buffer_copy(bytes(root_a)) if root_a is not None else None
    rb = (C.c_uint8 * 32).from_buffer_copy(bytes(root_b)) if root_b is not None else None
    rc = load_library().mi_entry_similar(C.byref(ea), C.byref(eb), int(ignore_time), ra, rb, C.byref(out))
    if rc:
        raise MiError(rc, "mi_entry_similar: unsupported type")
    return bool(out.value)


def commit_order(relpaths):
    """memLayer.rangeFiles' order (sort.Strings over absolute dst paths, whiteout markers under the
    path they delete) for a list of relpaths: list of indices in commit order."""
    n = len(relpaths)
    arr = (TreeEntry * max(n, 1))()
    keep = [os.fsencode(r) for r in relpaths]
    for i, r in enumerate(keep):
        arr[i].relpath = r
    out = (C.c_uint64 * max(n, 1))()
    rc = load_library().mi_entries_commit_order(arr, n, out)
    if rc:
        raise MiError(rc, "mi_entries_commit_order")
    return [int(out[i]) for i in range(n)]


def _tar_handle_entries(L, h, n):
    """the n entries of an mi_tar as tar_entries' dicts; the handle is freed"""
    try:
        arr = (TreeEntry * max(n, 1))()
        offs = (C.c_uint64 * max(n, 1))()
        rc = L.mi_tar_entries(h, arr, offs, n)
        if rc:
            raise MiError(rc, "mi_tar_entries")
        out = []
        for i in range(n):
            d = _entry_dict(arr[i])
            d["data_offset"] = int(offs[i])
            out.append(d)
        return out
    finally:
        L.mi_tar_free(h)


def tar_entries(path):
    """mi_tar_open + mi_tar_entries: the entries of an uncompressed layer tar as dicts (the keys of
    tree_walk(full=True) plus "data_offset": where a regular file's bytes start in the archive)."""
    L = load_library()
    h, n = C.c_void_p(), C.c_uint64()
    err = C.create_string_buffer(512)
    rc = L.mi_tar_open_ex(os.fsencode(path), C.byref(h), C.byref(n), None, err, len(err))
    if rc:
        raise MiError(rc, "mi_tar_open: %s" % err.value.decode(errors="replace"))
    return _tar_handle_entries(L, h, n.value)


def tar_inflate(blob_path, tar_path_out=None):
    """mi_tar_inflate: a stored (gzip) layer blob -> uncompressed tar file; returns
    dict(tar_bytes, tar_digest, blob_digest)."""
    nb = C.c_uint64()
    t, g = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
    err = C.create_string_buffer(512)
    rc = load_library().mi_tar_inflate(os.fsencode(blob_path),
                                       os.fsencode(tar_path_out) if tar_path_out is not None else None,
                                       C.byref(nb), t, g, err, len(err))
    if rc:
        raise MiError(rc, "mi_tar_inflate: %s" % err.value.decode(errors="replace"))
    return {"tar_bytes": nb.value, "tar_digest": Digest.from_raw(t), "blob_digest": Digest.from_raw(g)}


def inflate_index_build(blob, spacing=0, want_digest=False):
    """mi_inflate_index_build (host only): one whole gzip member -> (its index of checkpoints as bytes, info dict).  spacing 0: the
    default, INFLATE_INDEX_SPACING.  want_digest: info["tar_digest"] is the SHA-256 of the inflation, taken in the same pass.  A member
    that cannot be indexed (corrupt, two members, trailing bytes, a wrong CRC-32) raises MiError(-1) with the reason"""
    L = load_library()
    src = np.frombuffer(bytes(blob), dtype=np.uint8)
    p, n, info = C.c_void_p(), C.c_uint64(), InflateIndexInfo()
    sha = (C.c_uint8 * 32)() if want_digest else None
    err = C.create_string_buffer(512)
    rc = L.mi_inflate_index_build(src.ctypes.data if src.size else None, src.size, spacing, C.byref(p), C.byref(n), C.byref(info), sha, err, len(err))
    if rc:
        raise MiError(rc, err.value.decode(errors="replace") or "mi_inflate_index_build failed")
    try:
        index = C.string_at(p, n.value)
    finally:
        L.mi_inflate_index_free(p)
    d = dict((f, getattr(info, f)) for f, _ in InflateIndexInfo._fields_)
    if want_digest:
        d["tar_digest"] = Digest.from_raw(sha)
    return index, d


def inflate_index_check(index, blob=None):
    """mi_inflate_index_check (host only): an untrusted index -> (0, "ok"), or (the number of the first reason it is refused, its text);
    blob: the member it is said to belong to"""
    L = load_library()
    ix = np.frombuffer(bytes(index), dtype=np.uint8)
    gz = np.frombuffer(bytes(blob), dtype=np.uint8) if blob is not None else None
    r = L.mi_inflate_index_check(ix.ctypes.data if ix.size else None, ix.size, gz.ctypes.data if gz is not None and gz.size else None,
                                 gz.size if gz is not None else 0)
    return r, L.mi_inflate_index_refusal(r).decode()


def _entry_array(dicts, keep):
    arr = (TreeEntry * max(len(dicts), 1))()
    for i, d in enumerate(dicts):
        rp = os.fsencode(d.get("relpath", ""))
        lt = d.get("link_target")
        lt = os.fsencode(lt) if lt is not None else None
        keep += [rp, lt]
        arr[i].relpath, arr[i].link_target = rp, lt
        arr[i].file_index = d.get("file_index", -1)
        for k in ("size", "mtime_sec", "mode", "kind", "uid", "gid"):
            setattr(arr[i], k, d.get(k, 0))
    return arr


def apply_layer(base, layer, root=None, blacklist=()):
    """Harness helper over the MemFS handle (the library has ONE layer merge, mi_memfs_update_from_entries):
    UpdateFromTarReader of `base`, then of `layer`, into a fresh tree; returns mi_memfs_entries -- the merged tree in
    sorted-path order as entry dicts (relpaths without the leading "/", a "src" key; the directories addAncestors
    created are entries like any other).  root = the directory the layers are (or would be) untarred to: its
    blacklist / mountpoint filter applies; None = an empty scratch directory, where nothing is mounted or
    blacklisted (special files and ".wh..wh." metadata are skipped either way, as in the reference)."""
    import tempfile
    scratch = tempfile.mkdtemp(prefix="mi_memfs_") if root is None else None
    try:
        with MemFS(root if root is not None else scratch, blacklist) as fs:
            if base:
                fs.update_from_entries(base)
            fs.update_from_entries(layer)
            return fs.entries()
    finally:
        if scratch:
            os.rmdir(scratch)


def snapshot_diff(before, after, ignore_time=False, roots_before=None, roots_after=None, disk_root=None):
    """mi_snapshot_diff on two lists of entry dicts (tree_walk(..., full=True)); roots_* = (n_files,
    32) uint8 arrays indexed by file_index, or None.  Returns (flags per `after` entry, whiteout
    flags per `before` entry) as lists of ints."""
    keep = []
    sides = []
    for ents, roots in ((before, roots_before), (after, roots_after)):
        side = SnapshotSide()
        arr = _entry_array(ents, keep)
        keep.append(arr)
        side.entries, side.n = arr, len(ents)
        if roots is not None:
            r = np.ascontiguousarray(roots, dtype=np.uint8).reshape(-1, 32)
            keep.append(r)
            side.roots, side.root_stride = r.ctypes.data, 32
        sides.append(side)
    if disk_root is not None:
        sides[1].disk_root = os.fsencode(disk_root)
    flags = np.zeros(max(len(after), 1), dtype=np.uint8)
    wh = np.zeros(max(len(before), 1), dtype=np.uint8)
    rc = load_library().mi_snapshot_diff(C.byref(sides[0]), C.byref(sides[1]), int(ignore_time),
                                         flags.ctypes.data, wh.ctypes.data)
    if rc:
        raise MiError(rc, "mi_snapshot_diff")
    return flags[: len(after)].tolist(), wh[: len(before)].tolist()


def _entry_dict(e):
    return {"relpath": os.fsdecode(e.relpath), "link_target": os.fsdecode(e.link_target) if e.link_target else None,
            "file_index": e.file_index, "size": e.size, "mtime_sec": e.mtime_sec, "mode": e.mode,
            "kind": e.kind, "uid": e.uid, "gid": e.gid}


def tree_walk(root, rel_base=None, blacklist=(), mode=TREE_CONTEXT, full=False):
    """The reference's directory walk on its own (host logic, no GPU): list of
    (relpath, link_target, file_ordinal, size, kind, mode) in visit order (full=True: dicts
    with every mi_tree_entry field)."""
    L = load_library()
    bl = (C.c_char_p * max(len(blacklist), 1))(*[os.fsencode(x) for x in blacklist])
    h, n = C.c_void_p(), C.c_uint64()
    rc = L.mi_tree_walk(os.fsencode(root), os.fsencode(rel_base) if rel_base else None, bl,
                        len(blacklist), mode, C.byref(h), C.byref(n))
    if rc:
        raise MiError(rc, "mi_tree_walk(%s)" % root)
    try:
        arr = (TreeEntry * max(n.value, 1))()
        rc = L.mi_tree_entries(h, arr, n.value)
        if rc:
            raise MiError(rc, "mi_tree_entries")
        if full:
            return [_entry_dict(e) for e in arr[:n.value]]
        return [(os.fsdecode(e.relpath), os.fsdecode(e.link_target) if e.link_target else None,
                 e.file_index, e.size, e.kind, e.mode) for e in arr[:n.value]]
    finally:
        L.mi_tree_free(h)


def copy_op_resolve(n_srcs, work_dir, dst):
    """mi_copy_op_resolve: NewCopyOperation's checks + resolveDestination; returns the absolute dst."""
    out = C.create_string_buffer(4096)
    err = C.create_string_buffer(300)
    rc = load_library().mi_copy_op_resolve(n_srcs, os.fsencode(work_dir) if work_dir is not None else None, os.fsencode(dst), out,
                              len(out), err, len(err))
    if rc:
        raise MiError(rc, err.value.decode(errors="replace"))
    return os.fsdecode(out.value)


def resolve_chown(chown, preserve_owner=False):
    """mi_resolve_chown: (uid, gid) of a --chown string, the way utils.ResolveChown reads it."""
    uid, gid = C.c_int64(), C.c_int64()
    err = C.create_string_buffer(300)
    rc = load_library().mi_resolve_chown(os.fsencode(chown), int(preserve_owner), C.byref(uid), C.byref(gid), err, len(err))
    if rc:
        raise MiError(rc, err.value.decode(errors="replace"))
    return uid.value, gid.value


def path_match(pattern, name):
    """mi_path_match: Go's filepath.Match; raises MiError(MI_ERR_INVALID) for ErrBadPattern."""
    m = C.c_int()
    rc = load_library().mi_path_match(os.fsencode(pattern), os.fsencode(name), C.byref(m))
    if rc:
        raise MiError(rc, "syntax error in pattern")
    return bool(m.value)


def context_sources(context_root, from_paths):
    """mi_context_sources: addCopyStep.resolveFromPaths -- the sources joined to the context root and globbed."""
    arr = (C.c_char_p * max(len(from_paths), 1))(*[os.fsencode(x) for x in from_paths])
    n, nbytes = C.c_uint64(), C.c_uint64()
    L = load_library()
    rc = L.mi_context_sources(os.fsencode(context_root), arr, len(from_paths), None, 0, C.byref(n), C.byref(nbytes))
    if rc not in (0, -7):
        raise MiError(rc, "mi_context_sources")
    buf = C.create_string_buffer(max(nbytes.value, 1))
    rc = L.mi_context_sources(os.fsencode(context_root), arr, len(from_paths), buf, nbytes.value, C.byref(n), C.byref(nbytes))
    if rc:
        raise MiError(rc, "mi_context_sources")
    return [os.fsdecode(x) for x in buf.raw[:nbytes.value].split(b"\0")[:n.value]]


def _copy_op_array(ops, keep):
    cops = (CopyOp * max(len(ops), 1))()
    for i, o in enumerate(ops):
        srcs = [os.fsencode(x) for x in o["srcs"]]
        sarr = (C.c_char_p * max(len(srcs), 1))(*srcs)
        keep += [srcs, sarr]
        cops[i].src_root = os.fsencode(o["src_root"])
        cops[i].srcs, cops[i].n_srcs = sarr, len(srcs)
        cops[i].dst = os.fsencode(o["dst"])
        cops[i].uid, cops[i].gid = o.get("uid", 0), o.get("gid", 0)
    return cops


def _take_copy_layer(L, h, n, chunks=False):
    """mi_copy_layer -> list of entry dicts (commit order) with an extra "src" key and, for regular files of a
    content-aware commit, "root" (32 bytes); chunks: the layer of a handle with MEMFS_CHUNK_PACK, whose regular files also
    get "chunks", their recipes (asked for only then: two more calls per entry); frees the handle."""
    try:
        out = (TreeEntry * max(n, 1))()
        srcp = (C.c_char_p * max(n, 1))()
        rc = L.mi_copy_layer_entries(h, out, srcp, n)
        if rc:
            raise MiError(rc, "mi_copy_layer_entries")
        roots = np.zeros((max(n, 1), 32), dtype=np.uint8)
        has = np.zeros(max(n, 1), dtype=np.uint8)
        rc = L.mi_copy_layer_roots(h, roots.ctypes.data, has.ctypes.data, n)
        if rc:
            raise MiError(rc, "mi_copy_layer_roots")
        res = []
        for i in range(n):
            d = _entry_dict(out[i])
            d["src"] = os.fsdecode(srcp[i]) if srcp[i] is not None else ""
            if has[i]:
                d["root"] = roots[i].tobytes()
            nc = C.c_uint64()
            if chunks:
                rc = L.mi_copy_layer_chunks(h, i, None, None, 0, C.byref(nc))
                if rc:
                    raise MiError(rc, "mi_copy_layer_chunks")
            if nc.value:                                      # the file's recipe
                dg = np.zeros((nc.value, 32), dtype=np.uint8)
                ln = np.zeros(nc.value, dtype=np.uint32)
                rc = L.mi_copy_layer_chunks(h, i, dg.ctypes.data, ln.ctypes.data, nc.value, C.byref(nc))
                if rc:
                    raise MiError(rc, "mi_copy_layer_chunks")
                d["chunks"] = [(dg[k].tobytes(), int(ln[k])) for k in range(nc.value)]
            res.append(d)
        return res
    finally:
        L.mi_copy_layer_free(h)


COPY_CHOWN, COPY_INTERNAL, COPY_PRESERVE_OWNER = 1, 2, 4


def copy_op_execute(op, chown=False, internal=False, preserve_owner=False, blacklist=()):
    """mi_copy_op_execute: CopyOperation.Execute -- the on-disk copy of a COPY/ADD step."""
    keep = []
    cops = _copy_op_array([op], keep)
    bl = (C.c_char_p * max(len(blacklist), 1))(*[os.fsencode(x) for x in blacklist])
    err = C.create_string_buffer(600)
    flags = (COPY_CHOWN if chown else 0) | (COPY_INTERNAL if internal else 0) | (COPY_PRESERVE_OWNER if preserve_owner else 0)
    rc = load_library().mi_copy_op_execute(cops, flags, bl, len(blacklist), err, len(err))
    if rc:
        raise MiError(rc, "mi_copy_op_execute: %s" % err.value.decode(errors="replace"))


def copy_ops_layer(tree, tree_root, ops, now_sec=0):
    """Harness helper over the MemFS handle: a tree rooted at tree_root (an existing directory) that holds `tree`
    (entry dicts, merged as a base layer would be), then AddLayerByCopyOps(ops) -- ops = dicts(src_root, srcs, dst,
    uid, gid).  Returns the layer as entry dicts in commit order with an extra "src" key."""
    with MemFS(tree_root, now_sec=now_sec) as fs:
        if tree:
            fs.update_from_entries(tree)
        return fs.add_layer_by_copy_ops(ops)


class MemFS:
    """mi_memfs_*: the reference's MemFS (lib/snapshot/mem_fs.go) as a handle -- one tree for the life of a build.

    fs = MemFS(root, blacklist); fs.update_from_entries(tar_entries); layer = fs.add_layer_by_scan(walk_entries);
    layer = fs.add_layer_by_copy_ops([op, ...]); fs.entries()."""

    def __init__(self, root, blacklist=(), now_sec=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        bl = (C.c_char_p * max(len(blacklist), 1))(*[os.fsencode(x) for x in blacklist])
        rc = self._lib.mi_memfs_create(os.fsencode(root), bl, len(blacklist), now_sec, C.byref(self._h))
        if rc:
            raise MiError(rc, "mi_memfs_create: unable to stat root dir: %s" % root)
        self.root, self.blacklist = root, list(blacklist)
        self._chunk_pack = False                              # set_options(chunk_pack=True)
        self._chunk_zpack = False                             # set_options(chunk_zpack=True)
        self._pack_engine = None                              # the Engine of the last commit that could make a pack: take_pack's Pack is its child

    def _check(self, rc, what):
        if rc:
            raise MiError(rc, "%s: %s" % (what, self._lib.mi_memfs_error(self._h).decode(errors="replace")))

    def close(self):
        if self._h:
            self._lib.mi_memfs_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_clock(self, now_sec):
        self._check(self._lib.mi_memfs_set_clock(self._h, now_sec), "mi_memfs_set_clock")

    def reset(self):
        self._check(self._lib.mi_memfs_reset(self._h), "mi_memfs_reset")

    def update_from_entries(self, layer):
        """UpdateFromTarReader (untar = false); returns the number of headers merged."""
        keep = []
        arr = _entry_array(layer, keep)
        n = C.c_uint64()
        self._check(self._lib.mi_memfs_update_from_entries(self._h, arr, len(layer), C.byref(n)), "mi_memfs_update_from_entries")
        return n.value

    def update_from_tar(self, tar_path, untar=False):
        """UpdateFromTarPath on a PLAIN tar: its headers merged into the tree; untar=True also writes it below the root
        (untarOneItem).  Returns the number of headers merged."""
        ents = tar_entries(tar_path)
        if not untar:
            return self.update_from_entries(ents)
        keep = []
        arr = _entry_array(ents, keep)
        offs = (C.c_uint64 * max(len(ents), 1))(*[e["data_offset"] for e in ents])
        n = C.c_uint64()
        self._check(self._lib.mi_memfs_untar(self._h, os.fsencode(tar_path), arr, offs, len(ents), C.byref(n)), "mi_memfs_untar")
        return n.value

    def add_layer_by_scan(self, walked, roots=None):
        """createLayerByScan on a walk of the root (tree_walk(root, root, blacklist, TREE_SCAN, full=True)); roots: an
        (n_files, 32) uint8 array indexed by file_index, or None."""
        keep = []
        arr = _entry_array(walked, keep)
        h, n = C.c_void_p(), C.c_uint64()
        rp, stride = None, 0
        if roots is not None:
            roots = np.ascontiguousarray(roots, dtype=np.uint8)
            rp, stride = roots.ctypes.data, roots.strides[0] if roots.ndim == 2 else 32
        self._check(self._lib.mi_memfs_add_layer_by_scan(self._h, arr, len(walked), rp, stride, C.byref(h), C.byref(n)),
                    "mi_memfs_add_layer_by_scan")
        return _take_copy_layer(self._lib, h, n.value)

    def add_layer_by_copy_ops(self, ops):
        keep = []
        cops = _copy_op_array(ops, keep)
        h, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.mi_memfs_add_layer_by_copy_ops(self._h, cops, len(ops), C.byref(h), C.byref(n)),
                    "mi_memfs_add_layer_by_copy_ops")
        return _take_copy_layer(self._lib, h, n.value)

    def commit_layer(self, must_scan=False, ops=(), out_fd=-1, gzip_level=GZIP_DEFAULT, engine=None, mode_with_type=False, want_layer=True):
        """step.commitLayer: the layer by scan or by copy ops, written through the layer writer.  engine = an Engine: the
        content-aware commit (walk + stage + GPU scan + diff with chunk roots + tar from HBM, one call); a list of Engines: the
        same over several GPUs (mi_memfs_commit_layer_n); None: the reference's.  Returns None when there is nothing to do, else
        dict(tar_digest, gzip_digest, tar_bytes, gzip_bytes, n_entries, layer=[entries, with "root" for scanned files], stats={...});
        want_layer=False leaves the layer's entries in the library (layer=None): a timing harness should not measure 100 000 dicts."""
        keep = []
        cops = _copy_op_array(list(ops), keep)
        cfg = LayerConfig()
        self._lib.mi_layer_config_default(C.byref(cfg))
        cfg.out_fd, cfg.gzip_level = out_fd, gzip_level
        if mode_with_type:
            cfg.flags |= LAYER_MODE_WITH_TYPE
        res, h, done = LayerResult(), C.c_void_p(), C.c_int()
        hp = C.byref(h) if want_layer else None
        if isinstance(engine, (list, tuple)):
            for e in engine:
                e._children.add(self)
            ctxs = (C.c_void_p * max(len(engine), 1))(*[e._h for e in engine])
            self._check(self._lib.mi_memfs_commit_layer_n(self._h, ctxs, len(engine), int(must_scan), cops, len(ops), C.byref(cfg),
                                                          C.byref(res), hp, C.byref(done)), "mi_memfs_commit_layer_n")
        else:
            ctx = engine._h if engine is not None else None
            if engine is not None and (self._chunk_pack or self._chunk_zpack):
                self._pack_engine = engine                    # only such a commit makes (or drops) the handle's pack
            if engine is not None:
                engine._children.add(self)                    # the handle keeps a batch of that ctx: given back before it dies
            self._check(self._lib.mi_memfs_commit_layer(self._h, ctx, int(must_scan), cops, len(ops), C.byref(cfg), C.byref(res),
                                                        hp, C.byref(done)), "mi_memfs_commit_layer")
        if not done.value:
            return None
        return {"tar_digest": Digest.from_raw(res.tar_sha256), "gzip_digest": Digest.from_raw(res.gzip_sha256),
                "tar_bytes": res.tar_bytes, "gzip_bytes": res.gzip_bytes, "n_entries": res.n_entries,
                "layer": _take_copy_layer(self._lib, h, int(res.n_entries), self._chunk_pack or self._chunk_zpack) if want_layer else None, "stats": self.commit_stats()}

    def commit_stats(self):
        st = CommitStats()
        self._check(self._lib.mi_memfs_commit_stats(self._h, C.byref(st)), "mi_memfs_commit_stats")
        return st.as_dict()

    def set_index(self, index):
        """every content-aware commit adds its batch's chunks to `index` (a ChunkIndex of the same Engine); None stops"""
        self._index = index                                   # (kept alive)
        self._check(self._lib.mi_memfs_set_index(self._h, index._h if index is not None else None), "mi_memfs_set_index")

    def reserve_device(self, engine, files, nbytes):
        """the handle's batch ahead of its first commit (a ctx's first use costs: see the header)"""
        engine._children.add(self)
        self._check(self._lib.mi_memfs_reserve_device(self._h, engine._h, files, nbytes), "mi_memfs_reserve_device")

    def set_options(self, trust_ctime=False, chunk_pack=False, chunk_zpack=False, zpack_level=1, gzip_device=False):
        """MI_MEMFS_TRUST_CTIME: scan commits do not read files again whose inode is what it was when they were hashed.
        MI_MEMFS_CHUNK_PACK: a commit (one Engine, an index set) also packs the chunks the index did not know -- take_pack() --
        and its layer's regular files carry "chunks": [(digest, length), ...], their recipes.
        MI_MEMFS_CHUNK_ZPACK: the same with the chunks coded straight from the arena into a compressed pack -- take_zpack();
        both at once are refused (MI_ERR_INVALID); zpack_level=2 (MI_MEMFS_ZPACK_LEVEL2): that zpack is coded at level 2.
        MI_MEMFS_GZIP_DEVICE: a commit with an Engine codes the layer's gzip leg on its device (only the gzip digest and size differ)"""
        _zpack_level_flag(zpack_level)
        self._check(self._lib.mi_memfs_set_options(self._h, (MEMFS_TRUST_CTIME if trust_ctime else 0) | (MEMFS_CHUNK_PACK if chunk_pack else 0) |
                                                   (MEMFS_CHUNK_ZPACK if chunk_zpack else 0) | (MEMFS_ZPACK_LEVEL2 if zpack_level == 2 else 0) |
                                                   (MEMFS_GZIP_DEVICE if gzip_device else 0)),
                    "mi_memfs_set_options")
        self._chunk_pack, self._chunk_zpack = bool(chunk_pack), bool(chunk_zpack)

    def take_pack(self):
        """mi_memfs_take_pack: the Pack of the last commit made with chunk_pack, a child of the Engine that commit ran on"""
        h = C.c_void_p()
        self._check(self._lib.mi_memfs_take_pack(self._h, C.byref(h)), "mi_memfs_take_pack")
        return Pack(self._pack_engine, h)

    def take_zpack(self):
        """mi_memfs_take_zpack: the ZPack of the last commit made with chunk_zpack, a child of the Engine that commit ran on"""
        h = C.c_void_p()
        self._check(self._lib.mi_memfs_take_zpack(self._h, C.byref(h)), "mi_memfs_take_zpack")
        return ZPack(self._pack_engine, h)

    def release_device(self):
        if self._h:
            self._check(self._lib.mi_memfs_release_device(self._h), "mi_memfs_release_device")

    free = release_device                                     # what Engine.close asks of its children

    def root_of(self, path):
        """the chunk root the tree holds for a path ("/"-rooted below the root), or None if it was never scanned"""
        out = (C.c_uint8 * 32)()
        has = C.c_int()
        self._check(self._lib.mi_memfs_root_of(self._h, os.fsencode(path), out, C.byref(has)), "mi_memfs_root_of")
        return bytes(out) if has.value else None

    def checkpoint(self, new_root, sources):
        """MemFS.Checkpoint: copy what a later stage will COPY --from below new_root."""
        arr = (C.c_char_p * max(len(sources), 1))(*[os.fsencode(x) for x in sources])
        self._check(self._lib.mi_memfs_checkpoint(self._h, os.fsencode(new_root), arr, len(sources)), "mi_memfs_checkpoint")

    def scan(self):
        """walk the root with this MemFS's blacklist, then add_layer_by_scan"""
        return self.add_layer_by_scan(tree_walk(self.root, self.root, self.blacklist, TREE_SCAN, full=True))

    def entries(self):
        n = C.c_uint64()
        rc = self._lib.mi_memfs_entries(self._h, None, None, 0, C.byref(n))
        if rc not in (0, -7):
            self._check(rc, "mi_memfs_entries")
        out = (TreeEntry * max(n.value, 1))()
        srcp = (C.c_char_p * max(n.value, 1))()
        self._check(self._lib.mi_memfs_entries(self._h, out, srcp, n.value, C.byref(n)), "mi_memfs_entries")
        res = []
        for i in range(n.value):
            d = _entry_dict(out[i])
            d["src"] = os.fsdecode(srcp[i]) if srcp[i] is not None else ""
            res.append(d)
        return res


class Layer:
    """mi_layer_*: the layer tar writer with its two stream digests (host threads, no GPU).

    with Layer(out_fd=fd, gzip_level=GZIP_DEFAULT) as l:
        l.add(entry_dict, src_path); l.add_whiteout("/deleted/path"); pair = l.finish()
    finish() -> dict(tar_digest="sha256:..", gzip_digest=.., tar_bytes, gzip_bytes, n_entries)."""

    def __init__(self, out_fd=-1, gzip_level=GZIP_DEFAULT, mode_with_type=False):
        self._lib = load_library()
        cfg = LayerConfig()
        self._lib.mi_layer_config_default(C.byref(cfg))
        cfg.out_fd, cfg.gzip_level = out_fd, gzip_level
        cfg.flags = LAYER_MODE_WITH_TYPE if mode_with_type else 0
        self._gzip = gzip_level != GZIP_OFF
        self._h = C.c_void_p()
        rc = self._lib.mi_layer_begin(C.byref(cfg), C.byref(self._h))
        if rc:
            raise MiError(rc, "mi_layer_begin")

    def _check(self, rc):
        if rc:
            raise MiError(rc, self._lib.mi_layer_error(self._h).decode(errors="replace"))

    def set_gzip_engine(self, engine):
        """mi_layer_set_gzip_ctx: the gzip leg of this layer is coded on the Engine's device (before the first add; there is one
        device level, whatever gzip_level says).  The Engine must outlive the layer"""
        self._gzip_engine = engine
        self._check(self._lib.mi_layer_set_gzip_ctx(self._h, engine._h if engine is not None else None))

    def add(self, entry, src_path=None):
        keep = []
        arr = _entry_array([entry], keep)
        self._check(self._lib.mi_layer_add(self._h, arr, os.fsencode(src_path) if src_path is not None else None))

    def add_batch_file(self, entry, batch, file_index):
        """the entry with its content taken from a staged batch (the bytes the GPU scanned), not from a path"""
        keep = []
        arr = _entry_array([entry], keep)
        self._check(self._lib.mi_layer_add_batch_file(self._h, arr, batch._h, file_index))

    def io_counts(self):
        o, b = C.c_uint64(), C.c_uint64()
        self._check(self._lib.mi_layer_io_counts(self._h, C.byref(o), C.byref(b)))
        return o.value, b.value

    def add_whiteout(self, deleted_path):
        self._check(self._lib.mi_layer_add_whiteout(self._h, os.fsencode(deleted_path)))

    def finish(self):
        res = LayerResult()
        self._check(self._lib.mi_layer_finish(self._h, C.byref(res)))
        return {"tar_digest": Digest.from_raw(res.tar_sha256),
                "gzip_digest": Digest.from_raw(res.gzip_sha256) if self._gzip else None,
                "tar_sha256": bytes(res.tar_sha256), "gzip_sha256": bytes(res.gzip_sha256),
                "tar_bytes": res.tar_bytes, "gzip_bytes": res.gzip_bytes, "n_entries": res.n_entries}

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mi_layer_free(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def layer_header_bytes(entry, mode_with_type=False):
    """The tar header block(s) the layer writer emits for one entry dict (mode_with_type: the Mode field
    keeps the st_mode's file-type bits like Go <= 1.8 wrote them, MI_LAYER_MODE_WITH_TYPE)."""
    keep = []
    arr = _entry_array([entry], keep)
    n = C.c_uint64()
    buf = (C.c_uint8 * 8192)()
    rc = load_library().mi_layer_header_bytes(arr, LAYER_MODE_WITH_TYPE if mode_with_type else 0, buf, 8192, C.byref(n))
    if rc:
        raise MiError(rc, "mi_layer_header_bytes")
    return bytes(buf[: n.value])


def chunk_root(digests, alg=DIGEST_SHA256):
    """mi_chunk_root_alg: the file-level root of a list of chunk digests (bytes-like of n x 32, or an
    (n, 32) uint8 array) -- what a split file's parts combine to.  alg: the DIGEST_* of the ctx the
    digests came from (Engine.chunk_digest)."""
    a = np.ascontiguousarray(np.frombuffer(digests, dtype=np.uint8) if not isinstance(digests, np.ndarray) else digests,
                             dtype=np.uint8).reshape(-1, 32)
    out = np.zeros(32, dtype=np.uint8)
    rc = load_library().mi_chunk_root_alg(alg, a.ctypes.data if a.size else None, a.shape[0], out.ctypes.data)
    if rc:
        raise MiError(rc, "mi_chunk_root_alg")
    return out.tobytes()


def cache_key(cache_id):
    out = C.create_string_buffer(len(os.fsencode(cache_id)) + 64)
    rc = load_library().mi_cache_key(os.fsencode(cache_id), out, len(out))
    if rc:
        raise MiError(rc, "mi_cache_key")
    return out.value.decode()


def cache_create_entry(tar_sha256=None, gzip_sha256=None):
    """createEntry: raw 32-byte digests -> "tarHex,gzipHex"; (None, None) -> the empty marker."""
    out = C.create_string_buffer(160)
    t = (C.c_uint8 * 32).from_buffer_copy(tar_sha256) if tar_sha256 is not None else None
    g = (C.c_uint8 * 32).from_buffer_copy(gzip_sha256) if gzip_sha256 is not None else None
    rc = load_library().mi_cache_create_entry(t, g, out, len(out))
    if rc:
        raise MiError(rc, "mi_cache_create_entry")
    return out.value.decode()


def cache_parse_entry(entry):
    """parseEntry: -> None for the empty marker, else (tar Digest, gzip Digest); ValueError if malformed."""
    t, g, e = (C.c_uint8 * 32)(), (C.c_uint8 * 32)(), C.c_int()
    rc = load_library().mi_cache_parse_entry(entry.encode(), C.byref(e), t, g)
    if rc:
        raise ValueError("parse redis entry: %s" % entry)
    if e.value:
        return None
    return Digest.from_raw(t), Digest.from_raw(g)


def cache_parse_entry_str(entry):
    """parseEntry to the letter: ("sha256:<first half>", "sha256:<rest>"); ValueError without a comma."""
    raw = entry.encode()
    a, b = C.create_string_buffer(len(raw) + 16), C.create_string_buffer(len(raw) + 16)
    rc = load_library().mi_cache_parse_entry_str(raw, a, len(a), b, len(b))
    if rc:
        raise ValueError("parse redis entry: %s" % entry)
    return Digest(a.value.decode()), Digest(b.value.decode())


class ChunkIndex:
    """mi_index_*: device-resident digest set; add_batch() says which chunks earlier
    batches already held, export()/load() move it as bytes (keyvalue.Store value)."""

    def __init__(self, engine, capacity_hint=0):
        self._eng = engine
        self._lib = engine._lib
        self._h = C.c_void_p()
        engine._check(self._lib.mi_index_create(engine._h, capacity_hint, C.byref(self._h)))
        engine._children.add(self)

    def __len__(self):
        n = C.c_uint64()
        self._eng._check(self._lib.mi_index_count(self._h, C.byref(n)))
        return n.value

    def add_batch(self, batch):
        """-> (known flags per chunk as np.uint8, n_new, n_known)."""
        n = batch.counts()[1]
        known = np.zeros(max(n, 1), dtype=np.uint8)
        n_new, n_known = C.c_uint64(), C.c_uint64()
        self._eng._check(self._lib.mi_index_add_batch(self._h, batch._h, known.ctypes.data, n,
                                                      C.byref(n_new), C.byref(n_known)))
        return known[:n], n_new.value, n_known.value

    def export(self):
        n = len(self)
        out = np.zeros((max(n, 1), 32), dtype=np.uint8)
        self._eng._check(self._lib.mi_index_export(self._h, out.ctypes.data, n))
        return out[:n].tobytes()

    def load(self, blob):
        if len(blob) % 32:
            raise ValueError("index blob must be a multiple of 32 bytes")
        arr = np.frombuffer(blob, dtype=np.uint8)
        n_new = C.c_uint64()
        self._eng._check(self._lib.mi_index_import(self._h, arr.ctypes.data if arr.size else None,
                                                   len(blob) // 32, C.byref(n_new)))
        return n_new.value

    def query(self, digests):
        """mi_index_query: which of the digests (n x 32 bytes, repeats allowed) the index holds, without adding any
        -> held flags per row as np.uint8"""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        n = len(d)
        held = np.zeros(max(n, 1), dtype=np.uint8)
        self._eng._check(self._lib.mi_index_query(self._h, d.ctypes.data if n else None, n, held.ctypes.data, None))
        return held[:n]

    def query_batch(self, batch):
        """mi_index_query_batch: the same over the device-resident chunk digests of a batch that has run -- what add_batch
        would report as known, without adding -> held flags per chunk as np.uint8"""
        n = batch.counts()[1]
        held = np.zeros(max(n, 1), dtype=np.uint8)
        self._eng._check(self._lib.mi_index_query_batch(self._h, batch._h, held.ctypes.data, n, None))
        return held[:n]

    def prune(self, digests, keep=True):
        """mi_index_prune: forget digests.  digests (n x 32 bytes, repeats and unknown ones allowed): what STAYS (keep=True:
        everything else goes) or what GOES (keep=False).  The table is rebuilt for the survivors -> IndexPruneInfo"""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        info = IndexPruneInfo()
        self._eng._check(self._lib.mi_index_prune(self._h, d.ctypes.data if len(d) else None, len(d),
                                                  INDEX_PRUNE_KEEP if keep else INDEX_PRUNE_DROP, C.byref(info)))
        return info

    def retain(self, zset):
        """mi_index_retain_zset: keep exactly the digests a ZSet of the same Engine holds; no list crosses the host
        -> IndexPruneInfo"""
        info = IndexPruneInfo()
        self._eng._check(self._lib.mi_index_retain_zset(self._h, zset._h, C.byref(info)))
        return info

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mi_index_free(self._h)
            self._h = None

    free = close
    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Pack:
    """mi_pack_*: selected chunks of a batch as one blob in device memory (Batch.pack, MemFS.take_pack).  A child of its
    Engine, independent of the batch it came from."""

    def __init__(self, engine, handle):
        self._eng = engine
        self._lib = engine._lib
        self._h = handle
        engine._children.add(self)

    @property
    def info(self):
        out = PackInfo()
        self._eng._check(self._lib.mi_pack_get_info(self._h, C.byref(out)))
        return out

    def __len__(self):
        return self.info.n_entries

    def entries(self):
        """the entries in blob order: a numpy array of PACK_ENTRY_DTYPE"""
        n = self.info.n_entries
        out = np.zeros(max(n, 1), dtype=PACK_ENTRY_DTYPE)
        self._eng._check(self._lib.mi_pack_entries(self._h, out.ctypes.data, n))
        return out[:n]

    def read(self, offset, length):
        out = np.zeros(max(length, 1), dtype=np.uint8)
        self._eng._check(self._lib.mi_pack_read(self._h, offset, out.ctypes.data, length))
        return out[:length].tobytes()

    def bytes(self):
        """the whole blob"""
        return self.read(0, self.info.blob_bytes)

    def device(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._eng._check(self._lib.mi_pack_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def compress(self, verify=False, level=1, entropy=False):
        """mi_pack_compress: every chunk coded on its own as one LZ4 block (or kept raw) on the device -> ZPack; this pack
        is not changed.  level=2 (MI_ZPACK_LEVEL2): the denser parse, the same block format.  entropy=True (MI_ZPACK_ENTROPY):
        the level's form wrapped in a Huffman code where that is smaller by more than a sixteenth (form H)"""
        h = C.c_void_p()
        flags = (ZPACK_VERIFY if verify else 0) | _zpack_level_flag(level) | (ZPACK_ENTROPY if entropy else 0)
        self._eng._check(self._lib.mi_pack_compress(self._h, flags, C.byref(h)))
        return ZPack(self._eng, h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mi_pack_free(self._h)
            self._h = None

    free = close
    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ZPack:
    """mi_zpack_*: a compressed pack in device memory (Pack.compress).  A child of its Engine, independent of the pack it
    came from."""

    def __init__(self, engine, handle):
        self._eng = engine
        self._lib = engine._lib
        self._h = handle
        engine._children.add(self)

    @property
    def info(self):
        out = ZPackInfo()
        self._eng._check(self._lib.mi_zpack_get_info(self._h, C.byref(out)))
        return out

    def __len__(self):
        return self.info.n_entries

    def count_forms(self):
        """mi_zpack_count_forms: ZForms, counted on the device from every stored span's first bytes"""
        out = ZForms()
        self._eng._check(self._lib.mi_zpack_count_forms(self._h, C.byref(out)))
        return out

    def entries(self):
        """the entries in blob order: a numpy array of ZPACK_ENTRY_DTYPE"""
        n = self.info.n_entries
        out = np.zeros(max(n, 1), dtype=ZPACK_ENTRY_DTYPE)
        self._eng._check(self._lib.mi_zpack_entries(self._h, out.ctypes.data, n))
        return out[:n]

    def read(self, offset=0, length=None):
        """bytes [offset, offset + length) of the compressed blob; read() is the whole blob"""
        if length is None:
            length = self.info.blob_bytes - offset
        out = np.zeros(max(length, 1), dtype=np.uint8)
        self._eng._check(self._lib.mi_zpack_read(self._h, offset, out.ctypes.data, length))
        return out[:length].tobytes()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mi_zpack_free(self._h)
            self._h = None

    free = close
    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class PackSet:
    """mi_packset_*: packs resident on the engine's device, addressed by digest (Engine.packset): what Batch.add_recipes
    assembles files from.  A child of its Engine."""

    def __init__(self, engine, entries_hint=0):
        self._eng = engine
        self._lib = engine._lib
        h = C.c_void_p()
        engine._check(self._lib.mi_packset_create(engine._h, entries_hint, C.byref(h)))
        self._h = h
        engine._children.add(self)

    def add_blob(self, blob, entries, verify=False):
        """mi_packset_add_blob: a pack from host memory (blob: bytes-like; entries: PACK_ENTRY_DTYPE rows).  A failure raises
        MiError with .first_bad = the entry the call names."""
        b = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob).view(np.uint8)
        e = np.ascontiguousarray(entries, dtype=PACK_ENTRY_DTYPE)
        bad = C.c_uint64()
        rc = self._lib.mi_packset_add_blob(self._h, b.ctypes.data if b.size else None, b.size, e.ctypes.data if e.size else None, e.size,
                                           PACKSET_VERIFY if verify else 0, C.byref(bad))
        if rc:
            err = MiError(rc, self._lib.mi_last_error(self._eng._h).decode())
            err.first_bad = bad.value
            raise err

    def add_pack(self, pack, verify=False):
        """mi_packset_add_pack: a Pack of the same Engine, copied where it lies; the pack stays the caller's"""
        self._eng._check(self._lib.mi_packset_add_pack(self._h, pack._h, PACKSET_VERIFY if verify else 0))

    def add_zblob(self, blob, entries, verify=False):
        """mi_packset_add_zblob: a compressed pack from host memory (entries: ZPACK_ENTRY_DTYPE rows), decoded on the device;
        the set holds plain chunks as ever.  A failure raises MiError with .first_bad = the entry the call names."""
        b = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob).view(np.uint8)
        e = np.ascontiguousarray(entries, dtype=ZPACK_ENTRY_DTYPE)
        bad = C.c_uint64()
        rc = self._lib.mi_packset_add_zblob(self._h, b.ctypes.data if b.size else None, b.size, e.ctypes.data if e.size else None, e.size,
                                            PACKSET_VERIFY if verify else 0, C.byref(bad))
        if rc:
            self._raise(rc, bad.value)

    def add_zpack(self, zpack, verify=False):
        """mi_packset_add_zpack: a ZPack of the same Engine, decoded where it lies; the zpack stays the caller's"""
        self._eng._check(self._lib.mi_packset_add_zpack(self._h, zpack._h, PACKSET_VERIFY if verify else 0))

    @staticmethod
    def _request(digests, lengths):
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint32).reshape(-1)
        if ln is not None and len(ln) != len(d):
            raise ValueError("%d lengths for %d digests" % (len(ln), len(d)))
        return d, ln

    def _raise(self, rc, first_bad=None):
        err = MiError(rc, self._lib.mi_last_error(self._eng._h).decode())
        if first_bad is not None:
            err.first_bad = first_bad
        raise err

    def missing(self, digests, lengths=None):
        """mi_packset_missing: which of the request's digests (n x 32 bytes; lengths: n or None) the set lacks.
        -> (held: uint8[n], want_rows: uint64[n_want] -- the rows of first occurrence of every missing digest, ascending --,
        WantInfo)"""
        d, ln = self._request(digests, lengths)
        n = len(d)
        args = (self._h, d.ctypes.data if n else None, ln.ctypes.data if ln is not None and n else None, n)
        held = np.zeros(max(n, 1), dtype=np.uint8)
        info = WantInfo()
        rc = self._lib.mi_packset_missing(*args, held.ctypes.data, None, 0, C.byref(info))       # the sizing call
        if rc:
            self._raise(rc)
        want = np.zeros(max(info.n_want, 1), dtype=np.uint64)
        if info.n_want:
            rc = self._lib.mi_packset_missing(*args, held.ctypes.data, want.ctypes.data, info.n_want, C.byref(info))
            if rc:
                self._raise(rc)
        return held[:n], want[:info.n_want], info

    def pack(self, digests, lengths=None, verify=False):
        """mi_packset_pack: a Pack of every distinct requested digest once, in order of first occurrence, from whatever packs
        of the set hold them.  A failure raises MiError with .first_bad = the request row the call names."""
        d, ln = self._request(digests, lengths)
        n = len(d)
        h, bad = C.c_void_p(), C.c_uint64()
        rc = self._lib.mi_packset_pack(self._h, d.ctypes.data if n else None, ln.ctypes.data if ln is not None and n else None, n,
                                       SUBPACK_VERIFY if verify else 0, C.byref(h), C.byref(bad))
        if rc:
            self._raise(rc, bad.value)
        return Pack(self._eng, h)

    @property
    def info(self):
        out = PackSetInfo()
        self._eng._check(self._lib.mi_packset_get_info(self._h, C.byref(out)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mi_packset_free(self._h)
            self._h = None

    free = close
    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ZSet:
    """mi_zset_*: compressed packs resident on the engine's device AS STORED, addressed by digest (Engine.zset): what
    ZSet.zpack cuts compressed sub-packs out of without a coder and what Batch.add_zrecipes decodes files from, row by row,
    straight into the arena.  A child of its Engine."""

    def __init__(self, engine, entries_hint=0):
        self._eng = engine
        self._lib = engine._lib
        h = C.c_void_p()
        engine._check(self._lib.mi_zset_create(engine._h, entries_hint, C.byref(h)))
        self._h = h
        engine._children.add(self)

    def _raise(self, rc, first_bad=None):
        err = MiError(rc, self._lib.mi_last_error(self._eng._h).decode())
        if first_bad is not None:
            err.first_bad = first_bad
        raise err

    def add_zblob(self, blob, entries, verify=False):
        """mi_zset_add_zblob: a compressed pack from host memory (entries: ZPACK_ENTRY_DTYPE rows), kept as stored; verify:
        decoded into a scratch and hashed on the device first.  A failure raises MiError with .first_bad = the entry named."""
        b = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob).view(np.uint8)
        e = np.ascontiguousarray(entries, dtype=ZPACK_ENTRY_DTYPE)
        bad = C.c_uint64()
        rc = self._lib.mi_zset_add_zblob(self._h, b.ctypes.data if b.size else None, b.size, e.ctypes.data if e.size else None, e.size,
                                         ZSET_VERIFY if verify else 0, C.byref(bad))
        if rc:
            self._raise(rc, bad.value)

    def add_zpack(self, zpack, verify=False):
        """mi_zset_add_zpack: a ZPack of the same Engine, copied where it lies; the zpack stays the caller's"""
        self._eng._check(self._lib.mi_zset_add_zpack(self._h, zpack._h, ZSET_VERIFY if verify else 0))

    def zpack(self, digests, lengths=None, verify=False):
        """mi_zset_zpack: a ZPack of every distinct requested digest once, in order of first occurrence, the stored forms moved
        as they are -- byte for byte PackSet.pack(...).compress().  A failure raises MiError with .first_bad = the request row."""
        d, ln = PackSet._request(digests, lengths)
        n = len(d)
        h, bad = C.c_void_p(), C.c_uint64()
        rc = self._lib.mi_zset_zpack(self._h, d.ctypes.data if n else None, ln.ctypes.data if ln is not None and n else None, n,
                                     ZPACK_VERIFY if verify else 0, C.byref(h), C.byref(bad))
        if rc:
            self._raise(rc, bad.value)
        return ZPack(self._eng, h)

    def zpack_unwrapped(self, digests, lengths=None, verify=False):
        """mi_zset_zpack_unwrapped: ZSet.zpack for a reader built before the entropy stage -- an entry the set holds as form H
        carries its inner form (the LZ4 block, or the plain bytes as a raw entry), every other entry is moved as it is.  A
        failure raises MiError with .first_bad = the request row."""
        d, ln = PackSet._request(digests, lengths)
        n = len(d)
        h, bad = C.c_void_p(), C.c_uint64()
        rc = self._lib.mi_zset_zpack_unwrapped(self._h, d.ctypes.data if n else None, ln.ctypes.data if ln is not None and n else None, n,
                                               ZPACK_VERIFY if verify else 0, C.byref(h), C.byref(bad))
        if rc:
            self._raise(rc, bad.value)
        return ZPack(self._eng, h)

    def pack(self, digests, lengths=None, verify=False):
        """mi_zset_pack: PackSet.pack over the compressed set -- a plain Pack of every distinct requested digest once, in order
        of first occurrence, every stored form decoded straight to its place.  A failure raises MiError with .first_bad = the
        request row."""
        d, ln = PackSet._request(digests, lengths)
        n = len(d)
        h, bad = C.c_void_p(), C.c_uint64()
        rc = self._lib.mi_zset_pack(self._h, d.ctypes.data if n else None, ln.ctypes.data if ln is not None and n else None, n,
                                    SUBPACK_VERIFY if verify else 0, C.byref(h), C.byref(bad))
        if rc:
            self._raise(rc, bad.value)
        return Pack(self._eng, h)

    def missing(self, digests, lengths=None):
        """mi_zset_missing: PackSet.missing over the compressed set -- which of the request's digests (n x 32 bytes; lengths:
        n or None) the set lacks.  -> (held: uint8[n], want_rows: uint64[n_want] -- the rows of first occurrence of every
        missing digest, ascending --, WantInfo with held_bytes = the set's PLAIN lengths)"""
        d, ln = PackSet._request(digests, lengths)
        n = len(d)
        args = (self._h, d.ctypes.data if n else None, ln.ctypes.data if ln is not None and n else None, n)
        held = np.zeros(max(n, 1), dtype=np.uint8)
        info = WantInfo()
        rc = self._lib.mi_zset_missing(*args, held.ctypes.data, None, 0, C.byref(info))          # the sizing call
        if rc:
            self._raise(rc)
        want = np.zeros(max(info.n_want, 1), dtype=np.uint64)
        if info.n_want:
            rc = self._lib.mi_zset_missing(*args, held.ctypes.data, want.ctypes.data, info.n_want, C.byref(info))
            if rc:
                self._raise(rc)
        return held[:n], want[:info.n_want], info

    def prune(self, digests, keep=True, min_live_permille=0):
        """mi_zset_prune: drop digests in place and give memory back.  digests (n x 32 bytes, repeats and unknown ones allowed):
        what STAYS (keep=True: everything else goes) or what GOES (keep=False).  Blobs left with nothing live are freed; blobs
        whose live bytes fall under min_live_permille of their size have their survivors moved, verbatim, into one new blob.
        -> PruneInfo"""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        info = PruneInfo()
        rc = self._lib.mi_zset_prune(self._h, d.ctypes.data if len(d) else None, len(d), ZSET_PRUNE_KEEP if keep else ZSET_PRUNE_DROP,
                                     min_live_permille, C.byref(info))
        if rc:
            self._raise(rc)
        return info

    def recode(self, level=2, verify=False, scratch_bytes=0, entropy=False):
        """mi_zset_recode: code every chunk the set holds again at `level` and replace a stored form only where the new one is
        strictly smaller; the blobs that held a replaced form are rewritten into one new blob and freed, the others are not
        touched.  verify: every entry's bytes are hashed against its digest first, every replaced form again from the new blob.
        scratch_bytes bounds one round's scratch (0: 256 MiB); the result does not depend on it.  entropy=True (MI_ZPACK_ENTROPY):
        the candidate is the level's form with the entropy stage over it (form H where that is smaller).  -> RecodeInfo"""
        info = RecodeInfo()
        flags = _zpack_level_flag(level) | (ZSET_RECODE_VERIFY if verify else 0) | (ZPACK_ENTROPY if entropy else 0)
        rc = self._lib.mi_zset_recode(self._h, flags, scratch_bytes, C.byref(info))
        if rc:
            self._raise(rc)
        return info

    def set_epoch(self, epoch):
        """mi_zset_set_epoch: the first call turns ageing on (a stamp per table slot on the device, everything held stamped
        `epoch`); later calls advance the clock and never turn it back"""
        rc = self._lib.mi_zset_set_epoch(self._h, epoch)
        if rc:
            self._raise(rc)

    @property
    def epoch(self):
        """mi_zset_get_epoch -> (ageing: bool, epoch, stamp_bytes: device bytes of the stamps, 0 while ageing is off)"""
        on, ep, nbytes = C.c_uint32(), C.c_uint32(), C.c_uint64()
        rc = self._lib.mi_zset_get_epoch(self._h, C.byref(on), C.byref(ep), C.byref(nbytes))
        if rc:
            self._raise(rc)
        return bool(on.value), ep.value, nbytes.value

    def touch(self, digests):
        """mi_zset_touch: the stamp of every held digest among `digests` (n x 32 bytes, repeats and unknown ones allowed)
        becomes the set's epoch -> TouchInfo"""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        info = TouchInfo()
        rc = self._lib.mi_zset_touch(self._h, d.ctypes.data if len(d) else None, len(d), C.byref(info))
        if rc:
            self._raise(rc)
        return info

    def stamps(self, digests):
        """mi_zset_stamps -> uint32[n]: each row's stamp, STAMP_NONE where the set does not hold the digest"""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros(max(len(d), 1), dtype=np.uint32)
        rc = self._lib.mi_zset_stamps(self._h, d.ctypes.data if len(d) else None, len(d), out.ctypes.data)
        if rc:
            self._raise(rc)
        return out[:len(d)]

    def age_census(self, bounds):
        """mi_zset_age_census: bounds (1 to 255 strictly ascending epochs) -> a list of len(bounds) + 1 AgeBin: bin i holds the
        digests with bounds[i-1] <= stamp < bounds[i], the first begins at 0, the last is open above"""
        b = np.ascontiguousarray(bounds, dtype=np.uint32).reshape(-1)
        bins = (AgeBin * (len(b) + 1))()
        rc = self._lib.mi_zset_age_census(self._h, b.ctypes.data if len(b) else None, len(b), C.addressof(bins))
        if rc:
            self._raise(rc)
        return list(bins)

    def expire(self, min_epoch, min_live_permille=0):
        """mi_zset_expire: drop every digest whose stamp is below min_epoch, as prune(..., keep=False) drops a list; no list is
        involved -> PruneInfo"""
        info = PruneInfo()
        rc = self._lib.mi_zset_expire(self._h, min_epoch, min_live_permille, C.byref(info))
        if rc:
            self._raise(rc)
        return info

    def usage(self):
        """mi_zset_get_usage: blobs resident and the device bytes allocated for them, live bytes, the table -> ZSetUsage"""
        out = ZSetUsage()
        self._eng._check(self._lib.mi_zset_get_usage(self._h, C.byref(out)))
        return out

    def entries(self):
        """mi_zset_entries: what the set holds, in no stated order -> (digests uint8[n, 32], lengths uint32[n], stored uint32[n])"""
        n = C.c_uint64()
        self._eng._check(self._lib.mi_zset_entries(self._h, None, None, None, 0, C.byref(n)))
        k = n.value
        d, ln, st = np.zeros((max(k, 1), 32), dtype=np.uint8), np.zeros(max(k, 1), dtype=np.uint32), np.zeros(max(k, 1), dtype=np.uint32)
        if k:
            self._eng._check(self._lib.mi_zset_entries(self._h, d.ctypes.data, ln.ctypes.data, st.ctypes.data, k, C.byref(n)))
        return d[:k], ln[:k], st[:k]

    @property
    def info(self):
        out = ZSetInfo()
        self._eng._check(self._lib.mi_zset_get_info(self._h, C.byref(out)))
        return out

    def count_forms(self):
        """mi_zset_count_forms: ZForms of what the set holds now"""
        out = ZForms()
        self._eng._check(self._lib.mi_zset_count_forms(self._h, C.byref(out)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mi_zset_free(self._h)
            self._h = None

    free = close
    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def pack_check(blob, entries, alg=DIGEST_SHA256):
    """mi_pack_check (host logic, no GPU): None if the pack is sound, else the index of the first entry that is not -- off the
    16-byte grid, overlapping, past the end, a non-zero pad byte, a chunk that does not hash to its digest; an unknown alg
    raises."""
    if alg not in (DIGEST_SHA256, DIGEST_BLAKE2S):
        raise MiError(-1, "mi_pack_check: unknown digest algorithm %r" % (alg,))
    b = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob).view(np.uint8)
    e = np.ascontiguousarray(entries, dtype=PACK_ENTRY_DTYPE)
    bad = C.c_uint64()
    rc = load_library().mi_pack_check(b.ctypes.data if b.size else None, b.size, e.ctypes.data if e.size else None, e.size, alg,
                                      C.byref(bad))
    return None if rc == 0 else bad.value


def zpack_check(blob, entries, alg=DIGEST_SHA256):
    """mi_zpack_check (host logic, no GPU): None if the compressed pack is sound, else the index of the first entry that is
    not -- its structure, an LZ4 block the decoder refuses, a non-zero pad byte, bytes that do not hash to the digest; an
    unknown alg raises."""
    if alg not in (DIGEST_SHA256, DIGEST_BLAKE2S):
        raise MiError(-1, "mi_zpack_check: unknown digest algorithm %r" % (alg,))
    b = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob).view(np.uint8)
    e = np.ascontiguousarray(entries, dtype=ZPACK_ENTRY_DTYPE)
    bad = C.c_uint64()
    rc = load_library().mi_zpack_check(b.ctypes.data if b.size else None, b.size, e.ctypes.data if e.size else None, e.size, alg,
                                       C.byref(bad))
    return None if rc == 0 else bad.value


def default_config(**overrides):
    cfg = Config()
    rc = load_library().mi_config_default(C.byref(cfg))
    if rc:
        raise MiError(rc, "mi_config_default")
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


class Engine:
    """One mi_ctx: a device, its streams and the Gear parameters."""

    def __init__(self, **cfg_overrides):
        self._lib = load_library()
        self.cfg = default_config(**cfg_overrides)
        h = C.c_void_p()
        rc = self._lib.mi_ctx_create(C.byref(self.cfg), C.byref(h))
        if rc:
            raise MiError(rc, self._lib.mi_last_error(None).decode())
        self._h = h
        self._children = weakref.WeakSet()     # live batches / indexes: they die before the ctx

    def _check(self, rc):
        if rc:
            raise MiError(rc, self._lib.mi_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            for child in list(self._children):  # the library refuses to destroy a ctx with live children
                child.free()
            rc = self._lib.mi_ctx_destroy(self._h)
            if rc:
                raise MiError(rc, self._lib.mi_last_error(self._h).decode())
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def warm(self):
        """mi_ctx_warm: the reader threads, their pinned slabs and the kernels' code objects NOW instead of inside the first commit"""
        self._check(self._lib.mi_ctx_warm(self._h))

    def device_info(self):
        ncu, mhz, mem = C.c_int32(), C.c_int32(), C.c_uint64()
        name = C.create_string_buffer(256)
        self._check(self._lib.mi_device_info(self._h, C.byref(ncu), C.byref(mhz), C.byref(mem),
                                             name, 256))
        return {"n_cu": ncu.value, "clock_mhz": mhz.value, "hbm_bytes": mem.value,
                "name": name.value.decode()}

    def sha_valu_roof(self, waves_per_simd=0, blocks=0):
        """The SHA-256 VALU roof of this device right now, in bytes hashed per second (mi_sha_valu_roof)."""
        v = C.c_double()
        self._check(self._lib.mi_sha_valu_roof(self._h, waves_per_simd, blocks, C.byref(v)))
        return v.value

    def blake2s_valu_roof(self, waves_per_simd=0, blocks=0):
        """The BLAKE2s-256 VALU roof of this device right now, in bytes hashed per second (mi_blake2s_valu_roof)."""
        v = C.c_double()
        self._check(self._lib.mi_blake2s_valu_roof(self._h, waves_per_simd, blocks, C.byref(v)))
        return v.value

    @property
    def chunk_digest(self):
        """DIGEST_SHA256, or DIGEST_BLAKE2S for an engine made with FLAG_CHUNK_BLAKE2S (mi_ctx_chunk_digest)."""
        v = C.c_uint32()
        self._check(self._lib.mi_ctx_chunk_digest(self._h, C.byref(v)))
        return v.value

    def debug_sha_wave_stats(self, path):
        """mi_debug_sha_wave_stats: per-wave records of every chunk pass of THIS ctx go to `path` (None: off)."""
        self._check(self._lib.mi_debug_sha_wave_stats(self._h, os.fsencode(path) if path else None))

    def stats(self):
        st = Stats()
        self._check(self._lib.mi_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def batch(self, n_files_hint=0, bytes_hint=0):
        return Batch(self, n_files_hint, bytes_hint)

    def sha256_many(self, blobs):
        """Batched image.Digester.FromBytes: list of bytes-like -> list of 32-byte digests."""
        lens = np.array([len(b) for b in blobs], dtype=np.uint64)
        offs = np.zeros(len(blobs), dtype=np.uint64)
        if len(blobs):
            offs[1:] = np.cumsum(lens)[:-1]
        data = np.frombuffer(b"".join(bytes(b) for b in blobs), dtype=np.uint8)
        out = np.zeros((len(blobs), 32), dtype=np.uint8)
        u64p = C.POINTER(C.c_uint64)
        self._check(self._lib.mi_sha256_many(self._h, data.ctypes.data if data.size else None,
                                             offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p),
                                             len(blobs), out.ctypes.data))
        return [out[i].tobytes() for i in range(len(blobs))]

    def deflate_buffer(self, data):
        """mi_deflate_buffer: the device deflate leg's coder alone -> (blob, crc32, info dict).  The blob is the pieces' stored
        forms end to end: zlib.decompressobj(-15).decompress(blob + b"\\x03\\x00") gives data back"""
        src = np.frombuffer(bytes(data), dtype=np.uint8)
        cap = self._lib.mi_deflate_bound(src.size)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n, crc, info = C.c_uint64(), C.c_uint32(), DeflateInfo()
        self._check(self._lib.mi_deflate_buffer(self._h, src.ctypes.data if src.size else None, src.size, out.ctypes.data, cap, C.byref(n),
                                                C.byref(crc), C.byref(info)))
        return out[:n.value].tobytes(), crc.value, dict((f, getattr(info, f)) for f, _ in DeflateInfo._fields_)

    def inflate_buffer(self, blob):
        """mi_inflate_buffer: one whole gzip member -> (its inflation, info dict).  info["verdict"] is INFLATE_DONE, or
        INFLATE_NOT_PARALLEL with b"" (the caller inflates serially: info names the segment and the rule); a corrupt member raises
        MiError(-1)"""
        src = np.frombuffer(bytes(blob), dtype=np.uint8)
        n, info = C.c_uint64(), InflateInfo()
        cap = int.from_bytes(src[-4:].tobytes(), "little") if src.size >= 18 else 0       # ISIZE: the size, if the member is sound
        if cap > 1100 * src.size:                       # (deflate expands 1 032 times at the most: this ISIZE is not the size)
            cap = 0
        for _ in range(2):
            out = np.zeros(max(cap, 1), dtype=np.uint8)
            rc = self._lib.mi_inflate_buffer(self._h, src.ctypes.data if src.size else None, src.size, out.ctypes.data, cap, C.byref(n), C.byref(info))
            if rc != -7:                                # MI_ERR_CAPACITY: *out_bytes is the size needed
                break
            cap = n.value
        self._check(rc)
        return out[:n.value].tobytes(), _inflate_info_dict(info)

    def tar_inflate(self, blob_path, tar_path_out=None):
        """mi_tar_inflate_ctx: tar_inflate() through this engine's device -> its dict + info (info["fell_back"] = 1: the blob
        cannot be inflated in parallel and went through the host path)"""
        nb, info = C.c_uint64(), InflateInfo()
        t, g = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
        err = C.create_string_buffer(512)
        rc = self._lib.mi_tar_inflate_ctx(self._h, os.fsencode(blob_path), os.fsencode(tar_path_out) if tar_path_out is not None else None,
                                          C.byref(nb), t, g, C.byref(info), err, len(err))
        if rc:
            raise MiError(rc, "mi_tar_inflate_ctx: %s" % err.value.decode(errors="replace"))
        return {"tar_bytes": nb.value, "tar_digest": Digest.from_raw(t), "blob_digest": Digest.from_raw(g), "info": _inflate_info_dict(info)}

    def inflate_buffer_indexed(self, blob, index):
        """mi_inflate_buffer_indexed: one whole gzip member and its index of checkpoints (inflate_index_build) -> (its inflation, info
        dict).  info["verdict"] is INFLATE_DONE, or INFLATE_NOT_PARALLEL / INFLATE_INDEX_REFUSED with b"": the index is a hint, the
        caller inflates without it (info names the span and the rule, info["index_refusal"] the checker's number)"""
        src = np.frombuffer(bytes(blob), dtype=np.uint8)
        ix = np.frombuffer(bytes(index), dtype=np.uint8)
        keep = ix if ix.size else np.zeros(1, dtype=np.uint8)
        n, info = C.c_uint64(), InflateInfo()
        cap = 0
        for _ in range(2):
            out = np.zeros(max(cap, 1), dtype=np.uint8)
            rc = self._lib.mi_inflate_buffer_indexed(self._h, src.ctypes.data if src.size else None, src.size, keep.ctypes.data, ix.size,
                                                     out.ctypes.data, cap, C.byref(n), C.byref(info))
            if rc != -7:                                # MI_ERR_CAPACITY: *out_bytes is the size needed
                break
            cap = n.value
        self._check(rc)
        return out[:n.value].tobytes(), _indexed_info_dict(info)

    def tar_inflate_indexed(self, blob_path, index, tar_path_out=None):
        """mi_tar_inflate_ctx_indexed: Engine.tar_inflate with the blob's index of checkpoints (info["fell_back"] = 2: the index was
        refused and the blob went through the host path, 1: it is not parallel)"""
        ix = np.frombuffer(bytes(index), dtype=np.uint8)
        keep = ix if ix.size else np.zeros(1, dtype=np.uint8)
        nb, info = C.c_uint64(), InflateInfo()
        t, g = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
        err = C.create_string_buffer(512)
        rc = self._lib.mi_tar_inflate_ctx_indexed(self._h, os.fsencode(blob_path), keep.ctypes.data, ix.size,
                                                  os.fsencode(tar_path_out) if tar_path_out is not None else None, C.byref(nb), t, g, C.byref(info),
                                                  err, len(err))
        if rc:
            raise MiError(rc, "mi_tar_inflate_ctx_indexed: %s" % err.value.decode(errors="replace"))
        return {"tar_bytes": nb.value, "tar_digest": Digest.from_raw(t), "blob_digest": Digest.from_raw(g), "info": _indexed_info_dict(info)}

    def _spec_index(self, p, n):
        """the index a spec call returned (or None), copied and freed"""
        if not p.value:
            return None
        try:
            return C.string_at(p.value, n.value)
        finally:
            self._lib.mi_inflate_index_free(p)

    def inflate_buffer_spec(self, blob, piece_bytes=0, want_index=False):
        """mi_inflate_buffer_spec: one whole gzip member nobody indexed -> (its inflation, info dict, spec dict[, the index]).  The span
        table and the windows are made on the device from the member alone (piece_bytes: 0 = INFLATE_SPEC_PIECE).  info["verdict"] is
        INFLATE_DONE, or INFLATE_NOT_PARALLEL / INFLATE_INDEX_REFUSED with b"" (the caller inflates serially); a member whose live span
        breaks a rule raises MiError(-1).  want_index: a fourth value, the MIGZIX01 index of the spans (None unless DONE) -- it drives
        every indexed call"""
        src = np.frombuffer(bytes(blob), dtype=np.uint8)
        n, info, spec = C.c_uint64(), InflateInfo(), InflateSpecInfo()
        cap = 0
        for _ in range(2):
            out = np.zeros(max(cap, 1), dtype=np.uint8)
            p, nb = C.c_void_p(), C.c_uint64()
            rc = self._lib.mi_inflate_buffer_spec(self._h, src.ctypes.data if src.size else None, src.size, piece_bytes, out.ctypes.data, cap,
                                                  C.byref(n), C.byref(info), C.byref(spec), C.byref(p) if want_index else None,
                                                  C.byref(nb) if want_index else None)
            if rc != -7:                                # MI_ERR_CAPACITY: *out_bytes is the size needed
                break
            cap = n.value
        ix = self._spec_index(p, nb)
        self._check(rc)
        res = (out[:n.value].tobytes(), _indexed_info_dict(info), _spec_info_dict(spec))
        return res + (ix,) if want_index else res

    def tar_inflate_spec(self, blob_path, tar_path_out=None, piece_bytes=0, want_index=False):
        """mi_tar_inflate_ctx_spec: Engine.tar_inflate through speculative spans -- the first pull of a blob that has no index yet
        (info["fell_back"]: 1 not parallel, 2 refused in the write pass: the blob went through the host path).  -> tar_inflate's dict +
        "spec" and, with want_index, "index" (None when the call fell back)"""
        nb, info, spec = C.c_uint64(), InflateInfo(), InflateSpecInfo()
        t, g = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
        err = C.create_string_buffer(512)
        p, n = C.c_void_p(), C.c_uint64()
        rc = self._lib.mi_tar_inflate_ctx_spec(self._h, os.fsencode(blob_path), piece_bytes, os.fsencode(tar_path_out) if tar_path_out is not None else None,
                                               C.byref(nb), t, g, C.byref(info), C.byref(spec), C.byref(p) if want_index else None,
                                               C.byref(n) if want_index else None, err, len(err))
        ix = self._spec_index(p, n)
        if rc:
            raise MiError(rc, "mi_tar_inflate_ctx_spec: %s" % err.value.decode(errors="replace"))
        res = {"tar_bytes": nb.value, "tar_digest": Digest.from_raw(t), "blob_digest": Digest.from_raw(g), "info": _indexed_info_dict(info),
               "spec": _spec_info_dict(spec)}
        if want_index:
            res["index"] = ix
        return res

    def index(self, capacity_hint=0):
        """A chunk-digest set that outlives batches (dedup across layers)."""
        return ChunkIndex(self, capacity_hint)

    def packset(self, entries_hint=0):
        """mi_packset_create: packs on this device, addressed by digest (the source of Batch.add_recipes)"""
        return PackSet(self, entries_hint)

    def zset(self, entries_hint=0):
        """mi_zset_create: compressed packs on this device as stored, addressed by digest (the source of ZSet.zpack and of
        Batch.add_zrecipes)"""
        return ZSet(self, entries_hint)

    # ---- native RCCL exchange (what a Go host would use; bench.py drives torch instead) ----
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        rc = load_library().mi_comm_unique_id(buf)
        if rc:
            raise MiError(rc, load_library().mi_last_error(None).decode())
        return buf.raw

    def comm_init_rank(self, nranks, rank, uid):
        self._check(self._lib.mi_comm_init_rank(self._h, nranks, rank, uid))

    def comm_destroy(self):
        self._check(self._lib.mi_comm_destroy(self._h))

    def comm_ranks(self):
        """Ranks of this ctx's communicator as the collective library counts them (0: none)."""
        n = C.c_int()
        self._check(self._lib.mi_comm_ranks(self._h, C.byref(n)))
        return n.value

    def comm_exchange_ms(self):
        """(ms_gather, ms_marking) of this ctx's last exchange, device time from HIP events."""
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.mi_comm_exchange_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def dedup_mark_range(self, d_digests_ptr, n_total, own_first, own_n, d_dup_of_own_ptr):
        """dup_of (global indices) for the rows [own_first, own_first+own_n) of a job-wide,
        rank-major digest set; returns how many of them are job-wide first occurrences."""
        nf = C.c_uint64()
        self._check(self._lib.mi_dedup_mark_range(self._h, d_digests_ptr, n_total, own_first, own_n,
                                                  d_dup_of_own_ptr, C.byref(nf)))
        return nf.value

    def dedup_mark(self, d_digests_ptr, n, d_dup_of_ptr):
        """dup_of over a device-resident digest set (e.g. the all-gathered one)."""
        nu = C.c_uint64()
        self._check(self._lib.mi_dedup_mark(self._h, d_digests_ptr, n, d_dup_of_ptr, C.byref(nu)))
        return nu.value


def comm_init_all(engines):
    """mi_comm_init_all: one communicator over the ctxs of ONE process (rank i = engines[i])."""
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    rc = load_library().mi_comm_init_all(arr, len(engines))
    if rc:
        raise MiError(rc, engines[0]._lib.mi_last_error(engines[0]._h).decode())


def dedup_allgather_all(batches, form="allgather"):
    """mi_dedup_allgather_all (form="alltoall": mi_dedup_alltoall_all, the hash-partitioned form -- same results): the
    exchange + job-wide marking for the batches of comm_init_all's ctxs, rank order.  Returns (n_total, n_unique)."""
    arr = (C.c_void_p * len(batches))(*[b._h for b in batches])
    a, b_ = C.c_uint64(), C.c_uint64()
    fn = {"allgather": "mi_dedup_allgather_all", "alltoall": "mi_dedup_alltoall_all"}[form]
    rc = getattr(load_library(), fn)(arr, len(batches), C.byref(a), C.byref(b_))
    if rc:
        e = batches[0].engine
        raise MiError(rc, "; ".join(x.engine._lib.mi_last_error(x.engine._h).decode() for x in batches) or str(e))
    return a.value, b_.value


class Batch:
    def __init__(self, engine, n_files_hint=0, bytes_hint=0):
        self.engine = engine
        self._lib = engine._lib
        h = C.c_void_p()
        engine._check(self._lib.mi_batch_begin(engine._h, n_files_hint, bytes_hint, C.byref(h)))
        self._h = h
        engine._children.add(self)

    def _check(self, rc):
        self.engine._check(rc)

    def add_bytes(self, data, tag=0):
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else \
            np.ascontiguousarray(data).view(np.uint8)
        self._check(self._lib.mi_batch_add_bytes(self._h, a.ctypes.data if a.size else None,
                                                 a.size, tag))

    def reserve(self, more_files, more_bytes):
        """mi_batch_reserve: room for what is known to come, so that the arena does not grow under way."""
        self._check(self._lib.mi_batch_reserve(self._h, more_files, more_bytes))

    def add_path(self, path, size=None, tag=0):
        if size is None:
            size = os.stat(path).st_size
        self._check(self._lib.mi_batch_add_path(self._h, os.fsencode(path), size, tag))

    def add_paths(self, paths, sizes=None, tags=None):
        """Many files at once, opened by the reader threads (deferred: a missing file fails run())."""
        n = len(paths)
        if sizes is None:
            sizes = [os.stat(p).st_size for p in paths]
        arr = (C.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        sz = np.ascontiguousarray(sizes, dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        tg = np.ascontiguousarray(tags, dtype=np.uint64).ctypes.data_as(u64p) if tags is not None else None
        self._check(self._lib.mi_batch_add_paths(self._h, n, arr, sz.ctypes.data_as(u64p), tg))

    def add_path_range(self, path, offset, size, tag=0):
        """A file that is bytes [offset, offset+size) of `path` (a member of a layer tar)."""
        self._check(self._lib.mi_batch_add_path_range(self._h, os.fsencode(path), offset, size, tag))

    def add_tar(self, path):
        """Registers every regular file of an uncompressed layer tar straight from its byte range
        in the archive (no extraction).  Returns the archive's entries (tar_entries) with
        "file_index" rewritten to the files' indices in THIS batch."""
        ents = tar_entries(path)
        base = self.counts()[0]
        for e in ents:
            if e["kind"] == KIND_FILE:
                self.add_path_range(path, e["data_offset"], e["size"], tag=e["file_index"])
                e["file_index"] += base
        return ents

    def add_synthetic(self, sizes, content_ids=None, seed=0x4D414B49):
        s = np.ascontiguousarray(sizes, dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        cp = None
        if content_ids is not None:
            cids = np.ascontiguousarray(content_ids, dtype=np.uint64)
            assert cids.size == s.size
            cp = cids.ctypes.data_as(u64p)
        self._check(self._lib.mi_batch_add_synthetic(self._h, s.size, s.ctypes.data_as(u64p), cp,
                                                     seed))

    # ---- parts: one file split across batches / GPUs ------------------------------------
    def add_path_part(self, path, begin, end, file_size=None, tag=0):
        if file_size is None:
            file_size = os.stat(path).st_size
        self._check(self._lib.mi_batch_add_path_part(self._h, os.fsencode(path), file_size, begin, end, tag))

    def add_synthetic_part(self, file_size, content_id, begin, end, seed=0x4D414B49):
        self._check(self._lib.mi_batch_add_synthetic_part(self._h, file_size, content_id, seed, begin, end))

    def scan_cuts(self):
        """Blocking: stage + Gear marking + cut selection only (the parts' exits become known)."""
        self._check(self._lib.mi_batch_scan_cuts(self._h))
        return self

    def parts(self):
        n = C.c_uint64()
        self._check(self._lib.mi_batch_parts(self._h, None, 0, C.byref(n)))
        arr = (PartState * max(n.value, 1))()
        self._check(self._lib.mi_batch_parts(self._h, arr, n.value, None))
        return [{k: getattr(arr[i], k) for k, _ in PartState._fields_} for i in range(n.value)]

    def set_part_entry(self, file_index, entry):
        self._check(self._lib.mi_batch_set_part_entry(self._h, file_index, entry))

    def fix_cuts(self):
        self._check(self._lib.mi_batch_fix_cuts(self._h))
        return self

    def run(self):
        self._check(self._lib.mi_batch_run(self._h))
        return self

    def rerun(self):
        self._check(self._lib.mi_batch_rerun(self._h))
        return self

    def submit(self):
        """Enqueue the pipeline on the batch's own stream and return (no host sync)."""
        self._check(self._lib.mi_batch_submit(self._h))
        return self

    def wait(self):
        self._check(self._lib.mi_batch_wait(self._h))
        return self

    def counts(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.mi_batch_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def files(self):
        n = self.counts()[0]
        out = np.zeros(max(n, 1), dtype=FILE_DTYPE)
        self._check(self._lib.mi_batch_files(self._h, out.ctypes.data, n))
        return out[:n]

    def chunks(self):
        n = self.counts()[1]
        out = np.zeros(max(n, 1), dtype=CHUNK_DTYPE)
        self._check(self._lib.mi_batch_chunks(self._h, out.ctypes.data, n))
        return out[:n]

    def files_view(self):
        """The file rows WITHOUT a copy (same lifetime as chunks_view's)."""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.mi_batch_files_view(self._h, C.byref(p), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=FILE_DTYPE)
        buf = (C.c_char * (n.value * FILE_DTYPE.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=FILE_DTYPE)

    def roots(self):
        """the per-file chunk roots alone: an (n_files, 32) uint8 array"""
        n = self.counts()[0]
        out = np.zeros((max(n, 1), 32), dtype=np.uint8)
        self._check(self._lib.mi_batch_roots(self._h, out.ctypes.data, n))
        return out[:n]

    def read_file(self, file_index, offset=0, length=None):
        """bytes [offset, offset + length) of a staged file as they lie in HBM"""
        if length is None:
            raise ValueError("length")
        out = np.zeros(max(length, 1), dtype=np.uint8)
        self._check(self._lib.mi_batch_read_file(self._h, file_index, offset, out.ctypes.data, length))
        return out[:length].tobytes()

    def chunks_view(self):
        """The chunk rows WITHOUT a copy: a numpy array over the batch's own pinned buffer, valid
        until the batch is submitted again, marked globally, reset or freed."""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.mi_batch_chunks_view(self._h, C.byref(p), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=CHUNK_DTYPE)
        buf = (C.c_char * (n.value * CHUNK_DTYPE.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=CHUNK_DTYPE)

    def device_digests(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.mi_batch_device_digests(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def pack(self, select=None, verify=False):
        """mi_batch_pack_chunks: the rows with a non-zero flag in `select` (one per chunk row; None = every row) gathered
        into one blob on the device -> Pack"""
        h = C.c_void_p()
        ptr, n = None, 0
        if select is not None:
            sel = np.zeros(max(len(select), 1), dtype=np.uint8)      # (never NULL: NULL means every row)
            sel[:len(select)] = np.asarray(select) != 0
            ptr, n = sel.ctypes.data, len(select)
        self._check(self._lib.mi_batch_pack_chunks(self._h, ptr, n, PACK_VERIFY if verify else 0, C.byref(h)))
        return Pack(self.engine, h)

    def zpack(self, select=None, verify=False):
        """mi_batch_zpack_chunks: pack(select).compress() without the plain pack -- the selected rows coded where they lie in
        the arena, byte for byte the same ZPack; verify: decoded again and held against the batch's own digests"""
        return self.zpack_at(1, select, verify)

    def zpack_at(self, level, select=None, verify=False):
        """zpack() at a level: 2 is MI_ZPACK_LEVEL2, byte for byte pack(select).compress(level=2)"""
        h = C.c_void_p()
        ptr, n = None, 0
        if select is not None:
            sel = np.zeros(max(len(select), 1), dtype=np.uint8)      # (never NULL: NULL means every row)
            sel[:len(select)] = np.asarray(select) != 0
            ptr, n = sel.ctypes.data, len(select)
        self._check(self._lib.mi_batch_zpack_chunks(self._h, ptr, n, (ZPACK_VERIFY if verify else 0) | _zpack_level_flag(level), C.byref(h)))
        return ZPack(self.engine, h)

    def add_layer_blob(self, blob, tag_base=0):
        """mi_batch_add_layer_blob: a layer blob (gzip or plain tar) in host memory goes up once, is inflated on the device into this
        batch's arena where that is possible, and its regular members become the batch's files where they lie (batch index
        info["first_file"] + the entry's "file_index", tag tag_base + "file_index").  -> (entries as tar_entries gives them, their
        data offsets in the tar, info dict, the blob's SHA-256 as 32 bytes).  A failure raises MiError and leaves the batch as it was"""
        src = np.frombuffer(bytes(blob), dtype=np.uint8)
        keep = src if src.size else np.zeros(1, dtype=np.uint8)      # (never NULL: an empty blob is an empty archive)
        return self._add_layer(lambda h, sha, info: self._lib.mi_batch_add_layer_blob(self._h, keep.ctypes.data, src.size, tag_base, C.byref(h), sha,
                                                                                       C.byref(info)))

    def add_layer_path(self, path, tag_base=0):
        """mi_batch_add_layer_path: add_layer_blob for a blob file, mapped by the library"""
        return self._add_layer(lambda h, sha, info: self._lib.mi_batch_add_layer_path(self._h, os.fsencode(path), tag_base, C.byref(h), sha, C.byref(info)))

    def add_layer_blob_indexed(self, blob, index, tag_base=0):
        """mi_batch_add_layer_blob_indexed: add_layer_blob with the blob's index of checkpoints -- info["source"] is
        LAYER_SOURCE_INDEXED_GZIP when the spans were decoded straight into the arena; a refused index leaves the batch as it was and the
        call goes on as add_layer_blob does, with info["inflate"]["fell_back"] = 2"""
        src = np.frombuffer(bytes(blob), dtype=np.uint8)
        keep = src if src.size else np.zeros(1, dtype=np.uint8)
        ix = np.frombuffer(bytes(index), dtype=np.uint8)
        keep_ix = ix if ix.size else np.zeros(1, dtype=np.uint8)
        return self._add_layer(lambda h, sha, info: self._lib.mi_batch_add_layer_blob_indexed(self._h, keep.ctypes.data, src.size, keep_ix.ctypes.data,
                                                                                               ix.size, tag_base, C.byref(h), sha, C.byref(info)))

    def add_layer_path_indexed(self, path, index, tag_base=0):
        """mi_batch_add_layer_path_indexed: add_layer_blob_indexed for a blob file, mapped by the library"""
        ix = np.frombuffer(bytes(index), dtype=np.uint8)
        keep_ix = ix if ix.size else np.zeros(1, dtype=np.uint8)
        return self._add_layer(lambda h, sha, info: self._lib.mi_batch_add_layer_path_indexed(self._h, os.fsencode(path), keep_ix.ctypes.data, ix.size,
                                                                                               tag_base, C.byref(h), sha, C.byref(info)))

    def add_layer_blob_spec(self, blob, tag_base=0, piece_bytes=0):
        """mi_batch_add_layer_blob_spec: add_layer_blob for a gzip nobody indexed -- the speculative plan takes the index's place:
        info["source"] is LAYER_SOURCE_SPEC_GZIP when its spans were decoded straight into the arena (info["spec"]: the plan's figures);
        not parallel or refused, the batch is as it was and the call goes on as add_layer_blob does"""
        src = np.frombuffer(bytes(blob), dtype=np.uint8)
        keep = src if src.size else np.zeros(1, dtype=np.uint8)
        spec = InflateSpecInfo()
        res = self._add_layer(lambda h, sha, info: self._lib.mi_batch_add_layer_blob_spec(self._h, keep.ctypes.data, src.size, piece_bytes, tag_base,
                                                                                          C.byref(h), sha, C.byref(info), C.byref(spec)))
        res[2]["spec"] = _spec_info_dict(spec)
        return res

    def add_layer_path_spec(self, path, tag_base=0, piece_bytes=0):
        """mi_batch_add_layer_path_spec: add_layer_blob_spec for a blob file, mapped by the library"""
        spec = InflateSpecInfo()
        res = self._add_layer(lambda h, sha, info: self._lib.mi_batch_add_layer_path_spec(self._h, os.fsencode(path), piece_bytes, tag_base, C.byref(h),
                                                                                          sha, C.byref(info), C.byref(spec)))
        res[2]["spec"] = _spec_info_dict(spec)
        return res

    def _add_layer(self, call):
        h, sha, info = C.c_void_p(), (C.c_uint8 * 32)(), LayerBlobInfo()
        self._check(call(h, sha, info))
        entries = _tar_handle_entries(self._lib, h, info.n_entries)
        d = dict((f, getattr(info, f)) for f, _ in LayerBlobInfo._fields_ if f not in ("reserved", "inflate"))
        d["inflate"] = _inflate_info_dict(info.inflate)
        return entries, [e["data_offset"] for e in entries], d, bytes(sha)

    def add_recipes(self, packset, recipes, tags=None, verify=False):
        """mi_batch_add_recipes: one file per recipe, assembled on the device from the pack set.  recipes: a list of (digests:
        (n, 32) uint8, lengths: n uint32) pairs, or of lists of (digest bytes, length) rows as a MEMFS_CHUNK_PACK commit's layer
        gives them under "chunks".  -> RecipeStats"""
        return self._add_recipes(self._lib.mi_batch_add_recipes, packset, recipes, tags, verify)

    def add_zrecipes(self, zset, recipes, tags=None, verify=False):
        """mi_batch_add_zrecipes: add_recipes from a compressed set (Engine.zset): every row decoded by one wave straight to its
        place in the arena, no plain blob in between.  -> RecipeStats"""
        return self._add_recipes(self._lib.mi_batch_add_zrecipes, zset, recipes, tags, verify)

    def _add_recipes(self, call, packset, recipes, tags, verify):
        dig, lens, counts = [], [], []
        for rec in recipes:
            if isinstance(rec, tuple) and len(rec) == 2 and not isinstance(rec[0], (bytes, bytearray)):
                d = np.ascontiguousarray(rec[0], dtype=np.uint8).reshape(-1, 32)
                n = np.ascontiguousarray(rec[1], dtype=np.uint32).reshape(-1)
            else:
                d = np.frombuffer(b"".join(bytes(x[0]) for x in rec), dtype=np.uint8).reshape(-1, 32)
                n = np.array([int(x[1]) for x in rec], dtype=np.uint32)
            if len(d) != len(n):
                raise ValueError("a recipe of %d digests and %d lengths" % (len(d), len(n)))
            dig.append(d)
            lens.append(n)
            counts.append(len(n))
        d = np.ascontiguousarray(np.concatenate(dig)) if dig else np.zeros((0, 32), np.uint8)
        n = np.ascontiguousarray(np.concatenate(lens)) if lens else np.zeros(0, np.uint32)
        cnt = np.array(counts, dtype=np.uint64)
        tg = np.ascontiguousarray(tags, dtype=np.uint64) if tags is not None else None
        if tg is not None and tg.size != cnt.size:
            raise ValueError("%d tags for %d recipes" % (tg.size, cnt.size))
        out = RecipeStats()
        self._check(call(self._h, packset._h, cnt.size, cnt.ctypes.data if cnt.size else None, d.ctypes.data if d.size else None,
                         n.ctypes.data if n.size else None, tg.ctypes.data if tg is not None and tg.size else None,
                         RECIPE_VERIFY if verify else 0, C.byref(out)))
        return out

    def add_tree(self, root, rel_base=None, blacklist=(), mode=TREE_CONTEXT):
        """Walk `root` the way the reference does (filepath.Walk order) and add its regular
        files; returns the number of recorded entries so far."""
        bl = (C.c_char_p * max(len(blacklist), 1))(*[os.fsencode(x) for x in blacklist])
        n = C.c_uint64()
        self._check(self._lib.mi_batch_add_tree(self._h, os.fsencode(root),
                                                os.fsencode(rel_base) if rel_base else None,
                                                bl, len(blacklist), mode, C.byref(n)))
        return n.value

    def tree_entries(self, n):
        arr = (TreeEntry * max(n, 1))()
        self._check(self._lib.mi_batch_tree_entries(self._h, arr, n))
        return [(os.fsdecode(e.relpath), os.fsdecode(e.link_target) if e.link_target else None,
                 e.file_index, e.size, e.kind, e.mode) for e in arr[:n]]

    def context_checksum_tree(self, prefix):
        pre = bytes(prefix)
        out = C.c_uint32()
        self._check(self._lib.mi_context_checksum_tree(self._h, pre, len(pre), C.byref(out)))
        return "%x" % out.value

    def context_checksum(self, prefix, entries):
        """The reference's COPY/ADD running CRC32 (add_copy_step.go:102-238).

        entries: walk-ordered list of (relpath, link_target_or_None, file_index_or_-1);
        returns the cache ID the way SetCacheID prints it ("%x", unpadded)."""
        arr = (CtxEntry * max(len(entries), 1))()
        for i, (rel, link, idx) in enumerate(entries):
            arr[i].relpath = os.fsencode(rel)
            arr[i].link_target = os.fsencode(link) if link is not None else None
            arr[i].file_index = idx
        pre = bytes(prefix)
        out = C.c_uint32()
        self._check(self._lib.mi_context_checksum(self._h, pre, len(pre), arr, len(entries),
                                                  C.byref(out)))
        return "%x" % out.value

    def dedup_allgather(self):
        """Collective: RCCL all-gather of the digest sets + global marking inside the library.
        Returns (n_total, n_unique, first_global)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.mi_dedup_allgather(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def dedup_alltoall(self):
        """Collective: the hash-partitioned form of dedup_allgather (mi_dedup_alltoall) -- every digest travels to ONE
        owner rank and an 8-byte answer comes back.  Same results: (n_total, n_unique, first_global)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.mi_dedup_alltoall(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def mark_global(self, d_digests_all_ptr, n_total, own_first):
        """Job-wide marking of this batch's chunks (rows own_first.. of the gathered set) straight
        into its dup_of column; returns how many of them are job-wide first occurrences."""
        nf = C.c_uint64()
        self._check(self._lib.mi_batch_mark_global(self._h, d_digests_all_ptr, n_total, own_first,
                                                   C.byref(nf)))
        return nf.value

    def device_dup_of(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.mi_batch_device_dup_of(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_global_dedup(self, d_dup_of_global_ptr, first_global):
        self._check(self._lib.mi_batch_set_global_dedup(self._h, d_dup_of_global_ptr, first_global))

    def read_back(self):
        n = self.counts()[2]
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self._lib.mi_batch_read_back(self._h, out.ctypes.data, n))
        return out[:n]

    def stage_stats(self):
        """Staging counters (FLAG_VERIFY_STAGING) + "note": what the first mismatch looked like."""
        st = StageStats()
        self._check(self._lib.mi_batch_stage_stats(self._h, C.byref(st)))
        d = st.as_dict()
        d["note"] = self._lib.mi_batch_stage_note(self._h).decode(errors="replace")
        return d

    def reset(self):
        """Empty the batch, keep its device memory (next layer, same buffers)."""
        self._check(self._lib.mi_batch_reset(self._h))
        return self

    def free(self):
        if getattr(self, "_h", None):
            self._lib.mi_batch_free(self._h)
            self._h = None

    __del__ = free

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()
