"""What mi_batch_zpack_chunks must produce, in pure Python -- and the model holds NO new coder: it is the chunk pack's model
(pack_cases.model_pack: hashlib's digests, the layout restated) handed to the compressed pack's (zpack_cases.model_compress: the
parse restated).  A chunk's stored form is a pure function of its bytes, so coding a batch's rows where they lie must give what
packing them plain and compressing the pack gives.  Also the planted inputs tests/test_gpu_chunk_zbatch.py rests on, so that
tests/test_host_chunk_zbatch.py can state their properties without a GPU."""
import numpy as np

import pack_cases as pc
import zpack_cases as zc

TILE = 16384              # bytes of the zpack's blob one workgroup of the gather writes
PLAN_BLOCK = 2048         # rows per block of the plan's and the layout's scan
ENCODE_GRID = 1 << 15     # the encode launch's workgroups (one wave an entry): more entries take a second trip
PIECE = 4096


def model_zpack(rows, files, select=None, alg=pc.SHA256):
    """rows: (file_index, offset, length) per chunk row; files: the files' bytes by file_index; select: one flag per row or
    None.  -> (entries as a zpack_cases.ZENTRY_DTYPE array, the compressed blob as bytes)"""
    return zc.model_compress(*pc.model_pack(rows, files, select, alg))


def same_zentries(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]), np.asarray(want[f]))
                                         for f in ("digest", "offset", "chunk_index", "length", "stored"))


def mixed_file(seed=41, size=1 << 20):
    """4 KiB of random bytes and 4 KiB of zpack_cases.text_like, alternating: under small chunk sizes raw and coded entries lie
    side by side in the blob, each kind at every start residue"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(size // PIECE):
        out.append(rng.integers(0, 256, PIECE, dtype=np.uint8).tobytes() if k % 2 == 0 else zc.text_like(PIECE, k))
    return b"".join(out)


def kinds(entries):
    """per entry: True = coded (stored < length)"""
    return np.asarray(entries["stored"]) < np.asarray(entries["length"])


def tiles_with_both_kinds(entries):
    """the 16 KiB tiles of the blob into which a raw entry AND a coded one reach"""
    coded = kinds(entries)
    seen = {}
    for k in range(len(entries)):
        lo = int(entries["offset"][k])
        hi = lo + pc.round16(int(entries["stored"][k])) - 1
        for t in range(lo // TILE, hi // TILE + 1):
            seen.setdefault(t, set()).add(bool(coded[k]))
    return sorted(t for t, s in seen.items() if len(s) == 2)


def planted_files(prefix=7):
    """every chunk of zpack_cases.planted_chunks() as a file of its own (files begin on 256-byte boundaries of the arena: a first
    file of 1..15 bytes shifts nothing), and all of them in ONE file behind a prefix of `prefix` bytes: the coder's edges read at
    whatever residue the cuts give them"""
    chunks = [c for _, c, _ in zc.planted_chunks()]
    return chunks + [bytes(range(1, prefix + 1)) + b"".join(chunks)]
