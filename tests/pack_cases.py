"""The chunk pack's model, in pure Python: from the chunk rows, the files' bytes and the selection flags it produces the
entries and the blob mi_batch_pack_chunks must produce (include/makisu_mi.h "chunk packs").  No engine code is involved:
the digests are hashlib's, the layout is restated here -- selected rows in ascending row order, every chunk on the sum of
the lengths before it, each rounded up to 16, the pad bytes zero."""
import hashlib

import numpy as np

# mi_pack_entry as the header spells it, restated (the binding's PACK_ENTRY_DTYPE is held against a compiled probe elsewhere)
ENTRY_DTYPE = np.dtype({"names": ["digest", "offset", "chunk_index", "length", "reserved"],
                        "formats": [("u1", 32), "<u8", "<u8", "<u4", "<u4"], "offsets": [0, 32, 40, 48, 52], "itemsize": 56})
SHA256, BLAKE2S = 0, 1
HASHES = {SHA256: hashlib.sha256, BLAKE2S: hashlib.blake2s}


def round16(n):
    return (n + 15) // 16 * 16


def model_pack(rows, files, select=None, alg=SHA256):
    """rows: (file_index, offset, length) per chunk row, in row order; files: the files' bytes by file_index; select: one
    flag per row, or None for every row.  -> (entries as an ENTRY_DTYPE array, blob as bytes)"""
    rows = list(rows)
    if select is None:
        select = [1] * len(rows)
    assert len(select) == len(rows)
    picked = [i for i, s in enumerate(select) if s]
    entries = np.zeros(len(picked), dtype=ENTRY_DTYPE)
    parts, at = [], 0
    for k, i in enumerate(picked):
        f, off, length = (int(x) for x in rows[i])
        piece = bytes(files[f][off:off + length])
        assert len(piece) == length
        entries["digest"][k] = np.frombuffer(HASHES[alg](piece).digest(), dtype=np.uint8)
        entries["offset"][k], entries["chunk_index"][k], entries["length"][k] = at, i, length
        parts.append(piece + b"\0" * (round16(length) - length))
        at += round16(length)
    return entries, b"".join(parts)


def rows_of(chunks):
    """(file_index, offset, length) of an engine's chunk rows (Batch.chunks())"""
    return list(zip(chunks["file_index"].tolist(), chunks["offset"].tolist(), chunks["length"].tolist()))


def same_entries(got, want):
    """field by field (the two dtypes are equal in layout but need not be the same object)"""
    return (len(got) == len(want) and all(np.array_equal(np.asarray(got[f]), np.asarray(want[f]))
                                          for f in ("digest", "offset", "chunk_index", "length", "reserved")))


def random_cut_rows(rng, files, lo=1, hi=700):
    """rows without an engine: every file cut at random lengths in [lo, hi]"""
    rows = []
    for f, data in enumerate(files):
        at = 0
        while at < len(data):
            n = min(int(rng.integers(lo, hi + 1)), len(data) - at)
            rows.append((f, at, n))
            at += n
    return rows
