"""The restore's model, in pure Python: from packs -- entries and blob as pack_cases.model_pack produces them -- and recipes it
yields every file's bytes, as mi_batch_add_recipes must assemble them (include/makisu_mi.h "the consuming side"), and it counts
the 16-byte destination units that more than one row covers.  No engine code is involved: a chunk is blob[offset : offset +
length] of the first entry that carries its digest, a file is its recipe's chunks end to end."""
import numpy as np

import pack_cases as pc

FILE_ALIGN = 256          # files lie on 256-byte boundaries of the arena: a file's offset mod 16 is its arena offset's


def chunk_store(packs):
    """packs: (entries, blob) pairs -> digest bytes -> chunk bytes; a digest met again is kept once (the first wins)"""
    store = {}
    for entries, blob in packs:
        for en in entries:
            at, n = int(en["offset"]), int(en["length"])
            store.setdefault(bytes(en["digest"]), bytes(blob[at:at + n]))
    return store


def recipe_of(rows, files, f, alg=pc.SHA256):
    """the recipe of file f from (file_index, offset, length) rows: (digests as an (n, 32) uint8 array, lengths as uint32)"""
    mine = [(off, n) for fi, off, n in rows if fi == f]
    dig = np.zeros((len(mine), 32), dtype=np.uint8)
    for k, (off, n) in enumerate(mine):
        dig[k] = np.frombuffer(pc.HASHES[alg](bytes(files[f][off:off + n])).digest(), dtype=np.uint8)
    return dig, np.array([n for _, n in mine], dtype=np.uint32)


def model_restore(packs, recipes):
    """-> every recipe's file as bytes.  A digest no pack holds, or one held with another length, raises KeyError / ValueError."""
    store = chunk_store(packs)
    out = []
    for dig, lens in recipes:
        parts = []
        for d, n in zip(np.asarray(dig).reshape(-1, 32), np.asarray(lens).reshape(-1)):
            piece = store[bytes(d)]
            if len(piece) != int(n):
                raise ValueError("digest %s is held with %d bytes, the recipe states %d" % (bytes(d).hex(), len(piece), int(n)))
            parts.append(piece)
        out.append(b"".join(parts))
    return out


def joined_units(recipes):
    """how many aligned 16-byte units of the destination more than one row covers.  Every file begins on a FILE_ALIGN boundary,
    so its units are those of its own offsets and no unit holds bytes of two files."""
    total = 0
    for _, lens in recipes:
        lens = np.asarray(lens, dtype=np.int64).reshape(-1)
        if not len(lens):
            continue
        ends = np.cumsum(lens)
        first_unit, last_unit = (ends - lens) // 16, (ends - 1) // 16
        size_units = int((ends[-1] + 15) // 16)
        cover = np.zeros(size_units + 1, dtype=np.int64)
        np.add.at(cover, first_unit, 1)
        np.add.at(cover, last_unit + 1, -1)
        total += int((np.cumsum(cover)[:size_units] > 1).sum())
    return total


def unit_cover_histogram(lens):
    """rows per unit -> how many units, for one file (the tests state the mix their inputs have)"""
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    ends = np.cumsum(lens)
    cover = np.zeros(int((ends[-1] + 15) // 16) + 1, dtype=np.int64)
    np.add.at(cover, (ends - lens) // 16, 1)
    np.add.at(cover, (ends - 1) // 16 + 1, -1)
    per_unit = np.cumsum(cover)[:-1]
    return {int(k): int((per_unit == k).sum()) for k in np.unique(per_unit)}
