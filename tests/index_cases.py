"""The model of the chunk index as its query, prune and retain calls see it (mi_index_query, mi_index_prune, mi_index_retain_zset:
include/makisu_mi.h "the chunk index: asking without adding, forgetting"), in pure Python: a `set` of 32-byte
strings and the table-size rule.  It predicts the held set, the table's slots and every field of mi_index_prune_info except the
times -- peak_extra_bytes from the sizes of what the call allocates -- and crafts the digests whose probe chains an in-place
delete would break.  No engine code is involved."""
import numpy as np

MIN_SLOTS = 1024
INFO_FIELDS = ["n_rows", "n_unknown", "n_before", "n_dropped", "n_after", "slots_before", "slots_after", "rebuilt", "peak_extra_bytes"]


def alloc(n):
    """what an allocation of n bytes takes from the device: n rounded up to 256, plus 256 bytes of slack"""
    return (n + 255) // 256 * 256 + 256


def table_slots(survivors):
    """the table a prune builds: the smallest power of two >= max(1 024, 2 x survivors)"""
    slots = MIN_SLOTS
    while slots < 2 * survivors:
        slots *= 2
    return slots


def tag_of(digest):
    """a slot's tag: the digest's first 8 bytes, little endian; 0 is stored as 1 (0 marks an empty slot)"""
    return int.from_bytes(bytes(digest[:8]), "little") or 1


def home(digest, slots):
    """where a digest's walk begins in a table of `slots` slots"""
    return tag_of(digest) & (slots - 1)


def keys(digests):
    d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    return [bytes(x) for x in d]


def rows(key_list):
    """digests as the calls take them: an (n, 32) uint8 array"""
    return np.frombuffer(b"".join(key_list), dtype=np.uint8).reshape(-1, 32).copy()


def rebuild_bytes(survivors):
    """what a rebuild allocates: the new table's tags and digests, the survivors' records, the insert's row states, row slots
    and counters"""
    slots = table_slots(survivors)
    return alloc(slots * 8) + alloc(slots * 32) + alloc(survivors * 32) + alloc(survivors + 16) + alloc(survivors * 8 + 16) + alloc(64)


class Index:
    """a chunk index as the calls see it"""

    def __init__(self, hint=0):
        self.held = set()
        self.slots = table_slots(hint)

    def add(self, digests):
        """mi_index_import / mi_index_add_batch -> how many were new.  The table doubles until the digests held and ALL the
        request's rows fill at most half of it"""
        ks = keys(digests)
        if not ks:
            return 0
        need = (len(self.held) + len(ks)) * 2
        while self.slots < need:
            self.slots *= 2
        before = len(self.held)
        self.held.update(ks)
        return len(self.held) - before

    def query(self, digests):
        return [1 if k in self.held else 0 for k in keys(digests)]

    def _forget(self, info, victims, first_bytes):
        info["n_dropped"] = len(victims)
        info["peak_extra_bytes"] = first_bytes
        if victims:
            self.held -= victims
            info["peak_extra_bytes"] += rebuild_bytes(len(self.held))
            self.slots = table_slots(len(self.held))
            info["rebuilt"] = 1
        info["n_after"] = len(self.held)
        info["slots_after"] = self.slots
        return info

    def prune(self, digests, keep=True):
        """-> every field of mi_index_prune_info but the times; the index afterwards is what the engine's must be"""
        ks = keys(digests)
        named = set(ks)
        info = dict.fromkeys(INFO_FIELDS, 0)
        info.update(n_rows=len(ks), n_unknown=sum(1 for k in ks if k not in self.held), n_before=len(self.held), slots_before=self.slots)
        victims = {k for k in self.held if (k in named) != keep}
        return self._forget(info, victims, alloc(len(ks) * 32) + alloc(self.slots) + alloc(64))       # the request, the marks, the totals

    def retain(self, other):
        """mi_index_retain_zset: `other` is the set of digests the compressed set holds"""
        info = dict.fromkeys(INFO_FIELDS, 0)
        n = len(self.held)
        info.update(n_before=n, slots_before=self.slots)
        if n == 0:
            info.update(slots_after=self.slots)
            return info
        victims = {k for k in self.held if k not in other}
        # the exported digests, the set's three answers a row, the keep flags, the totals
        return self._forget(info, victims, alloc(n * 32) + 3 * alloc(n * 8) + alloc(n) + alloc(64))


# ---- crafted digests ---------------------------------------------------------------------------------------------------------------
def _random_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _with_first8(d, k, value):
    d[k, :8] = np.frombuffer(int(value).to_bytes(8, "little"), dtype=np.uint8)


def same_first8(k, rng):
    """(a) k distinct digests with equal first 8 bytes: one tag, one chain, told apart by the full compare alone"""
    d = _random_rows(rng, k)
    d[:, :8] = d[0, :8]
    return d


def same_home(k, rng, low16=0x2A7):
    """(b) k digests with DIFFERENT tags that agree in their low 16 bits: the same home slot in every table of 1 024 to 65 536
    slots"""
    d = _random_rows(rng, k)
    for i in range(k):
        _with_first8(d, i, ((0x1D00 + 37 * i) << 16) | low16)
    return d


def last_slot(k, rng):
    """(c) k digests whose home is the LAST slot of every table of up to 65 536 slots: their chain wraps to slot 0"""
    return same_home(k, rng, low16=0xFFFF)


def zero_and_one(rng):
    """(d) a digest whose first 8 bytes are zero and one whose first 8 bytes are 01 00 00 00 00 00 00 00: both stored under tag 1"""
    d = _random_rows(rng, 2)
    _with_first8(d, 0, 0)
    _with_first8(d, 1, 1)
    return d
