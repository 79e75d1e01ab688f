"""The model of a compressed pack set that ages (mi_zset_set_epoch, _touch, _stamps, _age_census, _expire, include/makisu_mi.h
"ageing a compressed set"), in pure Python over zprune_cases.py and zrecode_cases.py: Store with an epoch, an
ageing flag and a stamp per held digest.  It predicts every stamp, mi_touch_info, the census bins and every counter of
mi_prune_info for an expiry.  THE FORMULAS of peak_extra_bytes are stated here once:
  expire   zprune_cases.Store.prune's with n = 0 rows, plus alloc(4 * new_cap) -- the new stamp array -- when a table is rebuilt;
  prune, recode on an ageing set   their own, plus the same addend when a table is rebuilt; without ageing, their own.
No engine code is involved."""
import numpy as np

import zpack_cases as zc
import zprune_cases as pr
import zrecode_cases as rc

NONE = 0xFFFFFFFF                                      # no stamp: the digest is not held; as an epoch: reserved
alloc = pr.alloc


class Store(rc.Store):
    """zrecode_cases.Store (zprune_cases.Store with a recode) with a clock and a stamp per held digest"""

    def __init__(self, hint=0):
        super().__init__(hint)
        self.ageing, self.epoch, self.stamp = False, 0, {}

    # ---- the clock ----------------------------------------------------------------------------------------------------------
    def set_epoch(self, epoch):
        """-> None; raises ValueError where the call is MI_ERR_INVALID"""
        if epoch == NONE or (self.ageing and epoch < self.epoch):
            raise ValueError(epoch)
        if not self.ageing:
            self.ageing = True
            self.stamp = dict.fromkeys(self.held, epoch)
        self.epoch = epoch

    def stamp_bytes(self):
        return alloc(4 * self.slots) if self.ageing else 0

    # ---- uses ---------------------------------------------------------------------------------------------------------------
    def add(self, zentries, zblob):
        super().add(zentries, zblob)
        if self.ageing:                                # new or held already: a re-add is a use
            for en in zentries:
                self.stamp[bytes(en["digest"])] = self.epoch

    def touch(self, digests):
        """-> n_rows, n_unknown (per row), n_refreshed (DISTINCT digests whose stamp was older than the epoch)"""
        assert self.ageing
        keys = pr._keys(digests)
        unknown = sum(1 for k in keys if k not in self.held)
        refreshed = 0
        for k in set(keys):
            if k in self.held:
                refreshed += 1 if self.stamp[k] != self.epoch else 0
                self.stamp[k] = self.epoch
        return {"n_rows": len(keys), "n_unknown": unknown, "n_refreshed": refreshed}

    def stamps(self, digests):
        assert self.ageing
        return [self.stamp.get(k, NONE) for k in pr._keys(digests)]

    def census(self, bounds):
        """bin i: bounds[i-1] <= stamp < bounds[i]; bin 0 begins at 0, the last is open above -> [dict] * (len(bounds) + 1)"""
        assert self.ageing and 1 <= len(bounds) <= 255 and all(a < b for a, b in zip(bounds, bounds[1:]))
        bins = [dict.fromkeys(["n_digests", "stored_bytes", "live_bytes", "chunk_bytes"], 0) for _ in range(len(bounds) + 1)]
        for k, (length, span, stored, _) in self.held.items():
            b = bins[sum(1 for x in bounds if x <= self.stamp[k])]
            b["n_digests"] += 1
            b["stored_bytes"] += stored
            b["live_bytes"] += zc.round16(stored)
            b["chunk_bytes"] += length
        return bins

    # ---- the rebuilds: the stamps follow the survivors, and the new stamp array is counted ------------------------------------
    def prune(self, digests, keep=True, permille=0):
        info = super().prune(digests, keep=keep, permille=permille)
        if self.ageing and info["n_dropped"]:          # a prune that drops rebuilds the table: self.slots is the new one's
            info["peak_extra_bytes"] += alloc(4 * self.slots)
        self.stamp = {k: v for k, v in self.stamp.items() if k in self.held}
        return info

    def recode(self, level, verify=False, scratch_bytes=0):
        info = super().recode(level, verify=verify, scratch_bytes=scratch_bytes)
        if self.ageing and info["n_recoded"]:          # a recode that replaces rebuilds the table
            info["peak_extra_bytes"] += alloc(4 * self.slots)
        return info

    def victims(self, min_epoch):
        return [k for k in self.held if self.stamp[k] < min_epoch]

    def expire(self, min_epoch, permille=0):
        """prune(victims, keep=False, permille) with n_rows = n_unknown = 0 and the request's bytes those of an empty one"""
        assert self.ageing
        if min_epoch > self.epoch or permille > 1000:
            raise ValueError((min_epoch, permille))
        victims = self.victims(min_epoch)
        n = len(victims)
        info = self.prune(np.frombuffer(b"".join(victims), dtype=np.uint8).reshape(-1, 32), keep=False, permille=permille)
        assert info["n_unknown"] == 0 and info["n_dropped"] == n
        info["n_rows"] = 0
        info["peak_extra_bytes"] += alloc(0) - alloc(32 * n)
        return info
