"""NumPy model of an update of the 8-bit index (rihip_sq8_update_apply in recommendit_hip.h), written from that text:
ids, lists, the 64-row granule layout, padding, row ids, tag words and codes.  Codes come from sq8_reference.encode and
the clamp count from the unclamped rint in f32.  The model holds the PHYSICAL arrays and an update moves them the way
the specification says (kept rows keep their order inside their list, new rows go behind them, every list is padded to
a granule with zero rows of row id -1 and tag 0), so "step by step equals from scratch" is a statement about the
model, which tests/test_sq8_update_host.py checks, and the GPU tests compare the handle with either."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_reference as SQ  # noqa: E402

GRANULE = SQ.GRANULE


class Refused(ValueError):
    def __init__(self, kind, bad_id=0):
        super().__init__(f"update refused: kind {kind}, id {bad_id}")
        self.kind, self.bad_id = kind, bad_id


def dpad_of(d):
    return 64 if d <= 64 else 128


def clamp_count(X, m, s):
    """pairs (row, column) whose unclamped rint((x - m) / s), in f32, lies outside +-127"""
    if len(X) == 0:
        return 0
    v = np.rint((np.asarray(X, dtype=SQ.F) - np.asarray(m, dtype=SQ.F)[None, :]) / np.asarray(s, dtype=SQ.F)[None, :])
    assert v.dtype == SQ.F
    return int(((v > 127) | (v < -127)).sum())


def padded_codes(X, m, s, dpad):
    """int8 [n, dpad]: the codes of n rows, columns beyond the width 0"""
    out = np.zeros((len(X), dpad), dtype=np.int8)
    if len(X):
        out[:, :X.shape[1]] = SQ.encode(X, m, s)
    return out


class Sq8Model:
    """the state of a handle: physical arrays plus the insertion-order ids (and f32 rows, for the attached vectors)"""

    def __init__(self, nlist, m, s):
        self.nlist, self.m, self.s = int(nlist), np.asarray(m, dtype=SQ.F), np.asarray(s, dtype=SQ.F)
        self.d, self.dpad = len(self.m), dpad_of(len(self.m))
        self.stats = [0, 0, 0, 0]

    @classmethod
    def from_corpus(cls, X, ids, lists, nlist, m, s, tags=None):
        """from scratch: rows ascend inside a list"""
        self = cls(nlist, m, s)
        X = np.asarray(X, dtype=SQ.F)
        lists = np.zeros(len(X), dtype=np.int64) if lists is None else np.asarray(lists, dtype=np.int64)
        self.ids, self.X = np.asarray(ids, dtype=np.int64).copy(), X.copy()
        self.list_len = np.bincount(lists, minlength=self.nlist).astype(np.int64)
        self.poff = np.concatenate([[0], np.cumsum((self.list_len + GRANULE - 1) // GRANULE * GRANULE)]).astype(np.int64)
        Np = int(self.poff[-1])
        self.row_ids = np.full(Np, -1, dtype=np.int64)
        for c in range(self.nlist):
            rows = np.nonzero(lists == c)[0]
            self.row_ids[self.poff[c]:self.poff[c] + len(rows)] = rows
        real = self.row_ids >= 0
        self.codes = np.zeros((Np, self.dpad), dtype=np.int8)
        self.codes[real] = padded_codes(X[self.row_ids[real]], self.m, self.s, self.dpad)
        self.tags = None
        if tags is not None:
            self.tags = np.zeros(Np, dtype=np.uint32)
            self.tags[real] = np.asarray(tags, dtype=np.uint32)[self.row_ids[real]]
        return self

    # -- what the handle reports ---------------------------------------------------------------------------------
    def lists(self):
        """list of every row, insertion order"""
        out = np.empty(len(self.ids), dtype=np.int64)
        for c in range(self.nlist):
            seg = self.row_ids[self.poff[c]:self.poff[c + 1]]
            out[seg[seg >= 0]] = c
        return out

    def codes_by_row(self):
        out = np.empty((len(self.ids), self.d), dtype=np.int8)
        real = self.row_ids >= 0
        out[self.row_ids[real]] = self.codes[real, :self.d]
        return out

    def tags_by_row(self):
        if self.tags is None:
            return None
        out = np.empty(len(self.ids), dtype=np.uint32)
        real = self.row_ids >= 0
        out[self.row_ids[real]] = self.tags[real]
        return out

    # -- one update ------------------------------------------------------------------------------------------------
    def update(self, drop_ids, X_add, add_ids, add_lists=None, add_tags=None):
        """-> (rows dropped, code values clamped); Refused(kind) leaves the model as it was"""
        drop_ids = np.asarray(drop_ids, dtype=np.int64).reshape(-1)
        add_ids = np.asarray(add_ids, dtype=np.int64).reshape(-1)
        X_add = np.asarray(X_add, dtype=SQ.F).reshape(len(add_ids), self.d)
        if len(drop_ids) == 0 and len(add_ids) == 0:
            return 0, 0
        for arr in (add_ids, drop_ids):          # (the add ids' repeat is reported before the drop ids')
            u, cnt = np.unique(arr, return_counts=True)
            if (cnt > 1).any():
                raise Refused(1, int(u[cnt > 1][0]))
        keep = ~np.isin(self.ids, drop_ids)
        stays = np.isin(self.ids, add_ids) & keep
        if stays.any():
            raise Refused(2, int(self.ids[stays].min()))
        n_keep, n_add = int(keep.sum()), len(add_ids)
        if n_keep + n_add <= 0:
            raise Refused(3)
        n_gone = len(self.ids) - n_keep
        if n_gone == 0 and n_add == 0:
            return 0, 0
        add_lists = np.zeros(n_add, dtype=np.int64) if add_lists is None else np.asarray(add_lists, dtype=np.int64)
        new_row = np.cumsum(keep) - 1                                  # dense renumbering of the survivors
        add_codes = padded_codes(X_add, self.m, self.s, self.dpad)
        kept_phys, len_n = [], np.zeros(self.nlist, dtype=np.int64)
        for c in range(self.nlist):
            p = np.arange(self.poff[c], self.poff[c + 1])
            p = p[self.row_ids[p] >= 0]
            p = p[keep[self.row_ids[p]]]                               # old physical order
            kept_phys.append(p)
            len_n[c] = len(p) + int((add_lists == c).sum())
        poff_n = np.concatenate([[0], np.cumsum((len_n + GRANULE - 1) // GRANULE * GRANULE)]).astype(np.int64)
        Np_n = int(poff_n[-1])
        codes = np.zeros((Np_n, self.dpad), dtype=np.int8)
        row_ids = np.full(Np_n, -1, dtype=np.int64)
        tags = None if self.tags is None else np.zeros(Np_n, dtype=np.uint32)
        for c in range(self.nlist):
            p, j = kept_phys[c], np.nonzero(add_lists == c)[0]          # new rows in call order
            a, b = poff_n[c], poff_n[c] + len(p)
            codes[a:b], row_ids[a:b] = self.codes[p], new_row[self.row_ids[p]]
            codes[b:b + len(j)], row_ids[b:b + len(j)] = add_codes[j], n_keep + j
            if tags is not None:
                tags[a:b] = self.tags[p]
                tags[b:b + len(j)] = 0 if add_tags is None else np.asarray(add_tags, dtype=np.uint32)[j]
        clamped = clamp_count(X_add, self.m, self.s)
        self.codes, self.row_ids, self.tags, self.list_len, self.poff = codes, row_ids, tags, len_n, poff_n
        self.ids = np.concatenate([self.ids[keep], add_ids])
        self.X = np.concatenate([self.X[keep], X_add])
        for i, v in enumerate((1, n_gone, n_add, clamped)):
            self.stats[i] += v
        return n_gone, clamped


def same_state(a, b):
    """every array of two models is equal (tags: both None or equal)"""
    assert (a.tags is None) == (b.tags is None)
    pairs = [(a.codes, b.codes), (a.row_ids, b.row_ids), (a.list_len, b.list_len), (a.poff, b.poff), (a.ids, b.ids), (a.X, b.X)]
    if a.tags is not None:
        pairs.append((a.tags, b.tags))
    for x, y in pairs:
        np.testing.assert_array_equal(x, y)


def refine_ranges(X, codes, m, s):
    """(e, a) f64 [d] as rihip_sq8_refine_attach_vectors states them, over the rows X and their stored codes"""
    x = np.asarray(X, dtype=np.float64)
    dec = np.asarray(m, dtype=np.float64)[None, :] + np.asarray(s, dtype=np.float64)[None, :] * codes.astype(np.float64)
    return np.abs(x - dec).max(axis=0), np.abs(x).max(axis=0)
