"""NumPy model of a PQ handle under updates with frozen codebooks (rihip_pq_update_apply in recommendit_hip.h), written
from that text.  Nothing is restated here: the layout (ids, lists, 64-row granules, padding, row ids, tag words) and
its movement under an update are tests/sq8_update_reference.py's Sq8Model, the SQ8 code is tests/sq8_reference.py's
encode, the residual against the list codes is tests/pq_residual_reference.py's, and the entry of the smallest distance
is tests/pq_reference.py's assign.  What this file adds is the one rule of the update: a kept row keeps its M bytes, a
new row is encoded as S.encode -> (residual) clamp(c - K_l) -> P.assign against the frozen codebooks, and the clamp
counts and the summed smallest distances of the new rows are reported.

"step by step equals from scratch" is then a statement about the model (tests/test_pq_update_host.py checks it), and
the GPU tests compare the handle with either."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_reference as P  # noqa: E402
import pq_residual_reference as PR  # noqa: E402
import sq8_reference as S  # noqa: E402
import sq8_update_reference as U  # noqa: E402

Refused = U.Refused


class PqModel:
    """layout: an Sq8Model (whose `codes` are the rows' SQ8 codes, kept only as the layout's passenger); bytes: uint8
    [N, M] in insertion order.  book int8 [M, 256, dsub]; K int8 [nlist, dpad] (None: not residual)"""

    def __init__(self, layout, book, K):
        self.layout, self.book, self.K = layout, np.asarray(book, dtype=np.int8), K
        self.M, _, self.dsub = self.book.shape
        assert self.M * self.dsub == layout.dpad
        self.stats = [0, 0, 0, 0, 0, 0]      # updates, dropped, added, clamped, residual_clamped, distortion_added
        self.last = (0, 0)                   # residual_clamped, distortion of the last update that changed the model

    # -- the one encoding rule -------------------------------------------------------------------------------------
    def encode(self, X, lists, assign=P.assign):
        """-> (bytes uint8 [n, M], SQ8-grid clamps, residual clamps, summed smallest D) of rows X in the lists given"""
        L = self.layout
        X = np.asarray(X, dtype=S.F).reshape(-1, L.d)
        if len(X) == 0:
            return np.zeros((0, self.M), dtype=np.uint8), 0, 0, 0
        c = U.padded_codes(X, L.m, L.s, L.dpad)                       # S.encode, padding columns 0
        rcl = 0
        if self.K is not None:
            c, rcl = PR.residuals(c, self.K, np.asarray(lists, dtype=np.int64))
        codes, dist = assign(c, self.book)
        return codes, U.clamp_count(X, L.m, L.s), rcl, int(dist)

    @classmethod
    def from_corpus(cls, X, ids, lists, nlist, m, s, book, C=None, tags=None, assign=P.assign):
        """from scratch under injected codebooks; C f32 [nlist, d]: the centroids of a residual handle (None: plain).
        assign: P.assign, or P.assign_blas (the same integers through float64 matmuls) for a whole corpus"""
        layout = U.Sq8Model.from_corpus(X, ids, lists, nlist, m, s, tags)
        K = None if C is None else PR.list_codes(C, layout.m, layout.s, layout.dpad)
        self = cls(layout, book, K)
        self.bytes, _, self.build_residual_clamped, self.build_distortion = self.encode(layout.X, layout.lists(), assign)
        return self

    # -- what the handle reports -----------------------------------------------------------------------------------
    @property
    def ids(self):
        return self.layout.ids

    @property
    def X(self):
        return self.layout.X

    def lists(self):
        return self.layout.lists()

    def tags_by_row(self):
        return self.layout.tags_by_row()

    def pq_codes(self):
        """uint8 [N, M] in insertion order (PQIndex.pq_codes())"""
        return self.bytes

    def pq_physical(self):
        """uint8 [Np, M]: the stored matrix, padding rows 0"""
        out = np.zeros((len(self.layout.row_ids), self.M), dtype=np.uint8)
        real = self.layout.row_ids >= 0
        out[real] = self.bytes[self.layout.row_ids[real]]
        return out

    def decoded(self):
        """the decoded codes in insertion order, all dpad columns: int8, or int16 K_l + entry on a residual model"""
        if self.K is None:
            return P.decode(self.bytes, self.book)
        return PR.decode(self.bytes, self.book, self.K, self.lists())

    # -- one update ------------------------------------------------------------------------------------------------
    def update(self, drop_ids, X_add, add_ids, add_lists=None, add_tags=None):
        """-> dict(dropped, clamped, residual_clamped, distortion); Refused(kind) leaves the model as it was"""
        L = self.layout
        add_ids = np.asarray(add_ids, dtype=np.int64).reshape(-1)
        X_add = np.asarray(X_add, dtype=S.F).reshape(len(add_ids), L.d)
        add_lists = np.zeros(len(add_ids), dtype=np.int64) if add_lists is None else np.asarray(add_lists, dtype=np.int64)
        keep = ~np.isin(L.ids, np.asarray(drop_ids, dtype=np.int64).reshape(-1))
        updates_before = L.stats[0]
        n_gone, clamped = L.update(drop_ids, X_add, add_ids, add_lists, add_tags)      # (raises Refused before any change)
        if L.stats[0] == updates_before:                                               # nothing to do: nothing changes
            return dict(dropped=0, clamped=0, residual_clamped=0, distortion=0)
        new, clamped2, rcl, dist = self.encode(X_add, add_lists)
        assert clamped2 == clamped
        self.bytes = np.concatenate([self.bytes[keep], new])                           # a kept row keeps its bytes
        for i, v in enumerate((1, n_gone, len(add_ids), clamped, rcl, dist)):
            self.stats[i] += v
        self.last = (rcl, dist)
        return dict(dropped=n_gone, clamped=clamped, residual_clamped=rcl, distortion=dist)


def same_state(a, b):
    """every array of two models is equal"""
    U.same_state(a.layout, b.layout)
    np.testing.assert_array_equal(a.bytes, b.bytes)
    np.testing.assert_array_equal(a.pq_physical(), b.pq_physical())
    np.testing.assert_array_equal(a.book, b.book)
    assert (a.K is None) == (b.K is None)
    if a.K is not None:
        np.testing.assert_array_equal(a.K, b.K)
    np.testing.assert_array_equal(a.decoded(), b.decoded())
