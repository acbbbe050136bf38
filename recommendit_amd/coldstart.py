"""Cold-start users (not in the reference beyond its popularity fallback, src/serving/recommender.py:304-307,
:393-410): rating histories of users who have no trained row in the user tower, and the closed-form fold-in that
turns a history into a query vector and a ranking-feature row on the device (csrc/coldstart.hip; the definition is at
rihip_fold_in_users in include/recommendit_hip.h).

A cold user is a SLOT 0..n-1 of a ``UserHistories``, not a user id.  The histories are a CSR of (item id, rating)
pairs, item ids ascending and unique inside a row: the convention of ``SeenItems``, so ``as_seen()`` serves the same
rows as the slots' exclusion lists.

This module imports on a host without a GPU and builds its CSR there; the device tensors are made on first use.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from .seen import SeenItems

_I32_MAX = 2 ** 31 - 1
WEIGHTINGS = {"uniform": 0, "rating": 1}
ROW_WIDTH = 24      # the user-table row of rihip_rank_features_build


class UserHistories:
    """CSR of (item id, rating) per slot: row ``s`` = the history of cold user ``s``, item ids ascending and unique."""

    def __init__(self, offsets: np.ndarray, items: np.ndarray, ratings: np.ndarray):
        self._offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self._items = np.ascontiguousarray(items, dtype=np.int32)
        self._ratings = np.ascontiguousarray(ratings, dtype=np.int32)
        if self._items.shape != self._ratings.shape or self._offsets.ndim != 1 or self._offsets.shape[0] < 1:
            raise ValueError("UserHistories: offsets [n + 1], items and ratings of one length")
        self.n = int(self._offsets.shape[0] - 1)
        self.counts = np.diff(self._offsets).astype(np.int64)
        if self._offsets[0] != 0 or (self.counts < 0).any() or self._offsets[-1] != self._items.shape[0]:
            raise ValueError("UserHistories: offsets must ascend from 0 to the number of entries")
        self.max_count = int(self.counts.max()) if self.n else 0
        self._dev = None
        self._seen: Optional[SeenItems] = None

    # -- constructors ---------------------------------------------------------------------------
    @classmethod
    def from_pairs(cls, slots, items, ratings, n: Optional[int] = None) -> "UserHistories":
        ps = np.asarray(slots, dtype=np.int64).reshape(-1)
        pi = np.asarray(items, dtype=np.int64).reshape(-1)
        pr = np.asarray(ratings).reshape(-1)
        if pr.dtype.kind not in "iu":
            if pr.dtype.kind != "f" or not np.array_equal(pr, np.round(pr)):
                raise ValueError("UserHistories: ratings must be integers")
        pr = pr.astype(np.int64)
        if not ps.shape == pi.shape == pr.shape:
            raise ValueError(f"UserHistories: {ps.shape[0]} slots, {pi.shape[0]} item ids, {pr.shape[0]} ratings")
        if ps.shape[0] and ps.min() < 0:
            raise ValueError("UserHistories: negative slot")
        if pi.shape[0] and pi.max() > _I32_MAX:
            raise ValueError(f"UserHistories: item id {int(pi.max())} >= 2**31 (the device list holds int32 ids)")
        if pi.shape[0] and pi.min() < -_I32_MAX - 1:
            raise ValueError(f"UserHistories: item id {int(pi.min())} < -2**31")
        need = int(ps.max()) + 1 if ps.shape[0] else 0
        n = need if n is None else int(n)
        if n < need:
            raise ValueError(f"UserHistories: slot {need - 1} with n={n}")
        order = np.lexsort((pi, ps))
        ps, pi, pr = ps[order], pi[order], pr[order]
        same = (ps[1:] == ps[:-1]) & (pi[1:] == pi[:-1])
        if same.any():
            j = int(np.nonzero(same)[0][0])
            raise ValueError(f"UserHistories: item {int(pi[j])} appears twice in the history of slot {int(ps[j])}")
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(ps, minlength=n), out=offsets[1:])
        return cls(offsets, pi, np.clip(pr, -_I32_MAX - 1, _I32_MAX))

    @classmethod
    def from_frame(cls, df, slot_col: str = "slot", item_col: str = "item_id", rating_col: str = "rating",
                   n: Optional[int] = None) -> "UserHistories":
        return cls.from_pairs(df[slot_col].to_numpy(), df[item_col].to_numpy(), df[rating_col].to_numpy(), n)

    @classmethod
    def from_lists(cls, histories: Sequence[Sequence[Tuple[int, int]]]) -> "UserHistories":
        """histories[s] = [(item id, rating), ...] of slot s (any order; an empty list is a user without history)"""
        slots = [s for s, h in enumerate(histories) for _ in h]
        items = [p[0] for h in histories for p in h]
        ratings = [p[1] for h in histories for p in h]
        return cls.from_pairs(slots, items, ratings, len(histories))

    # -- host views -----------------------------------------------------------------------------
    def history_of(self, slot: int) -> Tuple[np.ndarray, np.ndarray]:
        lo, hi = self._offsets[slot], self._offsets[slot + 1]
        return self._items[lo:hi], self._ratings[lo:hi]

    @property
    def host(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(offsets i64 [n + 1], items i32, ratings i32) on the host"""
        return self._offsets, self._items, self._ratings

    def as_seen(self) -> SeenItems:
        """the same rows as a SeenItems: slot s excludes the items of its own history"""
        if self._seen is None:
            self._seen = SeenItems(self._offsets, self._items)
        return self._seen

    # -- device tensors (made on first use) -----------------------------------------------------------
    def device_tensors(self):
        """(offsets i64 [n + 1], items i32, ratings i32) on the device"""
        if self._dev is None:
            import torch
            from . import _lib as L
            dev = L.device()
            pad = np.zeros(1, np.int32)
            self._dev = (torch.from_numpy(self._offsets).to(dev),
                         torch.from_numpy(self._items if self._items.shape[0] else pad).to(dev),
                         torch.from_numpy(self._ratings if self._ratings.shape[0] else pad).to(dev))
        return self._dev


def fold_in_users_launch(hist: UserHistories, V, row_of, mu, min_rating: int = 4, weighting: str = "uniform",
                         beta: float = 1.0, item_table=None, user_meta=None):
    """one launch of rihip_fold_in_users, nothing synchronised -> (q f32 [nq, d], rows f64 [nq, 24], flags i32 [nq],
    err i32 [1]) on the device; err is the kernel's error word (bit 0: an item id < 0, bit 1: a rating outside 1..5)"""
    import torch
    from . import _lib as L
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting={weighting!r}: one of {sorted(WEIGHTINGS)}")
    if int(min_rating) != min_rating or not 1 <= int(min_rating) <= 5:
        raise ValueError(f"min_rating={min_rating!r} outside 1..5")
    if not 0.0 <= float(beta) <= 1.0:
        raise ValueError(f"beta={beta!r} outside [0, 1]")
    dev = L.device()
    if V.dim() != 2 or V.dtype != torch.float32 or not V.is_cuda or V.stride(1) != 1 and V.shape[0] > 1:
        raise ValueError("V must be a device float32 [n_rows, d] tensor with unit column stride")
    n_rows, d = V.shape
    ldv = V.stride(0) if n_rows > 1 else max(V.stride(0), d)
    if not 1 <= d <= 256:
        raise ValueError(f"d={d} outside 1..256")
    if row_of.dtype != torch.int32 or row_of.dim() != 1 or not row_of.is_cuda or not row_of.is_contiguous():
        raise ValueError("row_of must be a contiguous device int32 [n_ids] tensor")
    mu = mu.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(mu.shape) != (d,):
        raise ValueError(f"mu must be [{d}], got {tuple(mu.shape)}")
    nq = hist.n
    if item_table is not None:
        if item_table.dtype != torch.float64 or item_table.dim() != 2 or item_table.shape[1] != 23 or \
                not item_table.is_cuda or not item_table.is_contiguous():
            raise ValueError("item_table must be a contiguous device float64 [n_item_rows, 23] tensor")
    if user_meta is not None:
        user_meta = torch.as_tensor(user_meta, dtype=torch.float64).to(dev).contiguous()
        if tuple(user_meta.shape) != (nq, 4):
            raise ValueError(f"user_meta must be [{nq}, 4] (recency, gender, age, occupation), got {tuple(user_meta.shape)}")
    off, items, ratings = hist.device_tensors()
    q = torch.empty((nq, d), dtype=torch.float32, device=dev)
    rows = torch.empty((nq, ROW_WIDTH), dtype=torch.float64, device=dev)
    flags = torch.empty((nq,), dtype=torch.int32, device=dev)
    err = torch.empty((1,), dtype=torch.int32, device=dev)
    L.check(L.lib().rihip_fold_in_users(off.data_ptr(), items.data_ptr(), ratings.data_ptr(), nq, int(hist.host[1].shape[0]),
                                        V.data_ptr(), n_rows, ldv, d, row_of.data_ptr(), row_of.shape[0], mu.data_ptr(),
                                        int(min_rating), WEIGHTINGS[weighting], float(beta), L.ptr(item_table),
                                        0 if item_table is None else item_table.shape[0], L.ptr(user_meta),
                                        q.data_ptr(), rows.data_ptr(), flags.data_ptr(), err.data_ptr(), L.stream_ptr()),
            "fold_in_users")
    return q, rows, flags, err


def fold_in_users_device(hist: UserHistories, V, row_of, mu, min_rating: int = 4, weighting: str = "uniform",
                         beta: float = 1.0, item_table=None, user_meta=None):
    """Fold the histories in: -> (q f32 [nq, d], rows f64 [nq, 24], flags i32 [nq]) on the device.

    q[s] is the L2-normalised direction of (weighted mean of the stored vectors of the items slot s rated >=
    min_rating) - beta * mu, flags[s] = 1 (and q[s] = 0) when the slot has no such item or the direction vanishes: serve
    it from the popularity fallback.  rows[s] is the slot's row in the user-table layout of the ranking features.
    V f32 [n_rows, d] (a row stride > d is fine), row_of i32 [n_ids] and mu f64 [d] as FAISSIndex.item_vectors_device()
    returns them; weighting "uniform" (w = 1) or "rating" (w = r - (min_rating - 1)); item_table: the feature store's
    device item table (genre preference; None = zeros); user_meta f64 [nq, 4] = recency, gender, age, occupation (None =
    the serving defaults).  ValueError when a history holds an item id < 0 or a rating outside 1..5 (one
    synchronisation: the kernel's error word)."""
    q, rows, flags, err = fold_in_users_launch(hist, V, row_of, mu, min_rating, weighting, beta, item_table, user_meta)
    e = int(err.item())
    if e:
        what = [m for b, m in ((1, "an item id < 0"), (2, "a rating outside 1..5")) if e & b]
        raise ValueError("fold_in_users: the histories hold " + " and ".join(what))
    return q, rows, flags
