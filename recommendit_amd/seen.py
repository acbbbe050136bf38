"""Per-user seen-item store and the over-fetch plan that excludes it from retrieval (not in the reference, which
serves and evaluates every retrieved candidate whether the user has rated it or not: SURVEY.md §3.4, hazard ii).

The search itself is untouched.  For a query whose user has ``e`` excluded items the top ``k + e`` unfiltered results
hold at least ``k`` allowed ones, and the search returns a prefix of its full stable order, so dropping the excluded
ids from the top ``k_eff >= k + e`` and keeping the first ``k`` is exactly the top ``k`` of the corpus (for IVF: of
the probed lists) minus the excluded set.  ``overfetch_k`` picks ``k_eff``, ``plan_overfetch`` groups a batch so that
one heavy user does not push every query to a large ``k_eff``, and csrc/exclude.hip filters on the device.

This module imports on a host without a GPU and builds its CSR there; the device tensors are made on first use.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .eval_device import GroundTruth

# plan_overfetch: an over-fetch class with fewer queries than this joins the next larger one.  Measured on the MI355X
# with tools/exclude_bench.py (profiles/r06_exclude.md): every extra search of a batch costs more than
# over-fetching a few hundred queries further, so a batch of 256 is fastest as ONE group (1, 16 and 64 split it and
# are 1.3-3.3x slower), and 256 is the value that still splits the heavy users off a batch of 4 096.
MIN_GROUP = 256

_I32_MAX = 2 ** 31 - 1


class SeenItems:
    """CSR of excluded item ids per user id: row ``u`` = the ids of user ``u``, ascending and unique."""

    def __init__(self, offsets: np.ndarray, items: np.ndarray):
        self._offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self._items = np.ascontiguousarray(items, dtype=np.int32)
        self.n_users = int(self._offsets.shape[0] - 1)
        self.counts = np.diff(self._offsets).astype(np.int32)
        self.max_count = int(self.counts.max()) if self.n_users else 0
        self._dev = None

    # -- constructors ---------------------------------------------------------------------------
    @classmethod
    def from_pairs(cls, users, items, n_users: Optional[int] = None) -> "SeenItems":
        pu = np.asarray(users, dtype=np.int64).reshape(-1)
        pi = np.asarray(items, dtype=np.int64).reshape(-1)
        if pu.shape != pi.shape:
            raise ValueError(f"{pu.shape[0]} user ids for {pi.shape[0]} item ids")
        if pu.shape[0] and (pu.min() < 0 or pi.min() < 0):
            raise ValueError("SeenItems: negative user or item id")
        if pi.shape[0] and pi.max() > _I32_MAX:
            raise ValueError(f"SeenItems: item id {int(pi.max())} >= 2**31 (the device list holds int32 ids)")
        need = int(pu.max()) + 1 if pu.shape[0] else 0
        n = need if n_users is None else int(n_users)
        if n < need:
            raise ValueError(f"SeenItems: user id {need - 1} with n_users={n}")
        offsets, it, _ = GroundTruth.csr_from_pairs(np.arange(n, dtype=np.int64), pu, pi)
        return cls(offsets, it)

    @classmethod
    def from_frame(cls, df, user_col: str = "user_id", item_col: str = "item_id") -> "SeenItems":
        return cls.from_pairs(df[user_col].to_numpy(), df[item_col].to_numpy())

    @classmethod
    def from_dict(cls, seen: Dict[Any, Sequence[int]], n_users: Optional[int] = None) -> "SeenItems":
        users = [int(u) for u, v in seen.items() for _ in v]
        items = [int(x) for v in seen.values() for x in v]
        if n_users is None and seen:
            n_users = max(int(u) for u in seen) + 1
        return cls.from_pairs(users, items, n_users)

    def updated(self, users, items) -> "SeenItems":
        """a new store holding these pairs as well (merged on the host; this object is unchanged)"""
        pu = np.asarray(users, dtype=np.int64).reshape(-1)
        own = np.repeat(np.arange(self.n_users, dtype=np.int64), self.counts)
        n = max(self.n_users, int(pu.max()) + 1 if pu.shape[0] else 0)
        return SeenItems.from_pairs(np.concatenate([own, pu]),
                                    np.concatenate([self._items.astype(np.int64),
                                                    np.asarray(items, dtype=np.int64).reshape(-1)]), n)

    # -- host views -----------------------------------------------------------------------------
    def items_of(self, user_id: int) -> np.ndarray:
        if not 0 <= int(user_id) < self.n_users:
            return np.zeros(0, np.int32)
        return self._items[self._offsets[user_id]:self._offsets[user_id + 1]]

    def counts_of(self, user_ids) -> np.ndarray:
        """excluded items per query (int64); ids outside the table exclude nothing"""
        u = np.asarray(user_ids, dtype=np.int64).reshape(-1)
        ok = (u >= 0) & (u < self.n_users)
        out = np.zeros(u.shape[0], np.int64)
        out[ok] = self.counts[u[ok]]
        return out

    # -- device tensors (made on first use) -----------------------------------------------------------
    def _device(self):
        if self._dev is None:
            import torch
            from . import _lib as L
            dev = L.device()
            items = self._items if self._items.shape[0] else np.zeros(1, np.int32)
            self._dev = (torch.from_numpy(self._offsets).to(dev), torch.from_numpy(items).to(dev))
        return self._dev

    @property
    def offsets(self):
        """device int64 [n_users + 1]"""
        return self._device()[0]

    @property
    def items(self):
        """device int32 ids, row after row"""
        return self._device()[1]


def overfetch_k(k: int, extra: int, ntotal: int, k_max: int) -> int:
    """candidates to fetch so that ``k`` survive the removal of ``extra`` excluded ids: ``k`` itself when nothing is
    excluded, else the smallest power of two >= k + extra (the select buffer of the search is a power of two anyway),
    clipped to what the corpus and the search can return.  A corpus of at most ``k_max`` vectors can always be
    fetched whole; a larger one cannot serve k + extra > k_max."""
    k, extra, ntotal, k_max = int(k), int(extra), int(ntotal), int(k_max)
    if extra <= 0:
        return k
    need = k + extra
    if need > k_max and ntotal > k_max:
        raise ValueError(f"k + seen items = {k} + {extra} = {need} exceeds the search limit of {k_max} candidates on a "
                         f"corpus of {ntotal} vectors (a user with {extra} excluded items cannot be served; DESIGN.md §7)")
    p = 1
    while p < need:
        p <<= 1
    return min(p, ntotal, k_max)


def plan_overfetch(extra, k: int, ntotal: int, k_max: int, min_group: Optional[float] = None
                   ) -> List[Tuple[int, np.ndarray]]:
    """host-side plan of a batch: ``extra[q]`` excluded items for query q -> [(k_eff, positions)], one search per
    entry.  Queries are grouped by their overfetch_k class, ascending; a class with fewer than ``min_group`` queries
    joins the next larger non-empty class (min_group = inf: a single group; None: the module's MIN_GROUP); a group
    searches at its largest class.  Every position appears exactly once, ascending inside its group."""
    extra = np.asarray(extra, dtype=np.int64).reshape(-1)
    if extra.shape[0] == 0:
        return []
    mg = MIN_GROUP if min_group is None else min_group
    uniq, inv = np.unique(extra, return_inverse=True)
    cls = np.array([overfetch_k(k, int(e), ntotal, k_max) for e in uniq], dtype=np.int64)[inv]
    plan: List[Tuple[int, np.ndarray]] = []
    carry: List[np.ndarray] = []
    held = 0
    classes = np.unique(cls)
    for j, c in enumerate(classes):
        pos = np.nonzero(cls == c)[0]
        carry.append(pos)
        held += pos.shape[0]
        if j + 1 < len(classes) and (math.isinf(mg) or held < mg):
            continue
        plan.append((int(c), np.sort(np.concatenate(carry))))
        carry, held = [], 0
    return plan
