"""Validation during training by exact full-catalogue ranks (not in the reference, which keeps its "best" checkpoint by
training loss and evaluates once, after the last epoch, from top-k lists).

For every held-out (user, item) pair the device counts the non-excluded catalogue items that outrank the item
(csrc/rank_eval.hip; contract in include/recommendit_hip.h): one score sweep with a counting epilogue instead of an
index build, an over-fetched search with exclusion and a top-k selection.  The count is an integer, exact and
order-independent; the report is the one ``eval_device.TopKEvaluator`` gives for the full exact list.

* ``rank_targets_device``: the launch wrapper (rank, target score, error word; nothing is synchronised);
* ``RankValidator``: towers in eval mode -> ranks -> per-user metrics -> means, one host read per ``evaluate()``;
* ``leave_last_out``: the split (host, NumPy / pandas, once per run);
* ``select_epoch``: checkpoint choice and early stopping as a pure function.

This module imports on a host without a GPU; device tensors are made on first use.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .eval_device import GroundTruth
from .seen import SeenItems

LOWER_IS_BETTER = ("median_rank",)


def select_epoch(values: Sequence[float], mode: str = "max", patience: Optional[int] = None
                 ) -> Tuple[Optional[int], Optional[int]]:
    """(best, stop) of a sequence of validation values, read in order.  ``best`` is the index of the best value seen up
    to and including ``stop`` (mode "max" or "min"; a tie goes to the earlier index; NaN never improves).  ``stop`` is
    the first index that is ``patience`` validations past the best so far without an improvement, None when that never
    happens (or patience is None): training runs to the end.  Empty input: (None, None)."""
    if mode not in ("max", "min"):
        raise ValueError(f"select_epoch: mode must be 'max' or 'min', got {mode!r}")
    if patience is not None and (isinstance(patience, bool) or int(patience) != patience or int(patience) < 1):
        raise ValueError(f"select_epoch: patience must be an integer >= 1 or None, got {patience!r}")
    best: Optional[int] = None
    for i, v in enumerate(values):
        v = float(v)
        if not math.isnan(v):
            if best is None:
                best = i
            else:
                b = float(values[best])
                if (v > b) if mode == "max" else (v < b):
                    best = i
        ref = best if best is not None else -1   # nothing valid yet: counted from before the first validation
        if patience is not None and i - ref >= int(patience):
            return best, i
    return best, None


class HeldOutTruth(GroundTruth):
    """A GroundTruth built on the host whose device tensors are made on first use (the split runs without a GPU)."""

    def __init__(self, offsets: np.ndarray, items: np.ndarray, raw_counts: np.ndarray):
        self.n = int(raw_counts.shape[0])
        self.host_offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.host_items = np.ascontiguousarray(items, dtype=np.int64)
        self.host_raw = np.ascontiguousarray(raw_counts, dtype=np.int64)
        self._dev = None

    def _device(self):
        if self._dev is None:
            import torch
            from . import _lib as L
            dev = L.device()
            items = self.host_items if self.host_items.shape[0] else np.zeros(1, np.int64)
            self._dev = tuple(torch.from_numpy(a).to(dev) for a in (self.host_offsets, items, self.host_raw))
        return self._dev

    offsets = property(lambda self: self._device()[0])
    items = property(lambda self: self._device()[1])
    raw = property(lambda self: self._device()[2])


def leave_last_out(ratings_df, min_rating: float = 4, n_holdout: int = 1, max_users: Optional[int] = None, seed: int = 0):
    """Hold out each user's last ``n_holdout`` ratings >= ``min_rating``, ordered by (timestamp, input position).
    Users with fewer than ``n_holdout + 1`` such ratings are left whole and not validated; ``max_users`` keeps that
    many of the validated users, chosen by a seeded permutation (the others are left whole).
    -> (train_df: the frame without the held-out rows, in input order; GroundTruth over ``users``; users: the
    validated user ids, ascending, int64; SeenItems of train_df)."""
    if int(n_holdout) < 1:
        raise ValueError(f"leave_last_out: n_holdout must be >= 1, got {n_holdout!r}")
    n_holdout = int(n_holdout)
    u = ratings_df["user_id"].to_numpy().astype(np.int64)
    it = ratings_df["item_id"].to_numpy().astype(np.int64)
    r = ratings_df["rating"].to_numpy()
    ts = ratings_df["timestamp"].to_numpy() if "timestamp" in ratings_df.columns else np.zeros(len(u), np.int64)
    pos = np.arange(len(u), dtype=np.int64)
    liked = np.nonzero(r >= min_rating)[0]
    order = liked[np.lexsort((pos[liked], ts[liked], u[liked]))]   # by user, then time, then input position
    ou = u[order]
    # position from the end inside the user's run
    start = np.ones(len(order), bool)
    start[1:] = ou[1:] != ou[:-1]
    run_id = np.cumsum(start) - 1
    run_len = np.bincount(run_id) if len(order) else np.zeros(0, np.int64)
    run_end = np.cumsum(run_len)
    from_end = run_end[run_id] - 1 - np.arange(len(order)) if len(order) else np.zeros(0, np.int64)
    enough = run_len[run_id] >= n_holdout + 1 if len(order) else np.zeros(0, bool)
    users = np.unique(ou[enough]) if len(order) else np.zeros(0, np.int64)
    if max_users is not None and len(users) > int(max_users):
        perm = np.random.RandomState(seed).permutation(len(users))
        users = np.sort(users[perm[:int(max_users)]])
    held = order[enough & (from_end < n_holdout) & np.isin(ou, users)] if len(order) else order
    keep = np.ones(len(u), bool)
    keep[held] = False
    train_df = ratings_df[keep]
    truth = HeldOutTruth(*GroundTruth.csr_from_pairs(users, u[held], it[held]))
    seen = SeenItems.from_pairs(u[keep], it[keep])
    return train_df, truth, users, seen


def _i32_dev(a, dev):
    import torch
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _i64_dev(a, dev):
    import torch
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.int64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def rank_targets_device(U, Y, truth_rows_csr, excl_csr=None, grid_splits: int = 0):
    """rihip_rank_targets on device tensors.  U f32 [n_users, d], Y f32 [n_items, d]; truth_rows_csr = (offsets i64
    [n_users + 1], target rows of Y i32 [n_pairs]); excl_csr = the same for the excluded rows (ascending and unique
    inside a row) or None.  -> (rank i32 [n_pairs], target_score f32 [n_pairs], err i32 [1]) on the device; nothing
    is synchronised.  err bit 0: an exclusion row outside the catalogue (ignored); bit 1: a target outside it
    (rank -1)."""
    import torch
    from . import _lib as L
    dev = L.device()
    U, Y = L.f32c(U), L.f32c(Y)
    if U.dim() != 2 or Y.dim() != 2 or U.shape[1] != Y.shape[1]:
        raise ValueError(f"rank_targets_device: U {tuple(U.shape)} and Y {tuple(Y.shape)} must be [n, d] with one d")
    off, rows = _i64_dev(truth_rows_csr[0], dev), _i32_dev(truth_rows_csr[1], dev)
    n_users, n_pairs = int(U.shape[0]), int(rows.shape[0])
    if off.shape[0] != n_users + 1:
        raise ValueError(f"rank_targets_device: {off.shape[0]} pair offsets for {n_users} users")
    e_off = e_rows = None
    n_excl = 0
    if excl_csr is not None:
        e_off, e_rows = _i64_dev(excl_csr[0], dev), _i32_dev(excl_csr[1], dev)
        n_excl = int(e_rows.shape[0])
        if e_off.shape[0] != n_users + 1:
            raise ValueError(f"rank_targets_device: {e_off.shape[0]} exclusion offsets for {n_users} users")
    lib = L.lib()
    nbytes = int(lib.rihip_rank_targets_workspace_bytes(n_pairs, n_excl, int(U.shape[1])))
    if nbytes < 0:
        raise ValueError(f"rank_targets_device: sizes out of range (pairs={n_pairs}, excluded={n_excl}, "
                         f"d={int(U.shape[1])}: multiples of 16 up to 256)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rank = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    score = torch.empty(n_pairs, dtype=torch.float32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(lib.rihip_rank_targets(U.data_ptr(), n_users, Y.data_ptr(), int(Y.shape[0]), int(U.shape[1]),
                                   off.data_ptr(), rows.data_ptr(), n_pairs, L.ptr(e_off),
                                   L.ptr(e_rows) if n_excl else None, n_excl, int(grid_splits), rank.data_ptr(),
                                   score.data_ptr(), err.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr()),
            "rank_targets")
    return rank, score, err


class RankValidator:
    """Held-out retrieval quality of a two-tower model over the whole catalogue, on the device.

    ``item_ids`` [n_items] / ``genre_matrix`` [n_items, G]: the catalogue, row r = item_ids[r].  ``truth``: the
    held-out items (ids) of ``users``, row-aligned.  ``seen``: the items (ids) each user must not be ranked against
    (None: nothing excluded).  Ids are mapped to catalogue rows once, here: a ground-truth item outside the catalogue
    stays in the CSR as row -1 and is a miss; an exclusion item outside it is dropped."""

    def __init__(self, model, item_ids, genre_matrix, truth: GroundTruth, users, seen: Optional[SeenItems],
                 k_values: Sequence[int] = (10, 50)):
        import torch
        from . import _lib as L
        from .eval_device import _discount_tables
        dev = L.device()
        self.model = model
        self.k_values = [int(k) for k in k_values]
        if not self.k_values or min(self.k_values) < 1:
            raise ValueError(f"RankValidator: k_values must be positive, got {list(k_values)!r}")
        self.uniq = list(dict.fromkeys(self.k_values))
        ids = np.asarray(item_ids, dtype=np.int64).reshape(-1)
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        self.n_items, self.n = int(ids.shape[0]), int(users.shape[0])
        if truth.n != self.n:
            raise ValueError(f"RankValidator: ground truth has {truth.n} rows for {self.n} users")
        gm = np.asarray(genre_matrix, dtype=np.float32)
        if gm.shape[0] != self.n_items:
            raise ValueError(f"RankValidator: {gm.shape[0]} genre rows for {self.n_items} items")
        order = np.argsort(ids, kind="stable")
        sorted_ids = ids[order]

        def rows_of(x: np.ndarray) -> np.ndarray:
            if self.n_items == 0 or x.shape[0] == 0:
                return np.full(x.shape[0], -1, np.int64)
            loc = np.minimum(np.searchsorted(sorted_ids, x), self.n_items - 1)
            return np.where(sorted_ids[loc] == x, order[loc], -1)

        if isinstance(truth, HeldOutTruth):
            t_off, t_items = truth.host_offsets, truth.host_items
        else:
            t_off = truth.offsets.cpu().numpy()
            t_items = truth.items.cpu().numpy()[:int(t_off[-1])]
        self.pair_offsets = torch.from_numpy(np.ascontiguousarray(t_off, dtype=np.int64)).to(dev)
        self.pair_rows = torch.from_numpy(rows_of(t_items).astype(np.int32)).to(dev)
        self.n_pairs = int(t_items.shape[0])
        self.truth = truth
        self.excl = None
        if seen is not None:
            cnt = seen.counts_of(users)
            ok = (users >= 0) & (users < seen.n_users)
            start = np.where(ok, seen._offsets[np.clip(users, 0, max(seen.n_users - 1, 0))], 0) if seen.n_users else cnt
            tot = int(cnt.sum())
            row = np.repeat(np.arange(self.n, dtype=np.int64), cnt)
            first = np.zeros(self.n + 1, np.int64)
            np.cumsum(cnt, out=first[1:])
            src = np.repeat(start, cnt) + (np.arange(tot, dtype=np.int64) - np.repeat(first[:-1], cnt))
            r = rows_of(seen._items[src].astype(np.int64)) if tot else np.zeros(0, np.int64)
            keep = r >= 0
            row, r = row[keep], r[keep]
            idx = np.lexsort((r, row))          # ascending inside a row; ids are unique, so rows are
            e_off = np.zeros(self.n + 1, np.int64)
            np.cumsum(np.bincount(row, minlength=self.n), out=e_off[1:])
            e_rows = r[idx].astype(np.int32)
            self.excl = (torch.from_numpy(e_off).to(dev),
                         torch.from_numpy(e_rows if e_rows.shape[0] else np.zeros(1, np.int32)).to(dev)[:e_rows.shape[0]])
        self.item_ids_dev = torch.from_numpy(ids).to(dev)
        self.genres_dev = torch.from_numpy(np.ascontiguousarray(gm)).to(dev)
        self.users_dev = torch.from_numpy(users).to(dev)
        nk = len(self.uniq)
        self.vals = torch.empty((self.n, nk, 3), dtype=torch.float64, device=dev)
        self.rr = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.scored = torch.empty(self.n, dtype=torch.uint8, device=dev)
        self.disc, self.idcg = _discount_tables(max(max(self.uniq) + 1, 2))
        nparts = int(L.lib().rihip_eval_nparts())
        self.partials = torch.empty((nparts, 3 * nk + 3), dtype=torch.float64, device=dev)
        self.out = torch.empty(3 * nk + 5, dtype=torch.float64, device=dev)
        self._karr = (C.c_int * nk)(*self.uniq)
        self.rank = self.target_score = self.err = None

    def embed(self, batch: int = 65536):
        """(U [n_users, d], Y [n_items, d]) of the model in eval mode (no dropout); restores the training flag"""
        import torch
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                ys = [self.model.item_tower(self.item_ids_dev[s:s + batch], self.genres_dev[s:s + batch])
                      for s in range(0, self.n_items, batch)]
                Y = torch.cat(ys, 0) if len(ys) != 1 else ys[0]
                U = self.model.user_tower(self.users_dev)
        finally:
            self.model.train(was_training)
        return U, Y

    def enqueue(self, U, Y) -> None:
        """ranks -> per-user metrics -> means, launches only"""
        from . import _lib as L
        lib, s, nk = L.lib(), L.stream_ptr(), len(self.uniq)
        self.rank, self.target_score, self.err = rank_targets_device(U, Y, (self.pair_offsets, self.pair_rows), self.excl)
        L.check(lib.rihip_eval_ranks(self.rank.data_ptr(), self.pair_offsets.data_ptr(), self.n, self.n_pairs,
                                     self.truth.raw.data_ptr(), self._karr, nk, self.disc.data_ptr(),
                                     self.idcg.data_ptr(), self.disc.shape[0], self.vals.data_ptr(),
                                     self.rr.data_ptr(), self.scored.data_ptr(), s), "eval_ranks")
        L.check(lib.rihip_eval_reduce(self.n, nk, self.vals.data_ptr(), self.rr.data_ptr(), None,
                                      self.scored.data_ptr(), None, 0, 0, None, self.partials.data_ptr(), None,
                                      self.out.data_ptr(), s), "eval_reduce")

    def evaluate(self) -> Dict[str, Any]:
        """the report of TopKEvaluator.result() for the full exact list with the seen items removed, plus
        ``median_rank`` (lower median of the 0-based ranks; a target outside the catalogue counts as n_items) and
        ``n_scored``; one host read"""
        import torch
        if self.n == 0 or self.n_pairs == 0:
            return {"error": "No users to evaluate", "n_users": 0}
        U, Y = self.embed()
        self.enqueue(U, Y)
        r = torch.where(self.rank < 0, torch.full_like(self.rank, self.n_items), self.rank)
        med = torch.sort(r).values[(self.n_pairs - 1) // 2].to(torch.float64).reshape(1)
        out = torch.cat([self.out, med]).cpu().tolist()
        nk = len(self.uniq)
        res: Dict[str, Any] = {"n_users": self.n, "k_values": self.k_values}
        for k in self.k_values:
            j = self.uniq.index(k)
            res[f"ndcg@{k}"] = out[3 * j]
            res[f"recall@{k}"] = out[3 * j + 1]
            res[f"precision@{k}"] = out[3 * j + 2]
        res["mrr"] = out[3 * nk]
        res["n_scored"] = int(out[3 * nk + 2])
        res["median_rank"] = out[-1]
        return res

    def per_user(self) -> Dict[str, Any]:
        return {"vals": self.vals, "mrr": self.rr, "scored": self.scored, "rank": self.rank,
                "target_score": self.target_score, "err": self.err}


def report_keys(k_values: Sequence[int]) -> List[str]:
    """the keys of RankValidator.evaluate() a checkpoint rule may name"""
    keys = [f"{m}@{int(k)}" for k in k_values for m in ("ndcg", "recall", "precision")]
    return keys + ["mrr", "median_rank"]
