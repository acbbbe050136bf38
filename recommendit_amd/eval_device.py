"""The evaluation report on the GPU (not in the reference as such): the reference's evaluate_model
(src/evaluation/metrics.py:301-384) computed straight from a device top-K id tensor, without copying the ids to the
host.  Same keys, same key order and same values as metrics.evaluate_model on the equivalent dicts:

* ``rec_ids``: int64 [n, K] on the HIP device, -1 padded as retrieval and rank_topk produce it; row i is the list
  ``[x for x in rec_ids[i] if x >= 0]`` of the i-th user (padding may also sit inside a row);
* ``GroundTruth``: the users' relevant items as a CSR in the same row order (sorted, de-duplicated segments plus the
  raw list length for IDCG), built on the host with numpy and uploaded once;
* coverage needs the id space (``n_id_space`` > every id); diversity takes an f32 item-vector table [rows, g] with an
  optional presence mask (the table form of the reference's ``item_genre_vectors`` dict).

Kernels: recommendit_amd/csrc/eval.hip.  Everything is enqueued on the current stream; ``TopKEvaluator.enqueue`` can
be captured in a hipGraph and ``TopKEvaluator.result`` reads the one small output vector back.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

DEFAULT_K = [5, 10, 20]


class GroundTruth:
    """Relevant items per evaluated user, row-aligned with the rec_ids tensor."""

    def __init__(self, offsets: np.ndarray, items: np.ndarray, raw_counts: np.ndarray):
        self.n = int(raw_counts.shape[0])
        dev = L.device()
        self.offsets = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(dev)
        self.items = torch.from_numpy(np.ascontiguousarray(items, dtype=np.int64) if len(items) else
                                      np.zeros(1, np.int64)).to(dev)
        self.raw = torch.from_numpy(np.ascontiguousarray(raw_counts, dtype=np.int64)).to(dev)

    @staticmethod
    def csr_from_pairs(users: Sequence[int], pair_users, pair_items) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(offsets [n+1], unique sorted items per row, raw counts [n]) for rows in the order of ``users``; pairs of
        users not in ``users`` are ignored, duplicated pairs count once in a segment and every time in the raw count."""
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        n = users.shape[0]
        pu = np.asarray(pair_users, dtype=np.int64).reshape(-1)
        pi = np.asarray(pair_items, dtype=np.int64).reshape(-1)
        if n == 0 or pu.shape[0] == 0:
            return np.zeros(n + 1, np.int64), np.zeros(0, np.int64), np.zeros(n, np.int64)
        order = np.argsort(users, kind="stable")
        su = users[order]
        loc = np.minimum(np.searchsorted(su, pu), n - 1)
        ok = su[loc] == pu
        row = order[loc[ok]]
        it = pi[ok]
        raw = np.bincount(row, minlength=n).astype(np.int64)
        idx = np.lexsort((it, row))
        row, it = row[idx], it[idx]
        keep = np.ones(row.shape[0], bool)
        keep[1:] = (row[1:] != row[:-1]) | (it[1:] != it[:-1])
        cnt = np.bincount(row[keep], minlength=n)
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(cnt, out=offsets[1:])
        return offsets, it[keep], raw

    @classmethod
    def from_pairs(cls, users: Sequence[int], pair_users, pair_items) -> "GroundTruth":
        return cls(*cls.csr_from_pairs(users, pair_users, pair_items))

    @classmethod
    def from_dict(cls, truth: Dict[Any, Sequence[int]], users: Iterable[Any]) -> "GroundTruth":
        """rows = ``users`` in order (e.g. the keys of a recs dict); users missing from ``truth`` have no truth"""
        users = list(users)
        lens = [len(truth.get(u) or ()) for u in users]
        flat = [int(x) for u in users for x in (truth.get(u) or ())]
        rows = np.repeat(np.arange(len(users), dtype=np.int64), np.asarray(lens, dtype=np.int64))
        return cls(*cls.csr_from_pairs(np.arange(len(users)), rows, np.asarray(flat, dtype=np.int64)))

    @classmethod
    def from_frame(cls, df, users: Sequence[int], user_col: str = "user_id", item_col: str = "item_id") -> "GroundTruth":
        return cls.from_pairs(users, df[user_col].to_numpy(), df[item_col].to_numpy())


def vectors_from_dict(vecs: Dict[int, Any], n_rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """item_genre_vectors dict -> (f32 table [rows, g], u8 presence mask [rows]) on the device"""
    keys = [int(k) for k in vecs]
    if any(k < 0 for k in keys):
        raise ValueError("item ids must be >= 0")
    g = len(np.asarray(next(iter(vecs.values()))).reshape(-1)) if vecs else 1
    rows = max(n_rows or 0, (max(keys) + 1) if keys else 1)
    tab = np.zeros((rows, g), np.float32)
    present = np.zeros(rows, np.uint8)
    for k, v in vecs.items():
        tab[int(k)] = np.asarray(v, dtype=np.float32).reshape(-1)
        present[int(k)] = 1
    dev = L.device()
    return torch.from_numpy(tab).to(dev), torch.from_numpy(present).to(dev)


_TABLES: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}


def _discount_tables(n_tab: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """disc[i] = 1/math.log2(i+2) -- the Python term of ndcg_at_k bit for bit -- and idcg[m] = its left-to-right sum
    over i < m (the order Python's sum() adds in)"""
    size = 64
    while size < n_tab:
        size <<= 1
    key = (torch.cuda.current_device(), size)
    if key not in _TABLES:
        disc = [1.0 / math.log2(i + 2) for i in range(size)]
        idcg = [0.0] * size
        s = 0
        for m in range(1, size):
            s = s + disc[m - 1]
            idcg[m] = s
        dev = L.device()
        _TABLES[key] = (torch.tensor(disc, dtype=torch.float64, device=dev),
                        torch.tensor(idcg, dtype=torch.float64, device=dev))
    return _TABLES[key]


def _require_device(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"evaluate_topk_device: {what} must be a tensor on the HIP device")


class TopKEvaluator:
    """Buffers and launches of one evaluation shape (n users x K ids).  ``enqueue(rec_ids)`` only launches kernels
    (no host synchronisation, capturable); ``result()`` reads the means back and returns the report dict."""

    def __init__(self, truth: GroundTruth, n: int, K: int, k_values: Optional[Sequence[int]] = None,
                 catalog_size: Optional[int] = None, item_vectors: Optional[torch.Tensor] = None,
                 item_present: Optional[torch.Tensor] = None, n_id_space: Optional[int] = None):
        self.k_values = list(k_values) if k_values else list(DEFAULT_K)
        self.uniq = list(dict.fromkeys(int(k) for k in self.k_values))
        if truth.n != n:
            raise ValueError(f"ground truth has {truth.n} rows, rec_ids {n}")
        self.truth, self.n, self.K = truth, n, K
        self.catalog_size = catalog_size
        dev = L.device()
        nk = len(self.uniq)
        self.vals = torch.empty((n, nk, 3), dtype=torch.float64, device=dev)
        self.rr = torch.empty(n, dtype=torch.float64, device=dev)
        self.scored = torch.empty(n, dtype=torch.uint8, device=dev)
        self.disc, self.idcg = _discount_tables(max(max(self.uniq) + 1, 2))
        self.flags = None
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.n_id_space = 0
        if catalog_size:
            if not n_id_space or n_id_space <= 0:
                raise ValueError("coverage needs n_id_space (every id < n_id_space)")
            self.n_id_space = int(n_id_space)
            self.flags = torch.empty(self.n_id_space, dtype=torch.uint8, device=dev)
        self.div = None
        self.item_vectors = self.item_present = None
        if item_vectors is not None:
            _require_device(item_vectors, "item_vectors")
            if item_vectors.dim() != 2:
                raise ValueError("item_vectors must be [rows, g]")
            self.item_vectors = item_vectors.to(torch.float32).contiguous()
            if item_present is not None:
                _require_device(item_present, "item_present")
                if item_present.shape[0] != self.item_vectors.shape[0]:
                    raise ValueError("item_present must have one entry per item_vectors row")
                self.item_present = item_present.to(torch.uint8).contiguous()
            self.div = torch.empty(n, dtype=torch.float64, device=dev)
        nparts = int(L.lib().rihip_eval_nparts())
        self.partials = torch.empty((nparts, 3 * nk + 3), dtype=torch.float64, device=dev)
        self.cov_partials = torch.empty(nparts, dtype=torch.int64, device=dev)
        self.out = torch.empty(3 * nk + 5, dtype=torch.float64, device=dev)
        self._karr = (C.c_int * nk)(*self.uniq)

    def enqueue(self, rec_ids: torch.Tensor) -> None:
        _require_device(rec_ids, "rec_ids")
        if rec_ids.dim() != 2 or tuple(rec_ids.shape) != (self.n, self.K):
            raise ValueError(f"rec_ids must be [{self.n}, {self.K}], got {tuple(rec_ids.shape)}")
        if rec_ids.dtype != torch.int64 or not rec_ids.is_contiguous():
            rec_ids = rec_ids.to(torch.int64).contiguous()
        self._rec = rec_ids   # kept alive until the launches have run
        lib, s, nk, t = L.lib(), L.stream_ptr(), len(self.uniq), self.truth
        L.check(lib.rihip_eval_topk(rec_ids.data_ptr(), self.n, self.K, t.offsets.data_ptr(), t.items.data_ptr(),
                                    t.raw.data_ptr(), self._karr, nk, self.disc.data_ptr(), self.idcg.data_ptr(),
                                    self.disc.shape[0], self.vals.data_ptr(), self.rr.data_ptr(),
                                    self.scored.data_ptr(), L.ptr(self.flags), self.n_id_space,
                                    self.err.data_ptr(), s), "eval_topk")
        if self.div is not None:
            tab = self.item_vectors
            L.check(lib.rihip_eval_diversity(rec_ids.data_ptr(), self.n, self.K, self.scored.data_ptr(),
                                             self.k_values[-1], tab.data_ptr(), tab.shape[0], tab.shape[1],
                                             L.ptr(self.item_present), self.div.data_ptr(), s), "eval_diversity")
        L.check(lib.rihip_eval_reduce(self.n, nk, self.vals.data_ptr(), self.rr.data_ptr(), L.ptr(self.div),
                                      self.scored.data_ptr(), L.ptr(self.flags), self.n_id_space,
                                      int(self.catalog_size or 0), self.err.data_ptr(), self.partials.data_ptr(),
                                      self.cov_partials.data_ptr(), self.out.data_ptr(), s), "eval_reduce")

    def result(self) -> Dict[str, Any]:
        out = self.out.cpu().tolist()
        nk = len(self.uniq)
        if int(out[3 * nk + 4]):
            raise RuntimeError(f"evaluate_topk_device: a recommended id is >= n_id_space ({self.n_id_space})")
        n_scored = int(out[3 * nk + 2])
        res: Dict[str, Any] = {"n_users": self.n, "k_values": self.k_values}
        for k in self.k_values:
            j = self.uniq.index(int(k))
            res[f"ndcg@{k}"] = out[3 * j]
            res[f"recall@{k}"] = out[3 * j + 1]
            res[f"precision@{k}"] = out[3 * j + 2]
            # the reference never fills its per-k mrr / ap lists (metrics.py:341-344): always 0.0
            res[f"mrr@{k}"] = 0.0
            res[f"ap@{k}"] = 0.0
        res["mrr"] = out[3 * nk]
        if self.catalog_size and n_scored:
            res["coverage"] = out[3 * nk + 3]
        if self.div is not None and n_scored:
            res["avg_diversity"] = out[3 * nk + 1]
        return res

    def per_user(self) -> Dict[str, torch.Tensor]:
        d = {"vals": self.vals, "mrr": self.rr, "scored": self.scored}
        if self.div is not None:
            d["diversity"] = self.div
        return d


def evaluate_topk_device(rec_ids: torch.Tensor, truth: GroundTruth, k_values: Sequence[int] = (5, 10, 20),
                         catalog_size: Optional[int] = None, item_vectors: Optional[torch.Tensor] = None,
                         item_present: Optional[torch.Tensor] = None, n_id_space: Optional[int] = None,
                         per_user: bool = False) -> Dict[str, Any]:
    """metrics.evaluate_model on a device top-K tensor (module docstring).  ``n_id_space`` defaults to
    max(id) + 1 when coverage is asked for (one extra read of the ids).  per_user=True adds ``"per_user"``: the
    device tensors vals [n, n_k, 3] (ndcg, recall, precision for the distinct k in order), mrr [n], scored [n]
    and, with vectors, diversity [n]."""
    _require_device(rec_ids, "rec_ids")
    if rec_ids.dim() != 2:
        raise ValueError("rec_ids must be [n, K]")
    n, K = int(rec_ids.shape[0]), int(rec_ids.shape[1])
    if n == 0:
        return {"error": "No users to evaluate", "n_users": 0}
    if catalog_size and n_id_space is None:
        n_id_space = max(int(rec_ids.max()) + 1, 1)
    ev = TopKEvaluator(truth, n, K, list(k_values) if k_values else None, catalog_size, item_vectors, item_present,
                       n_id_space)
    ev.enqueue(rec_ids)
    res = ev.result()
    if per_user:
        res["per_user"] = ev.per_user()
    return res
