"""Seen-item exclusion around an index search (not in the reference: SURVEY.md §3.4 hazard ii; seen.py, csrc/exclude.hip):
the over-fetch plan, the search per group and the device filter, shared by FAISSIndex and SQ8Index.

A class that mixes this in has ``index.ntotal`` and a search that returns item ids; ``_deferred`` (False when the class
has no deferred exactness check) and ``_deficit`` are its only state here."""
from __future__ import annotations

import math
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import _lib as L


class ExcludingSearch:
    _deferred = False
    _deficit: Optional[torch.Tensor] = None

    def filter_excluded(self, scores: torch.Tensor, ids: torch.Tensor, k: int, seen, user_ids: Optional[torch.Tensor],
                        out_scores: torch.Tensor, out_ids: torch.Tensor, out_slot: Optional[torch.Tensor] = None) -> None:
        """rows of an over-fetched result [nq, k_eff] -> their first k allowed entries, written to row out_slot[q]
        (int32 device tensor; None: row q) of out_scores / out_ids [.., k]; user_ids None: list q of `seen` belongs to
        query q.  A result that already holds the whole corpus cannot have been fetched short: not counted."""
        if self._deficit is None:
            self._deficit = torch.zeros(1, dtype=torch.int32, device=scores.device)
        nq, kc = ids.shape
        whole = kc >= self.index.ntotal
        L.check(L.lib().rihip_exclude_topk(scores.data_ptr(), ids.data_ptr(), nq, kc, L.ptr(user_ids),
                                           seen.offsets.data_ptr(), seen.n_users, seen.items.data_ptr(), k,
                                           out_scores.data_ptr(), out_ids.data_ptr(), L.ptr(out_slot),
                                           None if whole else self._deficit.data_ptr(), L.stream_ptr()), "exclude_topk")

    def exclusion_deficit(self) -> int:
        """queries so far whose over-fetch was too small to fill k allowed entries (one synchronisation); 0 whenever
        the plan of seen.py chose k_eff"""
        return 0 if self._deficit is None else int(self._deficit.item())

    def _search_excluding(self, q: torch.Tensor, k: int, seen, user_ids, item_filter=None,
                          search: Optional[Callable] = None) -> Tuple[torch.Tensor, ...]:
        """q normalised f32 [nq,d] on device -> (scores, item ids) [nq,k] without each query's excluded items.
        user_ids: host sequence (queries are grouped by how far they have to over-fetch, one search per group), a
        device tensor (one group at the store's longest list) or None (list q of `seen` belongs to query q).
        search(q, k_eff, item_filter) -> (scores, item ids, *per-query tensors): the class's search by default; what it
        returns beyond the two lists (one row per query) is handed back behind them, in the batch's order."""
        from .faiss_index import _sub_filter
        from .seen import overfetch_k, plan_overfetch
        if search is None:
            def search(qq, kk, flt):
                return self._search_device(qq, kk, item_ids=True, item_filter=flt)
        nq, ntotal = q.shape[0], self.index.ntotal
        k_max = int(L.lib().rihip_ip_index_max_k())
        if isinstance(user_ids, torch.Tensor) and user_ids.is_cuda:
            uid = user_ids.to(dtype=torch.long).contiguous()
            plan = [(overfetch_k(k, seen.max_count, ntotal, k_max), None)]
            nothing = seen.max_count == 0
        else:
            host = np.arange(nq) if user_ids is None else np.asarray(user_ids, dtype=np.int64).reshape(-1)
            if host.shape[0] != nq:
                raise ValueError(f"{host.shape[0]} user ids for {nq} queries")
            # a deferred exactness check belongs to ONE search of the handle: no groups under it
            extra = seen.counts_of(host)
            plan = plan_overfetch(extra, k, ntotal, k_max, math.inf if self._deferred else None)
            uid = None if user_ids is None else torch.from_numpy(host).to(q.device)
            nothing = not extra.any()
        if len(plan) == 1:
            k_eff = plan[0][0]
            s, c, *more = search(q, k_eff, item_filter)
            if nothing:
                return (s, c, *more)
            scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
            ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            self.filter_excluded(s, c, k, seen, uid, scores, ids)
            return (scores, ids, *more)
        scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
        rest = None
        for k_eff, pos in plan:
            slot = torch.from_numpy(pos.astype(np.int32)).to(q.device)
            sel = slot.to(torch.long)
            s, c, *more = search(q[sel].contiguous(), k_eff, None if item_filter is None else _sub_filter(item_filter, sel))
            self.filter_excluded(s, c, k, seen, sel if uid is None else uid[sel], scores, ids, slot)
            if rest is None:
                rest = [torch.empty((nq,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in more]
            for dst, t in zip(rest, more):
                dst[sel] = t
        return (scores, ids, *rest)
