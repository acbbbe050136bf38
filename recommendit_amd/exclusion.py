"""Seen-item exclusion around an index search (not in the reference: SURVEY.md §3.4 hazard ii; seen.py, csrc/exclude.hip):
the over-fetch plan, the search per group and the device filter, shared by FAISSIndex and SQ8Index -- and the second
implementation, ``exclusion="scan"``: one search of the whole batch whose scans test a per-query bit mask of the seen rows
(csrc/search_exclude.hip), for the classes that have such a search (``_search_scan_excluding``).

A class that mixes this in has ``index.ntotal`` and a search that returns item ids; ``_deferred`` (False when the class
has no deferred exactness check) and ``_deficit`` are its only state here."""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import _lib as L


EXCLUSIONS = ("overfetch", "scan")


def check_exclusion(exclusion) -> str:
    """the name of an exclusion implementation, or ValueError (before anything is launched)"""
    if exclusion not in EXCLUSIONS:
        raise ValueError(f"exclusion must be one of {EXCLUSIONS}, got {exclusion!r}")
    return exclusion


def seen_user_ids(user_ids, nq: int, device) -> Optional[torch.Tensor]:
    """user ids of a batch as the device int64 [nq] the scan-side exclusion reads (None: list q belongs to query q)"""
    if user_ids is None:
        return None
    if isinstance(user_ids, torch.Tensor):
        uid = user_ids.to(device=device, dtype=torch.long).reshape(-1).contiguous()
    else:
        uid = torch.from_numpy(np.ascontiguousarray(np.asarray(user_ids, dtype=np.int64).reshape(-1))).to(device)
    if uid.shape[0] != nq:
        raise ValueError(f"{uid.shape[0]} user ids for {nq} queries")
    return uid


class ExcludingSearch:
    _deferred = False
    _deficit: Optional[torch.Tensor] = None
    _row_of_cache: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
    _EXCL_ABI: dict = {}      # the class's C entry points behind exclusion_mask / set_exclusion_budget / ...

    def _row_of_device(self) -> torch.Tensor:
        """int32 [max item id + 1] on the device: item id -> row, -1 = not stored (exclusion="scan").  Kept per index
        state: a build, load or update replaces the device id array, and the table with it."""
        ids_dev = self._item_ids_dev
        if self._row_of_cache is None or self._row_of_cache[0] is not ids_dev:
            ids = self.item_ids
            if ids.shape[0] and (ids.min() < 0 or ids.max() >= 2 ** 31 - 1):
                raise ValueError('exclusion="scan": item ids must lie in [0, 2**31 - 1) (row_of is indexed by item id)')
            row_of = torch.full((int(ids.max()) + 1,), -1, dtype=torch.int32, device=ids_dev.device)
            row_of[ids_dev] = torch.arange(ids.shape[0], dtype=torch.int32, device=ids_dev.device)
            self._row_of_cache = (ids_dev, row_of)
        return self._row_of_cache[1]

    @staticmethod
    def _check_row_of(row_of) -> torch.Tensor:
        if not isinstance(row_of, torch.Tensor) or row_of.dtype != torch.int32 or not row_of.is_cuda or row_of.dim() != 1:
            raise ValueError("row_of must be a one-dimensional int32 device tensor (item id -> row, -1 = not stored)")
        return row_of.contiguous()

    def exclusion_mask(self, seen, user_ids, nq: Optional[int] = None) -> np.ndarray:
        """uint32 [nq, W]: the mask an exclusion="scan" search of these users builds -- bit p & 31 of word p >> 5 of row q
        is set iff the row at scan position p (flat: the row; IVF: the list-major physical position) is excluded for
        query q.  user_ids None: list q of `seen` belongs to query q (nq of them)."""
        if self.index is None:
            raise RuntimeError("Index not built.")
        n = int(nq) if user_ids is None else int(np.asarray(user_ids.cpu() if isinstance(user_ids, torch.Tensor) else user_ids).reshape(-1).shape[0])
        abi = self._EXCL_ABI
        row_of = self._row_of_device()
        uid = seen_user_ids(user_ids, n, row_of.device)
        w = C.c_int64(0)
        L.check(getattr(L.lib(), abi["mask_words"])(self.index._h, C.byref(w)), abi["mask_words"])
        out = torch.empty((n, int(w.value)), dtype=torch.int32, device=row_of.device)
        L.check(getattr(L.lib(), abi["mask"])(self.index._h, n, L.ptr(uid), seen.offsets.data_ptr(), seen.n_users,
                                              seen.items.data_ptr(), row_of.data_ptr(), row_of.shape[0], out.data_ptr(),
                                              L.stream_ptr()), abi["mask"])
        return out.cpu().numpy().view(np.uint32)

    def set_exclusion_budget(self, n_bytes: int) -> None:
        """bytes of mask scratch an exclusion="scan" search may hold (0: the default); a batch whose mask is larger is
        searched in chunks of queries.  Results do not depend on it (a test hook)."""
        L.check(getattr(L.lib(), self._EXCL_ABI["budget"])(self.index._h, int(n_bytes)), self._EXCL_ABI["budget"])

    def exclusion_stats(self) -> Dict[str, int]:
        """exclusion="scan" since the handle was made: queries searched, of those re-done exactly, mask chunks"""
        out = (C.c_int64 * 3)()
        L.check(getattr(L.lib(), self._EXCL_ABI["stats"])(self.index._h, out), self._EXCL_ABI["stats"])
        return {"queries": int(out[0]), "redone": int(out[1]), "chunks": int(out[2])}

    def exclusion_scratch_nonzero(self) -> int:
        """non-zero words of the handle's mask scratch: 0 between searches (one synchronisation)"""
        n = C.c_int64(0)
        L.check(getattr(L.lib(), self._EXCL_ABI["nonzero"])(self.index._h, C.byref(n), L.stream_ptr()),
                self._EXCL_ABI["nonzero"])
        return int(n.value)

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

    def _search_scan_excluding(self, q: torch.Tensor, k: int, seen, uid: Optional[torch.Tensor], item_filter=None
                               ) -> Tuple[torch.Tensor, torch.Tensor]:
        raise NotImplementedError(f'{type(self).__name__} has no exclusion="scan" search')

    def _search_excluding(self, q: torch.Tensor, k: int, seen, user_ids, item_filter=None,
                          search: Optional[Callable] = None, exclusion: str = "overfetch") -> Tuple[torch.Tensor, ...]:
        """q normalised f32 [nq,d] on device -> (scores, item ids) [nq,k] without each query's excluded items.
        user_ids: host sequence (queries are grouped by how far they have to over-fetch, one search per group), a
        device tensor (one group at the store's longest list) or None (list q of `seen` belongs to query q).
        search(q, k_eff, item_filter) -> (scores, item ids, *per-query tensors): the class's search by default; what it
        returns beyond the two lists (one row per query) is handed back behind them, in the batch's order.
        exclusion="scan": the class's search with the exclusion inside its scans instead (one call, any list length)."""
        from .faiss_index import _sub_filter
        from .seen import overfetch_k, plan_overfetch
        if check_exclusion(exclusion) == "scan":
            # one call with the whole batch: no plan, no groups, no device filter, nothing added to the deficit
            if search is not None:
                raise NotImplementedError('exclusion="scan" under a custom search')
            return self._search_scan_excluding(q, k, seen, seen_user_ids(user_ids, q.shape[0], q.device), item_filter)
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
