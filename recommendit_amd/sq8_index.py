"""SQ8Index: an 8-bit scalar-quantised inner-product index (flat and IVF) next to FAISSIndex (not in the reference; faiss
has it as IndexScalarQuantizer / IndexIVFScalarQuantizer at 8 bits per dimension).

Built from a trained FAISSIndex (``SQ8Index.from_index``), which may be dropped afterwards: the catalogue then takes
64 or 128 bytes per item instead of 512 (d = 128) and the scan runs on the int8 matrix pipe.  The quantiser, the 16-bit
query transform and the integer score are specified at ``rihip_sq8_index_*`` in recommendit_hip.h; the quantiser is
not faiss's QT_8bit and faiss SQ files are not read or written.  Search results have FAISSIndex's shapes,
dtypes and -1 padding; scores are (float)(b + t * S) of the integer score S, i.e. the inner product of the query with
the DECODED vectors up to the query's own 16-bit rounding.

Refined search (opt-in): with the source's f32 vectors attached (``keep_vectors=True`` / ``attach_vectors``) a search
may re-score the 8-bit search's best ``k_scan = ceil(factor * k)`` candidates exactly in f32 and return the top k of
those, with a per-query certificate that the list is the exact top k of the probed lists (``refine=``,
``return_cert=``, ``set_refine``, ``search_certified``; rihip_sq8_refine_search in recommendit_hip.h).

Filtered retrieval and seen-item exclusion, as on FAISSIndex: ``set_item_tags`` gives every item a 32-bit tag word and
``item_filter=(any_of, all_of, none_of)`` restricts a search to the items whose word passes, tested inside the int8 scan
(rihip_sq8_filter_* in recommendit_hip.h); ``exclude=`` / ``user_ids=`` over-fetch and drop each query's seen items on
the device (exclusion.py).  Both compose with ``mode=``, ``refine=`` and ``return_cert=``.

Live catalogue, as on FAISSIndex and without one: ``add_items`` / ``remove_items`` / ``update_items`` are one repack
of the code matrix on the device under the index's own centroids and its own quantiser (rihip_sq8_update_* in
recommendit_hip.h, csrc/sq8_update.hip).  Kept rows keep their codes, new rows are encoded on the fly, tag words and
attached vectors travel along, and the handle ends bit for bit where ``from_index`` of the final corpus with
``ranges=quantizer()`` would leave it.  Neither centroids nor quantiser are retrained: ``update_stats()["clamped"]``
counts the code values of added rows that fell outside the quantiser's range.

There is no NumPy or torch path for encode, search or repack: everything runs in csrc/sq8_build.hip (encode),
csrc/sq8.hip over csrc/sq8_scan.hip (search), csrc/sq8_refine.hip (refined search), csrc/sq8_state.hip (save / load) and
csrc/sq8_update.hip (repack).
"""
from __future__ import annotations

import ctypes as C
import logging
import math
import pickle
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .exclusion import ExcludingSearch, check_exclusion, seen_user_ids
from .faiss_index import FAISSIndex, _filter_device, _sub_filter

logger = logging.getLogger(__name__)

MODES = {"auto": 0, "dense": 1, "thresholded": 2}
_DEFAULT = object()   # refine=: "the index's sticky factor (set_refine)"


class _SQ8Handle:
    """Owns one rihip sq8_index; exposes the two faiss attributes the callers touch."""

    def __init__(self, handle: int, owner: "SQ8Index"):
        self._h = C.c_void_p(handle)
        self._owner = owner

    @property
    def ntotal(self) -> int:
        return int(L.lib().rihip_sq8_index_ntotal(self._h))

    @property
    def nprobe(self) -> int:
        return self._owner.n_probe

    @nprobe.setter
    def nprobe(self, v: int) -> None:
        self._owner.n_probe = int(v)
        L.check(L.lib().rihip_sq8_index_set_nprobe(self._h, int(v)), "sq8_index_set_nprobe")

    @property
    def nlist(self) -> int:
        return int(L.lib().rihip_sq8_index_nlist(self._h))

    def __del__(self):
        try:
            if self._h:
                L.lib().rihip_sq8_index_destroy(self._h)
                self._h = None
        except Exception:
            pass


def _factor(refine) -> Optional[float]:
    """a refine factor as given by a caller -> None (plain search) or a finite float >= 1"""
    if refine is None:
        return None
    if isinstance(refine, bool) or not isinstance(refine, (int, float, np.integer, np.floating)):
        raise ValueError(f"SQ8Index: refine={refine!r} must be None or a number >= 1")
    f = float(refine)
    if not math.isfinite(f) or f < 1.0:
        raise ValueError(f"SQ8Index: refine={refine!r} must be finite and at least 1")
    return f


def _mode(mode) -> int:
    if mode not in MODES:
        raise ValueError(f"SQ8Index: unknown search mode {mode!r} (one of {sorted(MODES)})")
    return MODES[mode]


def _tag_words(tags, n: int) -> np.ndarray:
    """uint32 / int32 words [n] (host array or tensor) -> uint32 [n] on the host (FAISSIndex._tags_dev's checks)"""
    if isinstance(tags, torch.Tensor):
        a = tags.detach().cpu().numpy()
        a = a.view(np.uint32) if a.dtype == np.int32 else a.astype(np.uint32)
    else:
        a = np.asarray(tags)
        if a.dtype.kind not in "iu":
            raise ValueError(f"tags must be uint32 words, got {a.dtype}")
        if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 32)):
            raise ValueError("tags must fit 32 bits")
        a = (a.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    a = np.ascontiguousarray(a.reshape(-1))
    if a.shape[0] != n:
        raise ValueError(f"{a.shape[0]} tag words for {n} items")
    return a


def _check_source(cls_name: str, faiss_index) -> None:
    """what from_index asks of its source"""
    if not isinstance(faiss_index, FAISSIndex):
        raise ValueError(f"{cls_name}.from_index needs a FAISSIndex, got {type(faiss_index).__name__}")
    if faiss_index.index is None:
        raise RuntimeError("Index not built.")
    if faiss_index.search_pending():
        raise RuntimeError("a deferred search is pending: call finish_search() before encoding the index")


def _check_ranges(cls_name: str, ranges, d: int):
    """ranges= as given -> (centre, scale) f32 [d] contiguous, or (None, None)"""
    if ranges is None:
        return None, None
    if len(ranges) != 2:
        raise ValueError(f"{cls_name}: ranges must be (centre, scale)")
    m = np.ascontiguousarray(ranges[0], dtype=np.float32)
    s = np.ascontiguousarray(ranges[1], dtype=np.float32)
    if m.shape != (d,) or s.shape != (d,):
        raise ValueError(f"{cls_name}: ranges must be two [{d}] arrays, got {m.shape} and {s.shape}")
    if not (np.isfinite(m).all() and np.isfinite(s).all() and (s > 0).all()):
        raise ValueError(f"{cls_name}: ranges must be finite with scale > 0")
    return m, s


class SQ8Index(ExcludingSearch):
    _KIND = "SQ8"                                  # in messages; PQIndex: "PQ"
    _SAVE, _LOAD = "rihip_sq8_index_save", "rihip_sq8_index_load"
    _UPDATE = "rihip_sq8_update_apply"             # add_items / remove_items / update_items
    _EXCL_ABI = {"mask_words": "rihip_sq8_exclude_mask_words", "mask": "rihip_sq8_exclude_mask",
                 "budget": "rihip_sq8_exclude_set_exclusion_budget", "nonzero": "rihip_sq8_exclude_scratch_nonzero",
                 "stats": "rihip_sq8_exclude_exclusion_stats"}

    def __init__(self, embed_dim: int = 64, n_lists: int = 100, n_probe: int = 10, exact: bool = False):
        if not 1 <= int(embed_dim) <= 128:
            raise ValueError(f"SQ8Index: embed_dim={embed_dim} outside 1..128")
        self.embed_dim = int(embed_dim)
        self.n_lists = n_lists
        self.n_probe = n_probe
        self.exact = exact
        self.index: Optional[_SQ8Handle] = None
        self.item_ids: Optional[np.ndarray] = None
        self._item_id_to_faiss_idx: Dict[int, int] = {}
        self._item_ids_dev: Optional[torch.Tensor] = None
        self._refine: Optional[float] = None
        self._deficit: Optional[torch.Tensor] = None
        self._tags: Optional[np.ndarray] = None        # uint32 [ntotal] on the host, row order (the handle holds its own copy)
        self._pred_cache: Dict[Tuple[int, int, int], torch.Tensor] = {}   # shared predicates already on the device
                                                                          # (three words each: no row count in them)
        self._last_clamped = 0                         # code values clamped by the last update that changed the index

    @property
    def _item_id_to_faiss_idx(self) -> Dict[int, int]:
        """{item id: row}: the plain dict after from_index or load; after add_items / remove_items / update_items it is
        rebuilt from item_ids on the first read (save() reads it), not inside the update"""
        if self._id_map_stale:
            self._id_map = {int(iid): row for row, iid in enumerate(self.item_ids.tolist())}
            self._id_map_stale = False
        return self._id_map

    @_item_id_to_faiss_idx.setter
    def _item_id_to_faiss_idx(self, value: Dict[int, int]) -> None:
        self._id_map = value
        self._id_map_stale = False

    # -- build ----------------------------------------------------------------------------------------------------
    @classmethod
    def from_index(cls, faiss_index: FAISSIndex, ranges: Optional[Tuple[np.ndarray, np.ndarray]] = None,
                   keep_vectors: bool = False) -> "SQ8Index":
        """Encode the vectors of a built FAISSIndex (IVF: its lists and centroids; exact: one list).  ranges: (centre,
        scale), two f32 [embed_dim] arrays that replace the trained per-dimension quantiser; scale > 0.
        keep_vectors=True also copies the f32 vectors (attach_vectors), which a refined search needs.  A source with item
        tags hands them on (set_item_tags); one without leaves the new index untagged."""
        _check_source("SQ8Index", faiss_index)
        m, s = _check_ranges("SQ8Index", ranges, faiss_index.embed_dim)
        h = C.c_void_p()
        L.check(L.lib().rihip_sq8_index_from_ip_index(faiss_index.index._h, None if m is None else m.ctypes.data,
                                                      None if s is None else s.ctypes.data, C.byref(h), L.stream_ptr()),
                "sq8_index_from_ip_index")
        return cls._adopt(h.value, faiss_index, keep_vectors)

    @classmethod
    def _adopt(cls, handle: int, faiss_index: FAISSIndex, keep_vectors: bool):
        """the wrapper around a handle just built from faiss_index: its ids, and on request its vectors and tags"""
        ivf = bool(faiss_index.index.is_ivf)
        # a flat source becomes one list probed once: that is what the handle holds and what load() must hand back to it
        obj = cls(embed_dim=faiss_index.embed_dim, n_lists=faiss_index.n_lists, n_probe=faiss_index.n_probe if ivf else 1,
                  exact=not ivf)
        obj.index = _SQ8Handle(handle, obj)
        obj.item_ids = np.array(faiss_index.item_ids, dtype=np.int64)
        obj._item_ids_dev = torch.from_numpy(obj.item_ids).to(L.device())
        obj._item_id_to_faiss_idx = dict(faiss_index._item_id_to_faiss_idx)
        logger.info("%s index built: %d vectors, %d lists, probe=%d", cls._KIND, obj.index.ntotal, obj.index.nlist, obj.n_probe)
        if keep_vectors:
            obj.attach_vectors(faiss_index)
        if faiss_index._tags is not None:
            obj.set_item_tags(faiss_index.item_tags())
        return obj

    # -- live catalogue (FAISSIndex's add_items / remove_items / update_items on the 8-bit index) ---------------------
    # Every call is ONE repack of the code matrix on the device under the index's own centroids and its own quantiser
    # (csrc/sq8_update.hip): O(N), so batch the changes; no f32 index is needed.  Neither the centroids nor the
    # quantiser is retrained: watch update_stats()["clamped"], the code values of added rows that fell outside the
    # quantiser's range.  The handle ends bit for bit in the state from_index(f32 index of the final corpus with the same
    # centroids and lists, ranges=self.quantizer()) would give, tags and attached vectors included.
    def _apply_update(self, drop_ids, x_add: Optional[torch.Tensor], add_ids, tags=None) -> Tuple[int, int]:
        if self.index is None:
            raise RuntimeError("Index not built.")
        dev = self._item_ids_dev.device

        def ids_dev(ids):
            if ids is None:
                return None, 0
            if isinstance(ids, torch.Tensor):
                t = ids.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
            else:
                t = torch.from_numpy(np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))).to(dev)
            return t, int(t.shape[0])

        drop, n_drop = ids_dev(drop_ids)
        add, n_add = ids_dev(add_ids)
        x = None
        if n_add or x_add is not None:
            if x_add.dim() != 2 or x_add.shape[1] != self.embed_dim:
                raise ValueError(f"Expected embeddings [n, {self.embed_dim}], got {tuple(x_add.shape)}")
            if x_add.shape[0] != n_add:
                raise ValueError(f"{x_add.shape[0]} embeddings for {n_add} item ids")
            x = x_add.to(device=dev, dtype=torch.float32).contiguous()
        if tags is not None:
            if self._tags is None:
                raise ValueError("tags= on an index without tags: call set_item_tags() first")
            tags = _tag_words(tags, n_add)
        old_ids, old_tags = self._item_ids_dev, self._tags
        if old_tags is not None and tags is None and n_add:
            # the appended rows take the word their id carried before the call, else 0 (positions found on the device)
            srt, order = torch.sort(old_ids)
            pos = torch.searchsorted(srt, add).clamp(max=old_ids.shape[0] - 1)
            hit, rows = (srt[pos] == add).cpu().numpy(), order[pos].cpu().numpy()
            tags = np.where(hit, old_tags[rows], np.uint32(0)).astype(np.uint32)
        t_dev = None
        if old_tags is not None and n_add:
            t_dev = torch.from_numpy(np.ascontiguousarray(tags).view(np.int32)).to(dev)
        n_old = self.index.ntotal
        out = torch.empty(n_old + n_add, dtype=torch.int64, device=dev)
        n_total, n_dropped, n_clamped = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        bad_id, bad_kind = C.c_int64(0), C.c_int(0)
        entry = self._update_entry()
        rc = getattr(L.lib(), entry)(self.index._h, self._item_ids_dev.data_ptr(), L.ptr(drop) if n_drop else None,
                                     n_drop, L.ptr(x) if n_add else None, L.ptr(add) if n_add else None,
                                     L.ptr(t_dev), n_add, out.data_ptr(), C.byref(n_total), C.byref(n_dropped),
                                     C.byref(n_clamped), C.byref(bad_id), C.byref(bad_kind), L.stream_ptr())
        if rc != 0 and bad_kind.value != 0:
            raise ValueError(L.lib().rihip_last_error().decode("utf-8", "replace"))
        L.check(rc, entry[6:])
        if n_dropped.value == 0 and n_add == 0:
            return 0, 0
        self._last_clamped = int(n_clamped.value)
        self._log_update(int(n_dropped.value), n_add)
        self._item_ids_dev = out[:n_total.value]
        self.item_ids = self._item_ids_dev.cpu().numpy()
        self._id_map_stale = True
        if old_tags is not None:
            # the handle moved its own copy of the words inside the repack; the host mirror follows
            keep = np.ones(n_old, dtype=bool) if n_drop == 0 else (~torch.isin(old_ids, drop)).cpu().numpy()
            self._tags = np.ascontiguousarray(np.concatenate([old_tags[keep]] + ([tags] if n_add else [])), dtype=np.uint32)
            assert self._tags.shape[0] == n_total.value
        return int(n_dropped.value), n_add

    def _update_entry(self) -> str:
        """the C entry point _apply_update calls (PQIndex: its own, once frozen_updates is on)"""
        return self._UPDATE

    def _log_update(self, n_dropped: int, n_add: int) -> None:
        logger.info("SQ8 index updated: %d rows dropped, %d added, %d code values clamped", n_dropped, n_add,
                    self._last_clamped)

    def _normalised(self, embeddings: np.ndarray) -> torch.Tensor:
        embeddings = np.asarray(embeddings)
        if embeddings.dtype != np.float32:
            raise ValueError("Embeddings must be float32")
        if embeddings.ndim != 2 or embeddings.shape[1] != self.embed_dim:
            raise ValueError(f"Expected embeddings [n, {self.embed_dim}], got {embeddings.shape}")
        norms = np.linalg.norm(embeddings, axis=1, keepdims=True)
        return torch.from_numpy(np.ascontiguousarray(embeddings / np.maximum(norms, 1e-8), dtype=np.float32)).to(L.device())

    def add_items(self, embeddings: np.ndarray, item_ids, tags=None) -> int:
        """Append f32 [n, embed_dim] rows (normalised as build_ivf_index does) as rows N .. N+n-1 with these ids; -> n.
        ValueError for an id that is already stored or repeated.  tags: uint32 [n] tag words of the new rows of a tagged
        index (0 when omitted).  The rows are encoded with the index's own quantiser, which is not retrained."""
        if self.index is None:
            raise RuntimeError("Index not built.")
        return self.add_items_device(self._normalised(embeddings), item_ids, tags=tags)

    def add_items_device(self, x_dev: torch.Tensor, item_ids, tags=None) -> int:
        """add_items for rows that are already normalised and on the device"""
        return self._apply_update(None, x_dev, item_ids, tags)[1]

    def remove_items(self, item_ids) -> int:
        """Remove the stored items with these ids (ids that are not stored are ignored, as faiss remove_ids does);
        surviving rows keep their relative order and are renumbered densely.  -> number of items removed"""
        return self._apply_update(item_ids, None, None)[0]

    def update_items(self, embeddings: np.ndarray, item_ids, tags=None) -> Tuple[int, int]:
        """Upsert in one repack: a stored id is dropped and its new vector appended, an unknown id is appended; the
        result is that of remove_items(ids) followed by add_items(embeddings, ids).  -> (replaced, added).  tags: uint32
        [n] tag words of these ids on a tagged index; omitted, a replaced id keeps its word and a new id gets 0."""
        if self.index is None:
            raise RuntimeError("Index not built.")
        replaced, n = self._apply_update(item_ids, self._normalised(embeddings), item_ids, tags)
        return replaced, n - replaced

    def assign_lists(self, x_dev: torch.Tensor) -> torch.Tensor:
        """int32 [n] on device: the list each f32 [n,d] device row would be added to (arg-max inner product with the
        centroids, lowest list on ties; all 0 for an index encoded from an exact FAISSIndex)."""
        h = self._built()
        x = x_dev.to(device=L.device(), dtype=torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != self.embed_dim:
            raise ValueError(f"Expected embeddings [n, {self.embed_dim}], got {tuple(x.shape)}")
        out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
        if x.shape[0]:
            L.check(L.lib().rihip_sq8_update_assign(h._h, x.data_ptr(), x.shape[0], out.data_ptr(), L.stream_ptr()),
                    "sq8_update_assign")
        return out

    def update_stats(self) -> Dict:
        """cumulative since the handle was made: updates that changed the index, rows dropped, rows added, and the code
        values of added rows that the frozen quantiser clamped to +-127 (its drift signal)"""
        out = (C.c_int64 * 4)()
        L.check(L.lib().rihip_sq8_update_stats(self._built()._h, out), "sq8_update_stats")
        return {"updates": int(out[0]), "dropped": int(out[1]), "added": int(out[2]), "clamped": int(out[3]),
                "last_clamped": self._last_clamped}

    # -- item tags (filtered retrieval; FAISSIndex's semantics and error texts) ---------------------------------------
    def _push_tags(self) -> None:
        t = None if self._tags is None else torch.from_numpy(self._tags.view(np.int32)).to(L.device())
        L.check(L.lib().rihip_sq8_filter_set_tags(self.index._h, L.ptr(t), L.stream_ptr()), "sq8_filter_set_tags")

    def set_item_tags(self, tags, item_ids=None) -> None:
        """Give every stored item a 32-bit tag word.  tags uint32 [ntotal] in row order; with item_ids, tags[i] belongs to
        item_ids[i] and items that are not named keep their word (0 on an index that had none).  ValueError for an id
        that is not stored.  Tags are not saved: a loaded index has none."""
        if self.index is None:
            raise RuntimeError("Index not built.")
        n = int(self.item_ids.shape[0])
        if item_ids is None:
            new = _tag_words(tags, n)
        else:
            ids = np.asarray(item_ids, dtype=np.int64).reshape(-1)
            t = _tag_words(tags, ids.shape[0])
            order = np.argsort(self.item_ids, kind="stable")
            pos = np.minimum(np.searchsorted(self.item_ids[order], ids), n - 1)
            rows = order[pos]
            missing = self.item_ids[rows] != ids
            if missing.any():
                raise ValueError(f"item id {int(ids[missing][0])} is not stored")
            new = self._tags.copy() if self._tags is not None else np.zeros(n, dtype=np.uint32)
            new[rows] = t
        self._tags = new
        self._push_tags()

    def item_tags(self) -> Optional[np.ndarray]:
        """uint32 [ntotal] tag words in row order (None without tags)"""
        return None if self._tags is None else self._tags.copy()

    def clear_item_tags(self) -> None:
        self._tags = None
        if self.index is not None:
            self._push_tags()

    @property
    def has_item_tags(self) -> bool:
        return self.index is not None and bool(L.lib().rihip_sq8_filter_has_tags(self.index._h))

    def filtered_stats(self) -> Tuple[int, int]:
        """(queries searched with an item_filter, of those re-done dense by the thresholded pass) since the handle was made"""
        out = (C.c_int64 * 2)()
        L.check(L.lib().rihip_sq8_filter_stats(self._built()._h, out), "sq8_filter_stats")
        return int(out[0]), int(out[1])

    def _pred(self, item_filter, nq: int, device) -> Tuple[torch.Tensor, int]:
        """item_filter in any of FAISSIndex's forms -> (int32 device words, stride 3 or 0); host-only checks first"""
        if self._tags is None:
            raise ValueError("item_filter needs item tags: call set_item_tags() first")
        if isinstance(item_filter, tuple) and item_filter in self._pred_cache:
            return self._pred_cache[item_filter], 0
        pred, stride = _filter_device(item_filter, nq, device)
        if stride == 0 and isinstance(item_filter, tuple) and len(self._pred_cache) < 1024:
            self._pred_cache[item_filter] = pred
        return pred, stride

    # -- refined search: the f32 vectors next to the codes ------------------------------------------------------------
    def attach_vectors(self, faiss_index: FAISSIndex) -> None:
        """Copy the f32 vectors of the FAISSIndex this index was encoded from (it may be dropped afterwards).  An index
        with other rows, another row order or other lists -- one updated since the encode included -- is refused
        (RuntimeError) and leaves this index as it was."""
        h = self._built()
        if not isinstance(faiss_index, FAISSIndex):
            raise ValueError(f"SQ8Index.attach_vectors needs a FAISSIndex, got {type(faiss_index).__name__}")
        if faiss_index.index is None:
            raise RuntimeError("Index not built.")
        if faiss_index.search_pending():
            raise RuntimeError("a deferred search is pending: call finish_search() before attaching the index")
        L.check(L.lib().rihip_sq8_refine_attach_vectors(h._h, faiss_index.index._h, L.stream_ptr()), "sq8_refine_attach_vectors")

    def drop_vectors(self) -> None:
        L.check(L.lib().rihip_sq8_refine_drop_vectors(self._built()._h), "sq8_refine_drop_vectors")

    @property
    def has_vectors(self) -> bool:
        return self.index is not None and bool(L.lib().rihip_sq8_refine_has_vectors(self.index._h))

    def set_refine(self, factor: Optional[float]) -> None:
        """The refine factor of every search that does not name one (None: plain 8-bit search, the default).  Sticky, so
        a serve chain that calls batch_search_device(q, k, normalized=True) gets refined candidates and their f32
        scores."""
        f = _factor(factor)
        if f is not None and not self.has_vectors:
            raise RuntimeError("SQ8Index.set_refine: no vectors attached (from_index(keep_vectors=True) or attach_vectors)")
        self._refine = f

    def refine_ranges(self) -> Tuple[np.ndarray, np.ndarray]:
        """(e, a): f64 [embed_dim] each -- the largest decode error and the largest magnitude of every column"""
        h = self._built()
        e = np.empty(self.embed_dim, dtype=np.float64)
        a = np.empty(self.embed_dim, dtype=np.float64)
        L.check(L.lib().rihip_sq8_refine_get_ranges(h._h, e.ctypes.data, a.ctypes.data), "sq8_refine_get_ranges")
        return e, a

    def _k_scan(self, k: int, factor: float) -> int:
        return min(max(k, int(math.ceil(factor * k))), int(L.lib().rihip_ip_index_max_k()))

    def _built(self) -> _SQ8Handle:
        if self.index is None:
            raise RuntimeError("Index not built. Call SQ8Index.from_index() first.")
        return self.index

    # -- trained state ----------------------------------------------------------------------------------------------
    def quantizer(self) -> Tuple[np.ndarray, np.ndarray]:
        """(centre, scale): f32 [embed_dim] each"""
        h = self._built()
        m = np.empty(self.embed_dim, dtype=np.float32)
        s = np.empty(self.embed_dim, dtype=np.float32)
        L.check(L.lib().rihip_sq8_index_get_quantizer(h._h, m.ctypes.data, s.ctypes.data), "sq8_index_get_quantizer")
        return m, s

    def codes(self) -> np.ndarray:
        """int8 [N, embed_dim]: the stored codes in insertion order"""
        h = self._built()
        c = np.empty((h.ntotal, self.embed_dim), dtype=np.int8)
        L.check(L.lib().rihip_sq8_index_get_codes(h._h, c.ctypes.data), "sq8_index_get_codes")
        return c

    def reconstruct(self) -> np.ndarray:
        """f32 [N, embed_dim]: the decoded vectors centre + scale * code in insertion order"""
        h = self._built()
        x = np.empty((h.ntotal, self.embed_dim), dtype=np.float32)
        L.check(L.lib().rihip_sq8_index_reconstruct(h._h, x.ctypes.data), "sq8_index_reconstruct")
        return x

    def encode_queries(self, queries: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """the search's first stage on f32 [nq, embed_dim] device queries (taken as they are): (n int16 [nq, embed_dim],
        t f32 [nq], b f64 [nq]) on the device"""
        h = self._built()
        q = self._queries(queries)
        nq = q.shape[0]
        n = torch.empty((nq, self.embed_dim), dtype=torch.int16, device=q.device)
        t = torch.empty((nq,), dtype=torch.float32, device=q.device)
        b = torch.empty((nq,), dtype=torch.float64, device=q.device)
        L.check(L.lib().rihip_sq8_index_encode_queries(h._h, q.data_ptr(), nq, n.data_ptr(), t.data_ptr(), b.data_ptr(),
                                                       L.stream_ptr()), "sq8_index_encode_queries")
        return n, t, b

    # -- search -----------------------------------------------------------------------------------------------------
    def _queries(self, queries: torch.Tensor) -> torch.Tensor:
        if not isinstance(queries, torch.Tensor) or queries.dim() != 2 or queries.shape[1] != self.embed_dim:
            shape = tuple(queries.shape) if hasattr(queries, "shape") else type(queries).__name__
            raise ValueError(f"SQ8Index: queries must be a tensor [nq, {self.embed_dim}], got {shape}")
        if queries.shape[0] == 0:
            raise ValueError("SQ8Index: no queries")
        return queries.to(device=L.device(), dtype=torch.float32).contiguous()

    def _refined_device(self, q_dev: torch.Tensor, k: int, k_scan: int, item_ids: bool, mode: int, item_filter=None):
        """(scores f32 [nq, k], rows or ids i64 [nq, k], cert u8 [nq], bound f64 [nq]) of one refined search"""
        h = self._built()
        lib = L.lib()
        if not self.has_vectors:
            raise RuntimeError("SQ8Index: refine needs the f32 vectors (from_index(keep_vectors=True) or attach_vectors)")
        nq = q_dev.shape[0]
        pred = None if item_filter is None else self._pred(item_filter, nq, q_dev.device)
        L.check(lib.rihip_sq8_index_set_id_map(h._h, self._item_ids_dev.data_ptr() if item_ids else None),
                "sq8_index_set_id_map")
        scores = torch.empty((nq, k), dtype=torch.float32, device=q_dev.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=q_dev.device)
        cert = torch.empty((nq,), dtype=torch.uint8, device=q_dev.device)
        bound = torch.empty((nq,), dtype=torch.float64, device=q_dev.device)
        if pred is not None:
            L.check(lib.rihip_sq8_refine_search_filtered(h._h, q_dev.data_ptr(), nq, k, k_scan, mode, pred[0].data_ptr(), pred[1],
                                                         scores.data_ptr(), rows.data_ptr(), cert.data_ptr(), bound.data_ptr(),
                                                         L.stream_ptr()), "sq8_refine_search_filtered")
            return scores, rows, cert, bound
        L.check(lib.rihip_sq8_refine_search(h._h, q_dev.data_ptr(), nq, k, k_scan, mode, scores.data_ptr(),
                                                   rows.data_ptr(), cert.data_ptr(), bound.data_ptr(), L.stream_ptr()),
                "sq8_refine_search")
        return scores, rows, cert, bound

    def _search_device(self, q_dev: torch.Tensor, k: int, item_ids: bool, mode: int, return_int: bool, refine=_DEFAULT,
                       return_cert: bool = False, item_filter=None):
        h = self._built()
        lib = L.lib()
        factor = self._refine if refine is _DEFAULT else _factor(refine)
        if k < 1:
            raise ValueError(f"SQ8Index: k={k} must be at least 1")
        if k > int(lib.rihip_ip_index_max_k()):
            raise ValueError(f"k={k} exceeds the device select buffer ({int(lib.rihip_ip_index_max_k())})")
        if factor is not None:
            if return_int:
                raise ValueError("SQ8Index: return_int gives the 8-bit search's integer scores; a refined search has none")
            out = self._refined_device(q_dev, k, self._k_scan(k, factor), item_ids, mode, item_filter)
            return out if return_cert else out[:2]
        if return_cert:
            raise ValueError("SQ8Index: return_cert needs a refined search (refine= or set_refine)")
        nq = q_dev.shape[0]
        pred = None if item_filter is None else self._pred(item_filter, nq, q_dev.device)
        L.check(lib.rihip_sq8_index_set_id_map(h._h, self._item_ids_dev.data_ptr() if item_ids else None),
                "sq8_index_set_id_map")
        scores = torch.empty((nq, k), dtype=torch.float32, device=q_dev.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=q_dev.device)
        ints = torch.empty((nq, k), dtype=torch.int32, device=q_dev.device) if return_int else None
        if pred is not None:
            L.check(lib.rihip_sq8_filter_search(h._h, q_dev.data_ptr(), nq, k, mode, pred[0].data_ptr(), pred[1], scores.data_ptr(),
                                                rows.data_ptr(), L.ptr(ints), L.stream_ptr()), "sq8_filter_search")
            return (scores, rows, ints) if return_int else (scores, rows)
        L.check(lib.rihip_sq8_index_search(h._h, q_dev.data_ptr(), nq, k, mode, scores.data_ptr(), rows.data_ptr(),
                                           L.ptr(ints), L.stream_ptr()), "sq8_index_search")
        return (scores, rows, ints) if return_int else (scores, rows)

    def _scan_excluding(self, q: torch.Tensor, k: int, seen, uid: Optional[torch.Tensor], item_filter, mode: int,
                        return_int: bool, refine, return_cert: bool, row_of: Optional[torch.Tensor] = None,
                        k_scan: Optional[int] = None):
        """exclusion="scan": one rihip_sq8_exclude_search (with a refine factor: rihip_sq8_refine_search_excluding at
        k_scan = ceil(factor * k)) over the whole batch; the outputs of _search_device, item ids in place of rows"""
        h = self._built()
        lib = L.lib()
        factor = self._refine if refine is _DEFAULT else _factor(refine)
        if k < 1:
            raise ValueError(f"SQ8Index: k={k} must be at least 1")
        if k > int(lib.rihip_ip_index_max_k()):
            raise ValueError(f"k={k} exceeds the device select buffer ({int(lib.rihip_ip_index_max_k())})")
        if factor is not None and return_int:
            raise ValueError("SQ8Index: return_int gives the 8-bit search's integer scores; a refined search has none")
        if factor is None and return_cert:
            raise ValueError("SQ8Index: return_cert needs a refined search (refine= or set_refine)")
        if factor is not None and not self.has_vectors:
            raise RuntimeError("SQ8Index: refine needs the f32 vectors (from_index(keep_vectors=True) or attach_vectors)")
        nq = q.shape[0]
        row_of = self._row_of_device() if row_of is None else self._check_row_of(row_of)
        pred = (None, 0) if item_filter is None else self._pred(item_filter, nq, q.device)
        L.check(lib.rihip_sq8_index_set_id_map(h._h, self._item_ids_dev.data_ptr()), "sq8_index_set_id_map")
        scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
        seen_args = (L.ptr(uid), seen.offsets.data_ptr(), seen.n_users, seen.items.data_ptr(), row_of.data_ptr(),
                     row_of.shape[0], L.ptr(pred[0]), pred[1])
        if factor is not None:
            cert = torch.empty((nq,), dtype=torch.uint8, device=q.device)
            bound = torch.empty((nq,), dtype=torch.float64, device=q.device)
            ks = self._k_scan(k, factor) if k_scan is None else k_scan
            L.check(lib.rihip_sq8_refine_search_excluding(h._h, q.data_ptr(), nq, k, ks, mode, *seen_args, scores.data_ptr(),
                                                          ids.data_ptr(), cert.data_ptr(), bound.data_ptr(), L.stream_ptr()),
                    "sq8_refine_search_excluding")
            return (scores, ids, cert, bound) if return_cert else (scores, ids)
        ints = torch.empty((nq, k), dtype=torch.int32, device=q.device) if return_int else None
        L.check(lib.rihip_sq8_exclude_search(h._h, q.data_ptr(), nq, k, mode, *seen_args, scores.data_ptr(), ids.data_ptr(),
                                             L.ptr(ints), L.stream_ptr()), "sq8_exclude_search")
        return (scores, ids, ints) if return_int else (scores, ids)

    def _excluding(self, q: torch.Tensor, k: int, seen, user_ids, item_filter, mode: int, return_int: bool, refine,
                   return_cert: bool, exclusion: str = "overfetch"):
        """the search without each query's seen items: the over-fetched k_eff of seen.plan_overfetch is what is searched
        (and, with a refine factor, refined: k_scan = ceil(factor * k_eff)); a certificate then speaks of the over-fetched
        list, whose first k unseen entries are the result.  exclusion="scan": _scan_excluding instead"""
        if check_exclusion(exclusion) == "scan":
            return self._scan_excluding(q, k, seen, seen_user_ids(user_ids, q.shape[0], q.device), item_filter, mode,
                                        return_int, refine, return_cert)
        if return_int:
            raise ValueError("SQ8Index: return_int is not available with exclude (the device filter moves scores and ids only)")

        def run(qq, kk, flt):
            return self._search_device(qq, kk, True, mode, False, refine, return_cert, flt)
        return self._search_excluding(q, k, seen, user_ids, item_filter, search=run)

    def search(self, query_vector: np.ndarray, k: int = 500, refine=_DEFAULT, exclude_items=None, item_filter=None,
               exclusion: str = "overfetch") -> Tuple[np.ndarray, np.ndarray]:
        """exclude_items: item ids that must not be returned; item_filter: (any_of, all_of, none_of) over the items' tag
        words; exclusion: how exclude_items are kept out -- all as in batch_search_device"""
        check_exclusion(exclusion)
        h = self._built()
        query = np.atleast_2d(query_vector).astype(np.float32)
        if query.shape[1] != self.embed_dim:
            raise ValueError(f"SQ8Index: query width {query.shape[1]}, index width {self.embed_dim}")
        query = query / np.maximum(np.linalg.norm(query, axis=1, keepdims=True), 1e-8)
        k = min(k, h.ntotal)
        q_dev = torch.from_numpy(np.ascontiguousarray(query[:1])).to(L.device())
        if exclude_items is not None:
            from .seen import SeenItems
            ex = np.asarray(exclude_items, dtype=np.int64).reshape(-1)
            seen = SeenItems.from_pairs(np.zeros(ex.shape[0], np.int64), ex, 1)
            if exclusion == "scan":
                scores, ids = self._scan_excluding(q_dev, k, seen, None, item_filter, 0, False, refine, False)
                distances, ids = scores[0].cpu().numpy(), ids[0].cpu().numpy()
                return distances[ids >= 0], ids[ids >= 0]
            scores, ids = self._search_excluding(
                q_dev, k, seen, None, item_filter,
                search=lambda qq, kk, flt: self._search_device(qq, kk, True, 0, False, refine, False, flt))
            distances, ids = scores[0].cpu().numpy(), ids[0].cpu().numpy()
            return distances[ids >= 0], ids[ids >= 0]
        scores, rows = self._search_device(q_dev, k, False, 0, False, refine, item_filter=item_filter)
        distances, idx = scores[0].cpu().numpy(), rows[0].cpu().numpy()
        valid = idx >= 0
        return distances[valid], self.item_ids[idx[valid]]

    def batch_search(self, query_vectors: np.ndarray, k: int = 500, refine=_DEFAULT, return_cert: bool = False,
                     exclude=None, user_ids=None, item_filter=None, exclusion: str = "overfetch"):
        """(scores, item ids) as NumPy arrays; return_cert=True appends (cert u8 [nq], bound f64 [nq]); exclude /
        user_ids / item_filter / exclusion as in batch_search_device"""
        check_exclusion(exclusion)
        h = self._built()
        queries = np.asarray(query_vectors).astype(np.float32)
        if queries.ndim != 2 or queries.shape[1] != self.embed_dim:
            raise ValueError(f"SQ8Index: queries must be [nq, {self.embed_dim}], got {queries.shape}")
        queries = queries / np.maximum(np.linalg.norm(queries, axis=1, keepdims=True), 1e-8)
        k = min(k, h.ntotal)
        q_dev = torch.from_numpy(np.ascontiguousarray(queries)).to(L.device())
        if exclude is not None:
            out = self._excluding(self._queries(q_dev), k, exclude, user_ids, item_filter, 0, False, refine, return_cert,
                                  exclusion)
        else:
            out = self._search_device(self._queries(q_dev), k, True, 0, False, refine, return_cert, item_filter)
        return tuple(t.cpu().numpy() for t in out)

    def batch_search_device(self, queries: torch.Tensor, k: int = 500, normalized: bool = False, mode: str = "auto",
                            return_int: bool = False, refine=_DEFAULT, return_cert: bool = False, exclude=None,
                            user_ids=None, item_filter=None, exclusion: str = "overfetch"):
        """queries f32 [nq, embed_dim] on the device -> (scores f32, item ids i64) [nq, k] on the device, -1 padded;
        return_int=True appends the integer scores i32 [nq, k].  mode: "auto", "dense" or "thresholded" (the same bytes
        from each; "thresholded" synchronises the stream for its completeness check).

        refine: a factor >= 1 re-scores the best k_scan = min(max(k, ceil(factor * k)), max_k) candidates of the 8-bit
        search exactly in f32 and returns the top k of those with their f32 scores; None is the plain search; left
        out, the factor of set_refine.  return_cert=True appends (cert u8 [nq], bound f64 [nq]): cert = 1 proves the
        list is the exact top k of the probed lists.

        item_filter (needs set_item_tags): a 3-tuple of ints (any_of, all_of, none_of) shared by the batch, a uint32
        array [nq,3], or an int32 device tensor [nq,3] read as a bit pattern, as FAISSIndex.batch_search_device.  The
        result is the exact top k, by integer score, of the passing items of the probed lists, -1 padded when fewer
        pass; (0,0,0) equals the plain search.  The predicate is tested inside the int8 scan in every mode.  With
        refine the filtered search is stage 1 and cert = 1 proves the exact top k of the passing probed items.
        ValueError without tags or on a bad shape.

        exclude (a seen.SeenItems) with user_ids [nq]: query q never returns an item of row user_ids[q] of the store
        (user_ids None: of row q); host user ids are searched in groups by how far each has to over-fetch (seen.plan_overfetch), a device tensor as
        one group at the store's longest list.  The over-fetched k_eff is what is searched and, with refine, refined.
        With item_filter the result is filter AND not-seen.  Not with return_int.

        exclusion="scan" (opt-in; "overfetch", the default, is the paragraph above): the seen items are excluded inside
        the int8 scan -- one bit per (query, row) of a mask built on the device from the store, tested where the tag
        predicate is tested.  One search of the whole batch in every mode, no over-fetch and no limit on k plus a user's
        list; the result is the first k of the probed rows by (S descending, row ascending) that are not seen (and
        pass), bit for bit the scores the plain search reports for those rows; return_int works.  With refine the
        excluded search at k_scan = ceil(factor * k) is stage 1, and cert = 1 proves the exact top k of the probed rows
        that are not seen (and pass).  Item ids must lie in [0, 2**31 - 1).  Any other value: ValueError."""
        check_exclusion(exclusion)
        h = self._built()
        m = _mode(mode)
        q = self._queries(queries)
        if not normalized:
            q = q / torch.clamp(torch.linalg.norm(q, dim=1, keepdim=True), min=1e-8)
        if exclude is not None:
            return self._excluding(q, min(k, h.ntotal), exclude, user_ids, item_filter, m, return_int, refine, return_cert,
                                   exclusion)
        return self._search_device(q, min(k, h.ntotal), True, m, return_int, refine, return_cert, item_filter)

    def search_rows_device(self, queries: torch.Tensor, k: int, mode: str = "auto", return_int: bool = False, refine=_DEFAULT,
                           return_cert: bool = False, item_filter=None):
        """batch_search_device on queries taken as they are, returning ROWS (insertion order) instead of item ids and k
        as given (padded beyond ntotal)"""
        return self._search_device(self._queries(queries), k, False, _mode(mode), return_int, refine, return_cert, item_filter)

    def search_certified(self, queries: torch.Tensor, k: int = 500, start: float = 2.0, normalized: bool = False,
                         item_filter=None, exclude=None, user_ids=None, exclusion: str = "overfetch"):
        """Refine at factor `start`, then repeat only the queries without a certificate with k_scan doubled until they
        have one or k_scan reaches the select buffer's size.  -> (scores f32 [nq, k], item ids i64 [nq, k], cert u8 [nq])
        on the device; a query whose flag is still 0 is reported as it is, not repaired.  item_filter: as in
        batch_search_device; a repeat carries the predicates of the queries it repeats.  exclude / user_ids with
        exclusion="scan": every stage 1 is the excluded search, so a certificate speaks of the probed rows the user has
        not seen (the over-fetch route has no certified form: ValueError)."""
        check_exclusion(exclusion)
        if exclude is not None and exclusion != "scan":
            raise ValueError('SQ8Index.search_certified: exclude needs exclusion="scan"')
        h = self._built()
        f = _factor(start)
        if f is None:
            raise ValueError("SQ8Index.search_certified: start must be a number >= 1")
        q = self._queries(queries)
        if not normalized:
            q = q / torch.clamp(torch.linalg.norm(q, dim=1, keepdim=True), min=1e-8)
        max_k = int(L.lib().rihip_ip_index_max_k())
        k = min(k, h.ntotal)
        if k < 1 or k > max_k:
            raise ValueError(f"SQ8Index: k={k} outside 1..{max_k}")
        k_scan = self._k_scan(k, f)
        uid = None if exclude is None else seen_user_ids(np.arange(q.shape[0]) if user_ids is None else user_ids,
                                                         q.shape[0], q.device)

        def refined(qq, ks, flt, sel=None):
            if exclude is None:
                return self._refined_device(qq, k, ks, True, 0, flt)
            return self._scan_excluding(qq, k, exclude, uid if sel is None else uid[sel].contiguous(), flt, 0, False, 1.0,
                                        True, k_scan=ks)
        scores, ids, cert, _ = refined(q, k_scan, item_filter)
        while k_scan < max_k:
            todo = torch.nonzero(cert == 0).flatten()
            if todo.numel() == 0:
                break
            k_scan = min(2 * k_scan, max_k)
            s2, i2, c2, _ = refined(q[todo].contiguous(), k_scan,
                                    None if item_filter is None else _sub_filter(item_filter, todo), todo)
            scores[todo], ids[todo], cert[todo] = s2, i2, c2
        return scores, ids, cert

    # -- the calls a serve chain makes on its index; an SQ8 search has no pending state -------------------------------
    def set_deferred_check(self, enable: bool) -> None:
        self._built()

    def finish_search(self) -> int:
        return 0

    def search_pending(self) -> bool:
        return False

    def last_fail_count(self) -> int:
        return 0

    # -- persistence ------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        h = self._built()
        save_path = Path(path)
        save_path.parent.mkdir(parents=True, exist_ok=True)
        L.check(getattr(L.lib(), self._SAVE)(h._h, str(save_path).encode()), self._SAVE[6:])
        meta = {
            "item_ids": self.item_ids,
            "item_id_to_faiss_idx": self._item_id_to_faiss_idx,
            "embed_dim": self.embed_dim,
            "n_lists": self.n_lists,
            "n_probe": self.n_probe,
        }
        with open(save_path.with_suffix(".meta.pkl"), "wb") as f:
            pickle.dump(meta, f)
        logger.info("Saved %s index to %s", self._KIND, save_path)

    @classmethod
    def _loader(cls, load_path) -> str:
        """the C entry point that reads the file (PQIndex picks between its two formats)"""
        return cls._LOAD

    @classmethod
    def load(cls, path: str) -> "SQ8Index":
        load_path = Path(path)
        if not load_path.exists():
            raise FileNotFoundError(f"{cls._KIND} index not found at {load_path}")
        with open(load_path.with_suffix(".meta.pkl"), "rb") as f:
            meta = pickle.load(f)  # sidecar written by save() above
        obj = cls(embed_dim=meta["embed_dim"], n_lists=meta["n_lists"], n_probe=meta["n_probe"])
        h = C.c_void_p()
        loader = cls._loader(load_path)
        L.check(getattr(L.lib(), loader)(str(load_path).encode(), C.byref(h)), loader[6:])
        obj.index = _SQ8Handle(h.value, obj)
        obj.index.nprobe = meta["n_probe"]
        obj.item_ids = np.asarray(meta["item_ids"], dtype=np.int64)
        if obj.item_ids.shape[0] != obj.index.ntotal:
            raise ValueError(f"{load_path}: {obj.index.ntotal} vectors, {obj.item_ids.shape[0]} item ids in the sidecar")
        obj._item_ids_dev = torch.from_numpy(obj.item_ids).to(L.device())
        obj._item_id_to_faiss_idx = meta["item_id_to_faiss_idx"]
        return obj

    # -- utilities --------------------------------------------------------------------------------------------------
    def search_stats(self) -> Tuple[int, int]:
        """(queries searched by the thresholded pass, of those re-done dense) since the handle was made"""
        out = (C.c_int64 * 3)()
        L.check(L.lib().rihip_sq8_index_stats(self._built()._h, out), "sq8_index_stats")
        return int(out[0]), int(out[1])

    def stats(self) -> Dict:
        if self.index is None:
            return {"status": "not built"}
        out = (C.c_int64 * 3)()
        L.check(L.lib().rihip_sq8_index_stats(self.index._h, out), "sq8_index_stats")
        n = int(self.index.ntotal)
        bpv = 64 if self.embed_dim <= 64 else 128
        f32_row = 4 * (32 if self.embed_dim <= 32 else bpv)      # the f32 index stores rows at its kernel width
        return {
            "n_vectors": n,
            "embed_dim": self.embed_dim,
            "n_lists": self.index.nlist,
            "n_probe": self.n_probe,
            "metric": "inner_product",
            "n_item_ids": len(self.item_ids) if self.item_ids is not None else 0,
            "bytes_per_vector": bpv,
            "compression": f32_row / bpv,
            "device_bytes": int(out[2]),
            "queries_thresholded": int(out[0]),
            "queries_redone": int(out[1]),
            "has_vectors": self.has_vectors,
            "has_item_tags": self.has_item_tags,
            "refine": self._refine,
        }

    def set_n_probe(self, n_probe: int) -> None:
        if int(n_probe) < 1:
            raise ValueError(f"SQ8Index: n_probe={n_probe} must be at least 1")
        self.n_probe = int(n_probe)
        if self.index is not None:
            self.index.nprobe = int(n_probe)
