"""Drop-in FAISSIndex backed by the gfx950 inner-product index (no faiss).

Mirrors the reference's src/models/faiss_index.py (:23-228): constructor, build_ivf_index,
search, batch_search, save/load (+ ``<stem>.meta.pkl`` sidecar with the same keys), stats,
set_n_probe, and the ``index`` attribute (``index.ntotal``, writable ``index.nprobe``) that
tests/test_models.py:170-171,:223 read.  Error types/messages follow the reference.

Index files: ``save(path)`` writes the library's own "RIHIPIDX" format by default and a FAISS ``IndexIVFFlat`` /
``IndexFlatIP`` file with ``format="faiss"``; ``load(path)`` sniffs the magic and reads either (faiss_io.py; the FAISS
layout is restated from faiss 1.7.x and unverifiable offline: parity unpinned).  The k-means trainer is
the library's own, so the IVF list membership of an index TRAINED here differs from one trained by faiss; an index
LOADED from a faiss file keeps faiss's centroids and lists.  Limits the reference (faiss) does not have: embed_dim <= 128
(any width: rows are zero-padded to the 32/64/128 kernel width inside the handle), n_lists <= 2048, k <= 16384.

Filtered retrieval (not in the reference; faiss has it as ``SearchParameters.sel``): ``set_item_tags`` gives every item a
32-bit tag word and ``item_filter=(any_of, all_of, none_of)`` restricts a search to the items whose word passes, tested
inside the index scan.
"""
from __future__ import annotations

import ctypes as C
import logging
import pickle
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .exclusion import ExcludingSearch, check_exclusion, seen_user_ids

logger = logging.getLogger(__name__)

FAISS_AVAILABLE = True  # name kept for callers that probe it


class _IndexHandle:
    """Owns one rihip ip_index; exposes the two faiss attributes the callers touch."""

    def __init__(self, handle: int, owner: "FAISSIndex"):
        self._h = C.c_void_p(handle)
        self._owner = owner

    @property
    def ntotal(self) -> int:
        return int(L.lib().rihip_ip_index_ntotal(self._h))

    @property
    def nprobe(self) -> int:
        return self._owner.n_probe

    @nprobe.setter
    def nprobe(self, v: int) -> None:
        self._owner.n_probe = int(v)
        L.check(L.lib().rihip_ip_index_set_nprobe(self._h, int(v)), "ip_index_set_nprobe")

    @property
    def is_ivf(self) -> bool:
        return bool(L.lib().rihip_ip_index_is_ivf(self._h))

    def __del__(self):
        try:
            if self._h:
                L.lib().rihip_ip_index_destroy(self._h)
                self._h = None
        except Exception:
            pass


def genre_tags(genre_matrix) -> np.ndarray:
    """uint32 [n]: bit g of word i is set iff genre_matrix[i, g] > 0 (at most 32 columns; the reference's 18 genres take
    bits 0-17 and leave bits 18-31 to the caller)"""
    g = genre_matrix.detach().cpu().numpy() if isinstance(genre_matrix, torch.Tensor) else np.asarray(genre_matrix)
    if g.ndim != 2 or g.shape[1] > 32:
        raise ValueError(f"genre matrix must be [n, <=32], got {g.shape}")
    bits = np.uint32(1) << np.arange(g.shape[1], dtype=np.uint32)
    return ((g > 0).astype(np.uint32) * bits[None, :]).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def _word(v) -> int:
    v = int(v)
    if not -(1 << 31) <= v < (1 << 32):
        raise ValueError(f"item_filter word {v} does not fit 32 bits")
    return v & 0xFFFFFFFF


def item_filter_words(item_filter, nq: int) -> np.ndarray:
    """item_filter as uint32 [nq, 3] words (any_of, all_of, none_of): a 3-tuple of ints is shared by the batch, an
    integer array or tensor [nq, 3] (or [3]) holds one predicate per query and is read as a bit pattern"""
    if isinstance(item_filter, torch.Tensor):
        item_filter = item_filter.detach().cpu().numpy()
    if isinstance(item_filter, (tuple, list)) and len(item_filter) == 3 and all(np.ndim(v) == 0 for v in item_filter):
        return np.tile(np.array([_word(v) for v in item_filter], dtype=np.uint32), (nq, 1))
    a = np.asarray(item_filter)
    if a.dtype.kind not in "iu":
        raise ValueError(f"item_filter must hold integers, got {a.dtype}")
    if a.shape == (3,):
        a = np.tile(a, (nq, 1))
    if a.shape != (nq, 3):
        raise ValueError(f"item_filter must be a 3-tuple or [{nq}, 3], got {a.shape}")
    if a.dtype.itemsize == 4:
        return np.ascontiguousarray(a).view(np.uint32)
    return np.array([[_word(v) for v in row] for row in a.tolist()], dtype=np.uint32).reshape(nq, 3)


def _filter_device(item_filter, nq: int, device) -> Tuple[torch.Tensor, int]:
    """-> (int32 device tensor of predicate words, stride between two queries' words: 3, or 0 = shared)"""
    if isinstance(item_filter, torch.Tensor) and item_filter.is_cuda:
        if item_filter.dtype != torch.int32 or tuple(item_filter.shape) != (nq, 3):
            raise ValueError(f"a device item_filter must be int32 [{nq}, 3], got {item_filter.dtype} "
                             f"{tuple(item_filter.shape)}")
        return item_filter.contiguous(), 3
    shared = isinstance(item_filter, (tuple, list)) and len(item_filter) == 3 and all(np.ndim(v) == 0 for v in item_filter)
    w = item_filter_words(item_filter, 1 if shared else nq)
    return torch.from_numpy(w.view(np.int32).copy()).to(device), 0 if shared else 3


def _sub_filter(item_filter, sel: torch.Tensor):
    """the predicates of the queries `sel` (a device index tensor) of a batch"""
    if isinstance(item_filter, (tuple, list)):
        return item_filter
    if isinstance(item_filter, torch.Tensor):
        return item_filter[sel.to(item_filter.device)]
    a = np.asarray(item_filter)
    return a if a.ndim == 1 else a[sel.cpu().numpy()]


def _list_stats(sizes: np.ndarray) -> Dict:
    sizes = np.asarray(sizes, dtype=np.int64)
    n, tot = int(sizes.shape[0]), int(sizes.sum())
    sq = int((sizes.astype(object) ** 2).sum()) if n else 0
    return {"n_lists": n, "min": int(sizes.min()) if n else 0, "max": int(sizes.max()) if n else 0,
            "mean": tot / n if n else 0.0, "empty": int((sizes == 0).sum()),
            "imbalance": n * sq / (tot * tot) if tot else 0.0}


class FAISSIndex(ExcludingSearch):
    _EXCL_ABI = {"mask_words": "rihip_ip_index_exclusion_mask_words", "mask": "rihip_ip_index_exclusion_mask",
                 "budget": "rihip_ip_index_set_exclusion_budget", "nonzero": "rihip_ip_index_exclusion_scratch_nonzero",
                 "stats": "rihip_ip_index_exclusion_stats"}

    def __init__(self, embed_dim: int = 64, n_lists: int = 100, n_probe: int = 10, exact: bool = False):
        """exact=True skips the IVF partition (brute-force inner product; not in the reference)."""
        self.embed_dim = embed_dim
        self.n_lists = n_lists
        self.n_probe = n_probe
        self.exact = exact
        self.index: Optional[_IndexHandle] = None
        self.item_ids: Optional[np.ndarray] = None
        self._id_map: Dict[int, int] = {}
        self._id_map_stale = False
        self._item_ids_dev: Optional[torch.Tensor] = None
        self._deferred = False
        self._deficit: Optional[torch.Tensor] = None
        self._tags: Optional[torch.Tensor] = None      # int32 bit patterns [ntotal] on the device, row order
        self._pred_cache: Dict[Tuple[int, int, int], torch.Tensor] = {}   # shared predicates already on the device
        self._vec_cache: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None   # item_vectors_device()

    @property
    def _item_id_to_faiss_idx(self) -> Dict[int, int]:
        """{item id: row}: the plain dict after a build or load; after add_items / remove_items / update_items it is
        rebuilt from item_ids on the first read (save() reads it), not inside the update"""
        if self._id_map_stale:
            self._id_map = {int(iid): row for row, iid in enumerate(self.item_ids.tolist())}
            self._id_map_stale = False
        return self._id_map

    @_item_id_to_faiss_idx.setter
    def _item_id_to_faiss_idx(self, value: Dict[int, int]) -> None:
        self._id_map = value
        self._id_map_stale = False

    # -- build (faiss_index.py:45-82) ---------------------------------------------------------
    def build_ivf_index(self, embeddings: np.ndarray, item_ids: List[int], kmeans_iters: int = 20,
                        seed: int = 1234) -> None:
        assert embeddings.dtype == np.float32, "Embeddings must be float32"
        assert embeddings.shape[1] == self.embed_dim, (
            f"Expected embed_dim={self.embed_dim}, got {embeddings.shape[1]}"
        )
        norms = np.linalg.norm(embeddings, axis=1, keepdims=True)
        embeddings = np.ascontiguousarray(embeddings / np.maximum(norms, 1e-8), dtype=np.float32)
        x_dev = torch.from_numpy(embeddings).to(L.device())
        self.build_from_device(x_dev, np.array(item_ids, dtype=np.int64), kmeans_iters=kmeans_iters, seed=seed)
        self._item_id_to_faiss_idx = {int(iid): idx for idx, iid in enumerate(item_ids)}

    def build_from_device(self, x_dev: torch.Tensor, item_ids: np.ndarray, kmeans_iters: int = 20,
                          seed: int = 1234, init_centroids: Optional[np.ndarray] = None,
                          centroids: Optional[np.ndarray] = None, assign: Optional[np.ndarray] = None) -> None:
        """Build from already-normalised f32 [N,d] rows on the device (no host round trip).

        init_centroids f32[n_lists,d]: k-means starts from these instead of seeded rows (kmeans_iters=0 partitions
        by them as they are).  centroids + assign int32[N]: inject a trained partition (a FAISS IndexIVFFlat file)."""
        lib = L.lib()
        n = x_dev.shape[0]
        assert x_dev.dtype == torch.float32 and x_dev.shape[1] == self.embed_dim and x_dev.is_contiguous()
        h = C.c_void_p()
        L.check(lib.rihip_ip_index_create(self.embed_dim, C.byref(h)), "ip_index_create")
        self.index = _IndexHandle(h.value, self)
        L.check(lib.rihip_ip_index_set_vectors(self.index._h, x_dev.data_ptr(), n, 1, L.stream_ptr()),
                "ip_index_set_vectors")
        if not self.exact:
            nlist = max(1, min(self.n_lists, n))
            logger.info("Training IVF index on %d vectors (n_lists=%d)...", n, nlist)
            if centroids is not None:
                c = np.ascontiguousarray(centroids, dtype=np.float32)
                a = np.ascontiguousarray(assign, dtype=np.int32)
                assert c.shape == (nlist, self.embed_dim) and a.shape == (n,)
                L.check(lib.rihip_ip_index_set_ivf(self.index._h, nlist, c.ctypes.data, a.ctypes.data, L.stream_ptr()),
                        "ip_index_set_ivf")
            elif init_centroids is not None:
                c = np.ascontiguousarray(init_centroids, dtype=np.float32)
                assert c.shape == (nlist, self.embed_dim)
                L.check(lib.rihip_ip_index_train_ivf_from(self.index._h, nlist, kmeans_iters, c.ctypes.data,
                                                          L.stream_ptr()), "ip_index_train_ivf_from")
            else:
                L.check(lib.rihip_ip_index_train_ivf(self.index._h, nlist, kmeans_iters, seed, L.stream_ptr()),
                        "ip_index_train_ivf")
        L.check(lib.rihip_ip_index_set_nprobe(self.index._h, int(self.n_probe)), "ip_index_set_nprobe")
        self.item_ids = np.asarray(item_ids, dtype=np.int64)
        self._item_ids_dev = torch.from_numpy(self.item_ids).to(x_dev.device)
        self._tags = None
        self._vec_cache = None
        logger.info("Index built: %d vectors, %d lists, probe=%d", self.index.ntotal, self.n_lists, self.n_probe)

    # -- live catalogue (faiss add_with_ids / remove_ids; not in the reference, which rebuilds offline) ----------
    # Every call is ONE repack of the corpus on the device under the existing centroids (csrc/index_update.hip): O(N),
    # so batch the changes.  Centroids are not retrained: watch list_stats()["imbalance"].  The handle ends bit for bit
    # in the state a from-scratch build of the final corpus with the same centroids would give.  Serving: an item id
    # outside the feature store's item table (a new item the store has not seen) is not an error in
    # rihip_rank_features_build -- it reads row 0 of the table, the reference's cold-start defaults.
    def _apply_update(self, drop_ids, x_add: Optional[torch.Tensor], add_ids, tags=None) -> Tuple[int, int]:
        if self.index is None:
            raise RuntimeError("Index not built.")
        if self.search_pending():
            raise RuntimeError("a deferred search is pending: call finish_search() before changing the index")
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
            tags = self._tags_dev(tags, n_add)
        n_old = self.index.ntotal
        old_ids, old_tags = self._item_ids_dev, self._tags
        out = torch.empty(n_old + n_add, dtype=torch.int64, device=dev)
        n_total, n_dropped, bad_id, bad_kind = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
        rc = L.lib().rihip_ip_index_update(self.index._h, self._item_ids_dev.data_ptr(), L.ptr(drop) if n_drop else None,
                                           n_drop, L.ptr(x) if n_add else None, L.ptr(add) if n_add else None, n_add,
                                           out.data_ptr(), C.byref(n_total), C.byref(n_dropped), C.byref(bad_id),
                                           C.byref(bad_kind), L.stream_ptr())
        if rc != 0 and bad_kind.value != 0:
            raise ValueError(L.lib().rihip_last_error().decode("utf-8", "replace"))
        L.check(rc, "ip_index_update")
        self._vec_cache = None
        if n_dropped.value == 0 and n_add == 0:
            return 0, 0
        self._item_ids_dev = out[:n_total.value]
        self.item_ids = self._item_ids_dev.cpu().numpy()
        self._id_map_stale = True
        if old_tags is not None:
            # the update dropped the handle's tags (a new row order): surviving rows keep theirs in their new places, the
            # appended rows take `tags`, else the word their id carried before the call, else 0
            keep = torch.ones(n_old, dtype=torch.bool, device=dev) if n_drop == 0 else ~torch.isin(old_ids, drop)
            if tags is None and n_add:
                srt, order = torch.sort(old_ids)
                pos = torch.searchsorted(srt, add).clamp(max=n_old - 1)
                tags = torch.where(srt[pos] == add, old_tags[order[pos]], torch.zeros_like(old_tags[:1]))
            parts = [old_tags[keep]] + ([tags] if n_add else [])
            self._tags = torch.cat(parts).contiguous()
            assert self._tags.shape[0] == n_total.value
            self._push_tags()
        return int(n_dropped.value), n_add

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
        index (0 when omitted)."""
        if self.index is None:
            raise RuntimeError("Index not built.")
        return self.add_items_device(self._normalised(embeddings), item_ids, tags=tags)

    def add_items_device(self, x_dev: torch.Tensor, item_ids, tags=None) -> int:
        """add_items for rows that are already normalised and on the device (as build_from_device)"""
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

    # -- item tags (filtered retrieval; not in the reference) ------------------------------------------------------
    def _tags_dev(self, tags, n: int) -> torch.Tensor:
        """uint32 / int32 words [n] (host array or tensor) -> int32 bit patterns on the index's device"""
        if isinstance(tags, torch.Tensor):
            if tags.dtype != torch.int32:
                tags = torch.from_numpy(tags.detach().cpu().numpy().astype(np.uint32).view(np.int32))
        else:
            a = np.asarray(tags)
            if a.dtype.kind not in "iu":
                raise ValueError(f"tags must be uint32 words, got {a.dtype}")
            if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 32)):
                raise ValueError("tags must fit 32 bits")
            tags = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
        tags = tags.reshape(-1)
        if tags.shape[0] != n:
            raise ValueError(f"{tags.shape[0]} tag words for {n} items")
        return tags.to(self._item_ids_dev.device).contiguous()

    def _push_tags(self) -> None:
        L.check(L.lib().rihip_ip_index_set_tags(self.index._h, None if self._tags is None else self._tags.data_ptr(),
                                                L.stream_ptr()), "ip_index_set_tags")

    def set_item_tags(self, tags, item_ids=None) -> None:
        """Give every stored item a 32-bit tag word (bits 0-17: the reference's 18 genres by convention, see
        genre_tags; bits 18-31: the caller's).  tags uint32 [ntotal] in row order; with item_ids, tags[i] belongs to
        item_ids[i] and items that are not named keep their word (0 on an index that had none).  ValueError for an id
        that is not stored."""
        if self.index is None:
            raise RuntimeError("Index not built.")
        if self.search_pending():
            raise RuntimeError("a deferred search is pending: call finish_search() before changing the tags")
        n = self.index.ntotal
        if item_ids is None:
            self._tags = self._tags_dev(tags, n)
        else:
            ids = np.asarray(item_ids, dtype=np.int64).reshape(-1)
            t = self._tags_dev(tags, ids.shape[0])
            order = np.argsort(self.item_ids, kind="stable")
            pos = np.minimum(np.searchsorted(self.item_ids[order], ids), n - 1)
            rows = order[pos]
            missing = self.item_ids[rows] != ids
            if missing.any():
                raise ValueError(f"item id {int(ids[missing][0])} is not stored")
            cur = self._tags.clone() if self._tags is not None else torch.zeros(n, dtype=torch.int32, device=t.device)
            cur[torch.from_numpy(rows).to(t.device)] = t
            self._tags = cur
        self._push_tags()

    def item_tags(self) -> Optional[np.ndarray]:
        """uint32 [ntotal] tag words in row order (None without tags)"""
        return None if self._tags is None else self._tags.cpu().numpy().view(np.uint32)

    def clear_item_tags(self) -> None:
        self._tags = None
        if self.index is not None:
            self._push_tags()

    @property
    def has_item_tags(self) -> bool:
        return self.index is not None and bool(L.lib().rihip_ip_index_has_tags(self.index._h))

    def filtered_stats(self) -> Tuple[int, int]:
        """(queries searched with an item_filter, of those re-done by the exact fallback) since the handle was made"""
        out = (C.c_int64 * 2)()
        L.check(L.lib().rihip_ip_index_filtered_stats(self.index._h, out), "ip_index_filtered_stats")
        return int(out[0]), int(out[1])

    SEARCH_STATS = ("flat_dense", "flat_f32", "flat_fused", "flat_unfused", "ivf_unfiltered", "ivf_thresholded",
                    "sample_top", "prepare_small", "thr_queries", "redone", "redo_chunks", "passes")

    def search_stats(self) -> Dict[str, int]:
        """What the search driver did since the handle was made (rihip_ip_index_search_stats): internal passes per path,
        register top-T sample passes, one-launch IVF prepares, queries through a thresholded pass, of those re-done
        exactly (finish_search's included), re-do chunks, internal passes in all."""
        out = (C.c_int64 * len(self.SEARCH_STATS))()
        L.check(L.lib().rihip_ip_index_search_stats(self.index._h, out), "ip_index_search_stats")
        return {name: int(v) for name, v in zip(self.SEARCH_STATS, out)}

    def list_stats(self) -> Dict:
        """IVF list sizes: n_lists, min, max, mean, empty, imbalance = n_lists * sum(len^2) / sum(len)^2 (faiss
        imbalance_factor: 1.0 = even lists); it grows as updates drift away from the trained partition -- the signal
        to rebuild.  Flat index: {"n_lists": 0}."""
        if self.index is None:
            raise RuntimeError("Index not built.")
        if not self.index.is_ivf:
            return {"n_lists": 0}
        sizes = np.empty(int(L.lib().rihip_ip_index_nlist(self.index._h)), dtype=np.int64)
        L.check(L.lib().rihip_ip_index_list_sizes(self.index._h, sizes.ctypes.data), "ip_index_list_sizes")
        return _list_stats(sizes)

    # -- trained state (what faiss exposes as index.quantizer / index.invlists) ------------------
    def centroids(self) -> np.ndarray:
        """f32 [nlist,d] coarse centroids of the IVF partition."""
        nl = int(L.lib().rihip_ip_index_nlist(self.index._h))
        c = np.empty((nl, self.embed_dim), dtype=np.float32)
        L.check(L.lib().rihip_ip_index_get_ivf(self.index._h, c.ctypes.data, None), "ip_index_get_ivf")
        return c

    def list_assignment(self) -> np.ndarray:
        """int32 [N]: the inverted list every stored row (insertion order) belongs to."""
        a = np.empty(self.index.ntotal, dtype=np.int32)
        L.check(L.lib().rihip_ip_index_get_ivf(self.index._h, None, a.ctypes.data), "ip_index_get_ivf")
        return a

    def reconstruct(self) -> np.ndarray:
        """f32 [N,d]: the stored (normalised) vectors in insertion order (faiss reconstruct_n(0, ntotal))."""
        x = np.empty((self.index.ntotal, self.embed_dim), dtype=np.float32)
        L.check(L.lib().rihip_ip_index_reconstruct(self.index._h, x.ctypes.data), "ip_index_reconstruct")
        return x

    def item_vectors_device(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(V f32 [N, d], row_of i32 [max item id + 1], mu f64 [d]) on the device (not in the reference): the stored
        vectors in row order, item id -> row (-1 = not stored) and the mean of the stored vectors -- the inputs of the
        cold-start fold-in (coldstart.fold_in_users_device).  Built from the handle on the first call and kept until the
        index is built, loaded or updated again, so an item removed from the live catalogue stops contributing."""
        if self.index is None:
            raise RuntimeError("Index not built.")
        if self._vec_cache is None:
            dev = self._item_ids_dev.device
            ids = self.item_ids
            if ids.shape[0] and (ids.min() < 0 or ids.max() >= 2 ** 31 - 1):
                raise ValueError("item_vectors_device: item ids must lie in [0, 2**31 - 1) (row_of is indexed by item id)")
            V = torch.from_numpy(self.reconstruct()).to(dev)
            row_of = torch.full((int(ids.max()) + 1 if ids.shape[0] else 0,), -1, dtype=torch.int32, device=dev)
            row_of[self._item_ids_dev] = torch.arange(ids.shape[0], dtype=torch.int32, device=dev)
            mu = V.double().mean(0) if ids.shape[0] else torch.zeros(self.embed_dim, dtype=torch.float64, device=dev)
            self._vec_cache = (V, row_of, mu)
        return self._vec_cache

    def assign_lists(self, x_dev: torch.Tensor) -> torch.Tensor:
        """int32 [n] on device: arg-max-IP list of each f32 [n,d] device row (the IndexFlatIP quantizer)."""
        x = x_dev.to(dtype=torch.float32).contiguous()
        out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
        L.check(L.lib().rihip_ip_index_assign(self.index._h, x.data_ptr(), x.shape[0], out.data_ptr(), L.stream_ptr()),
                "ip_index_assign")
        return out

    # -- search (faiss_index.py:88-153) -------------------------------------------------------
    def _search_device(self, q_dev: torch.Tensor, k: int, item_ids: bool = False, item_filter=None
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
        """q_dev: normalised f32 [nq,d] on device -> (scores [nq,k], rows [nq,k]) on device; item_ids=True: the rows
        come back as item ids (faiss_index.py:123,148-152), mapped inside the search's last kernel.  item_filter: only
        rows whose tag word passes (batch_search_device)."""
        lib = L.lib()
        nq = q_dev.shape[0]
        pred = None
        if item_filter is not None:
            if self._tags is None:
                raise ValueError("item_filter needs item tags: call set_item_tags() first")
            if isinstance(item_filter, tuple) and item_filter in self._pred_cache:
                pred, stride = self._pred_cache[item_filter], 0      # (no host-to-device copy per request)
            else:
                pred, stride = _filter_device(item_filter, nq, q_dev.device)
                if stride == 0 and isinstance(item_filter, tuple) and len(self._pred_cache) < 1024:
                    self._pred_cache[item_filter] = pred
            if self.search_pending():
                raise RuntimeError("a deferred search is pending: call finish_search() before a filtered search")
        L.check(lib.rihip_ip_index_set_id_map(self.index._h, self._item_ids_dev.data_ptr() if item_ids else None),
                "ip_index_set_id_map")
        if k > int(lib.rihip_ip_index_max_k()):
            raise ValueError(f"k={k} exceeds the device select buffer ({int(lib.rihip_ip_index_max_k())}); "
                             "the reference (faiss) has no such limit -- see INTEGRATION.md")
        scores = torch.empty((nq, k), dtype=torch.float32, device=q_dev.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=q_dev.device)
        if pred is not None:
            L.check(lib.rihip_ip_index_search_filtered(self.index._h, q_dev.data_ptr(), nq, k, pred.data_ptr(), stride,
                                                       scores.data_ptr(), rows.data_ptr(), L.stream_ptr()),
                    "ip_index_search_filtered")
            return scores, rows
        L.check(lib.rihip_ip_index_search(self.index._h, q_dev.data_ptr(), nq, k, scores.data_ptr(), rows.data_ptr(),
                                          L.stream_ptr()), "ip_index_search")
        return scores, rows

    def set_deferred_check(self, enable: bool) -> None:
        """Serving chains (not in the reference): a thresholded IVF search then returns without its host
        synchronisation; call `finish_search()` after enqueueing the consumers of the result."""
        L.check(L.lib().rihip_ip_index_set_deferred_check(self.index._h, 1 if enable else 0), "ip_index_set_deferred_check")
        self._deferred = bool(enable)

    def finish_search(self) -> int:
        """-> number of queries of the last deferred search that had to be re-done exactly (their output rows were
        rewritten AFTER anything enqueued behind the search ran: run those consumers again); 0 almost always."""
        n = C.c_int(0)
        L.check(L.lib().rihip_ip_index_search_finish(self.index._h, C.byref(n), L.stream_ptr()), "ip_index_search_finish")
        return int(n.value)

    def search_pending(self) -> bool:
        return bool(L.lib().rihip_ip_index_search_pending(self.index._h))

    def last_fail_count(self) -> int:
        """after the REPLAY of a captured chain that holds a deferred search: synchronises, -> its failure count"""
        n = C.c_int(0)
        L.check(L.lib().rihip_ip_index_last_fail_count(self.index._h, C.byref(n), L.stream_ptr()), "ip_index_last_fail_count")
        return int(n.value)

    # -- seen-item exclusion: filter_excluded, exclusion_deficit and _search_excluding come from exclusion.ExcludingSearch

    def _search_scan_excluding(self, q: torch.Tensor, k: int, seen, uid: Optional[torch.Tensor], item_filter=None,
                               row_of: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """exclusion="scan": one rihip_ip_index_search_excluding over the batch -> (scores, item ids) [nq, k]"""
        lib = L.lib()
        nq = q.shape[0]
        row_of = self._row_of_device() if row_of is None else self._check_row_of(row_of)
        pred, stride = None, 0
        if item_filter is not None:
            if self._tags is None:
                raise ValueError("item_filter needs item tags: call set_item_tags() first")
            pred, stride = _filter_device(item_filter, nq, q.device)
        if self.search_pending():
            raise RuntimeError('a deferred search is pending: call finish_search() before an exclusion="scan" search')
        if k > int(lib.rihip_ip_index_max_k()):
            raise ValueError(f"k={k} exceeds the device select buffer ({int(lib.rihip_ip_index_max_k())})")
        L.check(lib.rihip_ip_index_set_id_map(self.index._h, self._item_ids_dev.data_ptr()), "ip_index_set_id_map")
        scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
        L.check(lib.rihip_ip_index_search_excluding(self.index._h, q.data_ptr(), nq, k, L.ptr(uid), seen.offsets.data_ptr(),
                                                    seen.n_users, seen.items.data_ptr(), row_of.data_ptr(), row_of.shape[0],
                                                    L.ptr(pred), stride, scores.data_ptr(), ids.data_ptr(), L.stream_ptr()),
                "ip_index_search_excluding")
        return scores, ids

    def search(self, query_vector: np.ndarray, k: int = 500, exclude_items=None, item_filter=None,
               exclusion: str = "overfetch") -> Tuple[np.ndarray, np.ndarray]:
        """exclude_items (not in the reference): item ids that must not be returned; item_filter (not in the reference):
        (any_of, all_of, none_of) over the items' tag words, as in batch_search_device; exclusion: how exclude_items are
        kept out, as in batch_search_device"""
        check_exclusion(exclusion)
        if self.index is None:
            raise RuntimeError("Index not built. Call build_ivf_index() first.")
        query = np.atleast_2d(query_vector).astype(np.float32)
        norm = np.linalg.norm(query, axis=1, keepdims=True)
        query = query / np.maximum(norm, 1e-8)
        k = min(k, self.index.ntotal)
        q_dev = torch.from_numpy(np.ascontiguousarray(query[:1])).to(L.device())
        if exclude_items is not None:
            from .seen import SeenItems
            ex = np.asarray(exclude_items, dtype=np.int64).reshape(-1)
            scores, ids = self._search_excluding(q_dev, k, SeenItems.from_pairs(np.zeros(ex.shape[0], np.int64), ex, 1),
                                                 None, item_filter, exclusion=exclusion)
            distances, ids = scores[0].cpu().numpy(), ids[0].cpu().numpy()
            return distances[ids >= 0], ids[ids >= 0]
        scores, rows = self._search_device(q_dev, k, item_filter=item_filter)
        distances = scores[0].cpu().numpy()
        faiss_indices = rows[0].cpu().numpy()
        valid_mask = faiss_indices >= 0
        distances = distances[valid_mask]
        faiss_indices = faiss_indices[valid_mask]
        return distances, self.item_ids[faiss_indices]

    def batch_search(self, query_vectors: np.ndarray, k: int = 500, exclude=None, user_ids=None, item_filter=None,
                     exclusion: str = "overfetch") -> Tuple[np.ndarray, np.ndarray]:
        """exclude / user_ids / item_filter / exclusion (not in the reference): as in batch_search_device"""
        check_exclusion(exclusion)
        if self.index is None:
            raise RuntimeError("Index not built.")
        queries = query_vectors.astype(np.float32)
        norms = np.linalg.norm(queries, axis=1, keepdims=True)
        queries = queries / np.maximum(norms, 1e-8)
        k = min(k, self.index.ntotal)
        q_dev = torch.from_numpy(np.ascontiguousarray(queries)).to(L.device())
        if exclude is not None:
            scores, rows = self._search_excluding(q_dev, k, exclude, self._require_user_ids(user_ids), item_filter,
                                                  exclusion=exclusion)
        else:
            scores, rows = self._search_device(q_dev, k, item_ids=True, item_filter=item_filter)
        return scores.cpu().numpy(), rows.cpu().numpy()

    @staticmethod
    def _require_user_ids(user_ids):
        if user_ids is None:
            raise ValueError("exclude needs user_ids: the row of the seen store every query reads")
        return user_ids

    def batch_search_device(self, queries: torch.Tensor, k: int = 500, normalized: bool = False, exclude=None,
                            user_ids=None, item_filter=None, exclusion: str = "overfetch"
                            ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Device-resident batch_search (not in the reference): queries f32 [nq,d] on the HIP device;
        returns (scores, item_ids) on device, -1 padded.  This is the QPS benchmark entry.

        exclude (a seen.SeenItems) with user_ids [nq]: query q never returns an item of row user_ids[q] of the store;
        the result is the top k of the corpus (IVF: of the probed lists) minus that row, -1 padded when fewer remain.
        user_ids as a host sequence: the batch is searched in groups by how far each query has to over-fetch
        (seen.plan_overfetch); as a device tensor: one search at the store's longest list.  ValueError when k plus a
        user's list exceeds the 16384-candidate limit of the search on a corpus larger than that.
        Under set_deferred_check(True) the filtered result is a consumer of the search like any other: when
        finish_search() returns > 0, call this again (it then runs as one group: one search, one finish).

        exclusion="scan" (opt-in; "overfetch", the default, is everything above): the seen items are excluded inside the
        index scan instead -- one bit per (query, row) of a mask built on the device from the store, tested where the
        tag predicate is tested.  One search of the whole batch whatever user_ids is, no over-fetch, no groups, nothing
        added to exclusion_deficit(), and no limit on k plus a user's list.  The same rows and scores bit for bit.  It
        always synchronises like a filtered search (RuntimeError while a deferred search is pending), a large flat index
        takes the all-f32 scan, and item ids must lie in [0, 2**31 - 1).  Any other value: ValueError.

        item_filter (needs set_item_tags): a 3-tuple of ints (any_of, all_of, none_of) shared by the batch, a uint32
        array [nq,3], or an int32 device tensor [nq,3] read as a bit pattern.  Item i passes iff (any_of == 0 or
        tag[i] & any_of) and tag[i] & all_of == all_of and tag[i] & none_of == 0; the result is the exact top k of the
        passing items (IVF: of the probed lists), -1 padded when fewer pass; (0,0,0) equals the plain search.  The
        predicate is tested inside the scan, so a filter that removes 99.9 % of the corpus needs no over-fetch.  With
        exclude the result is filter AND not-seen.  A filtered search always synchronises (no deferred check), and on
        a large flat index it takes the all-f32 scan.  ValueError without tags or on a bad shape."""
        check_exclusion(exclusion)
        if self.index is None:
            raise RuntimeError("Index not built.")
        q = queries.to(dtype=torch.float32).contiguous()
        if not normalized:
            q = q / torch.clamp(torch.linalg.norm(q, dim=1, keepdim=True), min=1e-8)
        k = min(k, self.index.ntotal)
        if exclude is not None:
            return self._search_excluding(q, k, exclude, self._require_user_ids(user_ids), item_filter, exclusion=exclusion)
        return self._search_device(q, k, item_ids=True, item_filter=item_filter)

    # -- persistence (faiss_index.py:159-205) -------------------------------------------------
    def save(self, path: str, format: str = "rihip") -> None:
        """format="faiss": a file faiss.read_index can open (IndexIVFFlat, or IndexFlatIP for exact=True)."""
        save_path = Path(path)
        save_path.parent.mkdir(parents=True, exist_ok=True)
        if format == "faiss":
            from . import faiss_io
            if self.index.is_ivf:
                faiss_io.write_ivf_flat(str(save_path), self.reconstruct(), self.centroids(), self.list_assignment(),
                                        self.n_probe)
            else:
                faiss_io.write_flat(str(save_path), self.reconstruct())
        elif format == "rihip":
            L.check(L.lib().rihip_ip_index_save(self.index._h, str(save_path).encode()), "ip_index_save")
        else:
            raise ValueError(f"unknown index file format {format!r}")
        meta_path = save_path.with_suffix(".meta.pkl")
        meta = {
            "item_ids": self.item_ids,
            "item_id_to_faiss_idx": self._item_id_to_faiss_idx,
            "embed_dim": self.embed_dim,
            "n_lists": self.n_lists,
            "n_probe": self.n_probe,
        }
        if self._tags is not None:   # (only then: an untagged index writes the sidecar it always wrote)
            meta["item_tags"] = self.item_tags()
        with open(meta_path, "wb") as f:
            pickle.dump(meta, f)
        logger.info("Saved index to %s (meta: %s)", save_path, meta_path)

    @classmethod
    def load(cls, path: str) -> "FAISSIndex":
        load_path = Path(path)
        if not load_path.exists():
            raise FileNotFoundError(f"FAISS index not found at {load_path}")
        meta_path = load_path.with_suffix(".meta.pkl")
        with open(meta_path, "rb") as f:
            meta = pickle.load(f)  # sidecar written by save() above
        obj = cls(embed_dim=meta["embed_dim"], n_lists=meta["n_lists"], n_probe=meta["n_probe"])
        from . import faiss_io
        if faiss_io.sniff(str(load_path)) == "faiss":        # written by faiss.write_index (or save(format="faiss"))
            f = faiss_io.read_index(str(load_path))
            if f["metric"] != faiss_io.METRIC_INNER_PRODUCT:
                raise ValueError("only METRIC_INNER_PRODUCT indexes are supported (faiss_index.py:70-72)")
            assert f["d"] == obj.embed_dim, (f["d"], obj.embed_dim)
            obj.exact = f["kind"] == "flat"
            x_dev = torch.from_numpy(f["vectors"]).to(L.device())
            ids = np.asarray(meta["item_ids"], dtype=np.int64)
            if obj.exact:
                obj.build_from_device(x_dev, ids)
            else:
                nlist, n = int(f["nlist"]), int(f["ntotal"])
                max_lists = 2048      # csrc/ip_index.h NLIST_MAX (probe bitset of the list-major scan)
                if nlist > max_lists:
                    raise faiss_io.FaissFormatError(
                        f"{load_path}: IndexIVFFlat with nlist={nlist} > {max_lists} lists is not supported by the HIP index")
                if nlist > n:
                    # more lists than vectors (faiss allows it; every search then probes mostly empty lists): serve the
                    # file's vectors exactly instead of failing
                    logger.warning("%s: nlist=%d > ntotal=%d, loading as a flat (exact) index", load_path, nlist, n)
                    obj.exact = True
                    obj.build_from_device(x_dev, ids)
                else:
                    obj.n_lists = nlist
                    obj.build_from_device(x_dev, ids, centroids=f["centroids"], assign=f["assign"])
                    # the sidecar's n_probe is what the reference restores (faiss_index.py:199-201); a file written by
                    # faiss itself carries its own nprobe, used only when the sidecar has none
                    if meta.get("n_probe") is None and f.get("nprobe"):
                        obj.set_n_probe(int(f["nprobe"]))
            obj._item_id_to_faiss_idx = meta["item_id_to_faiss_idx"]
            if meta.get("item_tags") is not None:
                obj.set_item_tags(meta["item_tags"])
            return obj
        h = C.c_void_p()
        L.check(L.lib().rihip_ip_index_load(str(load_path).encode(), C.byref(h)), "ip_index_load")
        obj.index = _IndexHandle(h.value, obj)
        obj._vec_cache = None
        obj.index.nprobe = meta["n_probe"]
        obj.item_ids = np.asarray(meta["item_ids"], dtype=np.int64)
        obj._item_ids_dev = torch.from_numpy(obj.item_ids).to(L.device())
        obj._item_id_to_faiss_idx = meta["item_id_to_faiss_idx"]
        obj.exact = not obj.index.is_ivf
        if meta.get("item_tags") is not None:
            obj.set_item_tags(meta["item_tags"])
        return obj

    # -- utilities (faiss_index.py:211-228) ---------------------------------------------------
    def stats(self) -> Dict:
        if self.index is None:
            return {"status": "not built"}
        return {
            "n_vectors": int(self.index.ntotal),
            "embed_dim": self.embed_dim,
            "n_lists": self.n_lists,
            "n_probe": self.n_probe,
            "metric": "inner_product",
            "n_item_ids": len(self.item_ids) if self.item_ids is not None else 0,
        }

    def set_n_probe(self, n_probe: int) -> None:
        self.n_probe = n_probe
        if self.index is not None:
            self.index.nprobe = n_probe
