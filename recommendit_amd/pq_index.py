"""PQIndex: a product-quantised inner-product index (flat and IVF) next to SQ8Index (not in the reference; faiss has it
as IndexPQ / IndexIVFPQ).

A row takes ``dpad / dsub`` bytes (d = 128: 16 bytes at ``dsub=8``, 8 at ``dsub=16``) instead of SQ8's 128: one byte per
sub-space of ``dsub`` dimensions, naming one of 256 int8 codebook entries.  The quantiser works on the rows' SQ8 codes in
integers only and is specified at ``rihip_pq_index_*`` in recommendit_hip.h; the scan is SQ8's, gathering its operand
bytes from the codebooks in LDS.  A PQIndex is therefore the SQ8Index of its own reconstruction: every search of
SQ8Index -- ``mode=``, ``item_filter=``, ``exclude=`` on both ``exclusion=`` routes, ``refine=`` / ``return_cert=`` /
``search_certified``, serving through GpuRecommendationPipeline -- returns what that SQ8Index would return, integer
scores included, and ``codes()`` / ``reconstruct()`` return the decoded matrix those scores are stated over.

Deviations from faiss: an own quantiser over SQ8 codes with int8 codebooks, residual encoding
against the IVF centroids only on request, no faiss PQ file interop.

``from_index(..., by_residual=True)`` (opt-in; an IVF source): the codebooks quantise each row's SQ8 code minus its
list's centroid snapped to the same SQ8 grid (``list_codes()``).  The decoded code is then list code + entry, an int16 in
[-254, 254] (``codes()`` returns int16), and the score splits into a per-(query, list) integer and the gathered dot
product the scan already forms, so every search keeps its exact integer contract over that int16 matrix.  The
certificate of a refined search uses 254 where it uses 127 otherwise.  A residual index has a file format of its own;
``save`` writes it and ``load`` picks the reader by the file's first bytes.

``codes()``, ``reconstruct()`` and ``attach_vectors()`` decode the whole index on the device: a transient
N * dpad bytes.  ``save`` / ``load`` are SQ8Index's on the PQ file format (``_SAVE`` / ``_LOAD``); each loader refuses the
other's file.

Live catalogue (opt-in): by default a PQ index is not updated in place (its codebooks are trained on the corpus):
``add_items``, ``remove_items`` and ``update_items`` raise NotImplementedError -- rebuild with ``from_index``.  With
``from_index(..., frozen_updates=True)`` or ``pq.frozen_updates = True`` they work as on SQ8Index, as one repack of the
entry-number matrix under the FROZEN centroids, quantiser, list codes and codebooks (csrc/pq_update.hip); the index ends
bit for bit where a from-scratch build of the final corpus with those injected would, and ``update_stats()`` carries
the drift signal of the frozen codebooks.

There is no NumPy or torch path for training, encoding or search: everything runs in csrc/pq.hip and the SQ8 index's
units (csrc/sq8.hip over csrc/sq8_scan.hip for the search).
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Dict, Optional, Tuple

import numpy as np

from . import _lib as L
from .faiss_index import FAISSIndex
from .sq8_index import SQ8Index, _check_ranges, _check_source

logger = logging.getLogger(__name__)

_REBUILD = ("a PQIndex is not updated in place (its codebooks are trained on the corpus): rebuild it with PQIndex.from_index, "
            "or set frozen_updates=True to add, remove and replace items under the codebooks it has")


class PQIndex(SQ8Index):
    _KIND = "PQ"
    _SAVE, _LOAD = "rihip_pq_index_save", "rihip_pq_index_load"    # save() / load(): SQ8Index's, on the PQ file format
    _frozen_updates = False                                        # the property below

    # -- build ----------------------------------------------------------------------------------------------------
    @classmethod
    def from_index(cls, faiss_index: FAISSIndex, dsub: int = 8, n_iter: int = 10,
                   ranges: Optional[Tuple[np.ndarray, np.ndarray]] = None, codebooks: Optional[np.ndarray] = None,
                   keep_vectors: bool = False, by_residual: bool = False, frozen_updates: bool = False) -> "PQIndex":
        """Encode the vectors of a built FAISSIndex (IVF: its lists and centroids; exact: one list).  dsub: 8 or 16
        dimensions per sub-space; n_iter: Lloyd steps of the codebook training; ranges: (centre, scale) of the SQ8 stage,
        as SQ8Index.from_index; codebooks: int8 [M, 256, dsub] with M = dpad / dsub (dpad = 64 up to 64 dimensions, else
        128), entries in [-127, 127] -- injected codebooks skip the training, as ranges= skips the range pass.
        keep_vectors / item tags: as SQ8Index.from_index.  by_residual=True: quantise the residuals against the IVF
        centroids (the module text above); injected codebooks are then residual codebooks.  ValueError on a flat source.
        frozen_updates=True: allow add_items / remove_items / update_items under the frozen codebooks (the property)."""
        _check_source("PQIndex", faiss_index)
        if not isinstance(frozen_updates, (bool, np.bool_)):
            raise ValueError(f"PQIndex: frozen_updates={frozen_updates!r} must be True or False")
        if not isinstance(by_residual, (bool, np.bool_)):
            raise ValueError(f"PQIndex: by_residual={by_residual!r} must be True or False")
        if by_residual and not faiss_index.index.is_ivf:
            raise ValueError("PQIndex: by_residual=True needs an IVF index (a flat index has one list and no centroids)")
        if dsub not in (8, 16):
            raise ValueError(f"PQIndex: dsub={dsub!r} (8 or 16)")
        if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or not 0 <= int(n_iter) <= 1000:
            raise ValueError(f"PQIndex: n_iter={n_iter!r} outside 0..1000")
        d = faiss_index.embed_dim
        dpad = 64 if d <= 64 else 128
        m, s = _check_ranges("PQIndex", ranges, d)
        book = None
        if codebooks is not None:
            book = np.asarray(codebooks)
            if book.dtype != np.int8 or book.shape != (dpad // dsub, 256, dsub):
                raise ValueError(f"PQIndex: codebooks must be int8 [{dpad // dsub}, 256, {dsub}], got {book.dtype} {book.shape}")
            if (book == -128).any():
                raise ValueError("PQIndex: codebook entries lie in [-127, 127]")
            book = np.ascontiguousarray(book)
        h = C.c_void_p()
        L.check(L.lib().rihip_pq_index_from_ip_index_residual(
            faiss_index.index._h, None if m is None else m.ctypes.data, None if s is None else s.ctypes.data, int(dsub),
            int(n_iter), None if book is None else book.ctypes.data, int(bool(by_residual)), C.byref(h), L.stream_ptr()),
            "pq_index_from_ip_index")
        obj = cls._adopt(h.value, faiss_index, keep_vectors)
        obj.frozen_updates = frozen_updates
        return obj

    # -- live catalogue under frozen codebooks (opt-in) -------------------------------------------------------------------
    # With frozen_updates on, the four calls are SQ8Index's over rihip_pq_update_apply (csrc/pq_update.hip): ONE repack of
    # the entry-number matrix under the index's own centroids, SQ8 quantiser, list codes and codebooks, none of which is
    # retrained (faiss IndexIVFPQ adds after train() in the same way).  Kept rows keep their bytes, new rows are encoded
    # against the frozen codebooks, and the index ends bit for bit where from_index(f32 index of the final corpus with the
    # same centroids and lists, dsub=self.dsub, ranges=self.quantizer(), codebooks=self.codebooks(),
    # by_residual=self.by_residual) + set_item_tags + attach_vectors would leave it; saved files are byte-identical.
    # Normalisation, add_items_device, the upsert tag rules, assign_lists and the refusals are SQ8Index's.
    @property
    def frozen_updates(self) -> bool:
        """whether add_items / remove_items / update_items work on this index (under its frozen codebooks) instead of
        raising NotImplementedError.  A Python-side switch: it is in no file, so a loaded index opts in again."""
        return self._frozen_updates

    @frozen_updates.setter
    def frozen_updates(self, on) -> None:
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"PQIndex: frozen_updates={on!r} must be True or False")
        self._frozen_updates = bool(on)

    def _update_entry(self) -> str:
        return "rihip_pq_update_apply" if self._frozen_updates else self._UPDATE

    def _log_update(self, n_dropped: int, n_add: int) -> None:
        st = self.update_stats()
        logger.info("PQ index updated: %d rows dropped, %d added, %d code values clamped, %d residual values clamped, "
                    "distortion %d", n_dropped, n_add, self._last_clamped, st["last_residual_clamped"], st["last_distortion"])

    def _frozen(self) -> None:
        if not self._frozen_updates:
            raise NotImplementedError(_REBUILD)

    def add_items(self, embeddings, item_ids, tags=None):
        self._frozen()
        return super().add_items(embeddings, item_ids, tags=tags)

    def add_items_device(self, x_dev, item_ids, tags=None):
        self._frozen()
        return super().add_items_device(x_dev, item_ids, tags=tags)

    def remove_items(self, item_ids):
        self._frozen()
        return super().remove_items(item_ids)

    def update_items(self, embeddings, item_ids, tags=None):
        self._frozen()
        return super().update_items(embeddings, item_ids, tags=tags)

    def update_stats(self) -> Dict:
        """SQ8Index.update_stats() plus, cumulative since the handle was made, residual_clamped (residual values of added
        rows that left [-127, 127]; 0 on a plain index) and distortion_added (the summed smallest distance D over all
        added rows and sub-spaces), and last_residual_clamped / last_distortion of the last update that changed the
        index.  The drift signal of frozen codebooks: compare distortion_added / added, the mean distortion of an added
        row, against train_stats()["distortion"][-1] / N_build, that of a row the codebooks were trained on; a ratio
        well above 1 says the new rows no longer look like the training corpus and a rebuild is due.  After load the
        trace is empty, so only the first half exists."""
        out = (C.c_int64 * 8)()
        L.check(L.lib().rihip_pq_update_stats(self._built()._h, out), "pq_update_stats")
        return {"updates": int(out[0]), "dropped": int(out[1]), "added": int(out[2]), "clamped": int(out[3]),
                "last_clamped": self._last_clamped, "residual_clamped": int(out[4]), "distortion_added": int(out[5]),
                "last_residual_clamped": int(out[6]), "last_distortion": int(out[7])}

    # -- trained state ----------------------------------------------------------------------------------------------
    def _dims(self) -> Tuple[int, int]:
        dsub, m = C.c_int(0), C.c_int(0)
        L.check(L.lib().rihip_pq_index_dims(self._built()._h, C.byref(dsub), C.byref(m)), "pq_index_dims")
        return int(dsub.value), int(m.value)

    @property
    def dsub(self) -> int:
        return self._dims()[0]

    @property
    def by_residual(self) -> bool:
        """whether the codebooks quantise residuals against the IVF centroids"""
        return self.index is not None and bool(L.lib().rihip_pq_index_is_residual(self.index._h))

    def list_codes(self) -> np.ndarray:
        """int8 [n_lists, dpad]: every list's centroid on the SQ8 grid, padding columns 0 (a residual index only)"""
        h = self._built()
        if not self.by_residual:
            raise RuntimeError("PQIndex.list_codes: not a residual index (from_index(by_residual=True))")
        out = np.empty((h.nlist, 64 if self.embed_dim <= 64 else 128), dtype=np.int8)
        L.check(L.lib().rihip_pq_index_get_list_codes(h._h, out.ctypes.data), "pq_index_get_list_codes")
        return out

    def pq_codes(self) -> np.ndarray:
        """uint8 [N, M]: the stored entry numbers in insertion order"""
        h = self._built()
        out = np.empty((h.ntotal, self._dims()[1]), dtype=np.uint8)
        L.check(L.lib().rihip_pq_index_get_codes(h._h, out.ctypes.data), "pq_index_get_codes")
        return out

    def codebooks(self) -> np.ndarray:
        """int8 [M, 256, dsub]"""
        h = self._built()
        dsub, m = self._dims()
        out = np.empty((m, 256, dsub), dtype=np.int8)
        L.check(L.lib().rihip_pq_index_get_codebooks(h._h, out.ctypes.data), "pq_index_get_codebooks")
        return out

    def train_stats(self) -> Dict:
        """distortion: int64 [passes], the summed smallest distance of every assignment pass of the build (n_iter + 1
        values; one with injected codebooks; none after load); peak_bytes: device bytes at the build's peak, the
        transient SQ8 codes included; *_ms: host time of the build's stages; by_residual and residual_clamped: the
        residual values of the build that left [-127, 127] and were clamped (0 after load and on a plain index)"""
        h = self._built()
        n = C.c_int(0)
        peak = L.c_i64(0)
        ms = (C.c_double * 3)()
        trace = (L.c_i64 * 1001)()
        L.check(L.lib().rihip_pq_index_train_stats(h._h, trace, 1001, C.byref(n), C.byref(peak), ms), "pq_index_train_stats")
        clamped = L.c_i64(0)
        L.check(L.lib().rihip_pq_index_residual_clamped(h._h, C.byref(clamped)), "pq_index_residual_clamped")
        return {"distortion": np.array(trace[:n.value], dtype=np.int64), "peak_bytes": int(peak.value),
                "range_encode_ms": float(ms[0]), "train_ms": float(ms[1]), "assign_ms": float(ms[2]),
                "by_residual": self.by_residual, "residual_clamped": int(clamped.value)}

    def codes(self) -> np.ndarray:
        """int8 [N, embed_dim]: the DECODED codes (codebook entries) in insertion order -- the matrix the search contract
        is stated over.  Decodes the whole index on the device: a transient N * dpad bytes.  A residual index returns
        int16 [N, embed_dim]: list code + entry, in [-254, 254] (a transient 2 * N * dpad bytes)."""
        if not self.by_residual:
            return super().codes()
        h = self._built()
        c = np.empty((h.ntotal, self.embed_dim), dtype=np.int16)
        L.check(L.lib().rihip_pq_index_get_decoded16(h._h, c.ctypes.data), "pq_index_get_decoded16")
        return c

    def reconstruct(self) -> np.ndarray:
        """f32 [N, embed_dim]: centre + scale * decoded code in insertion order (a transient N * dpad bytes on the device)"""
        return super().reconstruct()

    # -- persistence ------------------------------------------------------------------------------------------------
    @classmethod
    def _loader(cls, load_path) -> str:
        """the reader of the file's format: a residual index is saved under a magic of its own"""
        with open(load_path, "rb") as f:
            return "rihip_pq_index_load_residual" if f.read(8) == b"RIHIPPR1" else cls._LOAD

    # -- utilities --------------------------------------------------------------------------------------------------
    def stats(self) -> Dict:
        st = super().stats()
        if self.index is None:
            return st
        dsub, m = self._dims()
        f32_row = 4 * (32 if self.embed_dim <= 32 else (64 if self.embed_dim <= 64 else 128))
        st.update({"bytes_per_vector": m, "compression": f32_row / m, "dsub": dsub, "n_subspaces": m,
                   "codebook_bytes": m * 256 * dsub, "peak_build_bytes": self.train_stats()["peak_bytes"],
                   "by_residual": self.by_residual})
        return st
