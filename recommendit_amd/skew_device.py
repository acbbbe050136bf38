"""Training-serving skew on the GPU: the reference's kl_divergence_bins / detect_training_serving_skew
(src/evaluation/metrics.py:197-294) computed from samples that live on the device -- a training feature matrix and the
serving feature log of GpuRecommendationPipeline -- without copying them to the host.

* ``feature_histograms_device``: the raw per-column tensors (counts, edges, valid counts, KL, status) of two row-major
  f32 / f64 device matrices, with a column-index list per side and optional per-row ids (< 0 = row left out).
* ``kl_divergence_bins_device``: metrics.kl_divergence_bins of two 1-D device tensors (values taken as float64, as the
  detector's ``.astype(float)`` does).
* ``detect_training_serving_skew_device``: the detector's dict.  The column choice and the dict assembly are the host
  code of metrics.py (skew_columns, skew_report); only the per-column KL comes from the device.

Kernels: recommendit_amd/csrc/skew.hip.  Everything is enqueued on the current stream; the scalar results are read back
at the end (one synchronisation).
"""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import metrics as M

MAX_BINS = 128
STATUS_OK, STATUS_CONSTANT, STATUS_INFINITE, STATUS_NAN, STATUS_TOO_FEW, STATUS_BAD_COLUMN = range(6)


class SkewTensors(NamedTuple):
    counts: torch.Tensor   # int64 [nc, 2, n_bins]: train / serving histograms on the shared edges
    edges: torch.Tensor    # float64 [nc, n_bins + 1]: np.linspace(min, max, n_bins + 1) of the combined range
    valid: torch.Tensor    # int64 [nc, 2]: non-NaN values per side
    kl: torch.Tensor       # float64 [nc]: unrounded KL(train || serving)
    status: torch.Tensor   # int32 [nc]: STATUS_*


def _matrix(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: expected a device tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what}: a CPU tensor (the skew kernels read device memory)")
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: dtype {t.dtype} (float32 or float64)")
    if t.dim() == 1:
        t = t.reshape(-1, 1)
    if t.dim() != 2:
        raise ValueError(f"{what}: expected a 2-D matrix, got shape {tuple(t.shape)}")
    if t.shape[1] == 0:
        raise ValueError(f"{what}: no columns")
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _cols(cols, ncols: int, nc: Optional[int], what: str, dev) -> torch.Tensor:
    c = np.arange(ncols) if cols is None else np.asarray(cols, dtype=np.int64).reshape(-1)
    if nc is not None and c.shape[0] != nc:
        raise ValueError(f"column-count mismatch: {c.shape[0]} {what} columns against {nc}")
    if c.shape[0] == 0:
        raise ValueError(f"{what}: no columns selected")
    if (c < 0).any() or (c >= ncols).any():
        raise ValueError(f"{what}: column index outside [0, {ncols})")
    return torch.from_numpy(c.astype(np.int32)).to(dev)


def _ids(ids, n: int, what: str) -> Optional[torch.Tensor]:
    if ids is None:
        return None
    if not isinstance(ids, torch.Tensor) or not ids.is_cuda:
        raise ValueError(f"{what}: ids must be a device tensor")
    if ids.dtype != torch.int64 or ids.dim() != 1 or ids.shape[0] != n:
        raise ValueError(f"{what}: ids must be int64 [{n}], got {ids.dtype} {tuple(ids.shape)}")
    return ids.contiguous()


def _check_bins(n_bins) -> int:
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 1 <= int(n_bins) <= MAX_BINS:
        raise ValueError(f"n_bins={n_bins!r}: an integer in 1..{MAX_BINS}")
    return int(n_bins)


def feature_histograms_device(train: torch.Tensor, serving: torch.Tensor, cols_train: Optional[Sequence[int]] = None,
                              cols_serving: Optional[Sequence[int]] = None, ids_train: Optional[torch.Tensor] = None,
                              ids_serving: Optional[torch.Tensor] = None, n_bins: int = 20, epsilon: float = 1e-10,
                              min_count: int = 0, propagate_nan: bool = False) -> SkewTensors:
    """Per column c: train column cols_train[c] against serving column cols_serving[c] (default: every column, the
    two matrices being as wide).  Rows whose id is < 0 are left out.  min_count: fewer non-NaN values on either side
    gives STATUS_TOO_FEW (the detector's skip); propagate_nan: any NaN gives KL nan (kl_divergence_bins on raw input)."""
    n_bins = _check_bins(n_bins)
    A = _matrix(train, "train")
    B = _matrix(serving, "serving")
    if A.device != B.device:
        raise ValueError(f"train on {A.device}, serving on {B.device}")
    dev = A.device
    if cols_train is None and cols_serving is None and A.shape[1] != B.shape[1]:
        raise ValueError(f"column-count mismatch: train has {A.shape[1]} columns, serving {B.shape[1]}")
    ca = _cols(cols_train, A.shape[1], None, "train", dev)
    nc = ca.shape[0]
    cb = _cols(cols_serving if cols_serving is not None else (None if cols_train is None else cols_train),
               B.shape[1], nc, "serving", dev)
    ia = _ids(ids_train, A.shape[0], "train")
    ib = _ids(ids_serving, B.shape[0], "serving")
    lib = L.lib()
    ws_bytes = int(lib.rihip_skew_workspace_bytes(nc))
    with torch.cuda.device(dev):
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        counts = torch.empty((nc, 2, n_bins), dtype=torch.int64, device=dev)
        edges = torch.empty((nc, n_bins + 1), dtype=torch.float64, device=dev)
        valid = torch.empty((nc, 2), dtype=torch.int64, device=dev)
        kl = torch.empty((nc,), dtype=torch.float64, device=dev)
        status = torch.empty((nc,), dtype=torch.int32, device=dev)
        L.check(lib.rihip_skew_compute(A.data_ptr(), int(A.dtype == torch.float64), A.shape[0], A.stride(0),
                                       ca.data_ptr(), L.ptr(ia), B.data_ptr(), int(B.dtype == torch.float64),
                                       B.shape[0], B.stride(0), cb.data_ptr(), L.ptr(ib), nc, n_bins, float(epsilon),
                                       int(min_count), int(bool(propagate_nan)), ws.data_ptr(), ws_bytes,
                                       counts.data_ptr(), edges.data_ptr(), valid.data_ptr(), kl.data_ptr(),
                                       status.data_ptr(), L.stream_ptr()), "skew_compute")
    return SkewTensors(counts, edges, valid, kl, status)


def kl_divergence_bins_device(p_values: torch.Tensor, q_values: torch.Tensor, n_bins: int = 20,
                              epsilon: float = 1e-10) -> float:
    """metrics.kl_divergence_bins(p.astype(float), q.astype(float), n_bins, epsilon) of two 1-D device tensors"""
    n_bins = _check_bins(n_bins)
    for t, what in ((p_values, "p_values"), (q_values, "q_values")):
        if isinstance(t, torch.Tensor) and t.dim() != 1:
            raise ValueError(f"{what}: expected a 1-D tensor, got shape {tuple(t.shape)}")
    p = _matrix(p_values, "p_values")
    q = _matrix(q_values, "q_values")
    if p.shape[0] + q.shape[0] == 0:
        raise ValueError("zero-size samples: the combined range is undefined")
    r = feature_histograms_device(p, q, n_bins=n_bins, epsilon=epsilon, min_count=0, propagate_nan=True)
    return float(r.kl[0].item())


class _Segment(NamedTuple):
    matrix: torch.Tensor
    names: List[str]
    ids: Optional[torch.Tensor]


def _segments(src, columns: Optional[Sequence[str]], what: str) -> Tuple[Optional[List[_Segment]], Any]:
    """-> (segments holding the wanted columns, the source's column names for the column choice)"""
    if isinstance(src, torch.Tensor):
        names = list(columns) if columns is not None else None
        if names is None:
            raise ValueError(f"{what}: a tensor needs its column names (columns=)")
        m = _matrix(src, what)
        if len(names) != m.shape[1]:
            raise ValueError(f"column-count mismatch: {len(names)} names for {m.shape[1]} {what} columns")
        return [_Segment(m, names, None)], names
    if isinstance(src, (list, tuple)) and src and isinstance(src[0], _Segment):
        return list(src), [n for s in src for n in s.names]
    return None, src.columns


def _frame_segment(df, cols: Sequence[str], dev) -> _Segment:
    """the wanted columns of a DataFrame as one float64 [n, nc] device matrix (NaN kept: the kernels drop it)"""
    a = np.ascontiguousarray(df[list(cols)].to_numpy(dtype=np.float64)).reshape(len(df), len(cols))
    return _Segment(torch.from_numpy(a).to(dev), list(cols), None)


def _locate(segs: List[_Segment], col: str) -> Tuple[int, int]:
    for si, s in enumerate(segs):
        if col in s.names:
            return si, s.names.index(col)
    raise KeyError(col)


def _numeric_names(src, names) -> List[str]:
    if isinstance(src, torch.Tensor) or isinstance(src, (list, tuple)):
        return list(names)
    return list(src.select_dtypes(include=[np.number]).columns)


def detect_training_serving_skew_device(train, serving, threshold: float = 0.1,
                                        numeric_cols: Optional[List[str]] = None,
                                        columns: Optional[Sequence[str]] = None) -> Dict[str, Any]:
    """metrics.detect_training_serving_skew with the per-column KL on the device.  train / serving: a DataFrame (its
    numeric columns go up as float64) or a 2-D f32 / f64 device tensor whose column names are ``columns``."""
    dev = L.device()
    tsegs, tnames = _segments(train, columns, "train")
    ssegs, snames = _segments(serving, columns, "serving")
    cols = M.skew_columns(_numeric_names(train, tnames), list(snames), numeric_cols)
    if not cols:
        return M.skew_report({}, threshold)
    if tsegs is None:
        tsegs = [_frame_segment(train, cols, dev)]
    if ssegs is None:
        ssegs = [_frame_segment(serving, cols, dev)]
    # group the columns by (train segment, serving segment): one launch sequence per pair
    groups: Dict[Tuple[int, int], List[Tuple[int, int, int]]] = {}
    for k, c in enumerate(cols):
        ta, ja = _locate(tsegs, c)
        sb, jb = _locate(ssegs, c)
        groups.setdefault((ta, sb), []).append((k, ja, jb))
    kl = np.full(len(cols), np.nan)
    st = np.full(len(cols), STATUS_TOO_FEW, np.int32)
    outs = []
    for (ta, sb), items in groups.items():
        r = feature_histograms_device(tsegs[ta].matrix, ssegs[sb].matrix, [j for _, j, _ in items],
                                      [j for _, _, j in items], tsegs[ta].ids, ssegs[sb].ids, n_bins=20,
                                      epsilon=1e-10, min_count=M.SKEW_MIN_COUNT, propagate_nan=False)
        outs.append((items, r))
    for items, r in outs:
        k = [i for i, _, _ in items]
        kl[k] = r.kl.cpu().numpy()
        st[k] = r.status.cpu().numpy()
    feature_kl = {c: round(float(kl[k]), 6) for k, c in enumerate(cols) if st[k] != STATUS_TOO_FEW}
    return M.skew_report(feature_kl, threshold)
