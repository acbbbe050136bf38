"""Diversified top-k: greedy Maximal Marginal Relevance (MMR) re-ranking on the device.

Not in the reference, whose chain ends in ``nlargest(k)`` (src/serving/recommender.py:346) and only *measures* list
diversity (``intra_list_diversity``, src/evaluation/metrics.py:168-190).  ``rihip_rank_topk_diverse`` (definition:
include/recommendit_hip.h) trades the ranker score against exactly that cosine: ``diversity`` = 0 is the plain top-k,
larger values push similar items apart.  GpuRecommendationPipeline uses it as its last stage when a ``diversity`` is given;
``mmr_rerank_device`` is the same stage for callers with their own chain.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _lib as L

MAX_CANDIDATES = 4096     # kc of rihip_rank_topk_diverse
MAX_WIDTH = 256           # w


def check_diversity(diversity) -> float:
    """the weight as a float in [0, 1]; ValueError otherwise (NaN included)"""
    try:
        d = float(diversity)
    except (TypeError, ValueError):
        raise ValueError(f"diversity={diversity!r} is not a number") from None
    if math.isnan(d) or d < 0.0 or d > 1.0:
        raise ValueError(f"diversity={d} outside [0, 1]")
    return d


def check_shape(kc: int, k: int, width: int) -> None:
    if not 1 <= kc <= MAX_CANDIDATES:
        raise ValueError(f"{kc} candidates per request: the diversified top-k takes 1..{MAX_CANDIDATES}")
    if k < 1:
        raise ValueError(f"k={k} < 1")
    if not 1 <= width <= MAX_WIDTH:
        raise ValueError(f"vector width {width}: the diversified top-k takes 1..{MAX_WIDTH}")


def check_table(vectors: torch.Tensor, col0: int = 0, width: Optional[int] = None) -> Tuple[int, int]:
    """(col0, width) of the columns used of a [n, >= col0 + width] float64 table; ValueError otherwise"""
    if not isinstance(vectors, torch.Tensor) or vectors.dim() != 2 or vectors.dtype != torch.float64:
        raise ValueError("vectors: a float64 [n, w] tensor indexed by item id")
    col0 = int(col0)
    width = vectors.shape[1] - col0 if width is None else int(width)
    if col0 < 0 or width < 1 or col0 + width > vectors.shape[1]:
        raise ValueError(f"columns {col0}..{col0 + width - 1} of a table of {vectors.shape[1]} columns")
    if vectors.shape[0] and vectors.stride(1) != 1:
        raise ValueError("vectors: rows must be contiguous (stride 1 along the columns)")
    if width > MAX_WIDTH:
        raise ValueError(f"vector width {width}: the diversified top-k takes 1..{MAX_WIDTH}")
    return col0, width


def launch(scores: torch.Tensor, cand: torch.Tensor, retrieval_scores: torch.Tensor, k: int, diversity: float,
           vectors: torch.Tensor, col0: int, width: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """one launch of rihip_rank_topk_diverse on checked arguments (contiguous device tensors of the ABI's dtypes)"""
    nq, kc = cand.shape
    dev = cand.device
    ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
    top = torch.empty((nq, k), dtype=torch.float64, device=dev)
    trs = torch.empty((nq, k), dtype=torch.float32, device=dev)
    n_rows = vectors.shape[0]
    ld = vectors.stride(0) if n_rows > 1 else vectors.shape[1]
    L.check(L.lib().rihip_rank_topk_diverse(scores.data_ptr(), cand.data_ptr(), retrieval_scores.data_ptr(), nq, kc, k,
                                            vectors.data_ptr(), n_rows, ld, col0, width, diversity, ids.data_ptr(),
                                            top.data_ptr(), trs.data_ptr(), L.stream_ptr()), "rank_topk_diverse")
    return ids, top, trs


@torch.no_grad()
def mmr_rerank_device(scores: torch.Tensor, cand: torch.Tensor, retrieval_scores: torch.Tensor, k: int, diversity: float,
                      vectors: torch.Tensor, col0: int = 0, width: Optional[int] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Greedy MMR re-ranking of every request's candidates -> (item ids i64, ranker scores f64, retrieval scores f32),
    each [nq, k] on the device, in selection order.

    scores f64 / cand i64 (-1 = padding) / retrieval_scores f32: [nq, kc] in retrieval order, kc <= 4096.  vectors:
    device float64 [n, >= col0 + width], row index = item id (item-tower embeddings, genre vectors, ...); width None =
    every column from col0 on, at most 256.  diversity in [0, 1]: 0 is rihip_rank_topk bit for bit, 1 ignores the score
    after the first pick.  Candidates with NaN scores, then padding, come after the eligible ones; slots past kc are
    -1 / -inf.  One launch on the current stream, no synchronisation: capturable in a hipGraph.  Bad arguments raise
    ValueError before anything is launched."""
    d = check_diversity(diversity)
    if not (isinstance(cand, torch.Tensor) and cand.dim() == 2):
        raise ValueError("cand: an int64 [nq, kc] tensor")
    if tuple(scores.shape) != tuple(cand.shape) or tuple(retrieval_scores.shape) != tuple(cand.shape):
        raise ValueError(f"scores {tuple(scores.shape)} / retrieval_scores {tuple(retrieval_scores.shape)} do not match "
                         f"cand {tuple(cand.shape)}")
    col0, width = check_table(vectors, col0, width)
    k = int(k)
    check_shape(cand.shape[1], k, width)
    dev = L.device()
    if vectors.device != dev:
        raise ValueError(f"vectors live on {vectors.device}, the stage runs on {dev}")
    return launch(scores.to(device=dev, dtype=torch.float64).contiguous(), L.i64c(cand), L.f32c(retrieval_scores), k, d,
                  vectors, col0, width)
