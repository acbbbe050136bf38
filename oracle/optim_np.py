"""NumPy references for the optimiser, row-sparse and sampler kernels (TEST INFRASTRUCTURE).

Written from the contracts in include/recommendit_hip.h, not from the kernels' structure: float64 arithmetic on the
float32 values the ABI receives, plain Python grouping instead of a sort, and an integer restatement of the sampler's
documented keying.  Pinned against stock torch / NumPy in tests/test_optim_host.py; used by
tests/test_gpu_optim_kernels.py.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from .two_tower_np import splitmix64

U32 = 2.0 ** -24  # unit roundoff of float32


# --------------------------------------------------------------------------- norm and clip
def sumsq_f64(x) -> float:
    x = np.asarray(x).astype(np.float64).ravel()
    return float(np.sum(x * x))


def clip_coef_f32(sumsq: float, max_norm: float) -> Tuple[np.float32, np.float32]:
    """(coef, total_norm) of clip_grad_norm_: the norm is rounded to float32 once, the rest is float32."""
    tn = np.float32(math.sqrt(float(sumsq)))
    c = np.float32(max_norm) / (tn + np.float32(1e-6))
    return (c if c < np.float32(1.0) else np.float32(1.0)), tn


# --------------------------------------------------------------------------- Adam
def adam_hyper(lr32, b1_32, b2_32, t: int) -> Tuple[float, float]:
    """(lr / (1 - b1^t), sqrt(1 - b2^t)) in float64 from the float32 lr and betas the ABI receives.  1 - b^t is
    taken as -expm1(t log b): no cancellation at small t, no overflow at large t."""
    lr, b1, b2 = float(np.float32(lr32)), float(np.float32(b1_32)), float(np.float32(b2_32))
    bc1 = -math.expm1(t * math.log(b1))
    bc2 = -math.expm1(t * math.log(b2))
    return lr / bc1, math.sqrt(bc2)


class AdamOut(NamedTuple):
    p: np.ndarray      # updated parameter
    m: np.ndarray      # updated first moment
    v: np.ndarray      # updated second moment
    s_m: np.ndarray    # |b1 m| + |(1 - b1) g'|: the magnitude the rounding of m is relative to
    upd: np.ndarray    # lr' m / denom (what is subtracted from p)
    denom: np.ndarray  # sqrt(v) / sqrt(bc2) + eps


def adam_f64(p, g, m, v, hyper, b1, b2, eps, wd, coef: Optional[float] = None) -> AdamOut:
    """One torch.optim.Adam(weight_decay=wd) step (coupled L2) in float64.  hyper = (lr / bc1, sqrt(bc2)); b1, b2,
    eps, wd and coef are the float32 constants of the call; g is scaled by coef before anything else."""
    p, g, m, v = (np.asarray(a).astype(np.float64) for a in (p, g, m, v))
    b1, b2, eps, wd = (float(np.float32(x)) for x in (b1, b2, eps, wd))
    lr_bc1, sqrt_bc2 = float(hyper[0]), float(hyper[1])
    if coef is not None:
        g = g * float(np.float32(coef))
    if wd != 0.0:
        g = g + wd * p
    m_new = b1 * m + (1.0 - b1) * g
    v_new = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v_new) / sqrt_bc2 + eps
    upd = lr_bc1 * m_new / denom
    return AdamOut(p - upd, m_new, v_new, np.abs(b1 * m) + np.abs((1.0 - b1) * g), upd, denom)


# --------------------------------------------------------------------------- row-sparse path
def group_rows(ids, n_rows: int) -> Tuple[np.ndarray, List[np.ndarray]]:
    """uniq (ascending, each row once) and, per entry, the batch positions of its samples in batch order.  An id that
    is negative, or >= n_rows when n_rows > 0, counts as the padding row 0."""
    rows: dict = {}
    for pos, i in enumerate(np.asarray(ids, dtype=np.int64).tolist()):
        if i < 0 or (n_rows > 0 and i >= n_rows):
            i = 0
        rows.setdefault(i, []).append(pos)
    uniq = sorted(rows)
    return np.asarray(uniq, dtype=np.int64), [np.asarray(rows[u], dtype=np.int64) for u in uniq]


def reduce_rows_f64(dX, uniq, positions) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(G, A, count): G[k] = float64 sum of the dX rows of uniq[k] (zeros for the padding row 0), A[k] = the sum of
    their absolute values (the scale of the summation error bound), count[k] = number of samples."""
    dX = np.asarray(dX)
    d = dX.shape[1]
    G = np.zeros((len(uniq), d), np.float64)
    A = np.zeros((len(uniq), d), np.float64)
    cnt = np.zeros(len(uniq), np.int64)
    for k, (u, pos) in enumerate(zip(np.asarray(uniq).tolist(), positions)):
        cnt[k] = len(pos)
        if u == 0:
            continue
        x = dX[pos].astype(np.float64)
        G[k] = x.sum(axis=0)
        A[k] = np.abs(x).sum(axis=0)
    return G, A, cnt


# --------------------------------------------------------------------------- negative sampler
def sample_negatives_np(users, catalog, rated_keys, key_stride: int, seed: int, max_attempts: int
                        ) -> Tuple[np.ndarray, int]:
    """Exact integer restatement of rihip_sample_negatives: sample i draws attempt a from
    r = splitmix64(splitmix64(seed ^ splitmix64(i)) + a), pick = catalog[((r >> 32) * n_catalog) >> 32], and keeps the
    first pick whose key users[i] * key_stride + pick is not in rated_keys (sorted); after max_attempts it keeps the
    last pick and counts as given up.  Returns (neg, gave_up)."""
    users = np.asarray(users, dtype=np.int64)
    catalog = np.asarray(catalog, dtype=np.int64)
    rated = np.asarray(rated_keys, dtype=np.int64)
    n, nc = users.shape[0], np.uint64(catalog.shape[0])
    base = splitmix64(np.uint64(seed) ^ splitmix64(np.arange(n, dtype=np.uint64)))
    neg = np.full(n, catalog[0], dtype=np.int64)
    ok = np.zeros(n, dtype=bool)
    for a in range(max_attempts):
        live = np.flatnonzero(~ok)
        if live.size == 0:
            break
        with np.errstate(over="ignore"):
            r = splitmix64(base[live] + np.uint64(a))
            pick = catalog[(((r >> np.uint64(32)) * nc) >> np.uint64(32)).astype(np.int64)]
        key = users[live] * np.int64(key_stride) + pick
        at = np.searchsorted(rated, key)
        member = (at < rated.shape[0]) & (rated[np.minimum(at, max(rated.shape[0] - 1, 0))] == key) \
            if rated.shape[0] else np.zeros(live.size, dtype=bool)
        neg[live] = pick
        ok[live] = ~member
    return neg, int((~ok).sum())
