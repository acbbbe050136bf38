"""Host side of the popularity-weighted negative sampler (not in the reference, which draws uniformly).

``alias_table`` turns item weights into the two integer arrays that ``rihip_sample_negatives_multi`` reads: Walker's
alias method in Vose's construction.  A draw picks a column j uniformly and keeps it when a 32-bit coin is below
``prob[j]``, else takes ``alias[j]``: two dependent reads per attempt, whatever the catalogue size.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

_TWO32 = 4294967296.0


def popularity_weights(counts, alpha: float) -> np.ndarray:
    """(count + 1)^alpha, the word2vec / YouTube-DNN smoothing between uniform (alpha = 0) and popularity (alpha = 1).
    The + 1 is a choice: it keeps items that nobody liked drawable as negatives."""
    alpha = float(alpha)
    if not np.isfinite(alpha):
        raise ValueError(f"popularity_weights: alpha must be finite, got {alpha!r}")
    counts = np.asarray(counts, dtype=np.float64)
    if counts.ndim != 1 or not np.isfinite(counts).all() or (counts < 0).any():
        raise ValueError("popularity_weights: counts must be a 1-d array of finite values >= 0")
    return np.power(counts + 1.0, alpha)


def alias_table(weights) -> Tuple[np.ndarray, np.ndarray]:
    """(prob uint32 [n], alias int32 [n]) for weights [n]: column j is kept with probability prob[j] / 2^32 and hands
    over to item alias[j] otherwise, so item j is drawn with probability
        q_j = (prob[j] / 2^32 + sum over columns c != j with alias[c] == j of (1 - prob[c] / 2^32)) / n.
    Vose's construction in float64; the quantisation of prob to 2^-32 moves q_j by at most 2^-32 (each column by at most
    2^-32 / n, and an item collects from at most n columns).  A column that is always kept holds alias[j] = j (its
    probability, 1, has no 32-bit form: the kernel reads alias[j] == j as "always j").  An item of weight zero gets
    prob 0 and is nobody's alias: it is never drawn.  Weights must be finite, >= 0 and sum to more than 0 (ValueError)."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.shape[0] < 1:
        raise ValueError("alias_table: weights must be a non-empty 1-d array")
    if w.shape[0] > 2 ** 31 - 1:
        raise ValueError("alias_table: more than 2^31 - 1 weights")
    if not np.isfinite(w).all():
        raise ValueError("alias_table: weights must be finite")
    if (w < 0).any():
        raise ValueError("alias_table: weights must be >= 0")
    total = float(w.sum())
    if not (total > 0 and np.isfinite(total)):
        raise ValueError("alias_table: the weights must have a positive, finite sum")
    n = w.shape[0]
    p = w * (n / total)                       # mean 1: a column's own share of its 1/n
    keep = np.ones(n, dtype=np.float64)
    alias = np.arange(n, dtype=np.int64)
    # zero-weight columns are served first (popped last-in-first-out), while there is certainly a donor left
    order = np.argsort(-p, kind="stable")
    small = [int(j) for j in order if p[j] < 1.0]
    large = [int(j) for j in order[::-1] if p[j] >= 1.0]
    p = p.tolist()
    while small and large:
        s, g = small.pop(), large[-1]
        keep[s], alias[s] = p[s], g
        p[g] = (p[g] + p[s]) - 1.0
        if p[g] < 1.0:
            large.pop()
            small.append(g)
    # what is left on either list has p = 1 up to rounding: always kept.  (A weight-zero column cannot be left: the
    # others left with it would have to hold its share; it is given to the heaviest item all the same.)
    for s in small:
        if w[s] == 0.0:
            keep[s], alias[s] = 0.0, int(np.argmax(w))
    fixed = alias == np.arange(n)
    prob = np.clip(np.rint(keep * _TWO32), 0.0, _TWO32 - 1.0)
    prob[fixed] = _TWO32 - 1.0
    return prob.astype(np.uint32), alias.astype(np.int32)


def alias_probabilities(prob, alias) -> np.ndarray:
    """q_j of the docstring above (float64): what the integer arrays imply, for checks and for logQ corrections."""
    prob = np.asarray(prob, dtype=np.uint32)
    alias = np.asarray(alias, dtype=np.int64)
    n = prob.shape[0]
    cols = np.arange(n)
    alias = np.where((alias < 0) | (alias >= n), cols, alias)
    k = np.where(alias == cols, 1.0, prob.astype(np.float64) / _TWO32)
    q = k.copy()
    np.add.at(q, alias, 1.0 - k)
    return q / n
