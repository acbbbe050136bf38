"""NumPy float64 restatement of the cold-start definition (rihip_fold_in_users in include/recommendit_hip.h): the fold-in
query, the slot's ranking-feature row, the error word and the popularity fallback; plus the cluster construction the
behaviour tests share.  Plain loops: this is the definition, not a fast path."""
import math
from fractions import Fraction

import numpy as np

NG = 18
DEFAULT_ROW = np.array([3.5, 0.0, 0.5, 0.0, 0.3, 0.3] + [0.0] * NG)


def _fma(a, b, c):
    """round(a * b + c) once: exact rational arithmetic, one correctly rounded conversion"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _valid(item, r):
    return item >= 0 and 1 <= r <= 5


def error_word(items, ratings):
    e = 0
    for it, r in zip(np.asarray(items).tolist(), np.asarray(ratings).tolist()):
        e |= (1 if it < 0 else 0) | (2 if not 1 <= r <= 5 else 0)
    return e


def fold_in_reference(offsets, items, ratings, V, row_of, mu, min_rating=4, weighting=0, beta=1.0):
    """-> (q f32 [nq, d], flags i32 [nq], n f64 [nq]); V [n_rows, >= d] (its first d = len(mu) columns are read)"""
    offsets = np.asarray(offsets, dtype=np.int64)
    nq, d = offsets.shape[0] - 1, np.asarray(mu).shape[0]
    V = np.asarray(V)[:, :d].astype(np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    q = np.zeros((nq, d), np.float32)
    flags = np.zeros(nq, np.int32)
    norms = np.zeros(nq, np.float64)
    for s in range(nq):
        W, acc = 0, np.zeros(d, np.float64)
        for j in range(offsets[s], offsets[s + 1]):
            it, r = int(items[j]), int(ratings[j])
            if not _valid(it, r) or r < min_rating or it >= row_of.shape[0]:
                continue
            row = int(row_of[it])
            if not 0 <= row < V.shape[0]:
                continue
            w = r - (min_rating - 1) if weighting else 1
            W += w
            acc += w * V[row]
        if W == 0:
            flags[s] = 1
            continue
        m = acc / W - beta * mu
        n = math.sqrt(float(np.sum(m * m)))
        norms[s] = n
        if n < 1e-12:
            flags[s] = 1
            continue
        q[s] = (m / n).astype(np.float32)
    return q, flags, norms


def feature_rows_reference(offsets, items, ratings, item_tab=None, user_meta=None):
    """-> rows f64 [nq, 24]: the arithmetic of ltr_stats_kernel / ltr_finalize_user_kernel on integer accumulators"""
    offsets = np.asarray(offsets, dtype=np.int64)
    nq = offsets.shape[0] - 1
    n_item_rows = 0 if item_tab is None else item_tab.shape[0]
    rows = np.tile(DEFAULT_ROW, (nq, 1))
    for s in range(nq):
        cnt = tot = liked = 0
        acc = [0] * NG
        for j in range(offsets[s], offsets[s + 1]):
            it, r = int(items[j]), int(ratings[j])
            if not _valid(it, r):
                continue
            cnt += 1
            tot += r
            if r >= 4 and 0 < it < n_item_rows:
                liked += 1
                for g in range(NG):
                    if item_tab[it, 5 + g] != 0:
                        acc[g] += r - 3
        if cnt == 0:
            continue
        rows[s, 0] = np.float64(tot) / np.float64(cnt)
        rows[s, 1] = np.float64(np.float32(np.log1p(np.float64(cnt))))
        if user_meta is not None:
            rows[s, 2:6] = user_meta[s]
        v = [np.float64(a) / np.float64(liked) if liked > 0 else 0.0 for a in acc]
        ss = 0.0
        for g in range(NG):
            ss = _fma(v[g], v[g], ss)
        norm = math.sqrt(ss)
        rows[s, 6:] = [x / norm if norm > 0.0 else x for x in v]
    return rows


def default_popularity(item_tab, stored_ids):
    """the stored ids by item-table column log_rating_count descending, ties to the lower id (an id outside the table:
    the default row's 0.0)"""
    ids = sorted(set(int(i) for i in stored_ids))
    return [i for _, i in sorted((-(float(item_tab[i, 1]) if 0 <= i < item_tab.shape[0] else 0.0), i) for i in ids)]


def passes(tag, pred):
    any_of, all_of, none_of = (int(x) & 0xFFFFFFFF for x in pred)
    return (any_of == 0 or tag & any_of != 0) and tag & all_of == all_of and tag & none_of == 0


def popularity_reference(pop, k, width, history=None, tag_of=None, pred=None):
    """the reference's _popularity_recommendations: the first k entries of `pop` that pass `pred` over tag_of[id] and are
    not in `history` -> (ids i64, scores f64, retrieval scores f32) of `width` entries, -1 / -inf / -inf where it ends"""
    ids = np.full(width, -1, np.int64)
    sc = np.full(width, -np.inf, np.float64)
    rs = np.full(width, -np.inf, np.float32)
    hist = set() if history is None else set(int(i) for i in history)
    rank = 0
    for it in pop:
        if rank >= width:
            break
        if int(it) in hist or (pred is not None and not passes(int(tag_of.get(int(it), 0)), pred)):
            continue
        rank += 1
        ids[rank - 1] = int(it)
        sc[rank - 1] = 1.0 - (rank / (k + 1))
        rs[rank - 1] = 0.0
    return ids, sc, rs


# ---- the behaviour construction ------------------------------------------------------------------------------------
N_CLUSTERS, PER_CLUSTER, D_CLUSTER = 8, 256, 32


def cluster_case(seed=11):
    """8 orthonormal centres in d = 32, 256 items each = normalise(centre + 0.05 * noise); item id = row + 1; slot c
    likes 20 items of cluster c (ratings 4 / 5) and dislikes 5 items of other clusters (ratings 1 / 2).
    -> (X f32 [2048, 32], item_ids i64, cluster of every row, histories: list of [(item, rating)])"""
    rng = np.random.default_rng(seed)
    centres = np.linalg.qr(rng.standard_normal((D_CLUSTER, D_CLUSTER)))[0][:N_CLUSTERS]
    cluster = np.repeat(np.arange(N_CLUSTERS), PER_CLUSTER)
    X = centres[cluster] + 0.05 * rng.standard_normal((cluster.shape[0], D_CLUSTER))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    item_ids = np.arange(1, cluster.shape[0] + 1, dtype=np.int64)
    hists = []
    for c in range(N_CLUSTERS):
        own = rng.choice(np.nonzero(cluster == c)[0], 20, replace=False)
        other = rng.choice(np.nonzero(cluster != c)[0], 5, replace=False)
        hists.append([(int(item_ids[r]), int(rng.integers(4, 6))) for r in own]
                     + [(int(item_ids[r]), int(rng.integers(1, 3))) for r in other])
    return X, item_ids, cluster, hists
