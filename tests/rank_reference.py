"""NumPy restatement of the rank-validation contract (include/recommendit_hip.h, "validation by exact full-catalogue
ranks"), written from the definition and not from the kernels.  Scores are f64, the key rule is applied literally,
exclusion is set membership.  Two independent metric routes: from the ranks, and from full stable lists."""
import math

import numpy as np


def scores64(U, Y):
    return U.astype(np.float64) @ Y.astype(np.float64).T


def case_inputs(rng, n_pairs, n_items, d, exact=True):
    """users with 0, 1 and several pairs; targets in row 0, the last row and the last ragged 128-row tile; exclusion
    rows that are empty, hold the target, hold every other item, or a random subset"""
    counts, left = [], n_pairs
    pattern = [0, 1, 3, 1, 2, 1, 0, 4]
    i = 0
    while left > 0:
        c = min(pattern[i % len(pattern)], left, n_items)
        counts.append(c)
        left -= c
        i += 1
    counts.append(0)
    n_users = len(counts)
    if exact:
        U = rng.randint(-8, 9, size=(n_users, d)).astype(np.float32) / 8
        Y = rng.randint(-8, 9, size=(n_items, d)).astype(np.float32) / 8
    else:
        U = rng.standard_normal((n_users, d))
        Y = rng.standard_normal((n_items, d))
        U = (U / np.linalg.norm(U, axis=1, keepdims=True)).astype(np.float32)
        Y = (Y / np.linalg.norm(Y, axis=1, keepdims=True)).astype(np.float32)
    off = np.zeros(n_users + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    special = [0, n_items - 1, (n_items - 1) // 128 * 128, max(n_items - 2, 0)]
    items = np.zeros(n_pairs, np.int32)
    e_off, e_items = [0], []
    sp = 0
    for u, c in enumerate(counts):
        t = rng.choice(n_items, size=c, replace=False)
        if c:
            t[0] = special[sp % len(special)]
            sp += 1
            t = np.unique(t)
            while len(t) < c:
                t = np.unique(np.append(t, rng.randint(n_items)))
            t = rng.permutation(t)
        items[off[u]:off[u + 1]] = t
        kind = u % 4
        if kind == 0:
            ex = np.zeros(0, np.int64)
        elif kind == 1:
            ex = np.union1d(t, rng.choice(n_items, size=min(n_items, 9), replace=False))
        elif kind == 2 and c:
            ex = np.setdiff1d(np.arange(n_items), t[:1])       # every other item: rank 0 for the first target
        else:
            ex = np.sort(rng.choice(n_items, size=rng.randint(0, n_items + 1), replace=False))
        e_items.append(ex.astype(np.int32))
        e_off.append(e_off[-1] + len(ex))
    return dict(U=U, Y=Y, pair_off=off, pair_item=items, excl_off=np.asarray(e_off, np.int64),
                excl_items=np.concatenate(e_items).astype(np.int32) if e_items else np.zeros(0, np.int32))


def outranks(s_j, j, s_t, t):
    """literal key rule: score descending, row ascending"""
    return (s_j > s_t) | ((s_j == s_t) & (j < t))


def ranks(U, Y, pair_off, pair_item, excl_off=None, excl_items=None):
    """-> (rank i64 [n_pairs], target_score f64 [n_pairs], err)"""
    n_users, n_items = U.shape[0], Y.shape[0]
    S = scores64(U, Y) + 0.0
    rank = np.zeros(len(pair_item), np.int64)
    tscore = np.zeros(len(pair_item), np.float64)
    err = 0
    rows = np.arange(n_items)
    for u in range(n_users):
        ex = set()
        if excl_off is not None:
            for j in excl_items[excl_off[u]:excl_off[u + 1]]:
                if 0 <= j < n_items:
                    ex.add(int(j))
                else:
                    err |= 1
        for p in range(pair_off[u], pair_off[u + 1]):
            t = int(pair_item[p])
            if not 0 <= t < n_items:
                err |= 2
                rank[p], tscore[p] = -1, 0.0
                continue
            allowed = np.array([j != t and j not in ex for j in range(n_items)], bool)
            rank[p] = int((outranks(S[u], rows, S[u, t], t) & allowed).sum())
            tscore[p] = S[u, t]
    return rank, tscore, err


def rank_interval(U, Y, pair_off, pair_item, excl_off, excl_items, tau):
    """-> (lo, undecided) per pair: a competitor whose row is bytewise equal to the target's is decided by index, any
    other one when its f64 score differs from the target's by more than tau"""
    n_users, n_items = U.shape[0], Y.shape[0]
    S = scores64(U, Y)
    lo = np.zeros(len(pair_item), np.int64)
    und = np.zeros(len(pair_item), np.int64)
    rows = np.arange(n_items)
    for u in range(n_users):
        ex = np.zeros(n_items, bool)
        if excl_off is not None:
            ex[excl_items[excl_off[u]:excl_off[u + 1]]] = True
        for p in range(pair_off[u], pair_off[u + 1]):
            t = int(pair_item[p])
            allowed = ~ex & (rows != t)
            same = (Y.view(np.uint32) == Y[t].view(np.uint32)).all(axis=1)
            diff = S[u] - S[u, t]
            above = np.where(same, rows < t, diff > tau)
            open_ = ~same & (np.abs(diff) <= tau)
            lo[p] = int((above & allowed).sum())
            und[p] = int((open_ & allowed).sum())
    return lo, und


def disc_tables(n):
    disc = [1.0 / math.log2(i + 2) for i in range(n)]
    idcg = [0.0] * (n + 1)
    s = 0
    for m in range(1, n + 1):
        s = s + disc[m - 1]
        idcg[m] = s
    return disc, idcg


def metrics_from_ranks(rank, pair_off, raw, k_values):
    """-> (vals [n_users, n_k, 3], rr [n_users], scored [n_users]): hits = the user's ranks in [0, k), DCG added in
    ascending rank order"""
    n = len(pair_off) - 1
    disc, idcg = disc_tables(max(k_values) + 1)
    vals = np.zeros((n, len(k_values), 3))
    rr = np.zeros(n)
    scored = np.zeros(n, np.uint8)
    for u in range(n):
        r = sorted(int(x) for x in rank[pair_off[u]:pair_off[u + 1]])
        cnt = len(r)
        if cnt == 0 or raw[u] <= 0:
            continue
        scored[u] = 1
        good = [x for x in r if x >= 0]
        rr[u] = 1.0 / (1 + good[0]) if good else 0.0
        for a, k in enumerate(k_values):
            dcg, hits = 0.0, 0
            for x in good:
                if x < k:
                    dcg += disc[x]
                    hits += 1
            ideal = idcg[min(int(raw[u]), k)]
            vals[u, a] = (dcg / ideal if ideal else 0.0, hits / cnt, hits / k if k else 0.0)
    return vals, rr, scored


def full_lists(U, Y, excl_off=None, excl_items=None):
    """every user's exact list over the whole catalogue: full stable argsort by descending score (ties: row ascending),
    the excluded rows removed"""
    S = scores64(U, Y) + 0.0
    out = []
    for u in range(U.shape[0]):
        order = np.argsort(-S[u], kind="stable")
        if excl_off is not None:
            ex = set(int(j) for j in excl_items[excl_off[u]:excl_off[u + 1]])
            order = np.array([j for j in order if j not in ex], np.int64)
        out.append(order)
    return out


def metrics_from_lists(lists, pair_off, pair_item, raw, k_values):
    """the list route: walk the list, hit = membership in the user's truth set"""
    n = len(pair_off) - 1
    vals = np.zeros((n, len(k_values), 3))
    rr = np.zeros(n)
    scored = np.zeros(n, np.uint8)
    for u in range(n):
        truth = set(int(x) for x in pair_item[pair_off[u]:pair_off[u + 1]])
        if not truth or raw[u] <= 0:
            continue
        scored[u] = 1
        lst = [int(x) for x in lists[u]]
        for i, x in enumerate(lst):
            if x in truth:
                rr[u] = 1.0 / (i + 1)
                break
        for a, k in enumerate(k_values):
            dcg = sum(1.0 / math.log2(i + 2) for i, x in enumerate(lst[:k]) if x in truth)
            ideal = sum(1.0 / math.log2(i + 2) for i in range(min(int(raw[u]), k)))
            hits = len([x for x in lst[:k] if x in truth])
            vals[u, a] = (dcg / ideal if ideal else 0.0, hits / len(truth), hits / k if k else 0.0)
    return vals, rr, scored
