"""Independent NumPy reference of the diversified top-k (greedy MMR; the definition is the comment of
rihip_rank_topk_diverse in include/recommendit_hip.h), shared by tests/test_rerank_host.py and tests/test_gpu_rerank.py.

``mmr_row_scalar`` is the definition word for word: plain Python loops over np.float64 scalars, one rounded operation
per line.  ``mmr_row`` does the same operations in the same order for every candidate at once (the loop over the
components stays sequential; NumPy's elementwise multiply and add are two separately rounded passes, never an FMA), so
the large GPU cases take milliseconds; the host tests pin it to the scalar version bit for bit.
"""
import numpy as np

F = np.float64


def _classes(s, c):
    kc = len(c)
    elig = [i for i in range(kc) if c[i] >= 0 and not np.isnan(s[i])]
    nans = [i for i in range(kc) if c[i] >= 0 and np.isnan(s[i])]
    pads = [i for i in range(kc) if c[i] < 0]
    return elig, nans, pads


def _relevance(s, elig):
    """normalised score of every position (0 outside elig)"""
    rel = np.zeros(len(s), dtype=F)
    fin = [F(s[i]) for i in elig if np.isfinite(s[i])]
    if not fin:
        return rel
    lo, hi = min(fin), max(fin)
    if not hi > lo:
        return rel
    span = F(hi - lo)
    for i in elig:
        v = F(s[i])
        if v == np.inf:
            rel[i] = 1.0
        elif v == -np.inf:
            rel[i] = 0.0
        else:
            rel[i] = F(v - lo) / span
    return rel


def _finish(order, nans, pads, s, c, r, k):
    kc = len(c)
    ids = np.full(k, -1, np.int64)
    sc = np.full(k, -np.inf, F)
    rs = np.full(k, -np.inf, np.float32)
    seq = (list(order) + nans + pads)[:min(k, kc)]
    for t, i in enumerate(seq):
        ids[t] = c[i]
        sc[t] = s[i] if c[i] >= 0 else -np.inf
        rs[t] = r[i]
    return ids, sc, rs


def _better(oa, sa, pa, ob, sb, pb):
    if oa != ob:
        return oa > ob
    if sa != sb:
        return sa > sb
    return pa < pb


def mmr_row_scalar(s, c, r, k, delta, V, col0=0, w=None):
    """one request, scalar loops.  s f64 [kc], c i64 [kc], r f32 [kc]; V f64 [n_rows, >= col0 + w]"""
    w = V.shape[1] - col0 if w is None else w
    n_rows = V.shape[0]
    delta = F(delta)
    elig, nans, pads = _classes(s, c)
    rel = _relevance(s, elig)
    with np.errstate(all="ignore"):
        norm = {}
        for i in elig:
            n = F(0.0)
            if c[i] < n_rows:
                ss = F(0.0)
                for j in range(w):
                    x = F(V[c[i], col0 + j])
                    ss = F(ss + F(x * x))
                n = np.sqrt(ss)
            norm[i] = n
        one_minus = F(F(1.0) - delta)
        m = {i: F(0.0) for i in elig}
        order, left = [], list(elig)
        for t in range(min(k, len(c))):
            if not left:
                break
            if t > 0:
                p = order[-1]
                for i in left:
                    sim = F(0.0)
                    if norm[i] != 0.0 and norm[p] != 0.0:
                        dot = F(0.0)
                        for j in range(w):
                            dot = F(dot + F(F(V[c[i], col0 + j]) * F(V[c[p], col0 + j])))
                        sim = F(dot / F(norm[i] * norm[p]))
                    m[i] = sim if (t == 1 or sim > m[i]) else m[i]
            best = None
            for i in left:
                obj = F(F(one_minus * rel[i]) - F(delta * m[i]))
                if np.isnan(obj):
                    obj = F(-np.inf)
                if best is None or _better(obj, F(s[i]), i, *best):
                    best = (obj, F(s[i]), i)
            order.append(best[2])
            left.remove(best[2])
    return _finish(order, nans, pads, s, c, r, k)


def mmr_row(s, c, r, k, delta, V, col0=0, w=None):
    """mmr_row_scalar with the candidates of a step handled as arrays (same operations, same order, per candidate)"""
    w = V.shape[1] - col0 if w is None else w
    n_rows = V.shape[0]
    delta = F(delta)
    elig, nans, pads = _classes(s, c)
    rel = _relevance(s, elig)
    e = np.asarray(elig, dtype=np.int64)
    order = []
    if e.size:
        ce = np.asarray(c)[e]
        has = ce < n_rows
        X = np.zeros((e.size, w), dtype=F)
        X[has] = V[ce[has], col0:col0 + w]
        with np.errstate(all="ignore"):
            ss = np.zeros(e.size, dtype=F)
            for j in range(w):
                ss = ss + X[:, j] * X[:, j]
            norm = np.where(has, np.sqrt(ss), 0.0)
            one_minus = F(F(1.0) - delta)
            se, re = np.asarray(s, dtype=F)[e], rel[e]
            m = np.zeros(e.size, dtype=F)
            open_ = np.ones(e.size, dtype=bool)
            last = -1
            for t in range(min(k, len(c), e.size)):
                if t > 0:
                    dot = np.zeros(e.size, dtype=F)
                    for j in range(w):
                        dot = dot + X[:, j] * X[last, j]
                    sim = np.where((norm != 0.0) & (norm[last] != 0.0), dot / (norm * norm[last]), 0.0)
                    m = sim if t == 1 else np.where(sim > m, sim, m)
                obj = one_minus * re - delta * m
                obj = np.where(np.isnan(obj), -np.inf, obj)
                obj = np.where(open_, obj, -np.inf)
                # lexicographic best among the open ones: obj desc, score desc (==), position asc
                top = np.nonzero(open_ & (obj == obj[open_].max()))[0]
                top = top[se[top] == se[top].max()]
                last = int(top[0])
                open_[last] = False
                order.append(int(e[last]))
    return _finish(order, nans, pads, s, c, r, k)


def mmr_reference(scores, cand, rs, k, delta, V, col0=0, w=None, row=mmr_row):
    """batch: [nq, kc] inputs -> (ids i64, scores f64, retrieval scores f32), each [nq, k]"""
    out = [row(scores[q], cand[q], rs[q], k, delta, V, col0, w) for q in range(cand.shape[0])]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]))


def plain_topk(scores, cand, rs, k):
    """rihip_rank_topk / DataFrame.nlargest: score descending, ties keep the retrieval position; NaN scores after every
    number, padding last"""
    nq, kc = cand.shape
    ids = np.full((nq, k), -1, np.int64)
    sc = np.full((nq, k), -np.inf, F)
    r = np.full((nq, k), -np.inf, np.float32)
    for q in range(nq):
        elig, nans, pads = _classes(scores[q], cand[q])
        elig.sort(key=lambda i: (-scores[q][i], i))     # -0.0 and +0.0 give the same key
        o = _finish(elig, nans, pads, scores[q], cand[q], rs[q], k)
        ids[q], sc[q], r[q] = o
    return ids, sc, r


def intra_list_diversity(ids, V, col0=0, w=None):
    """mean of 1 - cos over the pairs of a list whose vectors both have a norm (metrics.py:168-190); 0 below two"""
    w = V.shape[1] - col0 if w is None else w
    vs = [V[i, col0:col0 + w] for i in ids if 0 <= i < V.shape[0]]
    tot, n = 0.0, 0
    for a in range(len(vs)):
        for b in range(a + 1, len(vs)):
            na, nb = np.linalg.norm(vs[a]), np.linalg.norm(vs[b])
            if na > 0 and nb > 0:
                tot += 1.0 - float(vs[a] @ vs[b]) / (na * nb)
                n += 1
    return tot / n if n else 0.0
