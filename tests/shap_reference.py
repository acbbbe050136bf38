"""Independent NumPy references of the per-feature TreeSHAP contributions (the definition is the comment of
rihip_gbdt_predict_contrib in include/recommendit_hip.h), shared by tests/test_contrib_host.py, tests/test_gpu_contrib.py
and tools/make_golden_g13.py.

``brute_force`` is the Shapley value word for word: for every subset S of the features a tree uses, the path-dependent
conditional expectation (follow the row at a split on a feature of S, average the children by count elsewhere), then the
Shapley weights.  Exponential: trees with at most 10 used features only.  ``tree_shap`` is the recursive Algorithm 2 of
Lundberg, Erion and Lee ("Consistent individualized feature attribution for tree ensembles") with a selectable
dtype (np.float64 / np.longdouble).  Both take the model dict of ``parse_model`` -- oracle.gbdt_np.parse_text_model
plus the ``leaf_count`` / ``internal_count`` lines it does not keep -- and decide with oracle.gbdt_np._decide_left.
``write_text_model_with_counts`` is oracle.gbdt_np.write_text_model with those two lines added, the counts taken from
a background sample routed through every tree plus 1 per leaf (no count is zero; an internal count is the sum of its
children's, as LightGBM writes them).
"""
import itertools
import math

import numpy as np

from oracle import gbdt_np as G


def parse_model(text):
    """parse_text_model + per tree ``leaf_count`` / ``internal_count`` (int64 arrays, or None when the line is absent)"""
    model = G.parse_text_model(text)
    blocks = text.split("Tree=")[1:]
    assert len(blocks) == len(model["trees"])
    for t, blk in zip(model["trees"], blocks):
        kv = dict(ln.split("=", 1) for ln in blk.splitlines() if "=" in ln)
        for key in ("leaf_count", "internal_count"):
            t[key] = np.array([int(x) for x in kv[key].split()], dtype=np.int64) if key in kv else None
    return model


def _rows(X):
    return np.asarray(X, dtype=np.float32).astype(np.float64)   # the device reads f32 features


def _goes_left(t, node, x):
    return bool(G._decide_left(np.array([x[t["split_feature"][node]]]), t, node)[0])


def _count(t, child):
    return int(t["internal_count"][child]) if child >= 0 else int(t["leaf_count"][~child])


def expected_value(model, dtype=np.float64):
    """sum over trees of sum(leaf_value * leaf_count) / count(root); a single-leaf tree adds its value"""
    e = dtype(0)
    for t in model["trees"]:
        if t["num_leaves"] <= 1:
            e = e + dtype(t["leaf_value"][0] if t["leaf_value"].size else 0.0)
            continue
        s = dtype(0)
        for v, c in zip(t["leaf_value"], t["leaf_count"]):
            s = s + dtype(v) * dtype(int(c))
        e = e + s / dtype(int(t["internal_count"][0]))
    return e


def _finish(model, phi, dtype):
    if model.get("average_output") and model["trees"]:
        phi = phi / dtype(len(model["trees"]))
    return phi


# ---- (a) brute force ---------------------------------------------------------------------------------------------
def _cond_exp(t, x, S, node=0):
    if node < 0:
        return float(t["leaf_value"][~node])
    l, r = int(t["left_child"][node]), int(t["right_child"][node])
    if int(t["split_feature"][node]) in S:
        return _cond_exp(t, x, S, l if _goes_left(t, node, x) else r)
    return (_count(t, l) * _cond_exp(t, x, S, l) + _count(t, r) * _cond_exp(t, x, S, r)) / _count(t, node)


def brute_force(model, X):
    """f64 [n, F + 1]: exact Shapley values of every tree's path-dependent value function, summed over trees; the last
    column is the value of the empty set (the expected value)"""
    X = _rows(X)
    nf = model["max_feature_idx"] + 1
    out = np.zeros((X.shape[0], nf + 1), dtype=np.float64)
    for t in model["trees"]:
        if t["num_leaves"] <= 1:
            out[:, nf] += t["leaf_value"][0] if t["leaf_value"].size else 0.0
            continue
        used = sorted(set(int(f) for f in t["split_feature"][:t["num_leaves"] - 1]))
        M = len(used)
        assert M <= 10, "brute force is exponential in the features a tree uses"
        for r in range(X.shape[0]):
            val = {}
            for k in range(M + 1):
                for S in itertools.combinations(used, k):
                    val[S] = _cond_exp(t, X[r], frozenset(S))
            out[r, nf] += val[()]
            for f in used:
                rest = [g for g in used if g != f]
                for k in range(M):
                    wgt = math.factorial(k) * math.factorial(M - k - 1) / math.factorial(M)
                    for S in itertools.combinations(rest, k):
                        out[r, f] += wgt * (val[tuple(sorted(S + (f,)))] - val[S])
    return _finish(model, out, np.float64)


# ---- (b) recursive Algorithm 2 ------------------------------------------------------------------------------------
def _extend(m, pz, po, pf, T):
    l = len(m)
    m.append([pf, pz, po, T(1) if l == 0 else T(0)])
    for i in range(l - 1, -1, -1):
        m[i + 1][3] = m[i + 1][3] + po * m[i][3] * T(i + 1) / T(l + 1)
        m[i][3] = pz * m[i][3] * T(l - i) / T(l + 1)


def _unwind(m, i, T):
    l = len(m) - 1
    o, z = m[i][2], m[i][1]
    n = m[l][3]
    for j in range(l - 1, -1, -1):
        if o != 0:
            t = m[j][3]
            m[j][3] = n * T(l + 1) / (T(j + 1) * o)
            n = t - m[j][3] * z * (T(l - j) / T(l + 1))
        else:
            m[j][3] = (m[j][3] / z) / (T(l - j) / T(l + 1))
    for j in range(i, l):
        m[j][0], m[j][1], m[j][2] = m[j + 1][0], m[j + 1][1], m[j + 1][2]
    m.pop()


def _unwound_sum(m, i, T):
    l = len(m) - 1
    o, z = m[i][2], m[i][1]
    n = m[l][3]
    total = T(0)
    for j in range(l - 1, -1, -1):
        if o != 0:
            tmp = n * T(l + 1) / (T(j + 1) * o)
            total = total + tmp
            n = m[j][3] - tmp * z * (T(l - j) / T(l + 1))
        else:
            total = total + (m[j][3] / z) / (T(l - j) / T(l + 1))
    return total


def _recurse(t, x, phi, node, m, pz, po, pf, T):
    m = [list(e) for e in m]
    _extend(m, pz, po, pf, T)
    if node < 0:
        v = T(t["leaf_value"][~node])
        for i in range(1, len(m)):
            phi[m[i][0]] = phi[m[i][0]] + _unwound_sum(m, i, T) * (m[i][2] - m[i][1]) * v
        return
    l, r = int(t["left_child"][node]), int(t["right_child"][node])
    hot, cold = (l, r) if _goes_left(t, node, x) else (r, l)
    f = int(t["split_feature"][node])
    iz, io = T(1), T(1)
    for k in range(1, len(m)):
        if m[k][0] == f:
            iz, io = m[k][1], m[k][2]
            _unwind(m, k, T)
            break
    cn = T(_count(t, node))
    _recurse(t, x, phi, hot, m, iz * (T(_count(t, hot)) / cn), io, f, T)
    _recurse(t, x, phi, cold, m, iz * (T(_count(t, cold)) / cn), T(0), f, T)


def tree_shap(model, X, dtype=np.float64):
    """dtype [n, F + 1]: Algorithm 2 evaluated in ``dtype`` throughout; the last column is ``expected_value``"""
    T = dtype
    X = _rows(X)
    nf = model["max_feature_idx"] + 1
    out = np.zeros((X.shape[0], nf + 1), dtype=T)
    out[:, nf] = expected_value(model, T)
    for t in model["trees"]:
        if t["num_leaves"] <= 1:
            continue
        for r in range(X.shape[0]):
            phi = [T(0)] * nf
            _recurse(t, X[r], phi, 0, [], T(1), T(1), -1, T)
            for f in range(nf):
                out[r, f] = out[r, f] + phi[f]
    return _finish(model, out, T)


# ---- (c) text writer with counts ------------------------------------------------------------------------------------
def add_counts(model, background):
    """leaf_count / internal_count of every tree: rows of ``background`` reaching the leaf, plus 1; internal = sum"""
    B = _rows(background)
    for t in model["trees"]:
        nl = t["num_leaves"]
        if nl <= 1:
            t["leaf_count"], t["internal_count"] = None, None
            continue
        lc = np.ones(nl, dtype=np.int64)
        node = np.zeros(B.shape[0], dtype=np.int64)
        active = node >= 0
        while active.any():
            for nd in np.unique(node[active]):
                sel = active & (node == nd)
                left = G._decide_left(B[sel, t["split_feature"][nd]], t, int(nd))
                node[sel] = np.where(left, t["left_child"][nd], t["right_child"][nd])
            active = node >= 0
        np.add.at(lc, ~node, 1)
        ic = np.zeros(nl - 1, dtype=np.int64)

        def total(n):
            if n < 0:
                return int(lc[~n])
            ic[n] = total(int(t["left_child"][n])) + total(int(t["right_child"][n]))
            return int(ic[n])
        total(0)
        t["leaf_count"], t["internal_count"] = lc, ic
    return model


def write_text_model_with_counts(model, average_output=None):
    """oracle.gbdt_np.write_text_model + the leaf_count / internal_count lines of ``add_counts``"""
    text = G.write_text_model(model, average_output)
    head, *blocks = text.split("Tree=")
    out = [head]
    for t, blk in zip(model["trees"], blocks):
        if t.get("leaf_count") is not None:
            extra = ("leaf_count=" + " ".join(str(int(c)) for c in t["leaf_count"]) + "\n" +
                     "internal_count=" + " ".join(str(int(c)) for c in t["internal_count"]) + "\n")
            blk = blk.replace("is_linear=0\n", extra + "is_linear=0\n", 1)
        out.append(blk)
    return "Tree=".join(out)


# ---- test forests ----------------------------------------------------------------------------------------------------
def chain_forest(n_trees, n_leaves, n_features, seed):
    """chain-shaped trees: node i splits on a feature of its own and hangs leaf i on one side (side at random) and node
    i + 1 on the other, so the longest path has min(n_leaves - 1, n_features) distinct features"""
    rng = np.random.RandomState(seed)
    trees = []
    for _ in range(n_trees):
        ni = n_leaves - 1
        sf = np.concatenate([rng.permutation(n_features), rng.randint(n_features, size=max(ni - n_features, 0))])[:ni]
        lc, rc = np.zeros(ni, np.int64), np.zeros(ni, np.int64)
        for i in range(ni):
            nxt = i + 1 if i + 1 < ni else ~(ni)
            if rng.rand() < 0.5:
                lc[i], rc[i] = ~i, nxt
            else:
                lc[i], rc[i] = nxt, ~i
        trees.append(dict(num_leaves=n_leaves, num_cat=0, split_feature=sf.astype(np.int64),
                          threshold=rng.randn(ni) * 0.7, decision_type=np.full(ni, 2, np.int64), left_child=lc,
                          right_child=rc, leaf_value=rng.randn(n_leaves) * 0.05, shrinkage=0.05))
    names = [f"Column_{i}" for i in range(n_features)]
    return dict(feature_names=names, max_feature_idx=n_features - 1, num_class=1, num_tree_per_iteration=1,
                average_output=False, objective="lambdarank", trees=trees)


def mixed_forest(n_trees, n_leaves, n_features, seed, cat_feature=None):
    """random trees (oracle.gbdt_np.random_forest_model) with decision types 0/2/6/8/10 mixed in and, with
    ``cat_feature``, that feature split categorically (bitset over 0..39) wherever it is used"""
    model = G.random_forest_model(n_trees, n_leaves, n_features, seed=seed)
    rng = np.random.RandomState(seed + 1000)
    for t in model["trees"]:
        ni = t["num_leaves"] - 1
        t["decision_type"] = rng.choice([0, 2, 6, 8, 10], size=ni).astype(np.int64)
        if cat_feature is not None:
            bounds, words = [0], []
            for i in range(ni):
                if t["split_feature"][i] == cat_feature:
                    t["decision_type"][i] = 1
                    t["threshold"][i] = float(len(bounds) - 1)
                    words += [int(rng.randint(1, 2 ** 31 - 1)), int(rng.randint(0, 256))]
                    bounds.append(len(words))
            if len(bounds) > 1:
                t["num_cat"] = len(bounds) - 1
                t["cat_boundaries"] = np.array(bounds, np.int64)
                t["cat_threshold"] = np.array(words, np.int64)
    return model
