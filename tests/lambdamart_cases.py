"""The inputs of tests/test_gpu_lambdamart_kernels.py (TEST INFRASTRUCTURE), in a module of their own so that
tests/test_lambdamart_oracle_host.py can check on the CPU that every case lands in the branch it is meant for.

Gradient cases: dict(scores f64, labels f32 as passed to the library, groups, gain, sigmoid, T, norm).
Trainer cases: dict(X f32, y f32, groups, params for oracle/lambdamart_np.train, optional Xv, yv, gv)."""
import numpy as np

GAIN5 = [0.0, 1.0, 3.0, 7.0, 15.0]
GAIN32 = [float(2 ** l - 1) for l in range(32)]
U = 2.0 ** -53

# ------------------------------------------------------------------ gradient cases
EDGE_GROUPS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 5, 300, 40]   # the last three: single label 2, single label 4, zeros


def _grad_inputs(seed, groups, n_gain=5, scale=1.0):
    rng = np.random.RandomState(seed)
    n = int(np.sum(groups))
    scores = scale * rng.randn(n)
    labels = rng.randint(0, n_gain, n).astype(np.float32)
    return scores, labels


def _edge_case(seed=11, **kw):
    scores, labels = _grad_inputs(seed, EDGE_GROUPS)
    off = np.concatenate([[0], np.cumsum(EDGE_GROUPS)])
    labels[off[10]:off[11]] = 2
    labels[off[11]:off[12]] = 4
    labels[off[12]:off[13]] = 0
    c = dict(scores=scores, labels=labels, groups=list(EDGE_GROUPS), gain=GAIN5, sigmoid=1.0, T=30, norm=True)
    c.update(kw)
    return c


def gradient_cases():
    cases = {}
    for T in (1, 2, 30, 32):
        cases[f"edge_T{T}"] = _edge_case(T=T)
    cases["norm_off"] = _edge_case(norm=False)
    cases["sigmoid_0.5"] = _edge_case(sigmoid=0.5)
    cases["sigmoid_2"] = _edge_case(sigmoid=2.0)
    small = [1, 2, 3, 65, 257]
    s, l = _grad_inputs(12, small)
    cases["equal_scores"] = dict(scores=np.full(len(s), 0.375), labels=l, groups=small, gain=GAIN5, sigmoid=1.0, T=30, norm=True)
    s, l = _grad_inputs(13, [2, 3, 64, 257, 600], scale=2.0)
    s = np.round(s)                                   # many ties; holds +0.0 and -0.0
    assert (s == 0).any() and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all()
    cases["integer_scores"] = dict(scores=s, labels=l, groups=[2, 3, 64, 257, 600], gain=GAIN5, sigmoid=1.0, T=30, norm=True)
    g = [2, 40, 257]
    s, l = _grad_inputs(14, g)
    s = s + np.where(np.random.RandomState(15).rand(len(s)) < 0.5, 800.0, -800.0)
    cases["far_apart"] = dict(scores=s, labels=l, groups=g, gain=GAIN5, sigmoid=1.0, T=30, norm=True)
    g = [3, 65, 500]
    s, l = _grad_inputs(16, g, n_gain=32)
    cases["gain32"] = dict(scores=s, labels=l, groups=g, gain=GAIN32, sigmoid=1.0, T=32, norm=True)
    s, l = _grad_inputs(17, g)
    l = np.random.RandomState(18).randint(-1, 9, len(l)).astype(np.float32)      # -1 .. 8 = n_gain + 3
    assert l.min() == -1 and l.max() == 8
    cases["clamped_labels"] = dict(scores=s, labels=l, groups=g, gain=GAIN5, sigmoid=1.0, T=30, norm=True)
    return cases


def big_query_case():
    s, l = _grad_inputs(19, [16384])
    return dict(scores=s, labels=l, groups=[16384], gain=GAIN5, sigmoid=1.0, T=30, norm=True)


def clamp_labels(labels, n_gain):
    """the library's documented reading of a label outside 0 .. n_gain - 1"""
    return np.clip(np.asarray(labels).astype(np.int64), 0, n_gain - 1)


# ------------------------------------------------------------------ trainer cases
def make_set(seed, sizes, F, grades=5, noise=0.5, informative=None):
    """a ranking set with a learnable signal: labels 0 .. grades-1 from the quantiles of a noisy linear relevance;
    `informative`: that column alone carries the signal"""
    rng = np.random.RandomState(seed)
    n = int(np.sum(sizes))
    X = rng.randn(n, F).astype(np.float32)
    if informative is None:
        w = np.random.RandomState(4321 + F).randn(F) / np.sqrt(F)
    else:
        w = np.zeros(F)
        w[informative] = 1.0
    rel = X.astype(np.float64) @ w + noise * rng.randn(n)
    cuts = np.quantile(rel, [0.5, 0.75, 0.9, 0.97][:grades - 1]) if grades <= 5 else np.quantile(rel, np.linspace(0, 1, grades + 1)[1:-1])
    y = np.zeros(n, np.float32)
    for c in cuts:
        y += rel > c
    return X, y, [int(s) for s in sizes]


BASE = dict(num_leaves=7, n_estimators=3, learning_rate=0.1, eval_at=[3, 10], min_child_samples=10)
WIDE = dict(num_leaves=4, n_estimators=1, learning_rate=0.1, eval_at=[3, 10], min_child_samples=10)
Q600 = [30] * 20
Q1500 = [50] * 30
MIXED = [1, 2, 3, 5, 8, 13, 40, 100, 257, 600]


def _case(X, y, g, params, **kw):
    return dict(X=X, y=y, groups=g, params=params, **kw)


def tie_case(which, order, hist):
    """F = 130, one informative column and bit-identical copies of it in other 64-feature chunks of split_kernel's last
    reduction; every feature is tried (feature_fraction 1)"""
    src, copies = {"70_to_5": (70, [5]), "3_to_67_129": (3, [67, 129])}[which]
    X, y, g = make_set(31, Q600, 130, informative=src, noise=0.3)
    for c in copies:
        X[:, c] = X[:, src]
    return _case(X, y, g, dict(WIDE, feature_fraction=1.0, split_order=order, hist_dtype=hist))


def _with_nan(X, seed, frac=0.15, keep=()):
    X = X.copy()
    m = np.random.RandomState(seed).rand(*X.shape) < frac
    for c in keep:
        m[:, c] = False
    X[m] = np.nan
    return X


def trainer_cases():
    c = {}
    for F in (1, 3, 4, 5, 50, 64, 65, 130, 255):
        X, y, g = make_set(20 + F, Q600, F)
        c[f"F{F}"] = _case(X, y, g, dict(BASE if F < 50 else WIDE))
    for which in ("70_to_5", "3_to_67_129"):
        for order in ("low", "lightgbm"):
            for hist in ("int20", "int40"):
                c[f"tie_{which}_{order}_{hist}"] = tie_case(which, order, hist)
    X, y, g = make_set(32, Q600, 12, informative=2, noise=0.3)
    X[:, 9] = X[:, 2]
    c["tie_in_one_chunk"] = _case(X, y, g, dict(BASE, feature_fraction=1.0))
    # the objective's parameters
    X, y, g = make_set(33, Q600, 6)
    c["truncation_1"] = _case(X, y, g, dict(BASE, truncation_level=1))
    c["truncation_32"] = _case(X, y, g, dict(BASE, truncation_level=32))
    c["norm_off"] = _case(X, y, g, dict(BASE, lambdarank_norm=False))
    c["sigmoid_2"] = _case(X, y, g, dict(BASE, sigmoid=2.0))
    X2, y2, g2 = make_set(34, Q600, 6, grades=2)
    c["two_gains"] = _case(X2, y2, g2, dict(BASE, label_gain=[0.0, 1.0]))
    X3, y3, g3 = make_set(35, Q600, 6, grades=32)
    assert y3.max() == 31
    c["thirty_two_gains"] = _case(X3, y3, g3, dict(BASE, label_gain=GAIN32))
    # the bin finder
    Xc, yc, gc = make_set(36, Q1500, 4)
    for mb in (2, 3, 16, 255):
        c[f"max_bin_{mb}"] = _case(Xc, yc, gc, dict(BASE, max_bin=mb))
    Xn = _with_nan(Xc, 37)
    for mb in (2, 255):
        c[f"max_bin_{mb}_missing"] = _case(Xn, yc, gc, dict(BASE, max_bin=mb, use_missing=True))
    Xo = Xc.copy()
    Xo = np.concatenate([Xo, np.zeros((len(Xo), 3), np.float32)], axis=1)
    Xo[:, 4] = 2.5                                                    # constant
    Xo[:, 5] = np.nan                                                 # all NaN
    Xo[:, 6] = np.where(np.random.RandomState(38).rand(len(Xo)) < 0.4, np.nan, -1.0)   # constant + NaN, informative below
    yo = yc.copy()
    yo[np.isnan(Xo[:, 6]) & (np.random.RandomState(39).rand(len(Xo)) < 0.5)] = 4
    for um in (True, False):
        c[f"odd_columns_missing_{int(um)}"] = _case(Xo, yo, gc, dict(BASE, feature_fraction=1.0, use_missing=um))
    Xs, ys, gs = make_set(40, [50] * 40, 4)
    c["bin_stride_7"] = _case(Xs, ys, gs, dict(BASE, bin_sample=300))
    Xu = Xs.copy()
    skipped = np.arange(len(Xu)) % 7 != 0
    Xu[skipped & (np.random.RandomState(41).rand(len(Xu)) < 0.3), 1] = np.nan
    c["bin_stride_7_unseen_nan"] = _case(Xu, ys, gs, dict(BASE, bin_sample=300, use_missing=True))
    # the tree grower
    X, y, g = make_set(42, Q600, 5)
    c["min_child_1"] = _case(X, y, g, dict(BASE, min_child_samples=1))
    c["min_child_5"] = _case(X, y, g, dict(BASE, min_child_samples=5))
    c["no_split_min_child"] = _case(X, y, g, dict(BASE, min_child_samples=301))
    c["no_split_equal_labels"] = _case(X, np.full(len(y), 2, np.float32), g, dict(BASE))
    c["no_regularisation"] = _case(X, y, g, dict(BASE, reg_alpha=0.0, reg_lambda=0.0))
    c["reg_alpha_zeroes_leaves"] = _case(X, y, g, dict(BASE, reg_alpha=1e6))
    c["feature_fraction_1"] = _case(X, y, g, dict(BASE, feature_fraction=1.0))
    X, y, g = make_set(43, Q600, 12)
    for seed in (2, 7):
        c[f"one_feature_per_tree_seed{seed}"] = _case(X, y, g, dict(BASE, n_estimators=4, feature_fraction=0.1, seed=seed))
    X, y, g = make_set(44, Q600, 5)
    c["num_leaves_2"] = _case(X, y, g, dict(BASE, num_leaves=2))
    X, y, g = make_set(45, [100] * 40, 4)
    c["num_leaves_128"] = _case(X, y, g, dict(BASE, num_leaves=128, n_estimators=1, min_child_samples=1))
    X, y, g = make_set(46, MIXED, 5)
    c["mixed_query_sizes"] = _case(X, y, g, dict(BASE))
    for n in (1024, 1025, 8192, 8193):
        sizes = [64] * (n // 64) + ([n % 64] if n % 64 else [])
        X, y, g = make_set(47 + n, sizes, 3)
        c[f"rows_{n}"] = _case(X, y, g, dict(BASE, n_estimators=2))
    # validation sets: the valid history is what pins tree_add_kernel
    X, y, g = make_set(48, Q600, 6)
    Xv, yv, gv = make_set(49, [30] * 10, 6)
    c["valid_missing"] = _case(_with_nan(X, 50, keep=(2,)), y, g, dict(BASE, use_missing=True),
                               Xv=_with_nan(Xv, 51), yv=yv, gv=gv)
    c["valid_nan_unseen_in_training"] = _case(X, y, g, dict(BASE, use_missing=True), Xv=_with_nan(Xv, 52), yv=yv, gv=gv)
    return c


def big_query_trainer_case():
    X, y, g = make_set(53, [16384], 3)
    return _case(X, y, g, dict(WIDE))


def int40_reduced_levels_case():
    """n = 2^22 + 1 rows: hist_bits 40 runs at 2^(62 - 23) = 2^39 levels"""
    sizes = [16384] * 256 + [1]
    rng = np.random.RandomState(54)
    n = int(np.sum(sizes))
    X = rng.randn(n, 1).astype(np.float32)
    y = np.clip(np.round(X[:, 0] + 0.5 * rng.randn(n) + 1.0), 0, 4).astype(np.float32)
    return _case(X, y, sizes, dict(num_leaves=2, n_estimators=1, learning_rate=0.1, eval_at=[10], min_child_samples=10,
                                   hist_dtype="int40"))


# (params override, expected status) -- every one is refused before the first launch; statuses: 1 = ARG, 3 = SHAPE
ARG_CASES = {
    "bin_sample_0": (dict(bin_sample=0), 1),
    "bin_sample_negative": (dict(bin_sample=-5), 1),
    "min_child_samples_0": (dict(min_child_samples=0), 1),
    "early_stopping_rounds_0": (dict(early_stopping_rounds=0), 1),
    "learning_rate_0": (dict(learning_rate=0.0), 1),
    "learning_rate_nan": (dict(learning_rate=float("nan")), 1),
    "learning_rate_inf": (dict(learning_rate=float("inf")), 1),
    "feature_fraction_0": (dict(feature_fraction=0.0), 1),
    "feature_fraction_nan": (dict(feature_fraction=float("nan")), 1),
    "sigmoid_0": (dict(sigmoid=0.0), 1),
    "sigmoid_negative": (dict(sigmoid=-1.0), 1),
    "reg_alpha_negative": (dict(reg_alpha=-0.1), 1),
    "reg_lambda_nan": (dict(reg_lambda=float("nan")), 1),
    "min_sum_hessian_inf": (dict(min_sum_hessian=float("inf")), 1),
    "eval_at_0": (dict(eval_at=[5, 0]), 1),
    "label_gain_decreasing": (dict(label_gain=[0.0, 3.0, 1.0, 7.0, 15.0]), 1),
    "truncation_level_33": (dict(truncation_level=33), 1),
    "truncation_level_0": (dict(truncation_level=0), 1),
}
