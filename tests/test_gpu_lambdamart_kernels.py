"""The kernels of csrc/gbdt_train.hip at the C ABI, over the trainer's whole parameter space.

Part a -- rihip_lambdarank_gradients (the gradient pass the trainer runs: segmented sort, lambdarank_kernel,
unsort_absmax_kernel) against tests/lambdarank_reference.py: a long-double restatement of the published
GetGradientsForOneQuery with exact sums.  Per document

    |got - ref| <= (P + c) u M + (ceil(cnt / 256) T + 10 + c_nf) u |ref| + P 2^-1012,     u = 2^-53

with P the document's pair count and M its un-cancelled magnitude (sum of the discounts, rho instead of rho (1 - rho)).
The count of roundings behind c and c_nf, operation by operation as lambdarank_kernel writes the formula (each + - x /
one u; exp and log2 at HIP's documented 1 ulp <= 2u):

    c    = T + 32 + 2 X:  T + 22 for a pair term (gain difference 1; the two discounts 3 each and their difference 1,
           relative to their SUM: 4; the two products 2; inv = 1 / max_dcg, max_dcg = T terms of 3 added in sequence:
           T + 3; delta, 0.01 + |delta| and the division 3; exp 2, 1 + e 1, the reciprocal 1; -sigma x and x rho 2; for
           a hessian sigma x sigma, 1 - rho and one more product: 3); the terms of a document are added with at most
           P - 1 additions in sequence and 10 in the fixed tree (6 wave levels, 3 across the waves, 1 onto the partner
           sum): P + 9, and x nf is 1: 10 next to P;
           2 X: sigma * delta reaches exp with two roundings, which exp turns into 2 |sigma delta| (1 - rho) <= 2 X of rho
           (X = the query's largest |sigma delta| (1 - rho), from the reference).
    c_nf = T + 22 + 2 X + 1 / ln(1 + S): every term of S = sum_lambdas carries T + 19 + 2 X and |S nf'/nf| <= 1 passes it
           on unchanged at most; 1 + S rounds once, which log2 turns into 1 / ln(1 + S); log2 2; the division 1.
    P 2^-1012: rho is 0 in float64 once exp overflows (rho < 2^-1022) and the other factors of a term stay below 2^10.

(tests/lambdarank_reference.gradient_bound is that formula.)  With T <= 32 and scores of order 1, c is 45 to 86.  The
NumPy oracle is held to the same bound on the CPU by tests/test_lambdamart_oracle_host.py.  Every test prints its worst
ratio before it asserts (pytest -s, lines starting [worst]); observed values: profiles/r14_lambdamart_kernel_tests.md.

Part b -- rihip_lambdamart_train against oracle/lambdamart_np.train, tree by tree: structure, thresholds and decision
types bitwise, leaf values to 1e-9, NDCG histories to 1e-9.  tests/lambdamart_cases.py holds the inputs;
tests/test_lambdamart_oracle_host.py shows on the CPU that each case takes the branch it is there for.  Every case is
small; the one slow test is test_int40_at_reduced_levels (4.2 M rows: about 6 s of oracle)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lambdamart_cases as CS  # noqa: E402
import lambdarank_reference as R  # noqa: E402
from oracle import gbdt_np as G  # noqa: E402
from oracle import lambdamart_np as LM  # noqa: E402

pytestmark = pytest.mark.gpu
needs_ld = pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_WHY)

OK, ERR_ARG, ERR_SHAPE = 0, 1, 3


def _L():
    from recommendit_amd import _lib
    return _lib


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _last_error():
    return _L().lib().rihip_last_error().decode("utf-8", "replace")


# ================================================================== part a: gradients
def gpu_gradients(c, n_gain=None, gain=None):
    """-> (status, lam, hes, sorted) of one rihip_lambdarank_gradients call"""
    import torch
    L = _L()
    s, l = _dev(c["scores"], np.float64), _dev(c["labels"], np.float32)
    g = np.ascontiguousarray(c["groups"], dtype=np.int32)
    gain = np.ascontiguousarray(c["gain"] if gain is None else gain, dtype=np.float64)
    n = len(c["scores"])
    lam = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    hes = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    srt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = L.lib().rihip_lambdarank_gradients(s.data_ptr(), l.data_ptr(), g.ctypes.data, n, len(g), gain.ctypes.data,
                                            len(gain) if n_gain is None else n_gain, float(c["sigmoid"]), int(c["T"]),
                                            1 if c["norm"] else 0, lam.data_ptr(), hes.data_ptr(), srt.data_ptr(),
                                            L.stream_ptr())
    torch.cuda.synchronize()
    return rc, lam.cpu().numpy(), hes.cpu().numpy(), srt.cpu().numpy()


def _reference(c):
    return R.lambdarank_reference(c["scores"], CS.clamp_labels(c["labels"], len(c["gain"])), c["groups"], c["gain"],
                                  c["sigmoid"], c["T"], c["norm"])


def _check_gradients(name, c, ref, lam, hes, srt):
    T = c["T"]
    nf_adds = np.ceil(ref["cnt"] / 256.0) * T + 10
    bl, bh, cc, cnf = R.gradient_bound(ref, T, nf_adds, c["norm"])
    assert np.isfinite(lam).all() and np.isfinite(hes).all(), name
    dl = np.abs(lam.astype(R.LD) - ref["lam"]).astype(np.float64)
    dh = np.abs(hes.astype(R.LD) - ref["hes"]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rl = np.where(bl > 0, dl / bl, np.where(dl > 0, np.inf, 0.0))
        rh = np.where(bh > 0, dh / bh, np.where(dh > 0, np.inf, 0.0))
    print(f"[worst] gradients {name}: lambda {rl.max():.4f} (document {int(rl.argmax())}), hessian {rh.max():.4f} "
          f"(document {int(rh.argmax())}) of the bound; c up to {cc.max():.1f}, c_nf up to {cnf.max():.1f}, "
          f"P up to {int(ref['P'].max())}")
    assert np.array_equal(srt, ref["sorted"]), name          # the stable descending order, bitwise
    assert rl.max() <= 1.0, (name, "lambda", rl.max())
    assert rh.max() <= 1.0, (name, "hessian", rh.max())
    # documents without a pair have exactly no gradient
    assert not lam[ref["P"] == 0].any() and not hes[ref["P"] == 0].any()


@pytest.fixture(scope="module")
def gcases():
    return CS.gradient_cases()


@pytest.fixture(scope="module")
def grefs(gcases):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _reference(gcases[name])
        return cache[name]
    return get


GRAD_NAMES = ["edge_T1", "edge_T2", "edge_T30", "edge_T32", "norm_off", "sigmoid_0.5", "sigmoid_2", "equal_scores",
              "integer_scores", "far_apart", "gain32", "clamped_labels"]


def test_gradient_case_list_is_complete(gcases):
    assert sorted(gcases) == sorted(GRAD_NAMES)


@needs_ld
@pytest.mark.parametrize("name", GRAD_NAMES)
def test_gradients_against_reference(gcases, grefs, name):
    c = gcases[name]
    rc, lam, hes, srt = gpu_gradients(c)
    assert rc == OK, _last_error()
    ref = grefs(name)
    _check_gradients(name, c, ref, lam, hes, srt)
    if name == "integer_scores":       # +0.0 and -0.0 are one score: ties in document order
        b = 0
        for cnt in c["groups"]:
            assert np.array_equal(srt[b:b + cnt], b + np.argsort(-c["scores"][b:b + cnt], kind="stable"))
            b += cnt
    if name == "far_apart":            # exp overflows on one side: those lambdas are 0, none is NaN, the rest is live
        lone = (ref["P"] > 0) & (np.abs(ref["lam"].astype(np.float64)) < 1e-300)
        assert lone.sum() > 5 and not lam[lone].any() and np.abs(lam).max() > 1e-3


@needs_ld
def test_gradients_one_query_of_16384_documents():
    """the largest query the kernel takes: 147 520 B of dynamic LDS (a test of its own)"""
    c = CS.big_query_case()
    rc, lam, hes, srt = gpu_gradients(c)
    assert rc == OK, _last_error()
    _check_gradients("query_16384", c, _reference(c), lam, hes, srt)


def test_gradients_are_reproducible_and_independent_of_the_batch(gcases):
    c = gcases["edge_T30"]
    a = gpu_gradients(c)
    b = gpu_gradients(c)
    assert a[0] == b[0] == OK
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    off = np.concatenate([[0], np.cumsum(c["groups"])])
    for q in (2, 8, 9):                 # 3, 257 and 1000 documents
        lo, hi = int(off[q]), int(off[q + 1])
        one = dict(c, scores=c["scores"][lo:hi], labels=c["labels"][lo:hi], groups=[hi - lo])
        rc, lam, hes, srt = gpu_gradients(one)
        assert rc == OK
        assert np.array_equal(lam, a[1][lo:hi]) and np.array_equal(hes, a[2][lo:hi]) and np.array_equal(srt + lo, a[3][lo:hi])


def test_gradients_refuse_bad_arguments(gcases):
    """each is refused on the host (check_grad_args / check_groups run before the first allocation): the outputs stay as
    they were"""
    c = gcases["equal_scores"]
    for over, kw, want in ((dict(T=33), {}, ERR_ARG), (dict(T=0), {}, ERR_ARG), (dict(sigmoid=0.0), {}, ERR_ARG),
                           ({}, dict(n_gain=1), ERR_ARG), ({}, dict(n_gain=33, gain=CS.GAIN32 + [1e10]), ERR_ARG),
                           ({}, dict(gain=[0.0, 3.0, 1.0, 7.0, 15.0]), ERR_ARG),
                           (dict(groups=[1, 2, 3, 65, 256]), {}, ERR_ARG)):
        rc, lam, hes, srt = gpu_gradients(dict(c, **over), **kw)
        assert rc == want and _last_error(), (over, kw, rc)
        assert np.isnan(lam).all() and (srt == -1).all()
    n = 16385
    big = dict(c, scores=np.zeros(n), labels=np.zeros(n, np.float32), groups=[n])
    rc, lam, _, srt = gpu_gradients(big)
    assert rc == ERR_SHAPE and "16385" in _last_error()
    assert np.isnan(lam).all() and (srt == -1).all()


# ================================================================== part b: the trainer against the oracle
def _params_struct(p):
    L = _L()
    s = L.LambdamartParams()
    s.num_leaves, s.n_estimators, s.learning_rate = int(p["num_leaves"]), int(p["n_estimators"]), float(p["learning_rate"])
    s.min_child_samples, s.max_bin, s.truncation_level = int(p["min_child_samples"]), int(p["max_bin"]), int(p["truncation_level"])
    s.early_stopping_rounds, s.lambdarank_norm, s.bin_sample = int(p["early_stopping_rounds"]), int(bool(p["lambdarank_norm"])), int(p["bin_sample"])
    s.reg_alpha, s.reg_lambda, s.feature_fraction = float(p["reg_alpha"]), float(p["reg_lambda"]), float(p["feature_fraction"])
    s.min_sum_hessian, s.sigmoid, s.seed = float(p["min_sum_hessian"]), float(p["sigmoid"]), int(p["seed"])
    s.hist_bits = {"int20": 20, "int40": 40}[p["hist_dtype"]]
    s.use_missing, s.split_order = int(bool(p["use_missing"])), {"low": 0, "lightgbm": 1}[p["split_order"]]
    s.n_eval_at = len(p["eval_at"])
    for i, k in enumerate(p["eval_at"]):
        s.eval_at[i] = int(k)
    s.n_label_gain = len(p["label_gain"])
    for i, v in enumerate(p["label_gain"]):
        s.label_gain[i] = float(v)
    return s


def gpu_train(c, F=None):
    """one rihip_lambdamart_train call -> dict(rc, text, model, history [rounds, 2, nk], best_iteration)"""
    import torch
    L = _L()
    p = LM.default_params(**c["params"])
    prm = _params_struct(p)
    X, y = _dev(c["X"], np.float32), _dev(c["y"], np.float32)
    g = np.ascontiguousarray(c["groups"], dtype=np.int32)
    has_v = c.get("Xv") is not None
    if has_v:
        Xv, yv = _dev(c["Xv"], np.float32), _dev(c["yv"], np.float32)
        gv = np.ascontiguousarray(c["gv"], dtype=np.int32)
    nk = len(p["eval_at"])
    hist = np.full((p["n_estimators"], 2, nk), np.nan)
    text_p, best_it, rounds = C.c_void_p(), C.c_int(0), C.c_int(0)
    rc = L.lib().rihip_lambdamart_train(X.data_ptr(), y.data_ptr(), g.ctypes.data, X.shape[0], X.shape[1] if F is None else F,
                                        len(g), Xv.data_ptr() if has_v else None, yv.data_ptr() if has_v else None,
                                        gv.ctypes.data if has_v else None, Xv.shape[0] if has_v else 0, len(gv) if has_v else 0,
                                        C.byref(prm), None, C.byref(text_p), C.byref(best_it), C.byref(rounds),
                                        hist.ctypes.data, L.stream_ptr())
    torch.cuda.synchronize()
    out = dict(rc=rc, text=None, model=None, history=hist[:rounds.value], best_iteration=best_it.value)
    if rc == OK:
        try:
            out["text"] = C.string_at(text_p.value).decode()
        finally:
            L.lib().rihip_free(text_p)
        out["model"] = G.parse_text_model(out["text"])
    else:
        assert not text_p.value
    return out


def oracle_train(c):
    return LM.train(c["X"], c["y"], c["groups"], c["params"], Xv=c.get("Xv"), yv=c.get("yv"), groups_v=c.get("gv"))


def _assert_same(name, got, o, has_valid):
    assert got["rc"] == OK, (name, _last_error())
    m = got["model"]
    assert len(m["trees"]) == len(o["trees"]), name
    assert got["best_iteration"] == o["best_iteration"], name
    for t, (a, b) in enumerate(zip(m["trees"], o["trees"])):
        assert a["num_leaves"] == b["num_leaves"], (name, t)
        if b["num_leaves"] > 1:
            for key in ("split_feature", "left_child", "right_child", "threshold", "decision_type"):
                np.testing.assert_array_equal(a[key], b[key], err_msg=f"{name} tree {t} {key}")
        np.testing.assert_allclose(a["leaf_value"], b["leaf_value"], rtol=1e-9, atol=1e-12, err_msg=f"{name} tree {t}")
    assert len(got["history"]) == len(o["history"]), name
    tr = np.array([h["train"] for h in o["history"]])
    np.testing.assert_allclose(got["history"][:, 0, :], tr, rtol=0, atol=1e-9, err_msg=f"{name} train NDCG")
    if has_valid:
        va = np.array([h["valid"] for h in o["history"]])
        np.testing.assert_allclose(got["history"][:, 1, :], va, rtol=0, atol=1e-9, err_msg=f"{name} valid NDCG")
    else:
        assert np.isnan(got["history"][:, 1, :]).all()


@pytest.fixture(scope="module")
def tcases():
    return CS.trainer_cases()


TRAIN_NAMES = ([f"F{F}" for F in (1, 3, 4, 5, 50, 64, 65, 130, 255)]
               + [f"tie_{w}_{o}_{h}" for w in ("70_to_5", "3_to_67_129") for o in ("low", "lightgbm") for h in ("int20", "int40")]
               + ["tie_in_one_chunk", "truncation_1", "truncation_32", "norm_off", "sigmoid_2", "two_gains", "thirty_two_gains",
                  "max_bin_2", "max_bin_3", "max_bin_16", "max_bin_255", "max_bin_2_missing", "max_bin_255_missing",
                  "odd_columns_missing_1", "odd_columns_missing_0", "bin_stride_7", "bin_stride_7_unseen_nan",
                  "min_child_1", "min_child_5", "no_split_min_child", "no_split_equal_labels", "no_regularisation",
                  "reg_alpha_zeroes_leaves", "feature_fraction_1", "one_feature_per_tree_seed2", "one_feature_per_tree_seed7",
                  "num_leaves_2", "num_leaves_128", "mixed_query_sizes", "rows_1024", "rows_1025", "rows_8192", "rows_8193",
                  "valid_missing", "valid_nan_unseen_in_training"])


def test_trainer_case_list_is_complete(tcases):
    assert sorted(tcases) == sorted(TRAIN_NAMES)


def _gpu_predict(text, X):
    import torch
    L = _L()
    h = C.c_void_p()
    b = text.encode()
    assert L.lib().rihip_gbdt_create_from_text(b, len(b), C.byref(h)) == OK, _last_error()
    try:
        Xd = _dev(X, np.float32)
        out = torch.full((len(X),), float("nan"), dtype=torch.float64, device="cuda")
        assert L.lib().rihip_gbdt_predict(h, Xd.data_ptr(), len(X), X.shape[1], out.data_ptr(), L.stream_ptr()) == OK, _last_error()
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        L.lib().rihip_gbdt_destroy(h)


@pytest.mark.parametrize("name", TRAIN_NAMES)
def test_trainer_against_oracle(tcases, name):
    c = tcases[name]
    got = gpu_train(c)
    o = oracle_train(c)
    _assert_same(name, got, o, c.get("Xv") is not None)
    if name.startswith("tie_70_to_5"):
        assert got["model"]["trees"][0]["split_feature"][0] == 5
    if name.startswith("tie_3_to"):
        assert got["model"]["trees"][0]["split_feature"][0] == 3
    if name in ("no_split_min_child", "no_split_equal_labels", "reg_alpha_zeroes_leaves"):
        # trees without any split: the text loads and predicts the oracle's scores
        assert all(t["num_leaves"] == 1 for t in got["model"]["trees"]) and len(got["model"]["trees"]) == 3
        np.testing.assert_allclose(_gpu_predict(got["text"], c["X"]), G.predict_raw(o, c["X"]), rtol=0, atol=1e-12)


def test_trainer_one_query_of_16384_documents():
    """the large-LDS gradient launch inside the trainer (a test of its own)"""
    c = CS.big_query_trainer_case()
    _assert_same("query_16384", gpu_train(c), oracle_train(c), False)


def test_int40_at_reduced_levels():
    """hist_bits 40 with n = 2^22 + 1 rows runs at 2^39 levels.  THE SLOW CASE of this file: the oracle takes about 6 s."""
    c = CS.int40_reduced_levels_case()
    _assert_same("int40_n_2^22+1", gpu_train(c), oracle_train(c), False)


def test_trainer_refuses_256_features(tcases):
    c = tcases["F255"]
    got = gpu_train(dict(c, X=np.concatenate([c["X"], c["X"][:, :1]], axis=1)))
    assert got["rc"] == ERR_ARG and _last_error()


@pytest.mark.parametrize("name", sorted(CS.ARG_CASES))
def test_trainer_refuses_bad_parameters(tcases, name):
    """refused by the checks at the top of rihip_lambdamart_train, before the bin finder's first copy: no launch"""
    over, want = CS.ARG_CASES[name]
    c = tcases["F3"]
    got = gpu_train(dict(c, params=dict(c["params"], **over)))
    assert got["rc"] == want and "lambdamart_train" in _last_error(), (name, got["rc"], _last_error())


def test_trainer_refuses_bad_groups(tcases):
    c = tcases["F3"]
    got = gpu_train(dict(c, groups=c["groups"][:-1] + [c["groups"][-1] + 1]))
    assert got["rc"] == ERR_ARG and "sum" in _last_error()
    n = 16385
    X, y, g = CS.make_set(1, [n], 2)
    got = gpu_train(dict(c, X=X, y=y, groups=g))
    assert got["rc"] == ERR_SHAPE and "16385" in _last_error()
