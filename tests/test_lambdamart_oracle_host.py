"""CPU: (1) oracle/lambdamart_np's gradients and NDCG against the independent long-double reference
tests/lambdarank_reference.py, inside the float64 error bound the GPU test holds the kernel to; (2) every case of
tests/test_gpu_lambdamart_kernels.py lands in the branch of csrc/gbdt_train.hip it is meant for, shown on the oracle."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lambdamart_cases as CS  # noqa: E402
import lambdarank_reference as R  # noqa: E402
from oracle import gbdt_np as G  # noqa: E402
from oracle import lambdamart_np as LM  # noqa: E402

needs_ld = pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_WHY)


def _inputs(seed, groups, scale=1.0, n_gain=5):
    rng = np.random.RandomState(seed)
    n = int(np.sum(groups))
    return scale * rng.randn(n), rng.randint(0, n_gain, n)


def _oracle_vs_reference(scores, labels, groups, gain, sigmoid, T, norm, tag):
    ref = R.lambdarank_reference(scores, labels, groups, gain, sigmoid, T, norm)
    lam, hes = LM.lambdarank_grads(scores, labels.astype(np.float32), groups,
                                   dict(label_gain=gain, sigmoid=sigmoid, truncation_level=T, lambdarank_norm=norm))
    # the oracle adds sum_lambdas in NumPy's order: never more than cnt + T additions deep
    bl, bh, _, _ = R.gradient_bound(ref, T, ref["cnt"] + T, norm)
    dl = np.abs(lam.astype(R.LD) - ref["lam"]).astype(np.float64)
    dh = np.abs(hes.astype(R.LD) - ref["hes"]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rl = np.where(bl > 0, dl / bl, np.where(dl > 0, np.inf, 0.0))
        rh = np.where(bh > 0, dh / bh, np.where(dh > 0, np.inf, 0.0))
    print(f"[worst] oracle {tag}: lambda {rl.max():.4f}, hessian {rh.max():.4f} of the bound")
    assert rl.max() <= 1.0 and rh.max() <= 1.0
    return ref, lam, hes


@needs_ld
@pytest.mark.parametrize("T", [1, 30, 32, 700])
@pytest.mark.parametrize("norm", [True, False])
def test_oracle_gradients_inside_the_float64_bound(T, norm):
    groups = [1, 2, 40, 257, 600]
    scores, labels = _inputs(1, groups)
    if T > 32:     # T above every query size: the oracle has no cap; the reference neither
        groups, scores, labels = groups[:4], scores[:300], labels[:300]
    _oracle_vs_reference(scores, labels, groups, CS.GAIN5, 1.0, T, norm, f"T={T} norm={norm}")


@needs_ld
def test_oracle_gradients_sigmoid_2_and_tied_scores():
    groups = [1, 2, 40, 257, 600]
    scores, labels = _inputs(2, groups)
    _oracle_vs_reference(scores, labels, groups, CS.GAIN5, 2.0, 30, True, "sigmoid=2")
    scores, labels = _inputs(3, groups, scale=2.0)
    scores = np.round(scores)
    ref, _, _ = _oracle_vs_reference(scores, labels, groups, CS.GAIN5, 1.0, 30, True, "integer scores")
    # many ties, and the order among them is the document order
    b = 0
    for cnt in groups:
        o = ref["sorted"][b:b + cnt]
        assert np.array_equal(o, b + np.argsort(-scores[b:b + cnt], kind="stable"))
        b += cnt
    assert len(np.unique(scores)) < 20


@needs_ld
def test_reference_properties():
    """what holds for the lambdarank gradients whatever the implementation: the lambdas of a query sum to zero, the
    hessians are positive, a query of one document or of one label has none, and 2-document arithmetic by hand"""
    groups = [1, 2, 40, 7]
    scores, labels = _inputs(4, groups)
    labels[-7:] = 3
    labels[1:3] = [0, 1]
    ref = R.lambdarank_reference(scores, labels, groups, CS.GAIN5, 1.0, 30, True)
    assert ref["lam"][0] == 0 and ref["P"][0] == 0 and not ref["lam"][-7:].any() and not ref["P"][-7:].any()
    assert abs(float(ref["lam"][3:43].sum())) < 1e-17 * float(np.abs(ref["lam"][3:43]).sum()) + 1e-30
    assert (ref["hes"][3:43] > 0).all() and (ref["M_lam"] >= np.abs(ref["lam"])).all()
    # two documents, labels 0 and 1, norm on: inv = 1 / gain[1] = 1, |disc0 - disc1| = 1 - 1/log2(3)
    s0, s1 = scores[1], scores[2]
    d = s1 - s0                                          # high label is document 2
    dn = (1.0 - 1.0 / np.log2(3.0)) / (0.01 + abs(d))
    rho = 1.0 / (1.0 + np.exp(d))
    S = 2 * dn * rho
    lam_high = -dn * rho * np.log2(1 + S) / S
    np.testing.assert_allclose(float(ref["lam"][2]), lam_high, rtol=1e-14)
    np.testing.assert_allclose(float(ref["lam"][1]), -lam_high, rtol=1e-14)
    assert ref["P"][1] == ref["P"][2] == 1


@needs_ld
@pytest.mark.parametrize("norm", [True, False])
def test_reference_equals_its_plain_double_loop(norm):
    """the array form of the reference against the scalar double loop over pairs: they differ in the order of three
    long-double products, i.e. by a few units of 2^-64 of the un-cancelled magnitude"""
    groups = [1, 2, 3, 40, 90]
    scores, labels = _inputs(6, groups)
    scores[10:20] = np.round(scores[10:20])                       # ties
    for sigmoid, T in ((1.0, 30), (2.0, 1), (0.5, 32), (1.0, 200)):
        ref = R.lambdarank_reference(scores, labels, groups, CS.GAIN5, sigmoid, T, norm)
        b = 0
        for cnt in groups:
            lam, hes, P = R.lambdarank_query_plain(scores[b:b + cnt], labels[b:b + cnt], CS.GAIN5, sigmoid, T, norm)
            sl = slice(b, b + cnt)
            assert np.array_equal(P, ref["P"][sl])
            assert (np.abs(lam - ref["lam"][sl]) <= 2.0 ** -58 * ref["M_lam"][sl]).all()
            assert (np.abs(hes - ref["hes"][sl]) <= 2.0 ** -58 * ref["M_hes"][sl]).all()
            b += cnt


@needs_ld
def test_oracle_ndcg_against_the_reference_and_label_order_ideal():
    groups = [1, 2, 40, 257, 600, 5]
    scores, labels = _inputs(5, groups)
    labels[-5:] = 0                                      # a query without a positive counts 1
    ks = [1, 5, 10, 300]
    got = LM.ndcg_at(scores, labels.astype(np.float32), groups, ks, np.asarray(CS.GAIN5))
    ref = R.ndcg_reference(scores, labels, groups, ks, CS.GAIN5)
    np.testing.assert_allclose(got, ref, rtol=0, atol=600 * CS.U)
    # all-zero query alone: exactly 1
    assert LM.ndcg_at(scores[-5:], np.zeros(5, np.float32), [5], [3], np.asarray(CS.GAIN5)) == [1.0]
    # a non-monotone label_gain: the reference refuses it; the oracle's ideal DCG goes by LABEL as the kernels' does
    bad = [0.0, 3.0, 1.0, 7.0, 15.0]
    with pytest.raises(ValueError):
        R.lambdarank_reference(scores, labels, groups, bad, 1.0, 30, True)
    with pytest.raises(ValueError):
        R.ndcg_reference(scores, labels, groups, ks, bad)
    lab = np.array([1, 2, 2, 0])
    assert LM._max_dcg(lab, 2, np.asarray(bad)) == 1.0 + 1.0 / np.log2(3.0)        # labels 2, 2 -- not gains 3, 1


@needs_ld
def test_gpu_gradient_cases_are_what_they_claim():
    """the reference answers of the GPU cases exist, stay finite, and each case has the property it is there for"""
    cases = CS.gradient_cases()
    ref = {}
    for name in ("edge_T1", "edge_T32", "equal_scores", "integer_scores", "far_apart", "gain32", "clamped_labels"):
        c = cases[name]
        ref[name] = R.lambdarank_reference(c["scores"], CS.clamp_labels(c["labels"], len(c["gain"])), c["groups"], c["gain"],
                                           c["sigmoid"], c["T"], c["norm"])
        assert np.isfinite(ref[name]["lam"].astype(np.float64)).all()
    e = ref["edge_T32"]
    off = np.concatenate([[0], np.cumsum(CS.EDGE_GROUPS)])
    assert e["P"][0] == 0 and not e["P"][off[10]:].any()           # the 1-document query and the three one-label queries
    assert e["P"][off[9]:off[10]].max() > 700 and ref["edge_T1"]["P"].max() < 1000
    assert (ref["equal_scores"]["S"][3:] > 0).all()                # best == worst: pairs exist, no 1/(0.01 + |ds|)
    f = ref["far_apart"]                                           # rho underflows on one side: lambdas that are 0 in f64
    lam64 = f["lam"].astype(np.float64)
    assert (f["X"] > 700).any() and ((f["P"] > 0) & (np.abs(lam64) < 1e-300)).sum() > 5 and np.abs(lam64).max() > 1e-3
    assert cases["gain32"]["labels"].max() == 31


# ------------------------------------------------------------------ trainer cases: which branch each one takes
@pytest.fixture(scope="module")
def tcases():
    return CS.trainer_cases()


def _bins(c):
    p = LM.default_params(**c["params"])
    bounds, nanbin = LM.find_bin_bounds(c["X"], p["max_bin"], p["bin_sample"], bool(p["use_missing"]))
    return [len(b) for b in bounds], nanbin, p


@pytest.mark.parametrize("which,winner,loser", [("70_to_5", 5, 70), ("3_to_67_129", 3, 67)])
def test_tie_cases_tie_across_chunks_and_the_lower_index_wins(tcases, which, winner, loser):
    c = tcases[f"tie_{which}_low_int20"]
    X = c["X"]
    assert winner // 64 != loser // 64 and np.array_equal(X[:, winner], X[:, loser])
    o = LM.train(X, c["y"], c["groups"], c["params"])
    root = o["trees"][0]
    assert root["split_feature"][0] == winner
    X2 = X.copy()
    X2[:, winner] = 0.0                                            # without the copy the other chunk's column wins,
    o2 = LM.train(X2, c["y"], c["groups"], c["params"])            # with the same gain and threshold: a true tie
    r2 = o2["trees"][0]
    assert r2["split_feature"][0] == loser and r2["split_gain"][0] == root["split_gain"][0]
    assert r2["threshold"][0] == root["threshold"][0]


def test_tie_inside_one_chunk(tcases):
    c = tcases["tie_in_one_chunk"]
    assert np.array_equal(c["X"][:, 2], c["X"][:, 9])
    o = LM.train(c["X"], c["y"], c["groups"], c["params"])
    assert o["trees"][0]["split_feature"][0] == 2


@pytest.mark.parametrize("name", ["no_split_min_child", "no_split_equal_labels", "reg_alpha_zeroes_leaves"])
def test_no_split_cases_have_one_leaf_trees_that_predict(tcases, name):
    c = tcases[name]
    o = LM.train(c["X"], c["y"], c["groups"], c["params"])
    assert len(o["trees"]) == 3 and all(t["num_leaves"] == 1 for t in o["trees"])
    assert all(float(t["leaf_value"][0]) == 0.0 for t in o["trees"])
    m = G.parse_text_model(G.write_text_model(o))
    np.testing.assert_array_equal(G.predict_raw(m, c["X"]), np.zeros(len(c["X"])))


def test_bin_finder_cases(tcases):
    nb, nanbin, _ = _bins(tcases["max_bin_2_missing"])
    assert nb == [2, 2, 2, 2] and nanbin == [1, 1, 1, 1]           # one real bin + the missing bin: only "real | missing"
    nb, nanbin, _ = _bins(tcases["max_bin_255_missing"])
    assert nb == [255] * 4 and nanbin == [254] * 4                 # 254 real bins, the missing bin in index 254
    for mb in (2, 3, 16, 255):
        nb, nanbin, _ = _bins(tcases[f"max_bin_{mb}"])
        assert nb == [mb] * 4 and nanbin == [-1] * 4
    for um in (0, 1):
        nb, nanbin, _ = _bins(tcases[f"odd_columns_missing_{um}"])
        assert nb[4] == 1 and nanbin[4] == -1                      # constant: one bin, never split
        assert (nb[5], nanbin[5]) == ((2, 1) if um else (1, -1))   # all NaN
        assert (nb[6], nanbin[6]) == ((2, 1) if um else (1, -1))   # constant + NaN (the bin sample leaves NaN out)
    c = tcases["odd_columns_missing_1"]
    o = LM.train(c["X"], c["y"], c["groups"], c["params"])
    sf = np.concatenate([t["split_feature"] for t in o["trees"]])
    thr = np.concatenate([t["threshold"] for t in o["trees"]])
    assert (sf == 6).any() and (thr[sf == 6] == 1.7976931348623157e308).all() and not np.isin(sf, [4, 5]).any()
    c = tcases["bin_stride_7"]
    p = LM.default_params(**c["params"])
    n = len(c["X"])
    assert n == 2000 and max(1, (n + p["bin_sample"] - 1) // p["bin_sample"]) == 7
    c = tcases["bin_stride_7_unseen_nan"]
    nb, nanbin, _ = _bins(c)
    assert np.isnan(c["X"][:, 1]).sum() > 100 and not np.isnan(c["X"][::7, 1]).any() and nanbin == [-1] * 4


def test_grower_cases(tcases):
    c = tcases["num_leaves_128"]
    assert LM.train(c["X"], c["y"], c["groups"], c["params"])["trees"][0]["num_leaves"] == 128
    c = tcases["num_leaves_2"]
    assert all(t["num_leaves"] == 2 for t in LM.train(c["X"], c["y"], c["groups"], c["params"])["trees"])
    for seed in (2, 7):
        c = tcases[f"one_feature_per_tree_seed{seed}"]
        o = LM.train(c["X"], c["y"], c["groups"], c["params"])
        assert len(o["trees"]) == 4 and all(len(set(t["split_feature"].tolist())) == 1 for t in o["trees"])
    a = [t["split_feature"][0] for t in LM.train(*[tcases["one_feature_per_tree_seed2"][k] for k in ("X", "y", "groups", "params")])["trees"]]
    b = [t["split_feature"][0] for t in LM.train(*[tcases["one_feature_per_tree_seed7"][k] for k in ("X", "y", "groups", "params")])["trees"]]
    assert a != b and len(set(a)) > 1
    assert [len(tcases[f"rows_{n}"]["X"]) for n in (1024, 1025, 8192, 8193)] == [1024, 1025, 8192, 8193]
    assert min(tcases["mixed_query_sizes"]["groups"]) == 1
    # min_child_samples 1 and 5 give different trees from each other (the bound is live)
    t1 = LM.train(*[tcases["min_child_1"][k] for k in ("X", "y", "groups", "params")])["trees"]
    t5 = LM.train(*[tcases["min_child_5"][k] for k in ("X", "y", "groups", "params")])["trees"]
    assert min(int(t["leaf_count"].min()) for t in t1) < 5 <= min(int(t["leaf_count"].min()) for t in t5)


def test_validation_cases_route_missing_values(tcases):
    c = tcases["valid_missing"]
    o = LM.train(c["X"], c["y"], c["groups"], c["params"], Xv=c["Xv"], yv=c["yv"], groups_v=c["gv"])
    dts = np.concatenate([t["decision_type"] for t in o["trees"]])
    assert (dts == 10).any() and np.isnan(c["Xv"]).any()           # default-left nodes, which tree_add_kernel must honour
    # routing every missing validation row to the right instead changes the validation history
    o0 = LM.train(c["X"], c["y"], c["groups"], c["params"], Xv=np.nan_to_num(c["Xv"], nan=1e30), yv=c["yv"], groups_v=c["gv"])
    assert [h["valid"] for h in o["history"]] != [h["valid"] for h in o0["history"]]
    c = tcases["valid_nan_unseen_in_training"]
    _, nanbin, _ = _bins(c)
    assert nanbin == [-1] * 6 and np.isnan(c["Xv"]).any() and not np.isnan(c["X"]).any()


def test_int40_case_runs_at_reduced_levels():
    sizes = [16384] * 256 + [1]
    n = int(np.sum(sizes))
    assert n == 2 ** 22 + 1 and min(40, 62 - int(np.ceil(np.log2(n)))) == 39
