"""GPU: per-feature TreeSHAP contributions (rihip_gbdt_predict_contrib, csrc/gbdt.hip) against the references of
tests/shap_reference.py -- brute-force Shapley values on small forests, the long double recursion from
tests/golden/g13_contrib.npz on the large ones -- plus local accuracy against predict_device, bitwise reproducibility,
the stated limits, the errors, and GpuRecommendationPipeline.explain_batch.

Tolerance (one rule for every comparison here): 64 * max(dev_ref, 2^-52 * sum over trees of max |leaf value|), divided
by the tree count for an average_output forest.  dev_ref is what the f64 recursion itself loses against long double on
the same rows (from the fixture, or measured at test time on the small forests); the floor keeps cases with dev_ref ~ 0
from demanding better than f64 rounding of a sum of that size; the factor 64 is the margin for the kernel's path-parallel
order of operations.  The deviations measured on an MI355X are in profiles/r12_contrib.md."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shap_reference as S  # noqa: E402
from oracle import fixtures as fx  # noqa: E402
from oracle import gbdt_np as G  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _ranker(text, tmp_path, name="m.lgbm"):
    from recommendit_amd import LightGBMRanker
    p = tmp_path / name
    p.write_text(text)
    return LightGBMRanker.load(str(p))


def _bound(model, dev_ref):
    floor = 2.0 ** -52 * sum(float(np.abs(t["leaf_value"]).max()) for t in model["trees"])
    b = 64.0 * max(float(dev_ref), floor)
    return b / len(model["trees"]) if model.get("average_output") else b


def _contrib(rk, X, ldx=None):
    X = np.asarray(X, dtype=np.float32)
    if ldx is not None:                       # a wider matrix: the columns past n_features must not be read as features
        W = np.full((X.shape[0], ldx), 1e30, dtype=np.float32)
        W[:, :X.shape[1]] = X
        X = W
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    out = rk.predict_contrib_device(Xd)
    score = rk.predict_device(Xd)
    torch.cuda.synchronize()
    return out.cpu().numpy(), score.cpu().numpy()


def _check(name, got, ref_ld, bound):
    dev = float(np.abs(got.astype(np.longdouble) - ref_ld).max())
    print(f"[contrib] {name}: deviation {dev:.3g}  bound {bound:.3g}  max|phi| {float(np.abs(ref_ld).max()):.3g}")
    assert np.isfinite(got).all()
    assert dev <= bound, (name, dev, bound)


def _refs(model, X):
    """(long double recursion, its f64 error on these rows)"""
    ld = S.tree_shap(model, X, np.longdouble)
    return ld, float(np.abs(S.tree_shap(model, X).astype(np.longdouble) - ld).max())


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "g13_contrib.npz"))
    out = {}
    for name in ("large", "chain"):
        text = bytes(z[f"text_{name}"]).decode()
        out[name] = dict(text=text, model=S.parse_model(text), X=z[f"X_{name}"], phi=z[f"phi_{name}"],
                         dev_ref=float(z[f"dev_ref_{name}"]))
    return out


def _repeats_forest():
    """6 features: random trees with mixed decision types and feature 4 categorical, plus chains of 11 splits over the
    features 0..2 only, so their long paths split one feature at least three times (usually four)"""
    model = S.mixed_forest(6, 12, 6, seed=3, cat_feature=4)
    chains = S.chain_forest(3, 12, 3, seed=8)["trees"]
    assert max(np.bincount(t["split_feature"]).max() for t in chains) >= 3
    for t, dt in zip(chains, (2, 10, 6)):
        t["decision_type"][:] = dt
    model["trees"] += chains
    rng = np.random.RandomState(5)
    bg = np.c_[rng.randn(400, 4), rng.randint(0, 40, 400), rng.randn(400)]
    X = rng.randn(9, 6).astype(np.float32)
    X[:, 4] = rng.randint(0, 40, 9)
    X[0, 0] = np.nan
    X[1, 1] = 0.0
    X[2, 4] = np.nan
    X[3, 4] = -3.0
    X[4, 2] = np.float32(chains[0]["threshold"][0])    # lands on the f32 side of a double threshold
    S.add_counts(model, bg)
    return model, X


# ---- 1, 2: small forests against brute force ---------------------------------------------------------------------
def test_tiny_forest_equals_brute_force(tmp_path):
    text = open(os.path.join(GOLDEN, "tiny_forest.txt")).read()
    model = S.parse_model(text)
    rk = _ranker(text, tmp_path)
    assert rk.model.has_counts()
    # thresholds are 0.5 (fa), -1 and 0 (fb), 0 (fc): rows on them, either side of them, 0.0 (missing type Zero in tree
    # 1) and NaN (missing type NaN with default right in tree 3, read as 0 in trees 0 and 1)
    X = np.array([[0.5, -1.0, 0.0], [0.5, 0.0, 1e-36], [0.6, -1.5, -2.0], [0.0, 0.0, 1.0], [np.nan, np.nan, np.nan],
                  [np.nan, 2.0, 0.0], [-1.0, np.nan, 3.0], [1.0, 1e-3, np.nan], [0.2, -0.5, -0.0]], dtype=np.float32)
    got, score = _contrib(rk, X)
    ld, dev_ref = _refs(model, X)
    bound = _bound(model, dev_ref)
    _check("tiny vs long double", got, ld, bound)
    _check("tiny vs brute force", got, S.brute_force(model, X).astype(np.longdouble), bound)
    assert np.abs(got.sum(1) - score).max() <= bound
    np.testing.assert_allclose(score, G.predict_raw(model, X), rtol=0, atol=bound)
    only2 = text.split("Tree=")
    single = _ranker("Tree=".join([only2[0], "0" + only2[3][1:]]) + "end of trees\n", tmp_path, "single.lgbm")
    one, _ = _contrib(single, X)
    np.testing.assert_array_equal(one, np.tile([0.0, 0.0, 0.0, 0.05], (len(X), 1)))   # a single leaf: expected column only


def test_repeated_feature_and_categorical_equal_brute_force(tmp_path):
    model, X = _repeats_forest()
    text = S.write_text_model_with_counts(model)
    model = S.parse_model(text)
    rk = _ranker(text, tmp_path)
    assert rk.model.predict_path() == 0          # categorical: the general predict kernel
    got, score = _contrib(rk, X)
    ld, dev_ref = _refs(model, X)
    bound = _bound(model, dev_ref)
    _check("repeats vs long double", got, ld, bound)
    _check("repeats vs brute force", got, S.brute_force(model, X).astype(np.longdouble), bound)
    assert np.abs(got.sum(1) - score).max() <= bound


# ---- 3, 4: the golden cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["large", "chain"])
def test_golden_case(golden, tmp_path, name):
    g = golden[name]
    rk = _ranker(g["text"], tmp_path)
    got, score = _contrib(rk, g["X"])
    bound = _bound(g["model"], g["dev_ref"])
    _check(f"golden {name}", got, g["phi"].astype(np.longdouble), bound)
    resid = float(np.abs(got.sum(1) - score).max())
    print(f"[contrib] golden {name}: local accuracy residual {resid:.3g}")
    assert resid <= bound


def test_limits_are_handled(tmp_path):
    """the largest shapes the entry takes: a path with 64 distinct features (the bin's 65th weight) and 128-leaf trees
    (both go-left words)"""
    rng = np.random.RandomState(3)
    deep = S.chain_forest(1, 66, 64, seed=4)
    assert len(set(deep["trees"][0]["split_feature"].tolist())) == 64
    S.add_counts(deep, rng.randn(3000, 64))
    wide = G.random_forest_model(2, 128, 20, seed=6)
    S.add_counts(wide, rng.randn(3000, 20))
    for name, model, nf in (("64 distinct features", deep, 64), ("128 leaves", wide, 20)):
        text = S.write_text_model_with_counts(model)
        model = S.parse_model(text)
        rk = _ranker(text, tmp_path, f"{nf}.lgbm")
        X = rng.randn(3, nf).astype(np.float32)
        got, score = _contrib(rk, X)
        ld, dev_ref = _refs(model, X)
        bound = _bound(model, dev_ref)
        _check(name, got, ld, bound)
        assert np.abs(got.sum(1) - score).max() <= bound


# ---- 6: local accuracy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,ldx", [("large", 257, 53), ("large", 1, None), ("chain", 65, 64)])
def test_local_accuracy_golden_forests(golden, tmp_path, name, n, ldx):
    """the fixture's rows, repeated to n: every copy sums to predict_device and equals the fixture"""
    g = golden[name]
    rk = _ranker(g["text"], tmp_path)
    X = np.tile(g["X"], (n // len(g["X"]) + 1, 1))[:n]
    got, score = _contrib(rk, X, ldx)
    bound = _bound(g["model"], g["dev_ref"])
    assert got.shape == (n, 51)
    assert np.abs(got.sum(1) - score).max() <= bound
    _check(f"{name} n={n}", got, np.tile(g["phi"], (n // len(g["X"]) + 1, 1))[:n].astype(np.longdouble), bound)


@pytest.mark.parametrize("n", [1, 65])
def test_local_accuracy_average_output(tmp_path, n):
    model, X = _repeats_forest()
    text = S.write_text_model_with_counts(model, average_output=True)
    model = S.parse_model(text)
    assert model["average_output"]
    rk = _ranker(text, tmp_path)
    X = np.tile(X, (n // len(X) + 1, 1))[:n]
    got, score = _contrib(rk, X, ldx=9)
    ld, dev_ref = _refs(model, X[:min(n, 9)])
    bound = _bound(model, dev_ref)
    _check(f"average_output n={n}", got[:9], ld, bound)
    assert np.abs(got.sum(1) - score).max() <= bound
    np.testing.assert_allclose(score, G.predict_raw(model, X), rtol=0, atol=bound)


# ---- 7: reproducibility ------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_and_row_independent(golden, tmp_path):
    rk = _ranker(golden["large"]["text"], tmp_path)
    rng = np.random.RandomState(9)
    X = rng.randn(65, 50).astype(np.float32)
    X[3, 5] = np.nan
    a, _ = _contrib(rk, X)
    b, _ = _contrib(rk, X)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    for r in (0, 3, 37, 64):                       # alone, and in a batch that puts it on another lane of the row tile
        alone, _ = _contrib(rk, X[r:r + 1])
        assert np.array_equal(alone.view(np.int64), a[r:r + 1].view(np.int64)), r
        moved, _ = _contrib(rk, X[max(r - 2, 0):r + 1])
        assert np.array_equal(moved[-1].view(np.int64), a[r].view(np.int64)), r


# ---- 8: errors, before any launch -------------------------------------------------------------------------------------
def test_errors_are_raised_before_any_launch(tmp_path):
    from recommendit_amd import _lib as L
    rng = np.random.RandomState(1)
    base = G.random_forest_model(3, 15, 5, seed=2)
    S.add_counts(base, rng.randn(200, 5))
    good = S.write_text_model_with_counts(base)
    zeroed = good.replace("internal_count=", "internal_count=0 ", 1)      # shifts a zero into the first tree's root
    big = G.random_forest_model(1, 130, 5, seed=3)
    S.add_counts(big, rng.randn(500, 5))
    deep = S.chain_forest(1, 70, 70, seed=5)
    S.add_counts(deep, rng.randn(500, 70))
    cases = [("no counts", G.write_text_model(base), 5, "leaf_count"),
             ("zero internal_count", zeroed, 5, "non-positive internal_count"),
             ("130 leaves", S.write_text_model_with_counts(big), 5, "at most 128 leaves"),
             ("69 distinct features", S.write_text_model_with_counts(deep), 70, "at most 64")]
    for name, text, nf, msg in cases:
        rk = _ranker(text, tmp_path, "bad.lgbm")
        assert rk.model.has_counts() == (name != "no counts")
        X = torch.from_numpy(rng.randn(4, nf).astype(np.float32)).cuda()
        with pytest.raises(RuntimeError, match=msg):
            rk.predict_contrib_device(X)
        with pytest.raises(RuntimeError, match=msg):
            rk.predict(pd_frame(X.cpu().numpy(), rk.feature_names), pred_contrib=True)
        out = torch.full((4, nf + 1), -7.0, dtype=torch.float64, device="cuda")
        rc = L.lib().rihip_gbdt_predict_contrib(rk.model._h, X.data_ptr(), 4, nf, out.data_ptr(), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and msg.encode() in L.lib().rihip_last_error(), name
        assert (out == -7.0).all(), name                                   # nothing was launched
        # the forest still predicts as ever
        np.testing.assert_allclose(rk.predict_device(X).cpu().numpy(),
                                   G.predict_raw(G.parse_text_model(text), X.cpu().numpy()), rtol=0, atol=1e-12)
    rk = _ranker(good, tmp_path, "good.lgbm")
    X = torch.zeros((2, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="feature columns"):
        rk.predict_contrib_device(X)
    frame = pd_frame(rng.randn(3, 5), rk.feature_names)
    got = rk.predict(frame, pred_contrib=True)
    assert got.shape == (3, 6) and got.dtype == np.float64
    np.testing.assert_allclose(got.sum(1), rk.predict(frame), rtol=0, atol=_bound(S.parse_model(good), 0.0))


def pd_frame(X, names):
    import pandas as pd
    return pd.DataFrame(np.asarray(X, dtype=np.float32), columns=list(names))


# ---- 9. the serving pipeline ----------------------------------------------------------------------------------------------
NU, NI, D, KC = 120, 900, 64, 60


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    """a small catalogue, as tests/test_gpu_rerank.py builds its own, with a ranker whose model text carries counts"""
    from recommendit_amd import FAISSIndex, LightGBMRanker, TwoTowerModel
    from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns
    sd = fx.make_state(NU, NI, D, 128, seed=21)
    model = TwoTowerModel(NU, NI, D, 128)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    rng = np.random.RandomState(2)
    item_ids = list(range(1, NI + 1))
    genres = (rng.rand(NI, 18) < 0.15).astype(np.float32)
    index = FAISSIndex(embed_dim=D, exact=True)
    index.build_ivf_index(model.get_item_embeddings(item_ids, genres), item_ids)
    forest = G.random_forest_model(30, 31, 50, seed=5, names=feature_columns())
    for t in forest["trees"]:
        t["threshold"] = np.abs(t["threshold"])            # the store's features are >= 0: keep both sides reachable
    S.add_counts(forest, np.abs(rng.randn(2000, 50)))
    text = S.write_text_model_with_counts(forest)
    p = tmp_path_factory.mktemp("explain") / "r.lgbm"
    p.write_text(text)
    ranker = LightGBMRanker.load(str(p))
    store = GpuFeatureStore(NU, NI)
    ut = store.user.copy(); it = store.item.copy()
    ut[1:, :6] = rng.rand(NU, 6) * [5, 8, 1, 1, 1, 1]; ut[1:, 6:] = rng.rand(NU, 18)
    it[1:, :5] = rng.rand(NI, 5) * [5, 9, 1, 1.5, 1]; it[1:, 5:] = genres
    store.load_arrays(ut, it)
    return dict(pipe=GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=KC, top_k_results=20),
                model=S.parse_model(text))


def test_explain_batch(pipe):
    from recommendit_amd.recommender import build_ranking_features_device
    p, bound = pipe["pipe"], _bound(pipe["model"], 0.0)
    uids = list(range(1, 8))
    ids, sc, _ = p.recommend_batch(uids, k=20)
    ids = ids.clone()
    phi = p.explain_batch(uids, ids)
    nf = len(p.ranker.feature_names)
    assert phi.shape == (7, 20, nf + 1) and phi.dtype == torch.float64 and phi.is_cuda
    # each row is predict_contrib_device of the features built for that pair, and sums to the score that was served
    X = build_ranking_features_device(p.store, torch.tensor(uids, device="cuda"), ids, p.ranker.feature_names)
    assert torch.equal(phi.view(-1, nf + 1), p.ranker.predict_contrib_device(X))
    assert float((phi.sum(-1) - sc).abs().max()) <= bound
    assert float(phi[..., :nf].abs().max()) > 1e-3
    # padding
    ids[1, 5:] = -1
    ids[4, 0] = -1
    padded, ti, tv = p.explain_batch(torch.tensor(uids, device="cuda"), ids, top=3)
    assert (padded[1, 5:] == 0).all() and (padded[4, 0] == 0).all()
    keep = ids >= 0
    assert torch.equal(padded[keep], phi[keep])
    # top = 3: torch.topk of |phi| over the feature columns
    exp = torch.topk(padded[..., :nf].abs(), 3, dim=-1)
    assert ti.shape == (7, 20, 3) and torch.equal(ti, exp.indices)
    assert torch.equal(tv.abs(), exp.values) and torch.equal(tv, torch.gather(padded[..., :nf], -1, ti))
    with pytest.raises(ValueError, match="top"):
        p.explain_batch(uids, ids, top=nf + 1)
    with pytest.raises(ValueError, match="item_ids"):
        p.explain_batch(uids, ids[:3])


def test_get_recommendations_explain(pipe):
    p = pipe["pipe"]
    plain = p.get_recommendations(3, k=5)
    assert all("contributions" not in r for r in plain)
    why = p.get_recommendations(3, k=5, explain=4)
    assert [r["item_id"] for r in why] == [r["item_id"] for r in plain]
    phi = p.explain_batch([3], torch.tensor([[r["item_id"] for r in plain]]))[0].cpu().numpy()
    names = list(p.ranker.feature_names)
    for r, row in zip(why, phi):
        assert len(r["contributions"]) == 4 and set(r["contributions"]) <= set(names)
        order = np.argsort(-np.abs(row[:-1]), kind="stable")[:4]
        assert sorted(r["contributions"].values(), key=abs) == sorted(row[order].tolist(), key=abs)
