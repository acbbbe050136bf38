"""GPU: the device LambdaMART data path (csrc/ltr_data.hip, feature_engineering.py, train_ranker.py).

Tables and join are checked against what the reference's FeatureEngineer produced (tests/golden/g12_ltr_features.npz,
written by tools/make_golden_g12.py); the pair stage -- which the reference cannot finish on these shapes and never
seeds -- is checked property by property against a NumPy plan written here.  Nothing here reads the reference tree."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from recommendit_amd import _lib as L
from recommendit_amd import synthetic
from recommendit_amd.feature_engineering import FeatureEngineer, interaction_dtypes
from recommendit_amd.ranker import LightGBMRanker
from recommendit_amd.recommender import GpuFeatureStore, build_ranking_features_device
from recommendit_amd.train_ranker import RankerTrainer, holdout_metrics_device

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden" / "g12_ltr_features.npz"
USER_DEFAULT = [3.5, 0.0, 0.5, 0.0, 0.3, 0.3] + [0.0] * 18
ITEM_DEFAULT = [3.5, 0.0, 0.0, 0.0, 0.5] + [0.0] * 18


@pytest.fixture(scope="module")
def g12():
    z = np.load(GOLD)
    return z, json.loads(str(z["meta"]))


def frames_of(z, k):
    r = pd.DataFrame({"user_id": z[f"s{k}_rating_user"].astype(np.int64), "item_id": z[f"s{k}_rating_item"].astype(np.int64),
                      "rating": z[f"s{k}_rating_value"].astype(np.int64),
                      "timestamp": pd.to_datetime(z[f"s{k}_rating_ts"], unit="s")})
    u = pd.DataFrame({"user_id": z[f"s{k}_users_id"].astype(np.int64), "gender": z[f"s{k}_users_gender"],
                      "age": z[f"s{k}_users_age"].astype(np.int64), "occupation": z[f"s{k}_users_occupation"].astype(np.int64),
                      "zip_code": "12345"})
    m = pd.DataFrame({"item_id": z[f"s{k}_movies_id"].astype(np.int64), "title": z[f"s{k}_movies_title"],
                      "genres": z[f"s{k}_movies_genres"]})
    return r, u, m


def users_frame(n_users):
    return pd.DataFrame({"user_id": np.arange(1, n_users + 1), "gender": np.where(np.arange(n_users) % 2, "F", "M"),
                         "age": np.array([1, 18, 25, 35, 45, 50, 56])[np.arange(n_users) % 7],
                         "occupation": np.arange(n_users) % 21, "zip_code": "12345"})


def engineer(ratings, users, movies, grid_blocks=0):
    fe = FeatureEngineer("unused")
    fe.set_data(ratings, users, movies)
    fe.grid_blocks = grid_blocks
    return fe


def ml600():
    r, m, _ = synthetic.ml1m_like(n_users=600, n_item_ids=1500, n_catalog=1450, n_ratings=60000, seed=7)
    r["timestamp"] = pd.to_datetime(r["timestamp"], unit="s")
    return r, users_frame(600), m


def rel_diff(a, b):
    s = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(s > 0, np.abs(a - b) / np.where(s > 0, s, 1.0), 0.0)))


def ulp_diff_f32(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, np.int64(-2 ** 31) - a, a)
    b = np.where(b < 0, np.int64(-2 ** 31) - b, b)
    return np.abs(a - b)


# ---- 1. tables -----------------------------------------------------------------------------------------------
def test_tables_match_the_reference(g12):
    """Columns built from exact integers by single roundings are bit-equal; rating_stddev and genre_pref (pandas'
    running variance, NumPy's norm) are within 4x the distance the generator MEASURED between the reference and the
    plain float64 restatement from integer sums (meta.measured_rel_diff: 3.4 and 1.9 float64 epsilons)."""
    z, meta = g12
    tol = meta["measured_rel_diff"]
    for k, s in enumerate(meta["sets"]):
        fe = engineer(*frames_of(z, k))
        ut, it = (t.cpu().numpy() for t in fe.build_tables_device())
        assert ut.shape == (s["n_users"] + 1, 24) and it.shape == (s["n_items"] + 1, 23)
        uid, iid = z[f"s{k}_ref_user_ids"], z[f"s{k}_ref_item_ids"]
        ref_us, ref_is = z[f"s{k}_ref_user_scalars"], z[f"s{k}_ref_item_scalars"]
        for j, c in enumerate(meta["user_scalars"]):
            assert np.array_equal(ut[uid, j], ref_us[:, j], equal_nan=True), (s["name"], "user", c)
        for j, c in enumerate(meta["item_scalars"]):
            if c != "rating_stddev":
                assert np.array_equal(it[iid, j], ref_is[:, j], equal_nan=True), (s["name"], "item", c)
        assert np.array_equal(it[iid, 5:], z[f"s{k}_ref_item_genre_vector"].astype(np.float64))
        d_std, d_pref = rel_diff(it[iid, 3], ref_is[:, 3]), rel_diff(ut[uid, 6:], z[f"s{k}_ref_user_genre_pref"])
        print(f"{s['name']}: rating_stddev rel diff {d_std:.3e}, genre_pref rel diff {d_pref:.3e}")
        assert d_std <= 4 * tol["rating_stddev"] and d_pref <= 4 * tol["genre_pref"]
        assert np.array_equal(it[iid, 3].astype(np.float32), ref_is[:, 3].astype(np.float32))
        rest_u = np.setdiff1d(np.arange(s["n_users"] + 1), uid)
        rest_i = np.setdiff1d(np.arange(s["n_items"] + 1), iid)
        assert (ut[rest_u] == USER_DEFAULT).all() and (it[rest_i] == ITEM_DEFAULT).all()
        # the DataFrame wrappers: names, dtypes and the integer columns of the reference's frames
        uf, itf = fe.build_user_features(), fe.build_item_features()
        assert [[c, str(uf[c].dtype)] for c in uf.columns] == s["user_columns"]
        assert [[c, str(itf[c].dtype)] for c in itf.columns] == s["item_columns"]
        assert np.array_equal(uf["user_id"], uid) and np.array_equal(uf["rating_count"], z[f"s{k}_ref_user_count"])
        assert np.array_equal(itf["item_id"], iid) and np.array_equal(itf["rating_count"], z[f"s{k}_ref_item_count"])


def test_feature_store_and_parquet_round_trip(g12, tmp_path):
    z, meta = g12
    k = [s["name"] for s in meta["sets"]].index("ml300")
    fe = engineer(*frames_of(z, k))
    st = fe.feature_store()
    ut, it = st.device_tables()
    assert ut.data_ptr() == fe.build_tables_device()[0].data_ptr()          # no host round trip
    fe.build_user_features()
    fe.build_item_features()
    fe.save_features(str(tmp_path))
    st2 = GpuFeatureStore.from_parquet(str(tmp_path), meta["sets"][k]["n_users"], meta["sets"][k]["n_items"])
    assert np.array_equal(st2.user, ut.cpu().numpy()) and np.array_equal(st2.item, it.cpu().numpy())
    fe2 = FeatureEngineer("unused")
    fe2.load_features(str(tmp_path))
    assert list(fe2.user_features.columns) == list(fe.user_features.columns)
    # serving from the device-built store gives the serving function's numbers on the same tables
    users = torch.tensor([1, 2], device=ut.device)
    cands = torch.tensor([[3, 4, 5], [6, 7, -1]], device=ut.device)
    names = fe.get_feature_columns()
    assert torch.equal(build_ranking_features_device(st, users, cands, names),
                       build_ranking_features_device(st2, users, cands, names))


# ---- 2. join ---------------------------------------------------------------------------------------------------
def test_join_matches_the_reference(g12):
    """Columns whose inputs are bit-equal are bit-equal in float32; the columns that carry rating_stddev or genre_pref
    may be one float32 ulp off, on at most 1 % of all elements."""
    z, meta = g12
    for k, s in enumerate(meta["sets"]):
        fe = engineer(*frames_of(z, k))
        pairs = z[f"s{k}_pairs"].astype(np.int64)
        cols = s["feature_columns"]
        X = fe.join_device(torch.from_numpy(pairs[:, 0]), torch.from_numpy(pairs[:, 1])).cpu().numpy()
        ref = z[f"s{k}_ref_X"].astype(np.float32)
        ulps = ulp_diff_f32(X, ref)
        loose = [cols.index(c) for c in meta["loose_join_columns"]]
        tight = [j for j in range(50) if j not in loose]
        print(f"{s['name']}: {int((ulps > 0).sum())} of {ulps.size} elements differ, max {int(ulps.max())} ulp")
        assert ulps[:, tight].max() == 0, [cols[j] for j in tight if ulps[:, j].max() > 0]
        assert ulps.max() <= 1
        assert (ulps > 0).mean() <= 0.01
        # a reordered / partial / unknown feature list goes through col_map
        sub = ["genre_affinity", "no_such_column", "user_item_popularity_ratio", "item_genre_3"]
        Xs = fe.join_device(torch.from_numpy(pairs[:, 0]), torch.from_numpy(pairs[:, 1]), sub).cpu().numpy()
        assert np.array_equal(Xs[:, 0], X[:, 13]) and (Xs[:, 1] == 0).all() and np.array_equal(Xs[:, 2], X[:, 12])
        assert np.array_equal(Xs[:, 3], X[:, 32 + 3])
        # the DataFrame wrapper
        fe.build_user_features()
        fe.build_item_features()
        pdf = pd.DataFrame({"user_id": pairs[:, 0], "item_id": pairs[:, 1], "label": 0, "query_id": 0})
        df = fe.build_interaction_features(pdf)
        assert [[c, str(df[c].dtype)] for c in df.columns] == s["interaction_columns"] == [list(c) for c in interaction_dtypes()]
        assert np.array_equal(df[cols].to_numpy(dtype=np.float32), X)


# ---- 3. pairs ---------------------------------------------------------------------------------------------------
def numpy_plan(r, n_neg):
    u, it, rv = r["user_id"].to_numpy(), r["item_id"].to_numpy(), r["rating"].to_numpy()
    cand = np.unique(it)
    plan = {}
    for uid in np.unique(u):
        sel = u == uid
        rated = set(it[sel].tolist())
        P = int((rv[sel] >= 4).sum())
        U = len(cand) - len(rated)
        if P == 0 or U < n_neg:
            continue
        plan[int(uid)] = (P, min(P * n_neg, U), rated, U)
    return plan, set(cand.tolist())


def check_pairs(r, users, movies, n_neg, test_ratio, seed, need_capped):
    fe = engineer(r, users, movies)
    ds = fe.build_ltr_dataset_device(n_negatives=n_neg, test_ratio=test_ratio, seed=seed)
    plan, cand = numpy_plan(r, n_neg)
    kept = sorted(plan)
    qid_of = {u: q for q, u in enumerate(kept)}
    assert ds.n_queries == len(kept) and ds.n_candidates == len(cand)
    n_test = max(1, int(len(kept) * test_ratio))
    assert len(ds.test.groups) == n_test and len(ds.train.groups) == len(kept) - n_test
    pos_sorted = r.assign(pos=np.arange(len(r))).sort_values(["user_id", "timestamp", "pos"], kind="stable")
    pos_sorted = pos_sorted[pos_sorted["rating"] >= 4]
    positives = {int(u): g for u, g in pos_sorted.groupby("user_id")}
    seen_q, capped = [], 0
    for part in (ds.train, ds.test):
        df = part.to_frame()
        groups = part.groups.numpy()
        assert groups.dtype == np.int32 and int(groups.sum()) == len(df) == part.X.shape[0]
        assert (np.diff(df["query_id"].to_numpy()) >= 0).all()                     # sorted by query id
        sizes = df.groupby("query_id", sort=False).size().to_numpy()
        assert np.array_equal(sizes, groups)
        start = 0
        for n in groups:
            g = df.iloc[start:start + n]
            start += n
            uid = int(g["user_id"].iloc[0])
            assert (g["user_id"] == uid).all() and uid in plan
            P, m, rated, U = plan[uid]
            assert n == P + m and (g["query_id"] == qid_of[uid]).all()
            seen_q.append(qid_of[uid])
            pos, neg = g.iloc[:P], g.iloc[P:]
            ref = positives[uid]
            assert (pos["label"] == 1).all() and np.array_equal(pos["item_id"], ref["item_id"])
            assert np.array_equal(pos["rating"], ref["rating"])
            ni = neg["item_id"].to_numpy()
            assert (neg["label"] == 0).all() and (neg["rating"] == 0).all()
            assert len(set(ni.tolist())) == m and not (set(ni.tolist()) & rated) and set(ni.tolist()) <= cand
            if P * n_neg > U:
                capped += 1
                assert set(ni.tolist()) == cand - rated                            # all U_u unrated items
        assert start == len(df)
    assert sorted(seen_q) == list(range(len(kept)))            # every kept user once: train and test are disjoint
    dropped = set(np.unique(r["user_id"]).tolist()) - set(kept)
    print(f"{len(kept)} kept users, {len(dropped)} dropped, {capped} capped at U_u, {len(ds.train) + len(ds.test)} rows")
    if need_capped:
        assert capped >= 1
    return ds, dropped


def test_pairs_exact_properties_ml600():
    ds, _ = check_pairs(*ml600(), n_neg=4, test_ratio=0.1, seed=11, need_capped=True)
    assert ds.max_query_rows == max(int(ds.train.groups.max()), int(ds.test.groups.max()))


def test_pairs_exact_properties_duplicate_rows(g12):
    z, meta = g12
    r, u, m = frames_of(z, 0)                                  # 2 000 random (user, item) draws: duplicates kept
    assert r.duplicated(["user_id", "item_id"]).any()
    # a user without a positive and one that rated (almost) everything must be dropped
    extra = pd.DataFrame({"user_id": 51, "item_id": np.arange(1, 100), "rating": 5,
                          "timestamp": pd.Timestamp("2004-01-01")})
    low = pd.DataFrame({"user_id": [52, 52], "item_id": [3, 4], "rating": [1, 3], "timestamp": pd.Timestamp("2004-01-02")})
    r = pd.concat([r, extra, low], ignore_index=True)
    u = users_frame(52)
    _, dropped = check_pairs(r, u, m, n_neg=4, test_ratio=0.25, seed=5, need_capped=True)
    assert dropped == {51, 52}
    # the DataFrame wrapper returns the same rows
    fe = engineer(r, u, m)
    tr, te = fe.build_training_pairs(n_negatives=4, test_ratio=0.25, seed=5)
    assert list(tr.columns) == ["user_id", "item_id", "label", "rating", "query_id"] == list(te.columns)
    assert not set(tr["query_id"]) & set(te["query_id"]) and tr["label"].dtype == np.int64


# ---- 4. determinism -------------------------------------------------------------------------------------------
def part_arrays(ds):
    out = []
    for p in (ds.train, ds.test):
        out += [p.X.cpu().numpy(), p.y.cpu().numpy(), p.groups.numpy(), p.user_id.cpu().numpy(), p.item_id.cpu().numpy(),
                p.query_id.cpu().numpy(), p.rating.cpu().numpy()]
    return out


def test_determinism_seed_and_launch_geometry():
    data = ml600()
    base = part_arrays(engineer(*data).build_ltr_dataset_device(4, 0.1, seed=3, split_seed=9))
    again = part_arrays(engineer(*data).build_ltr_dataset_device(4, 0.1, seed=3, split_seed=9))
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    for blocks in (1, 7, 300):
        fe = engineer(*data, grid_blocks=blocks)
        ut0, it0 = engineer(*data).build_tables_device()
        ut, it = fe.build_tables_device()
        assert torch.equal(ut, ut0) and torch.equal(it, it0)
        other = part_arrays(fe.build_ltr_dataset_device(4, 0.1, seed=3, split_seed=9))
        assert all(np.array_equal(a, b) for a, b in zip(base, other)), blocks
    # another draw seed: the negatives (and their rows of X) change, nothing else does
    other = part_arrays(engineer(*data).build_ltr_dataset_device(4, 0.1, seed=4, split_seed=9))
    for off in (0, 7):
        X0, y0, g0, u0, i0, q0, r0 = base[off:off + 7]
        X1, y1, g1, u1, i1, q1, r1 = other[off:off + 7]
        assert all(np.array_equal(a, b) for a, b in ((y0, y1), (g0, g1), (u0, u1), (q0, q1), (r0, r1)))
        pos = y0 > 0
        assert np.array_equal(i0[pos], i1[pos]) and np.array_equal(X0[pos], X1[pos])
        assert (i0[~pos] != i1[~pos]).mean() > 0.5
    # another split seed: other held-out users
    third = engineer(*data).build_ltr_dataset_device(4, 0.1, seed=3, split_seed=10)
    assert not np.array_equal(np.unique(third.test.user_id.cpu().numpy()), np.unique(base[7 + 3]))


# ---- 5. uniformity ----------------------------------------------------------------------------------------------
def test_negatives_are_uniform_and_keyed_by_user():
    """2 000 users with one identical history (40 of 200 items rated, 5 positives), n_negatives = 4: 40 000 draws over
    160 cells, expectation 250.  Pearson chi^2 has 159 degrees of freedom (mean 159, s.d. 17.8); the bound 250 is five
    standard deviations.  np.random.choice(160, 20, replace=False) for 2 000 users gave 117..157 over 20 seeds on the
    CPU.  The seed is fixed, so the test cannot flake."""
    n_users, n_items = 2000, 200
    hist_items = np.arange(1, 41)
    hist_rating = np.where(np.arange(40) < 5, 5, 2)
    u = np.repeat(np.arange(1, n_users + 1), 40)
    it = np.tile(hist_items, n_users)
    rv = np.tile(hist_rating, n_users)
    fill_u = np.repeat(np.arange(n_users + 1, n_users + 5), 40)          # 4 users without a positive rate the rest
    fill_i = np.arange(41, 201)
    r = pd.DataFrame({"user_id": np.concatenate([u, fill_u]), "item_id": np.concatenate([it, fill_i]),
                      "rating": np.concatenate([rv, np.full(160, 3)])})
    r["timestamp"] = pd.to_datetime(1_000_000_000 + np.arange(len(r)), unit="s")
    movies = pd.DataFrame({"item_id": np.arange(1, n_items + 1), "title": [f"M {i} (1990)" for i in range(n_items)],
                           "genres": "Drama"})
    fe = engineer(r, users_frame(n_users + 4), movies)
    pr = fe.build_pairs_device(n_negatives=4, test_ratio=0.1, seed=2024)
    assert pr["sizes"]["n_queries"] == n_users and pr["sizes"]["n_rows"] == n_users * 25
    item, lab, usr = (pr[k].cpu().numpy() for k in ("item_id", "label", "user_id"))
    neg = item[lab == 0]
    assert neg.min() >= 41 and neg.max() <= 200
    counts = np.bincount(neg, minlength=201)[41:]
    chi2 = float(((counts - 250.0) ** 2 / 250.0).sum())
    print(f"chi^2 = {chi2:.1f} over 160 cells (159 d.o.f.)")
    assert chi2 < 250
    order = np.argsort(usr[lab == 0], kind="stable")
    seqs = neg[order].reshape(n_users, 20)
    assert len({tuple(s) for s in seqs.tolist()}) == n_users


# ---- 6. end to end ----------------------------------------------------------------------------------------------
def test_train_device_equals_train_on_frames(g12):
    z, meta = g12
    k = [s["name"] for s in meta["sets"]].index("ml300")
    fe = engineer(*frames_of(z, k))
    ds = fe.build_ltr_dataset_device(n_negatives=2, test_ratio=0.1, seed=1)
    a = LightGBMRanker(num_leaves=15, n_estimators=20)
    ra = a.train_device(ds.train, valid=ds.test)
    b = LightGBMRanker(num_leaves=15, n_estimators=20)
    rb = b.train(ds.train.to_frame(), ds.feature_names, valid_df=ds.test.to_frame(), backend="hip")
    assert a._text == b._text and a.model.num_trees() >= 1
    assert ra == rb and a.feature_names == ds.feature_names
    with pytest.raises(ValueError, match="feature names"):
        LightGBMRanker(n_estimators=2).train_device(ds.train, feature_cols=["a", "b"])
    with pytest.raises(RuntimeError, match="HIP device"):
        host = type("P", (), {"X": ds.train.X.cpu(), "y": ds.train.y.cpu(), "groups": ds.train.groups})()
        LightGBMRanker(n_estimators=2).train_device(host, feature_cols=ds.feature_names)


def test_ranker_trainer_run(tmp_path):
    """The unranked baseline is the holdout rows in ascending item id: an order that cannot see the labels (the row
    order itself lists each query's positives first, so it is not a baseline)."""
    r, m, _ = synthetic.ml1m_like(n_users=300, n_item_ids=1000, n_catalog=950, n_ratings=24000, seed=21)
    synthetic.write_ml1m_files(str(tmp_path / "ml"), r, m, 300)
    t = RankerTrainer(data_dir=str(tmp_path / "ml"), model_output_path=str(tmp_path / "out" / "ranker.lgbm"),
                      features_dir=str(tmp_path / "features"), n_negatives=4, num_leaves=15, n_estimators=20)
    ranker = t.run()
    assert (tmp_path / "features" / "user_features.parquet").exists()
    loaded = LightGBMRanker.load(str(tmp_path / "out" / "ranker.lgbm"))
    assert loaded.model.num_trees() == ranker.model.num_trees() >= 1 and loaded.feature_names == ranker.feature_names
    print("holdout", t.holdout_metrics, "unranked", t.unranked_metrics, "timings", t.timings)
    assert t.holdout_metrics["n_queries"] == 30
    assert t.holdout_metrics["ndcg@10"] > t.unranked_metrics["ndcg@10"]
    assert 0.0 < t.holdout_metrics["recall@20"] <= 1.0 and set(t.timings) == {"data_s", "train_s", "holdout_s"}


# ---- 7. argument errors -------------------------------------------------------------------------------------------
def test_argument_errors_and_the_error_word(g12):
    z, _ = g12
    r, u, m = frames_of(z, 0)
    fe = engineer(r, u, m)
    for kw in ({"n_negatives": 0}, {"n_negatives": 1.5}, {"test_ratio": 1.5}, {"test_ratio": -0.1}):
        with pytest.raises(ValueError):
            fe.build_pairs_device(**kw)
    with pytest.raises(ValueError, match="differ in length"):
        fe.join_device(torch.tensor([1, 2]), torch.tensor([1]))
    with pytest.raises(ValueError, match="outside the feature tables"):
        fe.join_device(torch.tensor([1, 51]), torch.tensor([1, 1]))
    X = fe.join_device(torch.tensor([1, 51, -3]), torch.tensor([1, 1, 2]), check=False).cpu().numpy()
    assert X[0].any() and not X[1:].any()                          # the bad rows are zero, the good one is built
    bad = r.copy()
    bad.loc[5, "rating"] = 7
    with pytest.raises(ValueError, match="outside 1..5"):
        engineer(bad, u, m).build_tables_device()
    # the C entry points: ids beyond the sizes they are given set the error word, nothing is written out of bounds
    lib, dev = L.lib(), L.device()
    fe.build_tables_device()
    d = fe._dev
    nu, ni = 10, 20                                                # smaller than the ids in the ratings
    ua = torch.full((nu + 2, 24), -7, dtype=torch.int64, device=dev)      # one guard row each
    ia = torch.full((ni + 2, 3), -7, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(lib.rihip_ltr_stats(L.ptr(d["ru"]), L.ptr(d["ri"]), L.ptr(d["rv"]), L.ptr(d["rt"]), d["ru"].shape[0], nu, ni,
                                L.ptr(d["item_meta"]), L.ptr(d["in_cat"]), L.ptr(ua), L.ptr(ia), L.ptr(err), 0,
                                L.stream_ptr()))
    assert int(err.item()) & 1 and (ua[-1] == -7).all() and (ia[-1] == -7).all()
    ru, ri = d["ru"].cpu().numpy(), d["ri"].cpu().numpy()
    inside = (ru <= nu) & (ri <= ni)
    assert int(ua[:nu + 1, 0].sum()) == int(inside.sum()) == int(ia[:ni + 1, 0].sum())
    one = C.c_void_p(ua.data_ptr())
    assert lib.rihip_ltr_stats(None, None, None, None, 3, nu, ni, one, one, one, one, one, 0, None) == 1
    assert lib.rihip_ltr_join(one, -1, one, 1, one, one, 1, one, 50, one, one, 0, None) == 1
    assert lib.rihip_ltr_emit(None, None, None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 0, one,
                              one, one, one, one, 0, None) == 1


def test_query_larger_than_the_trainer_takes_is_an_error():
    n_items = 20000
    big = pd.DataFrame({"user_id": 1, "item_id": np.arange(1, 3501), "rating": 5})
    rest = pd.DataFrame({"user_id": 2, "item_id": np.arange(1, n_items + 1), "rating": 2})
    r = pd.concat([big, rest], ignore_index=True)
    r["timestamp"] = pd.to_datetime(1_000_000_000 + np.arange(len(r)), unit="s")
    movies = pd.DataFrame({"item_id": [1, 2], "title": ["A (1990)", "B (1991)"], "genres": ["Drama", "Comedy"]})
    fe = engineer(r, users_frame(2), movies)
    with pytest.raises(ValueError, match="at most 16384 documents per query"):
        fe.build_ltr_dataset_device(n_negatives=4)
    ds = fe.build_ltr_dataset_device(n_negatives=1)               # 7 000 rows in one query: fine
    assert ds.n_queries == 1 and len(ds.test) == 7000 and len(ds.train) == 0
