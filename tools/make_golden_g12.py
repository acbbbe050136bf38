#!/usr/bin/env python3
"""G12: the reference's FeatureEngineer (src/features/feature_engineering.py: build_user_features :91-166,
build_item_features :172-219, build_interaction_features :306-370) on three small seeded data sets ->
tests/golden/g12_ltr_features.npz.

Runs only where the reference tree is present: its module is loaded by file path and called unmodified; nothing of
it is copied, only its inputs and outputs are recorded.  build_training_pairs is NOT part of the fixture: it draws
from the unseeded global NumPy state and raises ValueError on these shapes as soon as one user has more positives
than unrated items / n_negatives.

Sets: ``ref50`` = the reference's own make_synthetic_data shape (50 users x 100 items x 2 000 ratings, duplicate
(user, item) rows); ``holes`` = the same with the ratings of two users and two items removed, three users.dat rows and
four movies.dat rows missing (what the left merges leave empty); ``ml300`` = synthetic.ml1m_like with 300 users.
Per set k the arrays are ``s{k}_*``: the inputs (ratings, users, movies), both feature tables as the reference built
them, and for a fixed list of (user, item) pairs written here the 50 ranking columns of build_interaction_features.
``meta`` (one JSON string) holds the column names and dtypes of every frame and the MEASURED distance between the
reference and the plain float64 restatement from integer sums (rating_stddev, genre_pref), which is what the GPU test
scales its tolerance from.

Usage: python tools/make_golden_g12.py REFERENCE_ROOT [out_npz] [--time-pairs]
  --time-pairs also times the reference's build_training_pairs(n_negatives=1) on a 1 000-user set (about 20 s).
"""
import importlib.util
import json
import sys
import time
import warnings
from pathlib import Path

import numpy as np
import pandas as pd

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
if not ARGS:
    sys.exit(__doc__)
REF = Path(ARGS[0])
OUT = Path(ARGS[1]) if len(ARGS) > 1 else ROOT / "tests" / "golden" / "g12_ltr_features.npz"
TIME_PAIRS = "--time-pairs" in sys.argv

from recommendit_amd import synthetic                                   # noqa: E402
from recommendit_amd.feature_engineering import FeatureEngineer as OurFE   # noqa: E402  (host-side parsing only)

USER_SCALARS = ["avg_rating", "log_rating_count", "recency_score", "gender_encoded", "age_normalized",
                "occupation_normalized"]
ITEM_SCALARS = ["avg_rating", "log_rating_count", "popularity_score", "rating_stddev", "year_normalized"]


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def users_frame(n_users, rng):
    return pd.DataFrame({"user_id": np.arange(1, n_users + 1), "gender": rng.choice(["M", "F"], n_users),
                         "age": rng.choice([1, 18, 25, 35, 45, 50, 56], n_users),
                         "occupation": rng.integers(0, 21, n_users), "zip_code": ["12345"] * n_users})


def data_sets(ref_root):
    sys.path.insert(0, str(ref_root))
    ref_tests = load_by_path("ref_test_features", ref_root / "tests" / "test_features.py")
    r, u, m = ref_tests.make_synthetic_data()
    r["rating"] = r["rating"].astype(np.int64)
    out = [("ref50", r, u, m)]
    r2 = r[~r["user_id"].isin([7, 13]) & ~r["item_id"].isin([5, 17])].reset_index(drop=True)
    u2 = u[~u["user_id"].isin([3, 7, 21])].reset_index(drop=True)
    m2 = m[~m["item_id"].isin([5, 9, 40, 77])].reset_index(drop=True)
    m2.loc[m2["item_id"] == 11, "title"] = "No year here"
    out.append(("holes", r2, u2, m2))
    r3, m3, _ = synthetic.ml1m_like(n_users=300, n_item_ids=1000, n_catalog=950, n_ratings=24000, seed=12)
    r3["timestamp"] = pd.to_datetime(r3["timestamp"], unit="s")
    out.append(("ml300", r3, users_frame(300, np.random.default_rng(5)), m3))
    return out


def pair_list(ratings, n_users, n_items, n, rng):
    """rated pairs, unrated pairs and a few ids that have no rating at all"""
    k = n // 2
    idx = rng.choice(len(ratings), size=min(k, len(ratings)), replace=False)
    a = np.stack([ratings["user_id"].to_numpy()[idx], ratings["item_id"].to_numpy()[idx]], 1)
    b = np.stack([rng.integers(1, n_users + 1, n - len(a)), rng.integers(1, n_items + 1, n - len(a))], 1)
    return np.concatenate([a, b]).astype(np.int64)


def restate_tables(fe_host, ratings):
    """plain float64 restatement from integer sums, in GpuFeatureStore's table layout (what the kernels compute)"""
    meta = fe_host.host_metadata()
    u, it, r, sec = fe_host.rating_arrays(ratings)
    nu, ni = int(meta["n_users"]), int(meta["n_items"])
    r = r.astype(np.int64)
    ucnt, usum = np.bincount(u, minlength=nu + 1), np.bincount(u, weights=r, minlength=nu + 1).astype(np.int64)
    icnt = np.bincount(it, minlength=ni + 1)
    isum = np.bincount(it, weights=r, minlength=ni + 1).astype(np.int64)
    isq = np.bincount(it, weights=r * r, minlength=ni + 1).astype(np.int64)
    last = np.full(nu + 1, np.iinfo(np.int64).min)
    np.maximum.at(last, u, sec)
    ut = np.zeros((nu + 1, 24))
    ut[:, :6] = [3.5, 0.0, 0.5, 0.0, 0.3, 0.3]
    has = ucnt > 0
    lo, hi = last[has].min(), last[has].max()
    ut[has, 0] = usum[has] / ucnt[has]
    ut[has, 1] = np.log1p(ucnt[has]).astype(np.float32)
    ut[has, 2] = ((last[has] - lo).astype(np.float64) / float(hi - lo)).astype(np.float32) if hi > lo else 1.0
    ut[has, 3:6] = meta["user_meta"][has]
    lk = (r >= 4) & (meta["item_in_catalog"][it] > 0)
    acc = np.zeros((nu + 1, 18), dtype=np.int64)
    np.add.at(acc, u[lk], ((r[lk] - 3)[:, None] * meta["item_meta"][it[lk], 1:]).astype(np.int64))
    n_lk = np.bincount(u[lk], minlength=nu + 1)
    for uu in np.nonzero(n_lk)[0]:
        v = acc[uu] / float(n_lk[uu])
        ss = 0.0
        for g in range(18):
            ss += v[g] * v[g]
        nrm = np.sqrt(ss)
        ut[uu, 6:] = v / nrm if nrm > 0 else v
    itab = np.zeros((ni + 1, 23))
    itab[:, :5] = [3.5, 0.0, 0.0, 0.0, 0.5]
    hi_ = icnt > 0
    n = icnt[hi_].astype(np.int64)
    lg = np.log1p(n).astype(np.float32)
    itab[hi_, 0] = isum[hi_] / n
    itab[hi_, 1] = lg
    itab[hi_, 2] = (lg / lg.max()).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        itab[hi_, 3] = np.where(n > 1, np.sqrt((n * isq[hi_] - isum[hi_] ** 2) / (n * (n - 1)).astype(np.float64)), 0.0)
    itab[hi_, 4] = meta["item_meta"][hi_, 0]
    itab[hi_, 5:] = meta["item_meta"][hi_, 1:]
    return ut, itab, has, hi_


def restate_join(ut, itab, has_u, has_i, pairs):
    """the 50 columns in float32, training semantics (left-merge holes and NaN -> 0.0)"""
    nan = np.nan
    U = np.where(has_u[pairs[:, 0], None], ut[pairs[:, 0]], nan)
    I = np.where(has_i[pairs[:, 1], None], itab[pairs[:, 1]], nan)
    X = np.zeros((len(pairs), 50), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        X[:, :6] = U[:, :6]
        X[:, 6:11] = I[:, :5]
        X[:, 11] = U[:, 0] - I[:, 0]
        X[:, 12] = U[:, 1].astype(np.float32) / (I[:, 1].astype(np.float32) + np.float32(1e-8))
        aff = np.zeros(len(pairs))
        for g in range(18):
            aff = aff + U[:, 6 + g] * I[:, 5 + g]
        X[:, 13] = aff
        X[:, 14:32] = U[:, 6:]
        X[:, 32:] = I[:, 5:]
    return np.nan_to_num(X, nan=0.0)


def ulp_diff_f32(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, np.int64(-2 ** 31) - a, a)
    b = np.where(b < 0, np.int64(-2 ** 31) - b, b)
    return np.abs(a - b)


def rel_diff(a, b):
    d = np.abs(a - b)
    s = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(s > 0, d / np.where(s > 0, s, 1.0), 0.0))) if d.size else 0.0


def main():
    ref_mod = load_by_path("ref_feature_engineering", REF / "src" / "features" / "feature_engineering.py")
    arrays, meta = {}, {"sets": [], "user_scalars": USER_SCALARS, "item_scalars": ITEM_SCALARS}
    tol_std = tol_pref = 0.0
    rng = np.random.default_rng(12)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, (name, ratings, users, movies) in enumerate(data_sets(REF)):
            fe = ref_mod.FeatureEngineer("unused")
            fe.ratings_df, fe.users_df, fe.movies_df = ratings.copy(), users.copy(), movies.copy()
            t0 = time.perf_counter()
            uf = fe.build_user_features()
            t1 = time.perf_counter()
            itf = fe.build_item_features()
            t2 = time.perf_counter()
            n_users = int(max(ratings["user_id"].max(), users["user_id"].max()))
            n_items = int(max(ratings["item_id"].max(), movies["item_id"].max()))
            pairs = pair_list(ratings, n_users, n_items, 700 if name == "ml300" else 400, rng)
            pdf = pd.DataFrame({"user_id": pairs[:, 0], "item_id": pairs[:, 1], "label": 0, "query_id": 0})
            t3 = time.perf_counter()
            inter = fe.build_interaction_features(pdf)
            t4 = time.perf_counter()
            assert len(inter) == len(pairs) and (inter["user_id"].to_numpy() == pairs[:, 0]).all()
            cols = fe.get_feature_columns()
            print(f"{name}: reference user table {t1 - t0:.3f} s, item table {t2 - t1:.3f} s, interaction join "
                  f"{t4 - t3:.3f} s for {len(pairs)} pairs ({len(ratings)} ratings)")

            # ---- the restatement against the reference, on the CPU -------------------------------------------
            ours = OurFE("unused")
            ours.set_data(ratings, users, movies)
            ut, itab, has_u, has_i = restate_tables(ours, ratings)
            uid, iid = uf["user_id"].to_numpy(), itf["item_id"].to_numpy()
            assert (np.nonzero(has_u)[0] == uid).all() and (np.nonzero(has_i)[0] == iid).all()
            ref_us = uf[USER_SCALARS].to_numpy(dtype=np.float64)
            ref_is = itf[ITEM_SCALARS].to_numpy(dtype=np.float64)
            ref_up = np.stack([np.asarray(v, dtype=np.float64) for v in uf["genre_pref"]])
            ref_iv = np.stack([np.asarray(v, dtype=np.float64) for v in itf["genre_vector"]])
            for j, c in enumerate(USER_SCALARS):
                assert np.array_equal(ut[uid, j], ref_us[:, j], equal_nan=True), (name, "user", c)
            for j, c in enumerate(ITEM_SCALARS):
                if c != "rating_stddev":
                    assert np.array_equal(itab[iid, j], ref_is[:, j], equal_nan=True), (name, "item", c)
            assert np.array_equal(itab[iid, 5:], ref_iv), (name, "genre_vector")
            tol_std = max(tol_std, rel_diff(itab[iid, 3], ref_is[:, 3]))
            tol_pref = max(tol_pref, rel_diff(ut[uid, 6:], ref_up))
            ref_X = inter[cols].to_numpy(dtype=np.float64)
            ulps = ulp_diff_f32(restate_join(ut, itab, has_u, has_i, pairs), ref_X.astype(np.float32))
            loose = [cols.index("rating_stddev"), cols.index("genre_affinity")] + [cols.index(f"user_genre_{g}") for g in range(18)]
            tight = [j for j in range(50) if j not in loose]
            assert ulps[:, tight].max() == 0, (name, [cols[j] for j in tight if ulps[:, j].max() > 0])
            assert ulps.max() <= 1, (name, int(ulps.max()))
            share = float((ulps > 0).mean())
            assert share <= 0.01, (name, share)
            print(f"  restatement: exact columns bit-equal; {int((ulps > 0).sum())} of {ulps.size} join elements 1 ulp off")

            sec = ours.rating_arrays(ratings)[3]
            arrays.update({
                f"s{k}_rating_user": ratings["user_id"].to_numpy().astype(np.int32),
                f"s{k}_rating_item": ratings["item_id"].to_numpy().astype(np.int32),
                f"s{k}_rating_value": ratings["rating"].to_numpy().astype(np.int8),
                f"s{k}_rating_ts": sec.astype(np.int64),
                f"s{k}_users_id": users["user_id"].to_numpy().astype(np.int32),
                f"s{k}_users_gender": users["gender"].to_numpy().astype("U1"),
                f"s{k}_users_age": users["age"].to_numpy().astype(np.int32),
                f"s{k}_users_occupation": users["occupation"].to_numpy().astype(np.int32),
                f"s{k}_movies_id": movies["item_id"].to_numpy().astype(np.int32),
                f"s{k}_movies_title": movies["title"].to_numpy().astype("U"),
                f"s{k}_movies_genres": movies["genres"].to_numpy().astype("U"),
                f"s{k}_ref_user_ids": uid.astype(np.int32), f"s{k}_ref_user_scalars": ref_us,
                f"s{k}_ref_user_count": uf["rating_count"].to_numpy().astype(np.int32),
                f"s{k}_ref_user_genre_pref": ref_up,
                f"s{k}_ref_item_ids": iid.astype(np.int32), f"s{k}_ref_item_scalars": ref_is,
                f"s{k}_ref_item_count": itf["rating_count"].to_numpy().astype(np.int32),
                f"s{k}_ref_item_genre_vector": ref_iv.astype(np.float32),
                f"s{k}_pairs": pairs.astype(np.int32), f"s{k}_ref_X": ref_X,
            })
            meta["sets"].append({
                "name": name, "n_users": n_users, "n_items": n_items, "n_ratings": int(len(ratings)),
                "user_columns": [[c, str(uf[c].dtype)] for c in uf.columns],
                "item_columns": [[c, str(itf[c].dtype)] for c in itf.columns],
                "interaction_columns": [[c, str(inter[c].dtype)] for c in inter.columns],
                "feature_columns": cols,
                "genre_pref_row_dtype": str(np.asarray(uf["genre_pref"].iloc[int(np.argmax(ref_up.any(1)))]).dtype),
                "genre_vector_row_dtype": str(np.asarray(itf["genre_vector"].iloc[0]).dtype)})
    meta["measured_rel_diff"] = {"rating_stddev": tol_std, "genre_pref": tol_pref,
                                 "what": "max relative difference, reference vs the float64 restatement from integer sums, "
                                         "over the sets of this file; the GPU test allows 4x"}
    meta["loose_join_columns"] = ["rating_stddev", "genre_affinity"] + [f"user_genre_{g}" for g in range(18)]
    print(f"measured: rating_stddev {tol_std:.3e} ({tol_std / 2 ** -52:.1f} eps), genre_pref {tol_pref:.3e} "
          f"({tol_pref / 2 ** -52:.1f} eps)")
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **arrays)
    print(f"{len(meta['sets'])} sets -> {OUT} ({OUT.stat().st_size} bytes)")

    if TIME_PAIRS:
        r, m, _ = synthetic.ml1m_like(n_users=1000, n_item_ids=4000, n_catalog=3900, n_ratings=100000, seed=3)
        r["timestamp"] = pd.to_datetime(r["timestamp"], unit="s")
        fe = ref_mod.FeatureEngineer("unused")
        fe.ratings_df, fe.users_df, fe.movies_df = r, users_frame(1000, np.random.default_rng(6)), m
        np.random.seed(0)
        t0 = time.perf_counter()
        fe.build_user_features()
        fe.build_item_features()
        t1 = time.perf_counter()
        tr, te = fe.build_training_pairs(n_negatives=1)
        t2 = time.perf_counter()
        fe.build_interaction_features(pd.concat([tr, te]))
        t3 = time.perf_counter()
        n = len(tr) + len(te)
        print(f"ml1m_like(1000 users, 100000 ratings): tables {t1 - t0:.2f} s, build_training_pairs(n_negatives=1) "
              f"{t2 - t1:.2f} s for {n} rows ({n / (t2 - t1):.0f} rows/s), interaction join {t3 - t2:.2f} s")


if __name__ == "__main__":
    main()
