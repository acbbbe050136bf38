"""Restatement of the ranking-feature glue between retrieval and ranking (TEST INFRASTRUCTURE).

Follows /root/reference/src/serving/recommender.py:213-263 (_build_ranking_features; duplicated
inline at src/pipelines/run_pipeline.py:188-213) and the 50-column order of
src/features/feature_engineering.py:434-443 (get_feature_columns).  Python floats (float64) exactly as
the reference computes them; the cast to float32 happens in LightGBMRanker.predict (ranker.py:173).
Pinned by tests/golden/g8_ranking_features.npz generated from the reference's own function.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np

N_GENRES = 18
USER_SCALARS = [("avg_rating", 3.5), ("log_rating_count", 0.0), ("recency_score", 0.5), ("gender_encoded", 0.0),
                ("age_normalized", 0.3), ("occupation_normalized", 0.3)]
ITEM_SCALARS = [("avg_rating", 3.5), ("log_rating_count", 0.0), ("popularity_score", 0.0), ("rating_stddev", 0.0),
                ("year_normalized", 0.5)]
ITEM_COLS = ["item_avg_rating", "item_log_rating_count", "popularity_score", "rating_stddev", "year_normalized"]


def feature_columns() -> List[str]:
    """feature_engineering.py:434-443"""
    return (["avg_rating", "log_rating_count", "recency_score", "gender_encoded", "age_normalized",
             "occupation_normalized", "item_avg_rating", "item_log_rating_count", "popularity_score", "rating_stddev",
             "year_normalized", "rating_diff", "user_item_popularity_ratio", "genre_affinity"]
            + [f"user_genre_{i}" for i in range(N_GENRES)] + [f"item_genre_{i}" for i in range(N_GENRES)])


def build_ranking_features(user_features: Dict[str, Any], item_features_batch: Dict[int, Optional[Dict[str, Any]]],
                           candidate_item_ids: List[int]) -> Dict[str, np.ndarray]:
    """Returns {column -> float64[n]} with exactly the reference's columns (item_id included)."""
    rows = []
    for item_id in candidate_item_ids:
        item_feat = item_features_batch.get(item_id) or {}
        row = {"item_id": item_id}
        for name, dflt in USER_SCALARS:
            row[name] = float(user_features.get(name, dflt))
        for (name, dflt), col in zip(ITEM_SCALARS, ITEM_COLS):
            row[col] = float(item_feat.get(name, dflt))
        row["rating_diff"] = row["avg_rating"] - row["item_avg_rating"]
        row["user_item_popularity_ratio"] = row["log_rating_count"] / (row["item_log_rating_count"] + 1e-8)
        ug = user_features.get("genre_pref", [0.0] * N_GENRES)
        ig = item_feat.get("genre_vector", [0.0] * N_GENRES)
        for i in range(N_GENRES):
            row[f"user_genre_{i}"] = float(ug[i]) if i < len(ug) else 0.0
            row[f"item_genre_{i}"] = float(ig[i]) if i < len(ig) else 0.0
        row["genre_affinity"] = sum(row[f"user_genre_{i}"] * row[f"item_genre_{i}"] for i in range(N_GENRES))
        rows.append(row)
    cols = list(rows[0].keys()) if rows else []
    return {c: np.array([r[c] for r in rows], dtype=np.float64) for c in cols}


def feature_matrix(cols: Dict[str, np.ndarray], feature_names: List[str]) -> np.ndarray:
    """What ranker.predict feeds the forest: df[feature_names] (missing columns -> 0.0, recommender.py:334-336)
    cast to float32 (ranker.py:173)."""
    n = len(next(iter(cols.values()))) if cols else 0
    X = np.zeros((n, len(feature_names)), dtype=np.float64)
    for j, name in enumerate(feature_names):
        if name in cols:
            X[:, j] = cols[name]
    return X.astype(np.float32)


# ---- the same glue over feature tables, vectorised (reference of the device kernels) ----
USER_WIDTH, ITEM_WIDTH = len(USER_SCALARS) + N_GENRES, len(ITEM_SCALARS) + N_GENRES


def canonical_matrix(user_rows: np.ndarray, item_rows: np.ndarray) -> np.ndarray:
    """float64 [n, 50] in feature_columns() order from user rows [n, 24] (the 6 scalars of USER_SCALARS, then
    genre_pref[18]) and item rows [n, 23] (the 5 scalars of ITEM_SCALARS, then genre_vector[18]).  The same float64
    operations as build_ranking_features row by row; genre_affinity accumulates genre by genre, left to right, from
    Python's sum() start value 0."""
    u = np.asarray(user_rows, dtype=np.float64)
    it = np.asarray(item_rows, dtype=np.float64)
    n, nu, ni = u.shape[0], len(USER_SCALARS), len(ITEM_SCALARS)
    out = np.empty((n, 14 + 2 * N_GENRES), dtype=np.float64)
    out[:, :nu] = u[:, :nu]
    out[:, nu:nu + ni] = it[:, :ni]
    out[:, 11] = u[:, 0] - it[:, 0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        out[:, 12] = u[:, 1] / (it[:, 1] + 1e-8)
        aff = np.zeros(n, dtype=np.float64)
        for g in range(N_GENRES):
            aff = aff + u[:, nu + g] * it[:, ni + g]
    out[:, 13] = aff
    out[:, 14:14 + N_GENRES] = u[:, nu:]
    out[:, 14 + N_GENRES:] = it[:, ni:]
    return out


def table_feature_matrix(user_tab: np.ndarray, item_tab: np.ndarray, user_ids: np.ndarray, cand_ids: np.ndarray,
                         col_map: np.ndarray) -> np.ndarray:
    """float32 [nq * kc, nf]: what the serving chain feeds the ranker for cand_ids [nq, kc] of users user_ids [nq].
    Row 0 of either table holds the reference's defaults: a user id outside [0, n_user_rows) and an item id at or above
    n_item_rows read it (an entity the feature store does not know); a negative candidate id is retrieval padding and
    gives a row of zeros.  col_map[j] is the canonical column of ranker feature j, -1 for a column the pipeline does not
    produce (0.0, recommender.py:334-336).  One cast to float32 at the end (ranker.py:173)."""
    user_tab, item_tab = np.asarray(user_tab, np.float64), np.asarray(item_tab, np.float64)
    cand = np.asarray(cand_ids, dtype=np.int64)
    nq, kc = cand.shape
    uid = np.repeat(np.asarray(user_ids, dtype=np.int64), kc)
    iid = cand.reshape(-1)
    pad = iid < 0
    uid = np.where((uid < 0) | (uid >= user_tab.shape[0]), 0, uid)
    iid = np.where(pad | (iid >= item_tab.shape[0]), 0, iid)
    canon = canonical_matrix(user_tab[uid], item_tab[iid])
    cm = np.asarray(col_map, dtype=np.int64)
    X = np.where(cm[None, :] >= 0, canon[:, np.where(cm >= 0, cm, 0)], 0.0)
    X[pad] = 0.0
    with np.errstate(over="ignore"):
        return X.astype(np.float32)
