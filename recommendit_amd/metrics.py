"""Ranking metrics used by the parity harness -- same definitions as the reference's
src/evaluation/metrics.py (ndcg_at_k :20-69, recall_at_k :72-87, precision_at_k :90-99, mrr :104-118,
average_precision :121-136, coverage :143-165, intra_list_diversity :168-190, evaluate_model :301-384: mean over
users that have at least one relevant item; kl_divergence_bins :197-231 and detect_training_serving_skew :234-294).
The device form of evaluate_model is eval_device.evaluate_topk_device, that of the skew detector
skew_device.detect_training_serving_skew_device."""
from __future__ import annotations

import math
import logging
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

logger = logging.getLogger(__name__)


def ndcg_at_k(recommended: Sequence[Any], relevant: Sequence[Any], k: int,
              relevance_scores: Optional[Dict[Any, float]] = None) -> float:
    relevant_set = set(relevant)
    dcg = 0.0
    if relevance_scores is None:
        for i, item in enumerate(list(recommended)[:k]):
            if item in relevant_set:
                dcg += 1.0 / math.log2(i + 2)
        idcg = sum(1.0 / math.log2(i + 2) for i in range(min(len(relevant), k)))
    else:   # graded relevance (:43-64): rel_i / log2(i+2), ideal = relevant items sorted by grade
        for i, item in enumerate(list(recommended)[:k]):
            rel = float(relevance_scores.get(item, 0.0))
            if rel > 0:
                dcg += rel / math.log2(i + 2)
        ideal = sorted([relevance_scores.get(item, 0.0) for item in relevant], reverse=True)[:k]
        idcg = sum(rel / math.log2(i + 2) for i, rel in enumerate(ideal) if rel > 0)
    return 0.0 if idcg == 0 else dcg / idcg


def recall_at_k(recommended: Sequence[Any], relevant: Sequence[Any], k: int) -> float:
    if not relevant:
        return 0.0
    relevant_set = set(relevant)
    return sum(1 for item in list(recommended)[:k] if item in relevant_set) / len(relevant_set)


def precision_at_k(recommended: Sequence[Any], relevant: Sequence[Any], k: int) -> float:
    if k == 0:
        return 0.0
    relevant_set = set(relevant)
    return sum(1 for item in list(recommended)[:k] if item in relevant_set) / k


def mrr(recommended: Sequence[Any], relevant: Sequence[Any]) -> float:
    relevant_set = set(relevant)
    for rank, item in enumerate(recommended, start=1):
        if item in relevant_set:
            return 1.0 / rank
    return 0.0


def average_precision(recommended: Sequence[Any], relevant: Sequence[Any]) -> float:
    if not relevant:
        return 0.0
    relevant_set = set(relevant)
    hits = 0
    total = 0.0
    for i, item in enumerate(recommended, start=1):
        if item in relevant_set:
            hits += 1
            total += hits / i
    return total / len(relevant_set)


def coverage(all_recommendations: Sequence[Sequence[Any]], catalog_size: int) -> float:
    if catalog_size == 0:
        return 0.0
    shown = set()
    for recs in all_recommendations:
        shown.update(recs)
    return len(shown) / catalog_size


def intra_list_diversity(recommendations: Sequence[Any], item_genre_vectors: Dict[Any, np.ndarray]) -> float:
    """mean of 1 - cos over the pairs of listed items that have a vector and a non-zero norm.  The arithmetic is
    numpy's on the given vectors, as in the reference: float32 vectors give float32 pair terms and a float32 total."""
    if len(recommendations) < 2:
        return 0.0
    vecs = [item_genre_vectors.get(i) for i in recommendations if i in item_genre_vectors]
    if len(vecs) < 2:
        return 0.0
    total = 0.0
    count = 0
    for i in range(len(vecs)):
        for j in range(i + 1, len(vecs)):
            n1 = np.linalg.norm(vecs[i])
            n2 = np.linalg.norm(vecs[j])
            if n1 > 0 and n2 > 0:
                total += 1 - np.dot(vecs[i], vecs[j]) / (n1 * n2)
                count += 1
    return total / count if count > 0 else 0.0


def evaluate_model(recommendations_by_user: Dict[Any, List[Any]], ground_truth_by_user: Dict[Any, List[Any]],
                   k_values: List[int] = None, catalog_size: Optional[int] = None,
                   item_genre_vectors: Optional[Dict[Any, np.ndarray]] = None) -> Dict[str, Any]:
    k_values = k_values or [5, 10, 20]
    if not recommendations_by_user:
        return {"error": "No users to evaluate", "n_users": 0}
    res: Dict[str, Any] = {"n_users": len(recommendations_by_user), "k_values": k_values}
    # the reference also keeps "mrr" and "ap" lists per k but never appends to them, so mrr@k and ap@k are always 0.0
    # (reference metrics.py:341-344, 352-356); reproduced as such
    per = {k: {"ndcg": [], "recall": [], "precision": [], "mrr": [], "ap": []} for k in k_values}
    mrrs = []
    shown = []
    divs = []
    for u, recs in recommendations_by_user.items():
        rel = ground_truth_by_user.get(u, [])
        if not rel:
            continue
        shown.append(recs)
        for k in k_values:
            per[k]["ndcg"].append(ndcg_at_k(recs, rel, k))
            per[k]["recall"].append(recall_at_k(recs, rel, k))
            per[k]["precision"].append(precision_at_k(recs, rel, k))
        mrrs.append(mrr(recs, rel))
        if item_genre_vectors:
            divs.append(intra_list_diversity(recs[:k_values[-1]], item_genre_vectors))
    for k in k_values:
        for name, v in per[k].items():
            res[f"{name}@{k}"] = float(sum(v) / len(v)) if v else 0.0
    res["mrr"] = float(sum(mrrs) / len(mrrs)) if mrrs else 0.0
    if catalog_size and shown:
        res["coverage"] = coverage(shown, catalog_size)
    if divs:
        res["avg_diversity"] = float(np.mean(divs))
    return res


def kl_divergence_bins(p_values: np.ndarray, q_values: np.ndarray, n_bins: int = 20, epsilon: float = 1e-10) -> float:
    """KL(P || Q) of two samples binned on the edges np.linspace(min, max, n_bins + 1) of their combined range;
    densities + epsilon, renormalised.  0.0 when the combined range is a single value; a NaN or an infinite value gives
    nan (numpy warns, nothing raises)."""
    combined = np.concatenate([p_values, q_values])
    lo, hi = combined.min(), combined.max()
    if lo == hi:
        return 0.0
    edges = np.linspace(lo, hi, n_bins + 1)
    p = np.histogram(p_values, bins=edges, density=True)[0] + epsilon
    q = np.histogram(q_values, bins=edges, density=True)[0] + epsilon
    p = p / p.sum()
    q = q / q.sum()
    return float(np.sum(p * np.log(p / q)))


SKEW_MIN_COUNT = 10   # a column with fewer non-NaN values on either side is not checked


def skew_columns(train_numeric: Sequence[str], serving_columns: Sequence[str],
                 numeric_cols: Optional[Sequence[str]] = None) -> List[str]:
    """the columns the detector checks: the given list, else train's numeric columns that serving also has, in train's
    order"""
    if numeric_cols is not None:
        return list(numeric_cols)
    have = set(serving_columns)
    return [c for c in train_numeric if c in have]


def skew_report(feature_kl: Dict[str, float], threshold: float) -> Dict[str, Any]:
    """the detector's result dict from the rounded per-column KL values"""
    flagged = [c for c, v in feature_kl.items() if v > threshold]
    res = {"feature_kl": feature_kl, "flagged_features": flagged,
           "max_kl": max(feature_kl.values()) if feature_kl else 0.0, "skew_detected": len(flagged) > 0,
           "threshold": threshold, "n_features_checked": len(feature_kl)}
    if flagged:
        logger.warning("Training-serving skew detected in %d features: %s", len(flagged), flagged[:5])
    else:
        logger.info("No significant training-serving skew detected.")
    return res


def detect_training_serving_skew(train_features_df, serving_features_df, threshold: float = 0.1,
                                 numeric_cols: Optional[List[str]] = None) -> Dict[str, Any]:
    """per-column kl_divergence_bins (default bins) of train against serving, NaN dropped per column; a column with
    fewer than SKEW_MIN_COUNT values on either side is skipped; values are stored rounded to 6 decimals and flagged
    when > threshold"""
    cols = skew_columns(train_features_df.select_dtypes(include=[np.number]).columns, serving_features_df.columns,
                        numeric_cols)
    feature_kl: Dict[str, float] = {}
    for c in cols:
        a = train_features_df[c].dropna().values.astype(float)
        b = serving_features_df[c].dropna().values.astype(float)
        if len(a) < SKEW_MIN_COUNT or len(b) < SKEW_MIN_COUNT:
            continue
        feature_kl[c] = round(kl_divergence_bins(a, b), 6)
    return skew_report(feature_kl, threshold)
