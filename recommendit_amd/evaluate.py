"""Batched offline evaluation -- the reference's ``PipelineRunner.run_evaluate`` protocol
(src/pipelines/run_pipeline.py:121-237) over the device-resident serving chain.

The reference walks the evaluation users one at a time: user tower -> FAISS search(500) -> per-candidate feature dicts
-> DataFrame -> ranker.predict -> nlargest(20) (:166-220).  Here the same protocol is ONE call per batch of users
through GpuRecommendationPipeline.recommend_batch; the split, the ground truth and the metric definitions are the
reference's: test set = the last ``max(1, int(len(ratings)*0.1/n_users))`` ratings of each user by timestamp (:153-157),
the first ``n_eval_users`` users of that set (:160), ground truth = their test items rated >= 4 (:171-173), users
without ground truth are skipped (:174-175), top-20 by ranker score, NDCG/Recall@{5,10,20} + MRR (+ catalog coverage)
from evaluate_model (:222-227),
all its keys (precision@k, mrr@k / ap@k, coverage, avg_diversity).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np
import torch

from .metrics import evaluate_model
from .recommender import GpuRecommendationPipeline


def run_evaluate(pipe: GpuRecommendationPipeline, ratings_df, movies_df=None, n_eval_users: Optional[int] = 200,
                 top_k: int = 20, batch_size: int = 256, k_values: Optional[List[int]] = None, on_device: bool = False,
                 item_genre_vectors: Optional[Dict[int, Any]] = None, exclude_train: bool = False) -> Dict[str, Any]:
    """on_device=True: the top-k ids stay on the device and eval_device scores them (same report).
    item_genre_vectors: the reference's optional diversity input (evaluate_model's avg_diversity).
    exclude_train=True (not in the reference: SURVEY.md §3.4 hazard ii): the standard protocol that never recommends
    a training item -- every rating outside the test split is excluded from its user's retrieval."""
    ratings = ratings_df.sort_values("timestamp")
    n_test = max(1, int(len(ratings) * 0.1 / ratings["user_id"].nunique()))
    test = ratings.groupby("user_id").tail(n_test)
    eval_users = test["user_id"].unique()
    if n_eval_users:
        eval_users = eval_users[:n_eval_users]
    sub = test[test["user_id"].isin(eval_users)]
    truth = {int(u): g[g["rating"] >= 4]["item_id"].tolist() for u, g in sub.groupby("user_id")}
    users = [int(u) for u in eval_users if truth.get(int(u))]
    catalog = int(movies_df["item_id"].nunique()) if movies_df is not None else None
    if exclude_train:
        from .seen import SeenItems
        attached = pipe.seen
        pipe.set_seen(SeenItems.from_frame(ratings.drop(test.index)))
        try:
            return _evaluate(pipe, users, truth, catalog, top_k, batch_size, k_values, on_device, item_genre_vectors, True)
        finally:
            pipe.set_seen(attached)
    return _evaluate(pipe, users, truth, catalog, top_k, batch_size, k_values, on_device, item_genre_vectors, False)


def _evaluate(pipe, users, truth, catalog, top_k, batch_size, k_values, on_device, item_genre_vectors, exclude):
    if on_device:
        from .eval_device import GroundTruth, evaluate_topk_device, vectors_from_dict
        parts = [pipe.recommend_batch(users[s:s + batch_size], k=top_k, exclude_seen=exclude)[0]
                 for s in range(0, len(users), batch_size)]
        if not parts:
            res = evaluate_model({}, truth, k_values or [5, 10, 20])
        else:
            ids = parts[0] if len(parts) == 1 else torch.cat(parts)
            vec = pres = None
            if item_genre_vectors:
                vec, pres = vectors_from_dict(item_genre_vectors)
            n_id = int(np.max(pipe.index.item_ids)) + 1 if catalog else None
            res = evaluate_topk_device(ids, GroundTruth.from_dict(truth, users), k_values or [5, 10, 20],
                                       catalog_size=catalog, item_vectors=vec, item_present=pres, n_id_space=n_id)
    else:
        recs: Dict[int, List[int]] = {}
        for s in range(0, len(users), batch_size):
            chunk = users[s:s + batch_size]
            ids, _, _ = pipe.recommend_batch(chunk, k=top_k, exclude_seen=exclude)
            ids = ids.cpu().numpy()
            for u, row in zip(chunk, ids):
                recs[u] = [int(x) for x in row if x >= 0]
        # catalog coverage: evaluate_model's catalog_size argument (run_pipeline.py:226)
        res = evaluate_model(recs, truth, k_values or [5, 10, 20], catalog_size=catalog,
                             item_genre_vectors=item_genre_vectors)
    res["n_eval_users"] = len(users)
    return res
