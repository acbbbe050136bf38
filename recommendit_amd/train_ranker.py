"""Drop-in RankerTrainer (reference src/training/train_ranker.py:21-175) whose data stage, training and holdout
evaluation all stay on the device: FeatureEngineer.build_ltr_dataset_device -> LightGBMRanker.train_device ->
eval_device.  The reference reads its defaults from src.config.settings; the same values are the defaults here
(config.py:9, :14, :21, :27-29)."""
from __future__ import annotations

import logging
import time
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch

from .eval_device import GroundTruth, evaluate_topk_device
from .feature_engineering import FeatureEngineer, LtrPart
from .ranker import LightGBMRanker

logger = logging.getLogger(__name__)


def rank_holdout_device(part: LtrPart, scores: Optional[torch.Tensor]) -> torch.Tensor:
    """rec_ids i64 [n_queries, K] for the evaluator: every query's item ids by descending score (ties keep the row
    order), padded with -1 to the largest query.  ``scores=None`` is the unranked baseline: ascending item id, an
    order that knows nothing of the labels (the row order itself lists a query's positives first)."""
    g = torch.as_tensor(part.groups).to(device=part.y.device, dtype=torch.int64)
    nq, n = int(g.shape[0]), int(part.y.shape[0])
    K = int(g.max().item()) if nq else 1
    start = torch.cumsum(g, 0) - g
    q = torch.repeat_interleave(torch.arange(nq, device=g.device), g)
    if scores is None:
        scores = -part.item_id.to(torch.float64)
    order = torch.argsort(scores, descending=True, stable=True)
    order = order[torch.argsort(q[order], stable=True)]
    rec = torch.full((nq, K), -1, dtype=torch.int64, device=g.device)
    rec[q, torch.arange(n, device=g.device) - start[q]] = part.item_id[order]
    return rec


def holdout_metrics_device(part: LtrPart, scores: Optional[torch.Tensor]) -> Dict[str, float]:
    """NDCG@10 / NDCG@20 / recall@20 over the holdout queries that have a positive (reference :139-175)"""
    nq = int(torch.as_tensor(part.groups).shape[0])
    if nq == 0:
        return {"ndcg@10": float("nan"), "ndcg@20": float("nan"), "recall@20": float("nan"), "n_queries": 0}
    rec = rank_holdout_device(part, scores)
    g = torch.as_tensor(part.groups).cpu().numpy().astype(np.int64)
    q = np.repeat(np.arange(nq), g)
    pos = part.y.cpu().numpy() > 0
    truth = GroundTruth.from_pairs(np.arange(nq), q[pos], part.item_id.cpu().numpy()[pos])
    rep = evaluate_topk_device(rec, truth, k_values=(10, 20))
    return {"ndcg@10": float(rep["ndcg@10"]), "ndcg@20": float(rep["ndcg@20"]), "recall@20": float(rep["recall@20"]),
            "n_queries": int(rep.get("n_users", nq))}


class RankerTrainer:
    """Orchestrates feature building, pair construction, LTR training and evaluation for the ranker."""

    def __init__(self, data_dir: str = None, model_output_path: str = None, features_dir: str = "data/features",
                 n_negatives: int = None, num_leaves: int = None, n_estimators: int = None, learning_rate: float = None,
                 seed: int = 0):
        self.data_dir = data_dir or "data/ml-1m"
        self.model_output_path = model_output_path or "models/ranker.lgbm"
        self.features_dir = features_dir
        self.n_negatives = n_negatives or 4
        self.num_leaves = num_leaves or 63
        self.n_estimators = n_estimators or 500
        self.learning_rate = learning_rate or 0.05
        self.seed = seed
        self.holdout_metrics: Dict[str, float] = {}
        self.unranked_metrics: Dict[str, float] = {}
        self.timings: Dict[str, float] = {}
        self.evals_result: Dict = {}

    def run(self) -> LightGBMRanker:
        """features -> pairs -> X -> train -> holdout metrics -> save (reference :45-137)"""
        fe = FeatureEngineer(self.data_dir)
        fe.load_data()
        t0 = time.perf_counter()
        feat_dir = Path(self.features_dir)
        if not ((feat_dir / "user_features.parquet").exists() and (feat_dir / "item_features.parquet").exists()):
            logger.info("Computing features from scratch ...")
            fe.build_user_features()
            fe.build_item_features()
            fe.save_features(self.features_dir)
        ds = fe.build_ltr_dataset_device(n_negatives=self.n_negatives, seed=self.seed)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        logger.info("Training set: %d samples, %d queries", len(ds.train), len(ds.train.groups))
        logger.info("Test set: %d samples, %d queries", len(ds.test), len(ds.test.groups))
        ranker = LightGBMRanker(num_leaves=self.num_leaves, n_estimators=self.n_estimators,
                                learning_rate=self.learning_rate)
        self.evals_result = ranker.train_device(ds.train, valid=ds.test if len(ds.test) else None, verbose_eval=50)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        self._evaluate_holdout(ranker, ds.test)
        t3 = time.perf_counter()
        self.timings = {"data_s": t1 - t0, "train_s": t2 - t1, "holdout_s": t3 - t2}
        ranker.save(self.model_output_path)
        logger.info("Top 10 features by gain: %s", ranker.top_features(10))
        return ranker

    def _evaluate_holdout(self, ranker: LightGBMRanker, test: LtrPart) -> Dict[str, float]:
        if len(test) == 0:
            return {}
        self.holdout_metrics = holdout_metrics_device(test, ranker.predict_device(test.X))
        self.unranked_metrics = holdout_metrics_device(test, None)
        logger.info("Holdout evaluation results:")
        for k, v in self.holdout_metrics.items():
            logger.info("  %s: %.4f", k, v)
        return self.holdout_metrics
