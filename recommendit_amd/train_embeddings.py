"""Mirror of the reference's src/training/train_embeddings.py for the MI355X path.

``UserItemDataset`` keeps the reference constructor and per-sample ``__getitem__`` (:23-79) and
adds a device-side batch sampler (positives shuffled on the GPU, one rejection-sampled negative per
positive drawn by a HIP kernel from the catalogue and rejected while in the user's *rated* set
-- :58-63 --, genre rows gathered from a device table), because the reference's own DataLoader tops out at ~21 k
samples/s and would starve the kernels.  Not in the reference: ``n_negatives=K`` negatives per positive
(``sample_negatives`` / ``epoch_batches``) and draws proportional to ``(count + 1)^alpha`` (``set_negative_sampling``).

``EmbeddingTrainer`` keeps the reference's constructor arguments and ``train()`` flow (:131-223:
Adam(lr, wd=1e-5) + clip 1.0 + CosineAnnealingLR stepped per epoch, best-loss checkpoint, final
precompute + save) and drives ``HipBPRTrainer`` instead of autograd.
"""
from __future__ import annotations

import logging
import time
from pathlib import Path
from typing import Any, Dict, Iterator, List, Optional, Tuple

import numpy as np
import pandas as pd
import torch

from . import _lib as L
from .negative_sampling import alias_table, popularity_weights
from .synthetic import GENRES, N_GENRES
from .trainer import HipBPRTrainer, cosine_lr
from .two_tower import TwoTowerModel, _check_hard_args

logger = logging.getLogger(__name__)
GENRE_TO_IDX = {g: i for i, g in enumerate(GENRES)}


def load_ml1m(data_dir: str) -> Tuple[pd.DataFrame, pd.DataFrame, pd.DataFrame]:
    """ratings/users/movies in the '::' format (reference src/features/feature_engineering.py:39-72)."""
    d = Path(data_dir)
    for sub in ("", "ml-1m"):
        if (d / sub / "ratings.dat").exists():
            d = d / sub
            break
    ratings = pd.read_csv(d / "ratings.dat", sep="::", engine="python", header=None,
                          names=["user_id", "item_id", "rating", "timestamp"], encoding="latin-1")
    users = pd.read_csv(d / "users.dat", sep="::", engine="python", header=None,
                        names=["user_id", "gender", "age", "occupation", "zip_code"], encoding="latin-1")
    movies = pd.read_csv(d / "movies.dat", sep="::", engine="python", header=None,
                         names=["item_id", "title", "genres"], encoding="latin-1")
    return ratings, users, movies


def build_item_genre_dict(movies_df: pd.DataFrame) -> Dict[int, np.ndarray]:
    """train_embeddings.py:118-129."""
    result = {}
    for iid, genres in zip(movies_df["item_id"].values, movies_df["genres"].values):
        vec = np.zeros(N_GENRES, dtype=np.float32)
        for g in str(genres).split("|"):
            idx = GENRE_TO_IDX.get(g)
            if idx is not None:
                vec[idx] = 1.0
        result[int(iid)] = vec
    return result


class UserItemDataset:
    def __init__(self, ratings_df: pd.DataFrame, item_genre_dict: Dict[int, np.ndarray], all_item_ids: List[int],
                 n_negatives: int = 4, min_rating: float = 4.0, device_tables: bool = True):
        """n_negatives is accepted and unused, like the reference's (:35,:40): it is the reference's quirk, and making
        its default of 4 live would silently change every existing run.  The number of negatives per positive is the
        n_negatives argument of sample_negatives / epoch_batches (default 1)."""
        self.item_genre_dict = item_genre_dict
        self.all_item_ids = all_item_ids
        self.n_negatives = n_negatives  # accepted and unused, like the reference (:35,:40)
        positives = ratings_df[ratings_df["rating"] >= min_rating][["user_id", "item_id"]]
        self.user_ids = positives["user_id"].values.astype(np.int64)
        self.item_ids = positives["item_id"].values.astype(np.int64)
        self.all_items_array = np.array(all_item_ids, dtype=np.int64)
        self._ratings_u = ratings_df["user_id"].values.astype(np.int64)
        self._ratings_i = ratings_df["item_id"].values.astype(np.int64)
        self._user_rated: Optional[Dict[int, set]] = None
        self._dev_ready = False
        self._neg_weights: Optional[np.ndarray] = None     # None = uniform draws
        self._alias_host: Optional[Tuple[np.ndarray, np.ndarray]] = None
        self._alias_dev: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        logger.info("Dataset: %d positive pairs", len(self.user_ids))

    def __len__(self) -> int:
        return len(self.user_ids)

    # ---- reference-compatible host path (train_embeddings.py:58-79) ---------------------------
    @property
    def user_rated(self) -> Dict[int, set]:
        if self._user_rated is None:
            df = pd.DataFrame({"u": self._ratings_u, "i": self._ratings_i})
            self._user_rated = df.groupby("u")["i"].apply(set).to_dict()
        return self._user_rated

    def _sample_negative(self, user_id: int) -> int:
        rated = self.user_rated.get(user_id, set())
        while True:
            neg_id = int(np.random.choice(self.all_items_array))
            if neg_id not in rated:
                return neg_id

    def __getitem__(self, idx: int):
        user_id = int(self.user_ids[idx])
        pos = int(self.item_ids[idx])
        neg = self._sample_negative(user_id)
        zero = np.zeros(N_GENRES, dtype=np.float32)
        return (torch.tensor(user_id, dtype=torch.long), torch.tensor(pos, dtype=torch.long),
                torch.tensor(self.item_genre_dict.get(pos, zero), dtype=torch.float32),
                torch.tensor(neg, dtype=torch.long),
                torch.tensor(self.item_genre_dict.get(neg, zero), dtype=torch.float32))

    # ---- device-side sampler ---------------------------------------------------------------------
    def _prepare_device(self) -> None:
        if self._dev_ready:
            return
        dev = L.device()
        self.M = int(max(self._ratings_i.max(), self.all_items_array.max())) + 1
        self.d_pos_u = torch.from_numpy(self.user_ids).to(dev)
        self.d_pos_i = torch.from_numpy(self.item_ids).to(dev)
        keys = np.unique(self._ratings_u * self.M + self._ratings_i)
        self.d_rated = torch.from_numpy(keys).to(dev)               # sorted (user*M + item) of every rating
        self.d_catalog = torch.from_numpy(self.all_items_array).to(dev)
        gm = np.zeros((self.M, N_GENRES), dtype=np.float32)          # ids absent from movies.dat -> zeros (:70-71)
        for iid, vec in self.item_genre_dict.items():
            if 0 <= iid < self.M:
                gm[iid] = vec
        self.d_genres = torch.from_numpy(gm).to(dev)
        self.d_gave_up = torch.zeros(1, dtype=torch.int32, device=dev)   # samples whose attempts ran out (never read per call)
        self._dev_ready = True

    def catalog_counts(self) -> np.ndarray:
        """count_j: the dataset's positives on catalogue position j (int64 [len(all_item_ids)]); positives on items
        outside the catalogue count nowhere"""
        order = np.argsort(self.all_items_array, kind="stable")
        sorted_items = self.all_items_array[order]
        at = np.searchsorted(sorted_items, self.item_ids)
        hit = (at < sorted_items.shape[0]) & (sorted_items[np.minimum(at, sorted_items.shape[0] - 1)] == self.item_ids)
        cnt = np.zeros(self.all_items_array.shape[0], dtype=np.int64)
        np.add.at(cnt, order[at[hit]], 1)
        return cnt

    def set_negative_sampling(self, alpha: float = 0.0, weights=None) -> None:
        """Popularity-weighted negatives (not in the reference, which draws uniformly): negatives are drawn from the
        catalogue with probability proportional to `weights` (one per catalogue position, finite, >= 0, positive sum;
        a weight of zero is never drawn), by default (count_j + 1)^alpha with count_j = catalog_counts().  The + 1 is a
        choice: it keeps items nobody liked drawable.  alpha = 0.75 is word2vec's customary value, not a measured
        optimum.  The weights become a Walker alias table (negative_sampling.alias_table, probabilities quantised to
        2^-32) that is uploaded on first use.  alpha == 0 with no weights clears the table: uniform draws, as before."""
        if weights is None:
            alpha = float(alpha)
            if not np.isfinite(alpha):
                raise ValueError(f"set_negative_sampling: alpha must be finite, got {alpha!r}")
            w = None if alpha == 0.0 else popularity_weights(self.catalog_counts(), alpha)
        else:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape != self.all_items_array.shape:
                raise ValueError(f"set_negative_sampling: weights must have one entry per catalogue item "
                                 f"({self.all_items_array.shape[0]}), got shape {w.shape}")
        self._alias_host = None if w is None else alias_table(w)    # raises ValueError on bad weights
        self._neg_weights = w
        self._alias_dev = None

    def _alias_ptrs(self):
        if self._alias_host is None:
            return None, None
        if self._alias_dev is None:
            dev = L.device()
            prob, alias = self._alias_host
            # (torch has no uint32 arithmetic: the words travel as int32 bit patterns)
            self._alias_dev = (torch.from_numpy(prob.view(np.int32).copy()).to(dev), torch.from_numpy(alias.copy()).to(dev))
        return self._alias_dev[0].data_ptr(), self._alias_dev[1].data_ptr()

    def sample_negatives(self, users: torch.Tensor, gen: torch.Generator, max_attempts: int = 1000,
                         n_negatives: int = 1) -> torch.Tensor:
        """One HIP launch for the whole batch (rihip_sample_negatives): uniform catalogue draws, re-drawn while the
        item is in the user's rated set -- the reference's rejection loop (:58-63), bounded at `max_attempts`.  A sample
        that exhausts them keeps its last draw, a RATED item, and is counted on the device (negatives_given_up).
        n_negatives = K > 1 or a table set by set_negative_sampling (rihip_sample_negatives_multi): [K n] negatives,
        k-major (negative k of sample i at k n + i), the K draws of a sample independent (with replacement)."""
        if isinstance(n_negatives, bool) or int(n_negatives) != n_negatives or int(n_negatives) < 1:
            raise ValueError(f"sample_negatives: n_negatives must be an integer >= 1, got {n_negatives!r}")
        K = int(n_negatives)
        self._prepare_device()
        u = users.contiguous()
        self._neg_calls = getattr(self, "_neg_calls", 0) + 1     # host-side counter: no device sync for the seed
        seed = (gen.initial_seed() * 0x9E3779B97F4A7C15 + self._neg_calls) & ((1 << 63) - 1)
        prob, alias = self._alias_ptrs()
        if K > 1 or prob is not None:
            neg = torch.empty((K * u.numel(),), dtype=u.dtype, device=u.device)
            L.check(L.lib().rihip_sample_negatives_multi(u.data_ptr(), u.numel(), K, self.d_catalog.data_ptr(),
                                                         self.d_catalog.numel(), prob, alias, self.d_rated.data_ptr(),
                                                         self.d_rated.numel(), self.M, seed, max_attempts,
                                                         neg.data_ptr(), self.d_gave_up.data_ptr(), L.stream_ptr()),
                    "sample_negatives_multi")
            return neg
        neg = torch.empty_like(u)
        L.check(L.lib().rihip_sample_negatives(u.data_ptr(), u.numel(), self.d_catalog.data_ptr(),
                                               self.d_catalog.numel(), self.d_rated.data_ptr(), self.d_rated.numel(),
                                               self.M, seed, max_attempts, neg.data_ptr(), self.d_gave_up.data_ptr(),
                                               L.stream_ptr()),
                "sample_negatives")
        return neg

    def negatives_given_up(self, reset: bool = False) -> int:
        """Samples since the last reset whose negative is a rated item because max_attempts ran out (one device read)."""
        if not self._dev_ready:
            return 0
        n = int(self.d_gave_up.item())
        if reset:
            self.d_gave_up.zero_()
        return n

    def epoch_batches(self, batch_size: int, gen: torch.Generator, with_negatives: bool = True, n_negatives: int = 1
                      ) -> Iterator[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """Shuffled, drop_last batches (DataLoader(shuffle=True, drop_last=True), :144-151) as device
        tensors: (user_ids [B], item_ids [2B]=pos||neg or [B], item_genres).  n_negatives = K: item_ids
        [(1+K)B] = pos || neg_0 || ... || neg_(K-1), the layout HipBPRTrainer(n_negatives=K).step takes."""
        if isinstance(n_negatives, bool) or int(n_negatives) != n_negatives or int(n_negatives) < 1:
            raise ValueError(f"epoch_batches: n_negatives must be an integer >= 1, got {n_negatives!r}")
        self._prepare_device()
        n = len(self)
        perm = torch.randperm(n, device=self.d_pos_u.device, generator=gen)
        for s in range(0, n - batch_size + 1, batch_size):
            idx = perm[s:s + batch_size]
            u, p = self.d_pos_u[idx], self.d_pos_i[idx]
            if with_negatives:
                items = torch.cat([p, self.sample_negatives(u, gen, n_negatives=int(n_negatives))])
            else:
                items = p
            yield u, items, self.d_genres[items]
        if with_negatives:
            n_bad = self.negatives_given_up(reset=True)      # the epoch's only read of the counter
            if n_bad:
                logger.warning("negative sampler: %d samples of this epoch exhausted their attempts and kept a RATED "
                               "item as the negative (a user rated almost the whole catalogue)", n_bad)


def item_log_q(item_ids: np.ndarray, n_rows: int) -> np.ndarray:
    """logQ of the in-batch softmax: log(count_j / n) for every item-table row j, counted over the n training pairs
    ``item_ids`` that batches are drawn from (a row's item appears as an in-batch negative with that probability).  A
    row that never appears gets the log of the smallest positive probability."""
    cnt = np.bincount(np.asarray(item_ids, dtype=np.int64), minlength=n_rows).astype(np.float64)
    assert len(cnt) == n_rows and cnt.sum() > 0
    prob = cnt / cnt.sum()
    prob[cnt == 0] = prob[cnt > 0].min()
    return np.log(prob).astype(np.float32)


class EmbeddingTrainer:
    def __init__(self, data_dir: str = "data/ml-1m", model_output_path: str = "models/two_tower.pt",
                 embed_dim: int = 64, epochs: int = 10, batch_size: int = 1024, learning_rate: float = 1e-3,
                 device: Optional[str] = None, loss_mode: str = "sampled", table_opt: str = "dense",
                 dropout: float = 0.1, seed: int = 0, temperature: float = 0.05, logq_correction: bool = True,
                 mask_duplicates: bool = True, n_hard: int = 8, hard_skip: int = 0, hard_weight: float = 0.1,
                 n_negatives: int = 1, negative_alpha: float = 0.0, validation=None, val_k=(10, 50), val_every: int = 1,
                 select_by: Optional[str] = None, patience: Optional[int] = None):
        """Defaults = the reference's settings (src/config.py:13,:24-26); `device` is accepted for
        signature compatibility -- training always runs on the HIP device.
        loss_mode="softmax" (not in the reference): in-batch sampled softmax with `temperature` (0.05 is a customary
        starting value, not a measured optimum), the logQ correction from the training pairs' item counts
        (item_log_q) and masking of duplicate items in a batch.
        loss_mode="hard" (not in the reference): in-batch BPR against each row's `n_hard` highest-scoring other items
        (ranks hard_skip .. hard_skip + n_hard - 1); 8 is a customary starting value, not a measured optimum.
        loss_mode="mixed" (not in the reference): in-batch BPR plus `hard_weight` times that hard-negative term, mined
        from the stored in-batch weights; 0.1 is a starting value, not a measured optimum (it collapsed in
        the one short run made, 0.01 did not).
        n_negatives, negative_alpha (loss_mode="sampled" only; not in the reference): K sampled negatives per positive,
        drawn with probability proportional to (count + 1)^negative_alpha (UserItemDataset.set_negative_sampling);
        the defaults 1 and 0.0 are the reference's one uniform negative.
        validation (not in the reference; validation.py): None = the reference's flow, nothing constructed.  "last":
        train() holds out every user's last rating >= 4 (validation.leave_last_out) and trains on the rest; or a ready
        (GroundTruth, users, SeenItems) triple.  Every `val_every` epochs the history row gains val_recall@k,
        val_ndcg@k, val_precision@k (k in `val_k`), val_mrr, val_median_rank and val_seconds: exact full-catalogue
        ranks of the held-out items with the seen items removed, for every loss_mode (the validator only reads the
        model).  select_by="recall@50" (any reported key) replaces "lowest training loss" as the checkpoint rule: the
        model train() returns and saves is the one of the best validation, ties to the earlier epoch.  patience=n
        stops after n validations without improvement of `select_by`."""
        if validation is None and (select_by is not None or patience is not None):
            raise ValueError("EmbeddingTrainer: select_by / patience need validation")
        if validation is not None:
            from .validation import report_keys, select_epoch
            if not (isinstance(validation, str) and validation == "last") and not (
                    isinstance(validation, (tuple, list)) and len(validation) == 3):
                raise ValueError(f"EmbeddingTrainer: validation must be None, 'last' or a (GroundTruth, users, SeenItems) "
                                 f"triple, got {validation!r}")
            if isinstance(val_every, bool) or int(val_every) != val_every or int(val_every) < 1:
                raise ValueError(f"EmbeddingTrainer: val_every must be an integer >= 1, got {val_every!r}")
            if select_by is not None and select_by not in report_keys(val_k):
                raise ValueError(f"EmbeddingTrainer: select_by={select_by!r} is not reported; one of {report_keys(val_k)}")
            if patience is not None:
                if select_by is None:
                    raise ValueError("EmbeddingTrainer: patience needs select_by (the value that has to improve)")
                select_epoch([], "max", patience)   # validates the value
        self.validation, self.val_k, self.val_every = validation, tuple(int(k) for k in val_k), int(val_every)
        self.select_by, self.patience = select_by, patience
        if isinstance(n_negatives, bool) or int(n_negatives) != n_negatives or int(n_negatives) < 1:
            raise ValueError(f"EmbeddingTrainer: n_negatives must be an integer >= 1, got {n_negatives!r}")
        if not np.isfinite(float(negative_alpha)):
            raise ValueError(f"EmbeddingTrainer: negative_alpha must be finite, got {negative_alpha!r}")
        if loss_mode != "sampled" and (int(n_negatives) != 1 or float(negative_alpha) != 0.0):
            raise ValueError(f"EmbeddingTrainer: n_negatives / negative_alpha need loss_mode='sampled' (the in-batch modes "
                             f"take their negatives from the batch), got loss_mode={loss_mode!r}")
        self.n_negatives, self.negative_alpha = int(n_negatives), float(negative_alpha)
        if loss_mode in ("hard", "mixed"):
            _check_hard_args(n_hard, hard_skip)
        self.n_hard, self.hard_skip, self.hard_weight = n_hard, hard_skip, hard_weight
        self.data_dir, self.model_output_path = data_dir, model_output_path
        self.embed_dim, self.epochs, self.batch_size, self.learning_rate = embed_dim, epochs, batch_size, learning_rate
        self.loss_mode, self.table_opt, self.dropout, self.seed = loss_mode, table_opt, dropout, seed
        self.temperature, self.logq_correction, self.mask_duplicates = temperature, logq_correction, mask_duplicates
        self.device = L.device()
        self.history: List[Dict] = []

    def load_data(self):
        return load_ml1m(self.data_dir)

    def train(self, ratings_df: Optional[pd.DataFrame] = None, movies_df: Optional[pd.DataFrame] = None
              ) -> TwoTowerModel:
        if ratings_df is None:
            ratings_df, _, movies_df = self.load_data()
        n_users = int(ratings_df["user_id"].max())
        n_items = int(ratings_df["item_id"].max())
        all_item_ids = sorted(movies_df["item_id"].unique().tolist())
        item_genre_dict = build_item_genre_dict(movies_df)
        held_out = None
        if self.validation is not None:
            from . import validation as V
            if isinstance(self.validation, str):
                ratings_df, truth, val_users, seen = V.leave_last_out(ratings_df)
                held_out = (truth, val_users, seen)
            else:
                held_out = tuple(self.validation)
        dataset = UserItemDataset(ratings_df, item_genre_dict, all_item_ids)
        if self.negative_alpha != 0.0:
            dataset.set_negative_sampling(alpha=self.negative_alpha)
        torch.manual_seed(self.seed)
        model = TwoTowerModel(n_users, n_items, embed_dim=self.embed_dim, hidden_dim=128, dropout=self.dropout)
        extra = {}
        if self.loss_mode == "softmax":
            logq = torch.from_numpy(item_log_q(dataset.item_ids, n_items + 1)) if self.logq_correction else None
            extra = dict(temperature=self.temperature, item_logq=logq, mask_duplicates=self.mask_duplicates)
        if self.loss_mode == "hard":
            extra = dict(n_hard=self.n_hard, hard_skip=self.hard_skip, mask_duplicates=self.mask_duplicates)
        if self.loss_mode == "mixed":
            extra = dict(n_hard=self.n_hard, hard_skip=self.hard_skip, mask_duplicates=self.mask_duplicates,
                         hard_weight=self.hard_weight)
        if self.n_negatives != 1:
            extra = dict(n_negatives=self.n_negatives)
        trainer = HipBPRTrainer(model, self.batch_size, lr=self.learning_rate, weight_decay=1e-5, max_norm=1.0,
                                loss_mode=self.loss_mode, table_opt=self.table_opt, seed=self.seed, **extra)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(self.seed)
        Path(self.model_output_path).parent.mkdir(parents=True, exist_ok=True)
        best = float("inf")
        validator, val_values, best_state = None, [], None
        if held_out is not None:
            genre_rows = np.stack([item_genre_dict.get(i, np.zeros(N_GENRES, np.float32)) for i in all_item_ids])
            validator = V.RankValidator(model, all_item_ids, genre_rows, held_out[0], held_out[1], held_out[2],
                                        k_values=self.val_k)
            val_mode = "min" if self.select_by in V.LOWER_IS_BETTER else "max"
        for epoch in range(1, self.epochs + 1):
            model.train()
            lr = cosine_lr(self.learning_rate, epoch - 1, self.epochs)
            t0 = time.time()
            tot = torch.zeros((), dtype=torch.float64, device=self.device)
            nb = 0
            for u, items, genres in dataset.epoch_batches(self.batch_size, gen, self.loss_mode == "sampled",
                                                          n_negatives=self.n_negatives):
                tot += trainer.step(u, items, genres, lr=lr).double()
                nb += 1
            avg = float(tot.item()) / max(nb, 1)   # one host sync per epoch (the reference syncs every step, :194)
            dt = time.time() - t0
            self.history.append({"epoch": epoch, "loss": avg, "seconds": dt, "pairs_per_sec": nb * self.batch_size / dt})
            logger.info("Epoch %d/%d - loss %.4f - %.1fs - lr %.6f", epoch, self.epochs, avg, dt, lr)
            stop = None
            if validator is not None and epoch % self.val_every == 0:
                t0 = time.time()
                rep = validator.evaluate()     # one host read
                row = self.history[-1]
                row.update({f"val_{k}": v for k, v in rep.items() if k in V.report_keys(self.val_k)})
                row["val_seconds"] = time.time() - t0
                logger.info("Epoch %d/%d - validation %s", epoch, self.epochs,
                            {k: round(v, 4) for k, v in row.items() if k.startswith("val_")})
                if self.select_by is not None:
                    val_values.append(rep[self.select_by])
                    best_val, stop = V.select_epoch(val_values, val_mode, self.patience)
                    if best_val == len(val_values) - 1:
                        row["val_best"] = True
                        best_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
                        model.save(self.model_output_path)
            if self.select_by is None and avg < best:
                best = avg
                model.save(self.model_output_path)
            if stop is not None:
                logger.info("Early stop after epoch %d: %d validations without a better %s", epoch, self.patience,
                            self.select_by)
                break
        if best_state is not None:
            model.load_state_dict(best_state)
        genre_matrix = np.stack([item_genre_dict.get(i, np.zeros(N_GENRES, np.float32)) for i in all_item_ids])
        model.precompute_item_embeddings(all_item_ids, genre_matrix, self.device)
        model.save(self.model_output_path)
        self.trainer = trainer
        return model


def retrieval_ndcg(model: TwoTowerModel, ratings_df: pd.DataFrame, movies_df: pd.DataFrame, k_candidates: int = 500,
                   n_eval_users: int = 200, exact: bool = True, on_device: bool = False) -> Dict[str, float]:
    """The reference's `run_evaluate` protocol (src/pipelines/run_pipeline.py:153-230) in its Redis-less form
    (identical default features -> ranker scores tie -> retrieval order decides):
    test set = last N ratings per user by timestamp, N = max(1, int(len*0.1/n_users)); first 200 users;
    ground truth = test items rated >= 4; candidates = top-500 by inner product; NDCG@{5,10,20} of the top 20.
    on_device=True: the candidate ids stay on the device and eval_device scores them (same report)."""
    from .faiss_index import FAISSIndex
    from .metrics import evaluate_model
    n_users = ratings_df["user_id"].nunique()
    n_test = max(1, int(len(ratings_df) * 0.1 / n_users))
    test = ratings_df.sort_values("timestamp").groupby("user_id").tail(n_test)
    eval_users = test["user_id"].unique()[:n_eval_users]
    item_ids = sorted(movies_df["item_id"].unique().tolist())
    gd = build_item_genre_dict(movies_df)
    gm = np.stack([gd.get(i, np.zeros(N_GENRES, np.float32)) for i in item_ids])
    embs = model.get_item_embeddings(item_ids, gm)
    index = FAISSIndex(embed_dim=model.embed_dim, exact=exact)
    index.build_ivf_index(embs.astype(np.float32), item_ids)
    U = model.get_user_embeddings(eval_users.astype(np.int64))
    truth = {int(u): g[g["rating"] >= 4]["item_id"].tolist() for u, g in test[test["user_id"].isin(eval_users)].groupby("user_id")}
    if on_device:
        from .eval_device import GroundTruth, evaluate_topk_device
        # the same f32 query normalisation as batch_search, so the search sees the same queries
        q = U.astype(np.float32)
        q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-8)
        _, ids = index.batch_search_device(torch.from_numpy(np.ascontiguousarray(q)).to(L.device()), k=k_candidates,
                                           normalized=True)
        users = [int(u) for u in eval_users]
        return evaluate_topk_device(ids[:, :20], GroundTruth.from_dict(truth, users), [5, 10, 20])
    _, ids = index.batch_search(U, k=k_candidates)
    recs = {int(u): [int(x) for x in ids[i][:20] if x >= 0] for i, u in enumerate(eval_users)}
    return evaluate_model(recs, truth, [5, 10, 20])


def evaluate_retrieval_all_users(model: TwoTowerModel, index, test_pairs, k_candidates: int = 500, top: int = 20,
                                 batch: int = 65536, k_values=(5, 10, 20), catalog_size: Optional[int] = None,
                                 item_vectors: Optional[torch.Tensor] = None,
                                 item_present: Optional[torch.Tensor] = None, exclude=None) -> Dict[str, Any]:
    """Whole-population retrieval evaluation (not in the reference, which scores 200 users): every user of
    ``test_pairs`` (a frame with user_id / item_id columns, or a (users, items) pair of arrays: the relevant items)
    is retrieved in batches of ``batch`` users (top ``k_candidates`` by inner product, the first ``top`` kept) into
    one device tensor, which eval_device scores; only the report comes back to the host.  Users in order of first
    appearance in ``test_pairs``.  exclude (a seen.SeenItems, e.g. of the training pairs): no user is recommended an
    item of its own row; every batch is searched in groups planned from the host ids (seen.plan_overfetch)."""
    from .eval_device import GroundTruth, evaluate_topk_device
    if isinstance(test_pairs, tuple):
        pu, pi = (np.asarray(x, dtype=np.int64) for x in test_pairs)
    else:
        pu, pi = test_pairs["user_id"].to_numpy(np.int64), test_pairs["item_id"].to_numpy(np.int64)
    _, first = np.unique(pu, return_index=True)
    users = pu[np.sort(first)]
    if users.shape[0] == 0:
        return {"error": "No users to evaluate", "n_users": 0}
    truth = GroundTruth.from_pairs(users, pu, pi)
    dev = L.device()
    top = min(top, k_candidates)
    recs = torch.full((users.shape[0], top), -1, dtype=torch.int64, device=dev)
    uid = torch.from_numpy(users).to(dev)
    for s in range(0, users.shape[0], batch):
        U = model.get_user_embeddings(uid[s:s + batch], as_tensor=True)
        _, ids = index.batch_search_device(U, k=k_candidates, exclude=exclude,
                                           user_ids=None if exclude is None else users[s:s + batch])
        recs[s:s + ids.shape[0], :min(top, ids.shape[1])] = ids[:, :top]
    n_id = int(np.max(index.item_ids)) + 1 if catalog_size else None
    return evaluate_topk_device(recs, truth, list(k_values), catalog_size=catalog_size, item_vectors=item_vectors,
                                item_present=item_present, n_id_space=n_id)
