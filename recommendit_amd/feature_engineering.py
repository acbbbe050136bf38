"""Drop-in FeatureEngineer whose arithmetic runs in the gfx950 HIP library (csrc/ltr_data.hip).

Mirrors the reference's src/features/feature_engineering.py (:24-443): same class, method names and DataFrame
layouts.  File and string parsing (ratings.dat / users.dat / movies.dat, titles, genre strings, the three
demographic normalisations) stays on the host -- a few thousand rows of strings -- and everything that scales with
the number of ratings or of training rows is a kernel: entity statistics, the two feature tables, the
(user, item, label) pairs with their sampled negatives, the 50-column join and the train / test split.

Device API underneath the DataFrame wrappers:
  build_tables_device()        -> (user_tab f64 [n_users+1, 24], item_tab f64 [n_items+1, 23])
  feature_store()              -> a GpuFeatureStore over those tables (serving), no host round trip
  join_device(users, items)    -> X f32 [n, nf] in training semantics
  build_ltr_dataset_device()   -> LtrDataset (train / test: X, y, groups, user_id, item_id, query_id, rating)

Deviations from the reference, all in build_training_pairs: a user whose positives ask for more
negatives than it has unrated items gets all of them (the reference's np.random.choice raises ValueError); the draws and
the split are seeded (the reference uses the global NumPy state).
"""
from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import torch

from . import _lib as L
from .ranker import MAX_DOCS_PER_QUERY
from .recommender import GpuFeatureStore, feature_columns
from .synthetic import GENRES, N_GENRES

logger = logging.getLogger(__name__)

GENRE_TO_IDX = {g: i for i, g in enumerate(GENRES)}
MAX_ITEMS = (1 << 20) - 1          # csrc/ltr_data.hip: the rated-item bitmap of one user lives in LDS

# column order and dtypes of the reference's frames (recorded in tests/golden/g12_ltr_features.npz)
USER_FEATURE_DTYPES = [("user_id", "int64"), ("avg_rating", "float64"), ("rating_count", "int64"),
                       ("recency_score", "float32"), ("log_rating_count", "float32"), ("gender_encoded", "float32"),
                       ("age_normalized", "float32"), ("occupation_normalized", "float32"), ("genre_pref", "object")]
ITEM_FEATURE_DTYPES = [("item_id", "int64"), ("avg_rating", "float64"), ("rating_count", "int64"),
                       ("rating_stddev", "float64"), ("log_rating_count", "float32"), ("popularity_score", "float32"),
                       ("title", "object"), ("genre_vector", "object"), ("year_normalized", "float32")]
PAIR_COLUMNS = ["user_id", "item_id", "label", "rating", "query_id"]
_F64_INTERACTION = {"avg_rating", "item_avg_rating", "rating_stddev", "rating_diff", "genre_affinity"}


def interaction_dtypes() -> List[Tuple[str, str]]:
    """(column, dtype) of build_interaction_features' frame: ids, label, query_id, then the 50 ranking columns in the
    merged frame's order (scalars, the two interaction columns, both genre expansions, genre_affinity last)"""
    cols = feature_columns()
    order = cols[:11] + ["rating_diff", "user_item_popularity_ratio"] + cols[14:] + ["genre_affinity"]
    out = [("user_id", "int64"), ("item_id", "int64"), ("label", "int64"), ("query_id", "int64")]
    for c in order:
        out.append((c, "float64" if c in _F64_INTERACTION or c.startswith("user_genre_") else "float32"))
    return out


def n_test_queries(n_queries: int, test_ratio: float) -> int:
    """max(1, int(n_queries * test_ratio)) (reference :289), never more than there are queries"""
    return min(int(n_queries), max(1, int(n_queries * test_ratio)))


def plan_pairs_host(rating_user, rating_item, rating_value, n_negatives: int) -> Dict[str, np.ndarray]:
    """The pair plan in NumPy, for checks and sizing: per user id (index) P = ratings >= 4, D = distinct rated items,
    U = items with a rating the user never rated, m = negatives, rows = P + m (0 = dropped), query_id (-1 = dropped)."""
    u = np.asarray(rating_user, dtype=np.int64)
    it = np.asarray(rating_item, dtype=np.int64)
    r = np.asarray(rating_value)
    if n_negatives < 1:
        raise ValueError("n_negatives must be >= 1")
    n = int(u.max()) + 1 if u.size else 1
    n_cand = int(np.unique(it).size)
    P = np.bincount(u[r >= 4], minlength=n).astype(np.int64)
    pairs = np.unique(np.stack([u, it], 1), axis=0) if u.size else np.zeros((0, 2), np.int64)
    D = np.bincount(pairs[:, 0], minlength=n).astype(np.int64)
    U = n_cand - D
    keep = (P > 0) & (D > 0) & (U >= n_negatives)
    m = np.where(keep, np.minimum(P * n_negatives, U), 0)
    rows = np.where(keep, P + m, 0)
    qid = np.where(keep, np.cumsum(keep) - 1, -1)
    return {"P": P, "D": D, "U": U, "m": m, "rows": rows, "query_id": qid, "n_candidates": np.int64(n_cand)}


@dataclass
class LtrPart:
    """One side of the split, rows sorted by query_id.  Device tensors except ``groups`` (int32 rows per query on
    the host, which is where rihip_lambdamart_train reads it)."""
    X: torch.Tensor
    y: torch.Tensor
    groups: torch.Tensor
    user_id: torch.Tensor
    item_id: torch.Tensor
    query_id: torch.Tensor
    rating: torch.Tensor
    feature_names: List[str]

    def __len__(self) -> int:
        return int(self.y.shape[0])

    def to_frame(self) -> pd.DataFrame:
        """host copy: ids, label, rating, query_id and one float32 column per feature"""
        df = pd.DataFrame({"user_id": self.user_id.cpu().numpy(), "item_id": self.item_id.cpu().numpy(),
                           "label": self.y.cpu().numpy().astype(np.int64), "rating": self.rating.cpu().numpy().astype(np.int64),
                           "query_id": self.query_id.cpu().numpy()})
        X = self.X.cpu().numpy()
        return pd.concat([df, pd.DataFrame(X, columns=self.feature_names)], axis=1)


@dataclass
class LtrDataset:
    train: LtrPart
    test: LtrPart
    feature_names: List[str]
    n_queries: int
    n_candidates: int
    max_query_rows: int


class DeviceFeatureStore(GpuFeatureStore):
    """GpuFeatureStore over tables that were built on the device: ``device_tables()`` returns them as they are; the
    host arrays ``user`` / ``item`` (which the per-entity setters edit) are copied back only when first touched."""

    def __init__(self, user_tab: torch.Tensor, item_tab: torch.Tensor):
        self._tabs = (user_tab, item_tab)
        self._host: List[Optional[np.ndarray]] = [None, None]
        self._dev = (user_tab, item_tab)

    def _get(self, k: int) -> np.ndarray:
        if self._host[k] is None:
            self._host[k] = self._tabs[k].cpu().numpy().copy()
        return self._host[k]

    user = property(lambda self: self._get(0), lambda self, v: self._host.__setitem__(0, v))
    item = property(lambda self: self._get(1), lambda self, v: self._host.__setitem__(1, v))


class FeatureEngineer:
    """Builds and manages all features for the RecommendIt pipeline (reference :24-443), on the GPU."""

    def __init__(self, data_dir: str = "data/ml-1m"):
        self.data_dir = Path(data_dir)
        self.ratings_df: Optional[pd.DataFrame] = None
        self.users_df: Optional[pd.DataFrame] = None
        self.movies_df: Optional[pd.DataFrame] = None
        self.user_features: Optional[pd.DataFrame] = None
        self.item_features: Optional[pd.DataFrame] = None
        self.grid_blocks = 0            # launch-geometry override for tests (results do not depend on it)
        self._dev: Optional[Dict[str, torch.Tensor]] = None
        self._sizes: Tuple[int, int] = (0, 0)

    # -- data loading (reference :39-72) ----------------------------------------------------------
    def load_data(self) -> None:
        logger.info("Loading MovieLens 1M data from %s", self.data_dir)
        self.ratings_df = pd.read_csv(self.data_dir / "ratings.dat", sep="::",
                                      names=["user_id", "item_id", "rating", "timestamp"], engine="python")
        self.ratings_df["timestamp"] = pd.to_datetime(self.ratings_df["timestamp"], unit="s")
        self.users_df = pd.read_csv(self.data_dir / "users.dat", sep="::",
                                    names=["user_id", "gender", "age", "occupation", "zip_code"], engine="python",
                                    encoding="latin-1")
        self.movies_df = pd.read_csv(self.data_dir / "movies.dat", sep="::", names=["item_id", "title", "genres"],
                                     engine="python", encoding="latin-1")
        self._dev = None
        logger.info("Loaded %d ratings, %d users, %d movies", len(self.ratings_df), len(self.users_df), len(self.movies_df))

    def set_data(self, ratings_df: pd.DataFrame, users_df: pd.DataFrame, movies_df: pd.DataFrame) -> None:
        """frames in load_data's layout, without the files (not in the reference, whose tests assign the attributes)"""
        self.ratings_df, self.users_df, self.movies_df = ratings_df, users_df, movies_df
        self._dev = None

    def _encode_genres(self, genre_str: str) -> np.ndarray:
        vec = np.zeros(N_GENRES, dtype=np.float32)
        for genre in str(genre_str).split("|"):
            idx = GENRE_TO_IDX.get(genre)
            if idx is not None:
                vec[idx] = 1.0
        return vec

    # -- host side: ids, integer ratings, seconds, the small metadata tables ----------------------------------
    @staticmethod
    def rating_arrays(ratings_df: pd.DataFrame) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(user i64, item i64, rating i32, seconds i64) of a ratings frame; ValueError on non-integer ratings"""
        u = ratings_df["user_id"].to_numpy().astype(np.int64)
        it = ratings_df["item_id"].to_numpy().astype(np.int64)
        r = ratings_df["rating"].to_numpy()
        if r.size and not np.all(np.isfinite(r.astype(np.float64)) & (r == np.round(r.astype(np.float64)))):
            raise ValueError("ratings must be integer-valued (1..5)")
        ts = ratings_df["timestamp"]
        if pd.api.types.is_datetime64_any_dtype(ts):
            sec = ts.to_numpy().astype("datetime64[s]").astype(np.int64)
        else:
            sec = ts.to_numpy().astype(np.int64)
        return u, it, r.astype(np.int32), sec

    def host_metadata(self) -> Dict[str, np.ndarray]:
        """user_meta f64 [n_users+1, 3], item_meta f64 [n_items+1, 19], item_in_catalog u8 [n_items+1] and the sizes;
        rows of users / items without a users.dat / movies.dat line are NaN (what the reference's left merges leave)."""
        if self.ratings_df is None or self.users_df is None or self.movies_df is None:
            raise RuntimeError("Call load_data() first.")
        ru = self.ratings_df["user_id"].to_numpy()
        ri = self.ratings_df["item_id"].to_numpy()
        uid = self.users_df["user_id"].to_numpy().astype(np.int64)
        mid = self.movies_df["item_id"].to_numpy().astype(np.int64)
        for name, a in (("user_id", ru), ("item_id", ri), ("user_id", uid), ("item_id", mid)):
            if a.size and int(a.min()) < 1:
                raise ValueError(f"{name} must be >= 1")
        n_users = int(max(ru.max() if ru.size else 0, uid.max() if uid.size else 0))
        n_items = int(max(ri.max() if ri.size else 0, mid.max() if mid.size else 0))
        if n_items > MAX_ITEMS:
            raise ValueError(f"item ids up to {n_items}: the device builder takes ids up to {MAX_ITEMS}")
        demo = self.users_df
        user_meta = np.full((n_users + 1, 3), np.nan, dtype=np.float64)
        user_meta[uid, 0] = (demo["gender"] == "F").astype(np.float32).to_numpy()                    # :150-152
        user_meta[uid, 1] = (demo["age"] / demo["age"].max()).astype(np.float32).to_numpy()
        user_meta[uid, 2] = (demo["occupation"] / demo["occupation"].max()).astype(np.float32).to_numpy()
        movies = self.movies_df
        year = movies["title"].str.extract(r"\((\d{4})\)$")[0].astype(float)                          # :200-204
        yn = ((year - year.min()) / (year.max() - year.min() + 1e-8)).astype(np.float32).fillna(0.5)
        item_meta = np.zeros((n_items + 1, 1 + N_GENRES), dtype=np.float64)
        item_meta[:, 0] = np.nan
        item_meta[mid, 0] = yn.to_numpy()
        if len(movies):
            item_meta[mid, 1:] = np.stack([self._encode_genres(g) for g in movies["genres"].to_numpy()])
        in_cat = np.zeros(n_items + 1, dtype=np.uint8)
        in_cat[mid] = 1
        return {"user_meta": user_meta, "item_meta": item_meta, "item_in_catalog": in_cat,
                "n_users": np.int64(n_users), "n_items": np.int64(n_items)}

    def _upload(self) -> Dict[str, torch.Tensor]:
        if self._dev is None:
            dev = L.device()
            meta = self.host_metadata()
            u, it, r, sec = self.rating_arrays(self.ratings_df)
            d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
                 for k, v in (("ru", u), ("ri", it), ("rv", r), ("rt", sec), ("user_meta", meta["user_meta"]),
                              ("item_meta", meta["item_meta"]), ("in_cat", meta["item_in_catalog"]))}
            self._sizes = (int(meta["n_users"]), int(meta["n_items"]))
            self._dev = d
        return self._dev

    @staticmethod
    def _check_err(err: torch.Tensor, what: str) -> None:
        e = int(err.item())
        if e & 1:
            raise ValueError(f"{what}: a rating has a user or item id outside 1..n")
        if e & 2:
            raise ValueError(f"{what}: a rating value outside 1..5")
        if e & 4:
            raise ValueError(f"{what}: a (user, item) pair has an id outside the feature tables")

    # -- device API ------------------------------------------------------------------------------------------
    def build_tables_device(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """statistics + finalize: (user_tab f64 [n_users+1, 24], item_tab f64 [n_items+1, 23]) in the layout of
        GpuFeatureStore / rihip_rank_features_build; entities without ratings hold the serving defaults"""
        d = self._upload()
        if "user_tab" in d:
            return d["user_tab"], d["item_tab"]
        lib, dev, (nu, ni) = L.lib(), L.device(), self._sizes
        R = int(d["ru"].shape[0])
        ua, ia = C.c_int(), C.c_int()
        L.check(lib.rihip_ltr_widths(C.byref(ua), C.byref(ia), None), "ltr_widths")
        d["user_acc"] = torch.empty((nu + 1, ua.value), dtype=torch.int64, device=dev)
        d["item_acc"] = torch.empty((ni + 1, ia.value), dtype=torch.int64, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(lib.rihip_ltr_stats(L.ptr(d["ru"]), L.ptr(d["ri"]), L.ptr(d["rv"]), L.ptr(d["rt"]), R, nu, ni,
                                    L.ptr(d["item_meta"]), L.ptr(d["in_cat"]), L.ptr(d["user_acc"]), L.ptr(d["item_acc"]),
                                    L.ptr(err), self.grid_blocks, L.stream_ptr()), "ltr_stats")
        ut = torch.empty((nu + 1, 24), dtype=torch.float64, device=dev)
        it = torch.empty((ni + 1, 23), dtype=torch.float64, device=dev)
        scratch = torch.empty(3, dtype=torch.int64, device=dev)
        L.check(lib.rihip_ltr_finalize(L.ptr(d["user_acc"]), L.ptr(d["item_acc"]), L.ptr(d["user_meta"]),
                                       L.ptr(d["item_meta"]), nu, ni, L.ptr(scratch), L.ptr(ut), L.ptr(it),
                                       L.stream_ptr()), "ltr_finalize")
        self._check_err(err, "build_tables_device")
        d["user_tab"], d["item_tab"] = ut, it
        return ut, it

    def feature_store(self) -> GpuFeatureStore:
        """the serving feature store over the tables just built: training and serving read the same numbers"""
        return DeviceFeatureStore(*self.build_tables_device())

    def _col_map(self, feature_names: Optional[Sequence[str]]) -> Tuple[List[str], torch.Tensor]:
        canon = feature_columns()
        names = list(feature_names) if feature_names is not None else canon
        if not 1 <= len(names) <= 64:
            raise ValueError("between 1 and 64 feature names")
        idx = {c: i for i, c in enumerate(canon)}
        cm = torch.tensor([idx.get(n, -1) for n in names], dtype=torch.int32, device=L.device())
        return names, cm

    def join_device(self, user_ids: torch.Tensor, item_ids: torch.Tensor,
                    feature_names: Optional[Sequence[str]] = None, check: bool = True) -> torch.Tensor:
        """X f32 [n, nf] for flat (user, item) rows in the semantics of build_interaction_features (:306-370)"""
        ut, it = self.build_tables_device()
        dev = L.device()
        names, cm = self._col_map(feature_names)
        uid, iid = L.i64c(user_ids).reshape(-1), L.i64c(item_ids).reshape(-1)
        if uid.shape != iid.shape:
            raise ValueError("user_ids and item_ids differ in length")
        X = torch.empty((uid.shape[0], len(names)), dtype=torch.float32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(L.lib().rihip_ltr_join(L.ptr(ut), ut.shape[0], L.ptr(it), it.shape[0], L.ptr(uid), L.ptr(iid), uid.shape[0], L.ptr(cm),
                                       len(names), L.ptr(X), L.ptr(err), self.grid_blocks, L.stream_ptr()), "ltr_join")
        if check:
            self._check_err(err, "join_device")
        return X

    def build_pairs_device(self, n_negatives: int = 4, test_ratio: float = 0.1, seed: int = 0,
                           split_seed: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """plan + emit: the (user, item, label, rating, query_id) rows as [train rows | test rows] plus the plan.
        ``seed`` keys the negative draws and, unless ``split_seed`` is given, the choice of held-out queries."""
        if int(n_negatives) != n_negatives or n_negatives < 1:
            raise ValueError("n_negatives must be an integer >= 1")
        if not 0.0 <= float(test_ratio) <= 1.0:
            raise ValueError("test_ratio must be within [0, 1]")
        self.build_tables_device()
        d, lib, dev, (nu, ni) = self._dev, L.lib(), L.device(), self._sizes
        R = int(d["ru"].shape[0])
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)     # noqa: E731
        i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)     # noqa: E731
        p = {"bucket_off": i64(nu + 2), "bucket": i32(max(R, 1)), "cursor": i32(2 * (nu + 1)), "cand_index": i32(ni + 1),
             "cand_items": i64(ni + 1), "user_rows": i32(nu + 1), "query_id": i32(nu + 1), "row_start": i64(nu + 1),
             "groups": i32(nu + 1), "totals": i64(8)}
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        split_seed = seed if split_seed is None else int(split_seed) & 0xFFFFFFFFFFFFFFFF
        L.check(lib.rihip_ltr_plan(L.ptr(d["ru"]), L.ptr(d["ri"]), L.ptr(d["rv"]), R, L.ptr(d["user_acc"]),
                                   L.ptr(d["item_acc"]), nu, ni, int(n_negatives), float(test_ratio), split_seed,
                                   L.ptr(p["bucket_off"]), L.ptr(p["bucket"]), L.ptr(p["cursor"]), L.ptr(p["cand_index"]),
                                   L.ptr(p["cand_items"]), L.ptr(p["user_rows"]), L.ptr(p["query_id"]),
                                   L.ptr(p["row_start"]), L.ptr(p["groups"]), L.ptr(p["totals"]), self.grid_blocks,
                                   L.stream_ptr()), "ltr_plan")
        tot = p["totals"].cpu().tolist()          # the one host synchronisation: the row count sizes the outputs
        n_rows, nq, n_train_rows, n_train_q, max_rows, n_cand = (int(v) for v in tot[:6])
        if max_rows > MAX_DOCS_PER_QUERY:
            raise ValueError(f"a user would contribute {max_rows} rows (positives + negatives) to its query; the device "
                             f"trainer takes at most {MAX_DOCS_PER_QUERY} documents per query -- lower n_negatives")
        out = {"user_id": i64(n_rows), "item_id": i64(n_rows), "query_id": i64(n_rows), "rating": i32(n_rows),
               "label": torch.empty(n_rows, dtype=torch.float32, device=dev)}
        L.check(lib.rihip_ltr_emit(L.ptr(d["ri"]), L.ptr(d["rv"]), L.ptr(d["rt"]), L.ptr(d["user_acc"]),
                                   L.ptr(p["bucket_off"]), L.ptr(p["bucket"]), L.ptr(p["cand_index"]),
                                   L.ptr(p["cand_items"]), L.ptr(p["user_rows"]), L.ptr(p["query_id"]),
                                   L.ptr(p["row_start"]), L.ptr(p["totals"]), nu, ni, n_rows, seed, L.ptr(out["user_id"]),
                                   L.ptr(out["item_id"]), L.ptr(out["label"]), L.ptr(out["rating"]),
                                   L.ptr(out["query_id"]), self.grid_blocks, L.stream_ptr()), "ltr_emit")
        out.update(groups=p["groups"][:nq], user_rows=p["user_rows"], user_query_id=p["query_id"],
                   row_start=p["row_start"])
        out["sizes"] = {"n_rows": n_rows, "n_queries": nq, "n_train_rows": n_train_rows, "n_train_queries": n_train_q,
                        "max_query_rows": max_rows, "n_candidates": n_cand, "n_test_queries": int(tot[6])}
        return out

    def build_ltr_dataset_device(self, n_negatives: int = 4, test_ratio: float = 0.1, seed: int = 0,
                                 feature_names: Optional[Sequence[str]] = None,
                                 split_seed: Optional[int] = None) -> LtrDataset:
        """ratings -> tables -> pairs -> X, y, groups for both sides of the split, all on the device"""
        pr = self.build_pairs_device(n_negatives, test_ratio, seed, split_seed)
        names, _ = self._col_map(feature_names)
        X = self.join_device(pr["user_id"], pr["item_id"], names)
        sz = pr["sizes"]
        groups = pr["groups"].cpu()
        ntr, ntq = sz["n_train_rows"], sz["n_train_queries"]

        def part(lo, hi, g):
            return LtrPart(X=X[lo:hi], y=pr["label"][lo:hi], groups=g, user_id=pr["user_id"][lo:hi],
                           item_id=pr["item_id"][lo:hi], query_id=pr["query_id"][lo:hi], rating=pr["rating"][lo:hi],
                           feature_names=list(names))

        return LtrDataset(train=part(0, ntr, groups[:ntq]), test=part(ntr, sz["n_rows"], groups[ntq:]),
                          feature_names=list(names), n_queries=sz["n_queries"], n_candidates=sz["n_candidates"],
                          max_query_rows=sz["max_query_rows"])

    # -- DataFrame wrappers with the reference's names and dtypes -------------------------------------------
    def build_user_features(self) -> pd.DataFrame:
        ut, _ = self.build_tables_device()
        t = ut.cpu().numpy()
        cnt = self._dev["user_acc"][:, 0].cpu().numpy()
        ids = np.nonzero(cnt > 0)[0].astype(np.int64)
        r = t[ids]
        df = pd.DataFrame({"user_id": ids, "avg_rating": r[:, 0], "rating_count": cnt[ids].astype(np.int64),
                           "recency_score": r[:, 2].astype(np.float32), "log_rating_count": r[:, 1].astype(np.float32),
                           "gender_encoded": r[:, 3].astype(np.float32), "age_normalized": r[:, 4].astype(np.float32),
                           "occupation_normalized": r[:, 5].astype(np.float32)})
        df["genre_pref"] = list(r[:, 6:])
        self.user_features = df
        logger.info("Built user features for %d users", len(df))
        return df

    def build_item_features(self) -> pd.DataFrame:
        _, it = self.build_tables_device()
        t = it.cpu().numpy()
        cnt = self._dev["item_acc"][:, 0].cpu().numpy()
        ids = np.nonzero(cnt > 0)[0].astype(np.int64)
        r = t[ids]
        titles = pd.Series(self.movies_df["title"].to_numpy(), index=self.movies_df["item_id"].to_numpy())
        titles = titles[~titles.index.duplicated(keep="first")]
        df = pd.DataFrame({"item_id": ids, "avg_rating": r[:, 0], "rating_count": cnt[ids].astype(np.int64),
                           "rating_stddev": r[:, 3], "log_rating_count": r[:, 1].astype(np.float32),
                           "popularity_score": r[:, 2].astype(np.float32), "title": titles.reindex(ids).to_numpy()})
        df["genre_vector"] = list(r[:, 5:].astype(np.float32))
        df["year_normalized"] = r[:, 4].astype(np.float32)
        self.item_features = df
        logger.info("Built item features for %d items", len(df))
        return df

    def build_training_pairs(self, ratings_df: Optional[pd.DataFrame] = None, n_negatives: int = 4,
                             test_ratio: float = 0.1, seed: int = 0) -> Tuple[pd.DataFrame, pd.DataFrame]:
        """(train_pairs_df, test_pairs_df) with columns [user_id, item_id, label, rating, query_id] (reference
        :225-300); a ``ratings_df`` other than the loaded one is planned on its own (feature tables untouched)."""
        fe = self
        if ratings_df is not None and ratings_df is not self.ratings_df:
            fe = FeatureEngineer(str(self.data_dir))
            fe.set_data(ratings_df, self.users_df, self.movies_df)
            fe.grid_blocks = self.grid_blocks
        pr = fe.build_pairs_device(n_negatives, test_ratio, seed)
        df = pd.DataFrame({"user_id": pr["user_id"].cpu().numpy(), "item_id": pr["item_id"].cpu().numpy(),
                           "label": pr["label"].cpu().numpy().astype(np.int64),
                           "rating": pr["rating"].cpu().numpy().astype(np.int64),
                           "query_id": pr["query_id"].cpu().numpy()})[PAIR_COLUMNS]
        ntr = pr["sizes"]["n_train_rows"]
        return df.iloc[:ntr].copy(), df.iloc[ntr:].copy()

    def build_interaction_features(self, pairs_df: pd.DataFrame) -> pd.DataFrame:
        """flat frame of the 50 ranking columns for pairs_df (reference :306-370); values are the float32 numbers the
        ranker trains on, stored with the reference's column dtypes"""
        if self.user_features is None or self.item_features is None:
            raise RuntimeError("Call build_user_features() and build_item_features() first.")
        uid = torch.from_numpy(pairs_df["user_id"].to_numpy().astype(np.int64))
        iid = torch.from_numpy(pairs_df["item_id"].to_numpy().astype(np.int64))
        canon = feature_columns()
        X = self.join_device(uid, iid, canon).cpu().numpy()
        cols = {"user_id": pairs_df["user_id"].to_numpy(), "item_id": pairs_df["item_id"].to_numpy(),
                "label": pairs_df["label"].to_numpy(), "query_id": pairs_df["query_id"].to_numpy()}
        idx = {c: i for i, c in enumerate(canon)}
        for name, dt in interaction_dtypes()[4:]:
            cols[name] = X[:, idx[name]].astype(dt)
        return pd.DataFrame(cols)

    # -- persistence (reference :376-432) ----------------------------------------------------------------------
    def save_features(self, output_dir: str = "data/features") -> None:
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        for df, vec, prefix, fname in ((self.user_features, "genre_pref", "genre_pref_", "user_features.parquet"),
                                       (self.item_features, "genre_vector", "genre_vec_", "item_features.parquet")):
            if df is None:
                continue
            mat = np.stack(df[vec].values)
            gdf = pd.DataFrame(mat, columns=[f"{prefix}{i}" for i in range(N_GENRES)])
            pd.concat([df.drop(columns=[vec]).reset_index(drop=True), gdf], axis=1).to_parquet(out / fname, index=False)
            logger.info("Saved features to %s", out / fname)

    def load_features(self, features_dir: str = "data/features") -> None:
        d = Path(features_dir)
        for attr, vec, prefix, fname in (("user_features", "genre_pref", "genre_pref_", "user_features.parquet"),
                                         ("item_features", "genre_vector", "genre_vec_", "item_features.parquet")):
            if not (d / fname).exists():
                continue
            df = pd.read_parquet(d / fname)
            gcols = [f"{prefix}{i}" for i in range(N_GENRES)]
            if all(c in df.columns for c in gcols):
                df[vec] = list(df[gcols].values.astype(np.float32))
                df.drop(columns=gcols, inplace=True)
            setattr(self, attr, df)
            logger.info("Loaded %s: %d rows", attr, len(df))

    def get_feature_columns(self) -> List[str]:
        return feature_columns()
