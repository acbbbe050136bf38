"""GPU-resident serving stage: user tower -> inner-product retrieval -> feature assembly -> LambdaMART.

Mirrors the online chain of the reference's RecommendationPipeline.get_recommendations
(src/serving/recommender.py:269-387): A11 get_user_embedding -> R2 search(k=500) -> feature fetch
(:319-322) -> S1 _build_ranking_features (:213-263) -> K1 ranker.predict (:338) -> nlargest(k) (:346),
but for a BATCH of users and without leaving the device between stages.  The reference class itself stays
the caller for single requests (drop-in through the three model classes); this module is the "next" row
§8f-1 of SURVEY.md: a GPU feature table that supersedes the Redis MGET + the 500-iteration Python loop.
"""
from __future__ import annotations

import math
import os

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import rerank as RR
from .coldstart import UserHistories, fold_in_users_device
from .faiss_index import FAISSIndex
from .ranker import LightGBMRanker
from .exclusion import check_exclusion
from .seen import SeenItems, overfetch_k, plan_overfetch
from .sq8_index import SQ8Index
from .two_tower import N_GENRES, TwoTowerModel

USER_SCALARS = [("avg_rating", 3.5), ("log_rating_count", 0.0), ("recency_score", 0.5), ("gender_encoded", 0.0),
                ("age_normalized", 0.3), ("occupation_normalized", 0.3)]            # recommender.py:227-232
_DEFAULT = object()     # "use the constructor's diversity" (None turns the stage off for one call)
ITEM_SCALARS = [("avg_rating", 3.5), ("log_rating_count", 0.0), ("popularity_score", 0.0), ("rating_stddev", 0.0),
                ("year_normalized", 0.5)]                                           # recommender.py:234-238


def feature_columns() -> List[str]:
    """The 50 ranking columns in the order of the reference's get_feature_columns
    (src/features/feature_engineering.py:434-443)."""
    return (["avg_rating", "log_rating_count", "recency_score", "gender_encoded", "age_normalized",
             "occupation_normalized", "item_avg_rating", "item_log_rating_count", "popularity_score", "rating_stddev",
             "year_normalized", "rating_diff", "user_item_popularity_ratio", "genre_affinity"]
            + [f"user_genre_{i}" for i in range(N_GENRES)] + [f"item_genre_{i}" for i in range(N_GENRES)])


class GpuFeatureStore:
    """float64 feature tables on the device; rows not loaded keep the reference's defaults.
    Replaces RedisFeatureStore.get_user_features / get_item_features_batch (src/features/feature_store.py:113-150)
    on the accelerated path (same keys inside the per-entity dicts)."""

    def __init__(self, n_users: int, n_items: int):
        UW, IW = 6 + N_GENRES, 5 + N_GENRES
        self.user = np.zeros((n_users + 1, UW), dtype=np.float64)
        self.item = np.zeros((n_items + 1, IW), dtype=np.float64)
        self.user[:, :6] = [d for _, d in USER_SCALARS]
        self.item[:, :5] = [d for _, d in ITEM_SCALARS]
        self._dev: Optional[Tuple[torch.Tensor, torch.Tensor]] = None

    def set_user_features(self, user_id: int, feat: Dict[str, Any]) -> None:
        row = self.user[user_id]
        for j, (name, dflt) in enumerate(USER_SCALARS):
            row[j] = float(feat.get(name, dflt))
        gp = feat.get("genre_pref", [0.0] * N_GENRES)
        for i in range(N_GENRES):
            row[6 + i] = float(gp[i]) if i < len(gp) else 0.0
        self._dev = None

    def set_item_features(self, item_id: int, feat: Optional[Dict[str, Any]]) -> None:
        feat = feat or {}
        row = self.item[item_id]
        for j, (name, dflt) in enumerate(ITEM_SCALARS):
            row[j] = float(feat.get(name, dflt))
        gv = feat.get("genre_vector", [0.0] * N_GENRES)
        for i in range(N_GENRES):
            row[5 + i] = float(gv[i]) if i < len(gv) else 0.0
        self._dev = None

    def load_arrays(self, user_tab: Optional[np.ndarray] = None, item_tab: Optional[np.ndarray] = None) -> None:
        """Bulk load (e.g. from the parquet feature files): arrays in the table layout, row index = id."""
        if user_tab is not None:
            self.user[: len(user_tab)] = user_tab
        if item_tab is not None:
            self.item[: len(item_tab)] = item_tab
        self._dev = None

    def load_all_features(self, user_features_df, item_features_df, batch_size: int = 500) -> None:
        """Bulk load from the DataFrames the reference's FeatureEngineer produces / saves (same entry point and column
        conventions as RedisFeatureStore.load_all_features, src/features/feature_store.py:156-228): scalar columns by
        name, `genre_pref_<i>` / `genre_vec_<i>` expanded columns (feature_engineering.py:382-404) or the un-expanded
        `genre_pref` / `genre_vector` array columns; columns that are absent keep the defaults of
        _build_ranking_features (recommender.py:227-238); ids beyond the table size grow it.  Vectorised: no per-row
        Python loop (the reference iterates rows and msgpack-serialises each one)."""
        def fill(tab, df, id_col, scalars, vec_prefix, vec_col, off):
            if df is None or len(df) == 0:
                return tab
            ids = df[id_col].to_numpy().astype(np.int64)
            if ids.min() < 0:
                raise ValueError(f"negative {id_col}")
            if ids.max() >= tab.shape[0]:          # grow, new rows at their defaults
                grown = np.repeat(tab[:1].copy(), int(ids.max()) + 1, axis=0)
                grown[:, :] = self._default_row(tab.shape[1], scalars)
                grown[: tab.shape[0]] = tab
                tab = grown
            for j, (name, _) in enumerate(scalars):
                if name in df.columns:
                    tab[ids, j] = df[name].to_numpy().astype(np.float64)
            vec_cols = [f"{vec_prefix}{i}" for i in range(N_GENRES)]
            if all(c in df.columns for c in vec_cols):
                tab[ids, off:off + N_GENRES] = df[vec_cols].to_numpy().astype(np.float64)
            elif vec_col in df.columns:
                tab[ids, off:off + N_GENRES] = np.stack([np.asarray(v, dtype=np.float64)[:N_GENRES]
                                                         for v in df[vec_col].to_numpy()])
            return tab

        self.user = fill(self.user, user_features_df, "user_id", USER_SCALARS, "genre_pref_", "genre_pref", 6)
        self.item = fill(self.item, item_features_df, "item_id", ITEM_SCALARS, "genre_vec_", "genre_vector", 5)
        self._dev = None

    @staticmethod
    def _default_row(width: int, scalars) -> np.ndarray:
        row = np.zeros((width,), dtype=np.float64)
        row[: len(scalars)] = [d for _, d in scalars]
        return row

    @classmethod
    def from_parquet(cls, features_dir: str, n_users: int = 0, n_items: int = 0) -> "GpuFeatureStore":
        """Device feature tables straight from `user_features.parquet` / `item_features.parquet` as written by
        FeatureEngineer.save_features (src/features/feature_engineering.py:376-406) -- the parquet -> device-table
        loader SURVEY.md §8f-1 names.  A missing file leaves that table at its defaults (the reference's
        load_features skips missing files too, :415, :425)."""
        import pandas as pd
        from pathlib import Path
        d = Path(features_dir)
        up, ip = d / "user_features.parquet", d / "item_features.parquet"
        udf = pd.read_parquet(up) if up.exists() else None
        idf = pd.read_parquet(ip) if ip.exists() else None
        nu = max(n_users, int(udf["user_id"].max()) if udf is not None and len(udf) else 0)
        ni = max(n_items, int(idf["item_id"].max()) if idf is not None and len(idf) else 0)
        st = cls(nu, ni)
        st.load_all_features(udf, idf)
        return st

    def item_genre_tags(self, item_ids) -> np.ndarray:
        """uint32 [n] tag words for FAISSIndex.set_item_tags: bit g is set iff item_ids[i]'s genre vector in the item
        table has genre g (an id outside the table gets 0)"""
        from .faiss_index import genre_tags
        ids = np.asarray(item_ids, dtype=np.int64).reshape(-1)
        ok = (ids >= 0) & (ids < self.item.shape[0])
        tags = np.zeros(ids.shape[0], dtype=np.uint32)
        tags[ok] = genre_tags(self.item[ids[ok], 5:5 + N_GENRES])
        return tags

    def device_tables(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._dev is None:
            dev = L.device()
            self._dev = (torch.from_numpy(self.user).to(dev), torch.from_numpy(self.item).to(dev))
        return self._dev


def build_ranking_features_device(store: GpuFeatureStore, user_ids: torch.Tensor, cand_ids: torch.Tensor,
                                  feature_names: Sequence[str], user_tab: Optional[torch.Tensor] = None) -> torch.Tensor:
    """X f32 [nq*kc, len(feature_names)] on device (the matrix ranker.predict would see).  user_tab: a device f64
    [n, 24] table that user_ids index instead of the store's user table (the transient rows of cold-start users)."""
    lib = L.lib()
    ut, it = store.device_tables()
    if user_tab is not None:
        ut = user_tab
    key = tuple(feature_names)
    col_map = store._col_maps.get(key) if hasattr(store, "_col_maps") else None
    if col_map is None or col_map.device != ut.device:   # one H2D copy per feature list, not per request
        canon = {n: i for i, n in enumerate(feature_columns())}
        col_map = torch.tensor([canon.get(n, -1) for n in feature_names], dtype=torch.int32, device=ut.device)
        if not hasattr(store, "_col_maps"):
            store._col_maps = {}
        store._col_maps[key] = col_map
    uid = L.i64c(user_ids)
    cand = L.i64c(cand_ids)
    nq, kc = cand.shape
    X = torch.empty((nq * kc, len(feature_names)), dtype=torch.float32, device=ut.device)
    L.check(lib.rihip_rank_features_build(ut.data_ptr(), ut.shape[0], it.data_ptr(), it.shape[0], uid.data_ptr(),
                                          cand.data_ptr(), nq, kc, col_map.data_ptr(), len(feature_names),
                                          X.data_ptr(), L.stream_ptr()), "rank_features_build")
    return X


class GpuRecommendationPipeline:
    def __init__(self, model: TwoTowerModel, index: FAISSIndex, ranker: LightGBMRanker, store: GpuFeatureStore,
                 top_k_candidates: int = 500, top_k_results: int = 20, feature_log_rows: int = 0,
                 seen: Optional[SeenItems] = None, diversity: Optional[float] = None,
                 diversity_vectors: Optional[torch.Tensor] = None, exclusion: str = "overfetch"):
        """defaults = settings.TOP_K_CANDIDATES / TOP_K_RESULTS (src/config.py:11-12).

        seen (not in the reference, which recommends what the user has already rated: SURVEY.md §3.4 hazard ii): a
        store of excluded item ids per user id; with one attached, retrieval over-fetches and a device filter drops
        each user's items, so features, the feature log, the ranker and the top-k still see top_k_candidates columns.
        exclusion="scan" (opt-in; "overfetch" is the sentence above): the seen items are excluded inside the index scan
        instead (FAISSIndex.batch_search_device(exclusion="scan")): recommend_batch, get_recommendations and
        recommend_cold_batch(exclude_history=True) run ONE chain over the whole batch, host and device ids alike, at
        top_k_candidates with no over-fetch, no groups, no device filter and no limit on a user's list; the same
        candidates bit for bit.  That search synchronises the stream, so graph=True then raises ValueError: keep
        "overfetch" for captured single requests.  Any other value: ValueError.

        diversity (not in the reference, whose chain ends in nlargest): None = the last stage is the plain top-k by
        ranker score, as ever.  A number in [0, 1] = greedy MMR re-ranking instead (rerank.py; the definition is at
        rihip_rank_topk_diverse in recommendit_hip.h): each pick maximises (1 - diversity) * normalised score -
        diversity * largest cosine to the items already picked, so 0 is the plain top-k again and larger values trade
        ranker score for avg_diversity, the metric the evaluation reports.  diversity_vectors: the vectors the cosine is
        taken over, a device float64 [n, w <= 256] tensor indexed by item id (e.g. item-tower embeddings); None = the
        genre columns of the feature store's item table, i.e. exactly intra_list_diversity's vectors.  The stage only
        replaces the one behind seen-item exclusion and item_filter, so it composes with both, and it is one launch
        without synchronisation: graph=True works.

        index may be an SQ8Index (the 8-bit scalar-quantised index, sq8_index.py): tower -> SQ8 search -> features ->
        ranker -> top-k, with the refined search when the index's set_refine is on.  recommend_batch(item_filter=...)
        runs the same chain on the filtered SQ8 search when the index has item tags (SQ8Index.set_item_tags) and raises
        ValueError, before anything is launched, when it has none.  A seen store on the pipeline, diversity, the
        cold-start calls and graph=True are not built for it: each raises ValueError (seen items can be excluded on the
        index itself: SQ8Index.batch_search_device(exclude=...)).

        feature_log_rows = R > 0 keeps the ranking-feature rows of the newest R served (user, candidate) pairs in a
        device ring (the "feature DataFrame from serving" of detect_training_serving_skew, metrics.py:234-260):
        serving_features(), detect_skew(), reset_feature_log().  0 leaves the chain as it is."""
        self.exclusion = check_exclusion(exclusion)
        self.model, self.index, self.ranker, self.store = model, index, ranker, store
        self._sq8 = isinstance(index, SQ8Index)
        if self._sq8:
            self._no_sq8("a seen store", seen is not None)
            self._no_sq8("diversity", diversity is not None)
        self.top_k_candidates, self.top_k_results = top_k_candidates, top_k_results
        self._graphs: Dict[Tuple[int, int, Optional[int], Optional[float]], Any] = {}
        self.diversity = None if diversity is None else RR.check_diversity(diversity)
        if diversity_vectors is not None:
            RR.check_table(diversity_vectors)
        self.diversity_vectors = diversity_vectors
        self.seen = seen
        self._pin: Dict[int, Any] = {}
        self._popularity: Optional[torch.Tensor] = None       # set_popularity's order (None: the default)
        self._pop_default: Optional[Tuple[Any, Any, torch.Tensor]] = None
        self._defer = os.environ.get("RIHIP_SERVE_DEFER", "1") != "0"   # 0: exactness check inside the search (experiments)
        self._log: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]] = None
        self.reset_feature_log(feature_log_rows)

    def _no_sq8(self, what: str, asked: bool) -> None:
        if self._sq8 and asked:
            raise ValueError(f"{what} is not supported on an SQ8 index (SQ8Index serves the plain and the filtered chain only)")

    def set_seen(self, seen: Optional[SeenItems]) -> None:
        """attach / replace / detach (None) the store of excluded items; captured graphs are re-captured"""
        self._no_sq8("a seen store", seen is not None)
        self.seen = seen

    def exclusion_deficit(self) -> int:
        """requests so far whose over-fetch could not fill top_k_candidates allowed candidates (one synchronisation);
        0 whenever the over-fetch was planned from the attached store"""
        return self.index.exclusion_deficit()

    def _diversity_stage(self, diversity, k: int):
        """the checked last stage of one call: None (plain top-k) or (weight, table, col0, width); ValueError for a bad
        weight or a shape outside the kernel's limits, before anything is launched"""
        d = self.diversity if diversity is _DEFAULT else diversity
        if d is None:
            return None
        d = RR.check_diversity(d)
        if self.diversity_vectors is not None:
            tab = self.diversity_vectors
            col0, w = RR.check_table(tab)
        else:
            tab, col0, w = None, 5, N_GENRES          # the item table, fetched where the chain runs
        RR.check_shape(min(self.top_k_candidates, max(int(self.index.index.ntotal), 1)), k, w)
        if tab is None:
            tab = self.store.device_tables()[1]
        elif not tab.is_cuda:
            raise ValueError("diversity_vectors must live on the device")
        return d, tab, col0, w

    @torch.no_grad()
    def recommend_batch(self, user_ids, k: Optional[int] = None, graph: bool = False,
                        exclude_seen: Optional[bool] = None, item_filter=None, diversity=_DEFAULT
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """recommendations of a batch of users (outputs: _recommend).  exclude_seen: drop each user's items of the
        attached seen store from retrieval; None = yes iff a store is attached.  With host ids the batch is served in
        groups by how far each user has to over-fetch (seen.plan_overfetch: one heavy user does not slow the rest), one
        run of the chain per group; graph=True and device ids run as one group at the store's longest list.

        item_filter (not in the reference; the index needs set_item_tags): (any_of, all_of, none_of) over the items' tag
        words, shared by the batch or one row per user (FAISSIndex.batch_search_device).  Retrieval then returns only
        passing items, -1 padded when fewer than top_k_candidates pass; features, ranker and top-k run as on any short
        retrieval result, and with a seen store the candidates are filter AND not-seen (one group at the batch's
        longest seen list).  The filtered search synchronises the stream for its exactness check, so it cannot be
        captured: graph=True with a filter raises ValueError.

        diversity: overrides the constructor's value for this call (a number in [0, 1], or None for the plain top-k);
        the outputs are then in MMR selection order, not in score order."""
        k = k or self.top_k_results
        self._no_sq8("graph=True", bool(graph))
        if self._sq8 and item_filter is not None and self.index._tags is None:      # (host state only: nothing is launched)
            raise ValueError("item_filter on an SQ8 index needs item tags: call SQ8Index.set_item_tags() first")
        self._no_sq8("exclude_seen", bool(exclude_seen))
        self._no_sq8("diversity", diversity is not _DEFAULT and diversity is not None)
        div = self._diversity_stage(diversity, k)
        if exclude_seen and self.seen is None:
            raise ValueError("exclude_seen=True without a seen store (set_seen)")
        if self.exclusion == "scan" and self.seen is not None and exclude_seen is not False:
            if graph:
                raise ValueError('graph=True cannot serve exclusion="scan": the excluded search synchronises the stream '
                                 '(keep exclusion="overfetch" for captured requests)')
            if self._sq8 and item_filter is not None and self.index._tags is None:
                raise ValueError("item_filter on an SQ8 index needs item tags: call SQ8Index.set_item_tags() first")
            return self._chain(self._ids_to_device(user_ids), k, item_filter=item_filter, div=div, scan_seen=self.seen)
        if item_filter is not None:
            if graph:
                raise ValueError("graph=True cannot serve an item_filter: the filtered search synchronises the stream")
            k_eff = None
            if self.seen is not None and exclude_seen is not False:
                ntotal = self.index.index.ntotal
                if isinstance(user_ids, torch.Tensor) and user_ids.is_cuda:
                    most = self.seen.max_count
                else:
                    host = np.asarray(user_ids.tolist() if isinstance(user_ids, torch.Tensor) else user_ids, dtype=np.int64)
                    most = int(self.seen.counts_of(host).max()) if host.size else 0
                if most:
                    k_eff = overfetch_k(min(self.top_k_candidates, ntotal), most, ntotal, int(L.lib().rihip_ip_index_max_k()))
            return self._chain(self._ids_to_device(user_ids), k, k_eff=k_eff, item_filter=item_filter, div=div)
        if self.seen is None or exclude_seen is False:
            return self._recommend(user_ids, k, graph, None, div)
        ntotal = self.index.index.ntotal
        kc = min(self.top_k_candidates, ntotal)
        k_max = int(L.lib().rihip_ip_index_max_k())
        if graph or (isinstance(user_ids, torch.Tensor) and user_ids.is_cuda):
            return self._recommend(user_ids, k, graph, overfetch_k(kc, self.seen.max_count, ntotal, k_max)
                                   if self.seen.max_count else None, div)
        host = np.asarray(user_ids.tolist() if isinstance(user_ids, torch.Tensor) else user_ids, dtype=np.int64)
        extra = self.seen.counts_of(host)
        if not extra.any():
            return self._recommend(user_ids, k, False, None, div)
        plan = plan_overfetch(extra, kc, ntotal, k_max)
        if len(plan) == 1:
            return self._recommend(user_ids, k, False, plan[0][0], div)
        outs = None
        for k_eff, pos in plan:
            part = self._recommend(host[pos].tolist(), k, False, k_eff if extra[pos].any() else None, div)
            if outs is None:
                outs = tuple(torch.empty((host.shape[0],) + tuple(p.shape[1:]), dtype=p.dtype, device=p.device)
                             for p in part)
            sel = torch.from_numpy(pos).to(part[0].device)
            for o, p in zip(outs, part):
                o.index_copy_(0, sel, p)
        return outs

    def _recommend(self, user_ids, k: int, graph: bool, k_eff: Optional[int], div=None
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (item_ids i64 [nq,k], ranker scores f64 [nq,k], retrieval scores f32 [nq,k]) on device; -1 padded
        where retrieval returned fewer than k candidates.  Ties in the ranker score keep retrieval order
        (DataFrame.nlargest(keep='first'), recommender.py:346).

        graph=True (small request batches): the ~20 launches of the chain are captured once per (batch size, k) into a
        hipGraph and replayed -- a single request is launch-bound otherwise.  The returned tensors are the graph's static
        outputs: valid until the next replay of the same shape.  Falls back to the eager chain when the shape takes a
        path with a host synchronisation inside the chain.

        k_eff: None = retrieval as it is; else retrieval fetches k_eff candidates and the seen filter keeps the
        first top_k_candidates allowed ones (a consumer of the search like the stages behind it: it runs again with
        the chain after an exactness re-do).

        div: None = the last stage is rihip_rank_topk; else _diversity_stage's tuple and it is rihip_rank_topk_diverse."""
        # The retrieval stage's exactness check is deferred to the END of the chain (FAISSIndex.set_deferred_check): the
        # thresholded IVF pass of a large batch used to stop for a host round trip in the middle of the chain (a 54 us
        # hole at 256 requests, and the reason such batches could not be captured as a hipGraph).  In the rare case that
        # queries had to be re-done exactly, the chain runs again on the corrected candidates (not deferred).
        if not self._defer:
            out = self._replay(user_ids, k, k_eff, div) if graph else None
            if out is not None:
                return out[0]
            return self._chain(self._ids_to_device(user_ids), k, k_eff=k_eff, div=div)
        self.index.set_deferred_check(True)
        try:
            out = self._replay(user_ids, k, k_eff, div) if graph else None
            uid = None
            if out is not None:
                out, redone = out
            else:
                uid = self._ids_to_device(user_ids)
                out = self._chain(uid, k, k_eff=k_eff, div=div)
                redone = self.index.finish_search()
        finally:
            self.index.set_deferred_check(False)
        if redone:
            if uid is None:
                uid = self._ids_to_device(user_ids)
            if self._log is not None:       # the batch is logged again with its final candidates: drop the first rows
                L.check(L.lib().rihip_feature_log_rewind(self._log[3].data_ptr(), L.stream_ptr()), "feature_log_rewind")
            out = self._chain(uid, k, k_eff=k_eff, div=div)
        return out

    def _ids_to_device(self, user_ids) -> torch.Tensor:
        """user ids -> device without stalling the host: `torch.as_tensor(list, device=...)` is a pageable copy, which
        blocks the host until everything already enqueued on the stream (the previous batch's chain) has run -- a 0.1 ms
        hole per 256-request batch.  A pinned staging buffer per batch size + an asynchronous copy lets the host enqueue
        batch k+1 while the GPU still works on batch k."""
        if isinstance(user_ids, torch.Tensor) and user_ids.is_cuda:
            return user_ids.to(dtype=torch.long)
        n = len(user_ids)
        ent = self._pin.get(n)
        if ent is None:
            ent = (torch.empty((n,), dtype=torch.long).pin_memory(), torch.empty((n,), dtype=torch.long, device=L.device()),
                   torch.cuda.Event())
            self._pin[n] = ent
        pin, dev_t, ev = ent
        ev.synchronize()                        # the previous copy out of the staging buffer has executed
        pin.copy_(torch.as_tensor(user_ids, dtype=torch.long))
        dev_t.copy_(pin, non_blocking=True)
        ev.record()
        return dev_t

    def _graph_state(self, div=None):
        """everything a captured chain bakes in besides the torch-owned tensors of its own pool: the library's scratch
        generation (handle-owned buffers that are freed when they grow, nprobe, id map, index / forest content) and the
        identity of the feature tables and of the three stage objects; with a diversified last stage (div) also its
        weight and the identity of its vector table"""
        ut, it = self.store.device_tables()
        return (int(L.lib().rihip_scratch_generation()), ut.data_ptr(), it.data_ptr(), id(self.index), id(self.ranker),
                id(self.model), self.top_k_candidates, tuple(self.ranker.feature_names),
                None if self._log is None else (self._log[0].data_ptr(), self._log[0].shape[0]),
                None if self.seen is None else (self.seen.offsets.data_ptr(), self.seen.items.data_ptr(),
                                                self.seen.n_users),
                None if div is None else (div[0], div[1].data_ptr(), tuple(div[1].shape), tuple(div[1].stride()),
                                          div[2], div[3]))

    def _replay(self, user_ids, k: int, k_eff: Optional[int] = None, div=None):
        nq = len(user_ids)
        key = (nq, k, k_eff, None if div is None else div[0])
        ent = self._graphs.get(key)
        if ent is not None and ent is not False and ent[3] != self._graph_state(div):
            # an eager call (or a capture of a larger shape) grew a scratch buffer, nprobe changed, the feature tables
            # were reloaded, ...: the pointers inside this graph are stale -- drop it and capture again
            ent = None
            del self._graphs[key]
        if ent is None:
            dev = L.device()
            su = torch.ones((nq,), dtype=torch.long, device=dev)
            try:
                cur = torch.cuda.current_stream(dev)
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(cur)
                with torch.cuda.stream(side):      # warm-up: scratch buffers, LDS grants, lazy module loads
                    for _ in range(2):
                        self._chain(su, k, log=False, k_eff=k_eff, div=div)
                        self.index.finish_search()
                cur.wait_stream(side)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = self._chain(su, k, k_eff=k_eff, div=div)
                deferred = self.index.search_pending()      # the captured search left its exactness check to the caller
                self.index.set_deferred_check(True)         # (capture ran nothing: drop the pending state)
                ent = (g, su, out, self._graph_state(div), deferred)   # state recorded AFTER capture: the warm-up may have grown scratch
            except Exception:                        # a path with a host sync cannot be captured: stay eager for this shape
                torch.cuda.synchronize()
                ent = False
            self._graphs[key] = ent
        if ent is False:
            return None
        g, su, out, _, deferred = ent
        su.copy_(torch.as_tensor(user_ids, dtype=torch.long), non_blocking=True)
        g.replay()
        # a replay runs no host code: the failure count of its deferred search is read here (one synchronisation)
        return out, (self.index.last_fail_count() if deferred else 0)

    def _chain(self, uid: torch.Tensor, k: int, log: bool = True, k_eff: Optional[int] = None, item_filter=None,
               div=None, q: Optional[torch.Tensor] = None, user_tab: Optional[torch.Tensor] = None,
               seen: Optional[SeenItems] = None, log_uid: Optional[torch.Tensor] = None,
               scan_seen: Optional[SeenItems] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """q, user_tab, seen, log_uid (the cold-start chain): precomputed normalised queries instead of the user tower,
        a table uid indexes instead of the store's user table, the exclusion store uid indexes instead of the attached
        one, and the user ids the feature log records instead of uid.  scan_seen (exclusion="scan"): the store whose
        row uid[q] retrieval excludes inside its scan; k_eff is then None and nothing is filtered behind the search"""
        if q is None:
            q = self.model.get_user_embeddings(uid, as_tensor=True)
        # tower outputs are already L2-normalised (two_tower.py:42): the wrapper's re-normalisation (faiss_index.py:108-110)
        # would divide by 1 +- 1e-7 and cost three tensor ops per request
        if scan_seen is not None:
            rs, cand = self.index.batch_search_device(q, k=self.top_k_candidates, normalized=True, exclude=scan_seen,
                                                      user_ids=uid, item_filter=item_filter, exclusion="scan")
        elif item_filter is None:
            rs, cand = self.index.batch_search_device(q, k=k_eff or self.top_k_candidates, normalized=True)
        else:
            rs, cand = self.index.batch_search_device(q, k=k_eff or self.top_k_candidates, normalized=True,
                                                      item_filter=item_filter)
        nq, kc = cand.shape
        if k_eff is not None:       # over-fetched: keep each user's first top_k_candidates unseen candidates
            kc = min(self.top_k_candidates, self.index.index.ntotal)
            fs = torch.empty((nq, kc), dtype=torch.float32, device=cand.device)
            fc = torch.empty((nq, kc), dtype=torch.int64, device=cand.device)
            self.index.filter_excluded(rs, cand, kc, self.seen if seen is None else seen, uid, fs, fc)
            rs, cand = fs, fc
        X = build_ranking_features_device(self.store, uid, cand, self.ranker.feature_names, user_tab)
        if log and self._log is not None:
            self._append_log(X, uid if log_uid is None else log_uid, cand)
        scores = self.ranker.predict_device(X)
        k = min(k, kc)
        if div is not None:
            return RR.launch(scores, cand, rs, k, div[0], div[1], div[2], div[3])
        ids = torch.empty((nq, k), dtype=torch.int64, device=cand.device)
        top = torch.empty((nq, k), dtype=torch.float64, device=cand.device)
        trs = torch.empty((nq, k), dtype=torch.float32, device=cand.device)
        L.check(L.lib().rihip_rank_topk(scores.data_ptr(), cand.data_ptr(), rs.data_ptr(), nq, kc, k, ids.data_ptr(),
                                        top.data_ptr(), trs.data_ptr(), L.stream_ptr()), "rank_topk")
        return ids, top, trs

    # ---- cold-start users (not in the reference beyond the popularity fallback) ------------------------------------
    def set_popularity(self, item_ids) -> None:
        """the order the popularity fallback serves (most popular first; the reference's _popularity_fallback list,
        recommender.py:393-410); None = back to the default: the items stored in the index by the item table's
        log_rating_count, descending, ties to the lower item id"""
        if item_ids is None:
            self._popularity = None
            return
        ids = np.asarray(item_ids.detach().cpu().numpy() if isinstance(item_ids, torch.Tensor) else item_ids,
                         dtype=np.int64).reshape(-1)
        if ids.shape[0] and ids.min() < 0:
            raise ValueError("set_popularity: negative item id")
        self._popularity = torch.from_numpy(ids.copy()).to(L.device())

    def popularity_order(self) -> torch.Tensor:
        """device i64 item ids, most popular first: what set_popularity set, else the default order (rebuilt when the
        index or the item table changes)"""
        if self._popularity is not None:
            return self._popularity
        ids, tab = self.index.item_ids, self.store.device_tables()[1]
        c = self._pop_default
        if c is None or c[0] is not ids or c[1] is not tab:
            host = np.unique(np.asarray(ids, dtype=np.int64))
            val = np.zeros(host.shape[0], dtype=np.float64)          # an id outside the table: the default row's 0.0
            ok = (host >= 0) & (host < self.store.item.shape[0])
            val[ok] = self.store.item[host[ok], 1]
            order = np.lexsort((host, -val))
            c = self._pop_default = (ids, tab, torch.from_numpy(host[order]).to(L.device()))
        return c[2]

    def _popularity_rows(self, hist: UserHistories, slots: np.ndarray, k: int, width: int, exclude_history: bool,
                         item_filter) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """the reference's _popularity_recommendations for the slots `slots` of hist: the first k entries of the
        popularity order that pass item_filter and (exclude_history) are not in the slot's history -> (ids i64, scores
        f64 = 1 - rank / (k + 1), retrieval scores f32 = 0) [len(slots), width], -1 / -inf / -inf where the list runs out"""
        dev = L.device()
        pop = self.popularity_order()
        if item_filter is None:         # nothing but a slot's own items can be skipped: a prefix of the order is enough
            pop = pop[:width + (int(hist.counts[slots].max()) if exclude_history and slots.shape[0] else 0)]
        nf, npop = int(slots.shape[0]), int(pop.shape[0])
        ok = torch.ones((nf, npop), dtype=torch.bool, device=dev)
        if item_filter is not None:
            if self.index._tags is None:
                raise ValueError("item_filter needs item tags: call set_item_tags() first")
            from .faiss_index import item_filter_words
            if isinstance(item_filter, torch.Tensor):
                item_filter = item_filter.detach().cpu().numpy()
            words = torch.from_numpy(item_filter_words(item_filter, hist.n)[slots].astype(np.int64)).to(dev)
            _, row_of, _ = self.index.item_vectors_device()
            row = torch.full_like(pop, -1)
            inside = pop < row_of.shape[0]
            row[inside] = row_of[pop[inside]].to(torch.int64)
            tag = torch.where(row >= 0, self.index._tags[row.clamp(min=0)].to(torch.int64) & 0xFFFFFFFF,
                              torch.zeros_like(pop))[None, :]          # an id that is not stored carries no tag
            any_of, all_of, none_of = words[:, 0:1], words[:, 1:2], words[:, 2:3]
            ok &= ((any_of == 0) | ((tag & any_of) != 0)) & ((tag & all_of) == all_of) & ((tag & none_of) == 0)
        if exclude_history and npop:
            off, items, _ = hist.host
            cnt = hist.counts[slots]
            local = np.repeat(np.arange(nf, dtype=np.int64), cnt)
            pos = np.concatenate([np.arange(off[s], off[s + 1]) for s in slots]) if nf else np.zeros(0, np.int64)
            keys = torch.from_numpy((local << 32) | items[pos.astype(np.int64)].astype(np.int64)).to(dev)
            grid = (torch.arange(nf, device=dev, dtype=torch.int64)[:, None] << 32) | pop[None, :]
            ok &= ~torch.isin(grid, keys)
        ids = torch.full((nf, width), -1, dtype=torch.int64, device=dev)
        rank = torch.cumsum(ok, dim=1) - 1                 # the 0-based position of every allowed entry in its list
        r, c = torch.nonzero(ok & (rank < width), as_tuple=True)
        ids[r, rank[r, c]] = pop[c]
        # (on the host: a true f64 division, where a device tensor / scalar multiplies by the reciprocal)
        score = torch.from_numpy(1.0 - np.arange(1, width + 1, dtype=np.float64) / np.float64(k + 1)).to(dev)
        filled = ids >= 0
        sc = torch.where(filled, score[None, :], torch.full((), -math.inf, dtype=torch.float64, device=dev))
        rs = torch.where(filled, torch.zeros((), dtype=torch.float32, device=dev),
                         torch.full((), -math.inf, dtype=torch.float32, device=dev))
        return ids, sc, rs

    @torch.no_grad()
    def recommend_cold_batch(self, histories: UserHistories, k: Optional[int] = None, exclude_history: bool = True,
                             item_filter=None, diversity=_DEFAULT, user_meta=None, labels=None, beta: float = 1.0,
                             weighting: str = "uniform", min_rating: int = 4
                             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """Serve users who have no trained row, from their rating histories (coldstart.UserHistories; slot s of the
        batch is history s) -> (item ids i64, ranker scores f64, retrieval scores f32 [nq, k], fallback bool [nq]) on
        the device.

        Each history is folded in (coldstart.fold_in_users_device over the index's own vectors,
        FAISSIndex.item_vectors_device: the definition is at rihip_fold_in_users) into a query vector and a transient
        user-table row, and the serve chain runs on those: search, seen-item exclusion, features, ranker, top-k or MMR.
        Not the reference's behaviour, and its retrieval quality is not pinned.
        exclude_history: a slot is never recommended an item of its own history (the history doubles as its exclusion
        list: one over-fetched search at the longest history, ValueError beyond the search limit as in recommend_batch).
        item_filter, diversity: as in recommend_batch.  user_meta f64 [nq, 4]: recency, gender, age, occupation of the
        slots (None = the serving defaults).  labels: the user ids the feature log records for the slots (default -1).
        beta, weighting, min_rating: the fold-in's parameters.

        fallback[s] = True: the slot has no usable history (no stored item rated >= min_rating, or a vanishing
        direction) and was served the reference's _popularity_recommendations instead: the first k entries of
        popularity_order() that pass item_filter and (exclude_history) are not in its history, score 1 - rank / (k + 1),
        retrieval score 0, -1 padded; no diversity stage, nothing logged.  The chain runs eager with the search's
        synchronous exactness check, like the item_filter branch of recommend_batch: there is no graph= option."""
        self._no_sq8("recommend_cold_batch (cold start)", True)
        if not isinstance(histories, UserHistories):
            raise ValueError("recommend_cold_batch: histories must be a coldstart.UserHistories")
        k = k or self.top_k_results
        div = self._diversity_stage(diversity, k)
        dev = L.device()
        nq = histories.n
        ntotal = self.index.index.ntotal
        kc = min(self.top_k_candidates, ntotal)
        width = min(k, kc)
        if labels is not None:
            labels = torch.as_tensor(labels, dtype=torch.int64).reshape(-1)
            if labels.shape[0] != nq:
                raise ValueError(f"{labels.shape[0]} labels for {nq} histories")
        V, row_of, mu = self.index.item_vectors_device()
        q, rows, flags = fold_in_users_device(histories, V, row_of, mu, min_rating, weighting, beta,
                                              self.store.device_tables()[1], user_meta)
        fallback = flags != 0
        ids = torch.full((nq, width), -1, dtype=torch.int64, device=dev)
        sc = torch.full((nq, width), -math.inf, dtype=torch.float64, device=dev)
        rs = torch.full((nq, width), -math.inf, dtype=torch.float32, device=dev)
        if nq == 0:
            return ids, sc, rs, fallback
        fb_host = fallback.cpu().numpy()
        warm, cold = np.nonzero(~fb_host)[0], np.nonzero(fb_host)[0]
        if warm.shape[0]:
            whole = warm.shape[0] == nq
            most = int(histories.counts[warm].max()) if exclude_history else 0
            scan = self.exclusion == "scan" and most > 0
            k_eff = overfetch_k(kc, most, ntotal, int(L.lib().rihip_ip_index_max_k())) if most and not scan else None
            uid = torch.arange(nq, dtype=torch.int64, device=dev) if whole else torch.from_numpy(warm).to(dev)
            log_uid = torch.full((warm.shape[0],), -1, dtype=torch.int64, device=dev) if labels is None \
                else labels[torch.from_numpy(warm)].to(dev)
            from .faiss_index import _sub_filter
            out = self._chain(uid, k, k_eff=k_eff, div=div, q=q if whole else q[uid].contiguous(), user_tab=rows,
                              item_filter=item_filter if item_filter is None or whole else _sub_filter(item_filter, uid),
                              seen=histories.as_seen(), log_uid=log_uid, scan_seen=histories.as_seen() if scan else None)
            if whole:
                ids, sc, rs = out
            else:
                for dst, src in zip((ids, sc, rs), out):
                    dst.index_copy_(0, uid, src)
        if cold.shape[0]:
            sel = torch.from_numpy(cold).to(dev)
            for dst, src in zip((ids, sc, rs), self._popularity_rows(histories, cold, k, width, exclude_history,
                                                                     item_filter)):
                dst.index_copy_(0, sel, src)
        return ids, sc, rs, fallback

    # ---- serving feature log -------------------------------------------------------------------------------------
    def reset_feature_log(self, rows: Optional[int] = None) -> None:
        """clear the log; rows (optional) resizes the ring (0 turns logging off).  A resize re-captures graphs."""
        R = (0 if self._log is None else self._log[0].shape[0]) if rows is None else int(rows)
        if R < 0:
            raise ValueError(f"feature_log_rows={R} < 0")
        if R == 0:
            self._log = None
            return
        nf = len(self.ranker.feature_names)
        if self._log is None or self._log[0].shape != (R, nf):
            dev = L.device()
            self._log = (torch.zeros((R, nf), dtype=torch.float32, device=dev),
                         torch.empty((R,), dtype=torch.int64, device=dev),
                         torch.empty((R,), dtype=torch.int64, device=dev),
                         torch.empty((2,), dtype=torch.int64, device=dev))
        ring, ru, ri, cur = self._log
        ru.fill_(-1)
        ri.fill_(-1)                  # never-written slots read as padding: the detector skips them
        cur.zero_()

    @property
    def feature_log_rows(self) -> int:
        return 0 if self._log is None else int(self._log[0].shape[0])

    def _append_log(self, X: torch.Tensor, uid: torch.Tensor, cand: torch.Tensor) -> None:
        ring, ru, ri, cur = self._log
        n, nf = X.shape
        if nf != ring.shape[1]:
            raise RuntimeError(f"feature log holds {ring.shape[1]} features, the ranker builds {nf}: reset_feature_log()")
        L.check(L.lib().rihip_feature_log_append(X.data_ptr(), n, nf, uid.data_ptr(), cand.data_ptr(), cand.shape[1],
                                                 ring.data_ptr(), ru.data_ptr(), ri.data_ptr(), ring.shape[0],
                                                 cur.data_ptr(), L.stream_ptr()), "feature_log_append")

    def _log_order(self) -> torch.Tensor:
        """ring slots oldest -> newest (one synchronisation: the cursor)"""
        R = self._log[0].shape[0]
        c = int(self._log[3][0].item())
        dev = self._log[0].device
        if c <= R:
            return torch.arange(c, device=dev)
        return (torch.arange(R, device=dev) + c) % R

    def serving_features(self):
        """DataFrame [user_id, item_id, *ranker.feature_names] of the logged rows, oldest to newest, padded candidates
        dropped: the serving side of metrics.detect_training_serving_skew"""
        import pandas as pd
        if self._log is None:
            raise RuntimeError("the feature log is off (feature_log_rows=0)")
        ring, ru, ri, _ = self._log
        o = self._log_order()
        keep = o[ri[o] >= 0]
        X = ring[keep].cpu().numpy()
        cols = {"user_id": ru[keep].cpu().numpy(), "item_id": ri[keep].cpu().numpy()}
        for j, name in enumerate(self.ranker.feature_names):
            cols[name] = X[:, j]
        return pd.DataFrame(cols)

    def detect_skew(self, train_features, threshold: float = 0.1, numeric_cols: Optional[List[str]] = None,
                    columns: Optional[Sequence[str]] = None) -> Dict[str, Any]:
        """skew_device.detect_training_serving_skew_device of train_features against the logged rows, read in place on
        the device (the ring is not copied to the host); the same result as the host detector on serving_features()"""
        from . import skew_device as S
        if self._log is None:
            raise RuntimeError("the feature log is off (feature_log_rows=0)")
        ring, ru, ri, _ = self._log
        ids = torch.stack([ru, ri], dim=1).to(torch.float64)
        serving = [S._Segment(ring, list(self.ranker.feature_names), ri), S._Segment(ids, ["user_id", "item_id"], ri)]
        return S.detect_training_serving_skew_device(train_features, serving, threshold, numeric_cols, columns)

    # ---- explanation (not in the reference) ----------------------------------------------------------------------
    @torch.no_grad()
    def explain_batch(self, user_ids, item_ids, top: Optional[int] = None):
        """Why these items: the TreeSHAP contribution of every ranking feature to the ranker score of each (user, item)
        pair (LightGBMRanker.predict_contrib_device; definition at rihip_gbdt_predict_contrib in recommendit_hip.h).

        item_ids: [nq, k] item ids per user, typically what recommend_batch just returned; only these pairs' features
        are built (k rows per user, not top_k_candidates).  Returns contributions f64 [nq, k, F + 1] on the device, F =
        len(ranker.feature_names), the expected value last: a pair's row sums to its ranker score.  Rows of padding
        (item id -1) are zero.  With top=n also (indices i64 [nq, k, n], values f64 [nq, k, n]) of the n features of
        largest |contribution| per pair, largest first.  A separate call after the serve chain: nothing is captured."""
        uid = self._ids_to_device(user_ids)
        items = torch.as_tensor(item_ids, dtype=torch.int64).to(uid.device)
        if items.dim() != 2 or items.shape[0] != uid.shape[0]:
            raise ValueError(f"explain_batch: item_ids must be [nq, k] with nq = {uid.shape[0]} users, got {tuple(items.shape)}")
        nq, k = items.shape
        nf = len(self.ranker.feature_names)
        if top is not None and not 1 <= int(top) <= nf:
            raise ValueError(f"explain_batch: top={top} outside 1..{nf}")
        if nq == 0 or k == 0:
            phi = torch.zeros((nq, k, nf + 1), dtype=torch.float64, device=uid.device)
        else:
            X = build_ranking_features_device(self.store, uid, items.contiguous(), self.ranker.feature_names)
            phi = self.ranker.predict_contrib_device(X).view(nq, k, nf + 1)
            phi = torch.where((items >= 0).unsqueeze(-1), phi, torch.zeros((), dtype=phi.dtype, device=phi.device))
        if top is None:
            return phi
        idx = torch.topk(phi[..., :nf].abs(), int(top), dim=-1).indices
        return phi, idx, torch.gather(phi[..., :nf], -1, idx)

    def get_recommendations(self, user_id: int, k: Optional[int] = None, graph: bool = False,
                            exclude_seen: Optional[bool] = None, item_filter=None, diversity=_DEFAULT,
                            explain: Optional[int] = None, history=None) -> List[Dict[str, Any]]:
        """item_filter, diversity: as in recommend_batch (graph=True with a filter raises ValueError); with a diversity
        the list is in selection order and "rank" is the position in it.  explain=n adds "contributions" to every
        result: {feature name: contribution} of the n features that moved its score most (explain_batch).

        history=[(item id, rating), ...] (not in the reference): serve this rating history instead of user_id's trained
        row (recommend_cold_batch of the one history; user_id is only what the feature log records; exclude_seen=False
        keeps the history's own items in; graph and explain are not offered).  Every result then carries "cold": True,
        and "fallback": True when the history was unusable and the popularity list was served."""
        if history is not None:
            if graph or explain:
                raise ValueError("get_recommendations(history=...) runs the eager cold-start chain: no graph=, no explain=")
            ids, sc, rs, fb = self.recommend_cold_batch(UserHistories.from_lists([list(history)]), k,
                                                        exclude_history=exclude_seen is not False,
                                                        item_filter=item_filter, diversity=diversity, labels=[user_id])
            fell = bool(fb[0].item())
            return [{"item_id": int(i), "score": float(s), "rank": rank, "retrieval_score": float(r), "cold": True,
                     "fallback": fell}
                    for rank, (i, s, r) in enumerate(zip(ids[0].tolist(), sc[0].tolist(), rs[0].tolist()), start=1) if i >= 0]
        ids, sc, rs = self.recommend_batch([user_id], k, graph=graph, exclude_seen=exclude_seen, item_filter=item_filter,
                                           diversity=diversity)
        why = None
        if explain:
            _, fi, fv = self.explain_batch([user_id], ids, top=int(explain))
            names = list(self.ranker.feature_names)
            why = [{names[j]: float(v) for j, v in zip(jr, vr)} for jr, vr in zip(fi[0].tolist(), fv[0].tolist())]
        out = []
        for rank, (i, s, r) in enumerate(zip(ids[0].tolist(), sc[0].tolist(), rs[0].tolist()), start=1):
            if i >= 0:
                out.append({"item_id": int(i), "score": float(s), "rank": rank, "retrieval_score": float(r)})
                if why is not None:
                    out[-1]["contributions"] = why[rank - 1]
        return out
