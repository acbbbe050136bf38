"""GPU: cold-start users (csrc/coldstart.hip, recommendit_amd/coldstart.py, GpuRecommendationPipeline.recommend_cold_batch)
against the NumPy restatement of the definition (tests/coldstart_reference.py): the fold-in kernel (flags and feature
rows bit for bit, q within 2^-22), cancellation, the feature row against rihip_ltr_stats + rihip_ltr_finalize, retrieval
on a clustered corpus, the serve chain against its stages run by hand, the popularity fallback, the live catalogue and
the single-request entry."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coldstart_reference as R  # noqa: E402
from oracle import fixtures as fx  # noqa: E402
from oracle import gbdt_np as G  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025]
Q_TOL = 2.0 ** -22      # derived (see test_kernel_matches_reference), not measured


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _host(out):
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


# ---- 1. the kernel against the reference --------------------------------------------------------------------------------
N_IDS, N_ROWS, N_ITEM_ROWS = 3000, 2500, 2000


def _kernel_case(d, ldv, seed):
    """histories of the LENGTHS: ids up to N_IDS + 200 (some >= n_ids), item 0, ids whose row_of is -1 or outside the
    table, items beyond the item table; slot 3 (63 entries) rates nothing above 2"""
    from recommendit_amd.coldstart import UserHistories
    rng = np.random.default_rng(seed)
    Vfull = np.full((N_ROWS, ldv), 7.0, np.float32)                 # columns >= d are never read
    X = rng.standard_normal((N_ROWS, d))
    Vfull[:, :d] = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    row_of = np.full(N_IDS, -1, np.int32)
    stored = rng.permutation(N_IDS)[:N_ROWS]
    row_of[stored] = rng.permutation(N_ROWS).astype(np.int32)
    row_of[rng.permutation(N_IDS)[:40]] = N_ROWS + 5                # a row outside the table reads as not stored
    slots, items, ratings = [], [], []
    for s, n in enumerate(LENGTHS):
        it = np.sort(rng.choice(N_IDS + 200, n, replace=False))
        if n >= 63:
            it[0] = 0
        r = rng.integers(1, 6, n)
        if s == 3:
            r = rng.integers(1, 3, n)
        slots += [s] * n; items += it.tolist(); ratings += r.tolist()
    hist = UserHistories.from_pairs(slots, items, ratings, n=len(LENGTHS))
    item_tab = np.zeros((N_ITEM_ROWS, 23))
    item_tab[:, :5] = rng.random((N_ITEM_ROWS, 5))
    item_tab[:, 5:] = rng.random((N_ITEM_ROWS, 18)) < 0.2
    meta = rng.random((len(LENGTHS), 4))
    return hist, Vfull, row_of, item_tab, meta


def _launch(hist, Vd, row_of_d, mu_d, min_rating, weighting, beta, item_tab_d, meta_d):
    from recommendit_amd.coldstart import fold_in_users_launch
    q, rows, flags, err = _host(fold_in_users_launch(hist, Vd, row_of_d, mu_d, min_rating,
                                                     ("uniform", "rating")[weighting], beta, item_tab_d, meta_d))
    return q, rows, flags, int(err[0])


@pytest.mark.parametrize("d,ldv", [(24, 24), (64, 72), (128, 128), (3, 3), (24, 25), (30, 32), (200, 200), (256, 256)])
def test_kernel_matches_reference(d, ldv):
    """flags and feature rows bit for bit; |q - q_ref| <= 2^-22 per component: the f64 accumulation error is far below
    half an f32 ulp, the one final rounding of a component of magnitude <= 1 costs <= 2^-24, and doubling covers a
    double-rounding tie (the reference checks n >= 1e-3 for every unflagged slot, so the bound holds).  d 24 / 64 / 128
    take the 16-byte gather at 8 / 16 / 32 lanes a row, 200 and 256 at 64; (24, 25), 30 and 3 the one-float gather."""
    hist, Vfull, row_of, item_tab, meta = _kernel_case(d, ldv, seed=d + ldv)
    Vd = _dev(Vfull)[:, :d]
    assert Vd.stride(0) == ldv
    mu = Vfull[:, :d].astype(np.float64).mean(0)
    row_of_d, mu_d, tab_d, meta_d = _dev(row_of), _dev(mu), _dev(item_tab), _dev(meta)
    off, items, ratings = hist.host
    full = d in (24, 64, 128)
    rows_ref = {True: R.feature_rows_reference(off, items, ratings, item_tab, meta),
                False: R.feature_rows_reference(off, items, ratings, item_tab, None)}
    combos = [(mr, w, b) for mr in (3, 4) for w in (0, 1) for b in (0.0, 1.0)] if full else [(4, 1, 1.0), (3, 0, 0.0)]
    worst = 0.0
    for i, (mr, w, beta) in enumerate(combos):
        with_meta = i % 2 == 0
        q, rows, flags, err = _launch(hist, Vd, row_of_d, mu_d, mr, w, beta, tab_d, meta_d if with_meta else None)
        q_ref, flags_ref, n_ref = R.fold_in_reference(off, items, ratings, Vfull, row_of, mu, mr, w, beta)
        assert err == 0
        assert (n_ref[flags_ref == 0] >= 1e-3).all()
        assert flags_ref[0] == 1 and flags_ref[3] == 1 and flags_ref[4:].sum() == 0          # empty, nothing liked
        assert np.array_equal(flags, flags_ref), (mr, w, beta)
        assert np.array_equal(_bits(rows), _bits(rows_ref[with_meta])), (mr, w, beta)
        diff = float(np.abs(q.astype(np.float64) - q_ref.astype(np.float64)).max())
        worst = max(worst, diff)
        assert diff <= Q_TOL, (mr, w, beta, diff)
        assert not q[flags_ref == 1].any() and np.isfinite(q).all()
        again = _launch(hist, Vd, row_of_d, mu_d, mr, w, beta, tab_d, meta_d if with_meta else None)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((q, rows, flags), again[:3]))
    print(f"d={d} ldv={ldv}: max |q - q_ref| = {worst:.3e} (bound {Q_TOL:.3e})")
    # no item table: the genre preference is zero, everything else as before
    q, rows, flags, err = _launch(hist, Vd, row_of_d, mu_d, 4, 0, 1.0, None, None)
    assert np.array_equal(_bits(rows), _bits(R.feature_rows_reference(off, items, ratings, None, None)))


def test_kernel_error_word_and_skipped_entries():
    """a rating 0, a rating 6 and an id -1: bits 1 and 0 of the error word, the entries skipped everywhere"""
    from recommendit_amd.coldstart import UserHistories, fold_in_users_device
    hist, Vfull, row_of, item_tab, meta = _kernel_case(64, 64, seed=5)
    Vd, row_of_d, tab_d = _dev(Vfull), _dev(row_of), _dev(item_tab)
    mu = Vfull.astype(np.float64).mean(0)
    off, items, ratings = (a.copy() for a in hist.host)
    liked = [j for j in range(off[8], off[9]) if ratings[j] >= 4 and items[j] < N_IDS and 0 <= row_of[items[j]] < N_ROWS]
    cases = {"rating": ([(liked[0], None, 0), (liked[1], None, 6)], 2), "id": ([(off[8], -1, 5)], 1),
             "both": ([(liked[0], None, 0), (liked[1], None, 6), (off[8], -1, 5), (off[5], -1, 9)], 3)}
    for name, (edits, word) in cases.items():
        it2, r2 = items.copy(), ratings.copy()
        for j, new_item, new_rating in edits:
            if new_item is not None:
                it2[j] = new_item                       # the first entry of its row: the row stays ascending
            r2[j] = new_rating
        bad = UserHistories(off, it2, r2)
        q, rows, flags, err = _launch(bad, Vd, row_of_d, _dev(mu), 4, 1, 1.0, tab_d, None)
        assert err == word == R.error_word(it2, r2), name
        q_ref, flags_ref, _ = R.fold_in_reference(off, it2, r2, Vfull, row_of, mu, 4, 1, 1.0)
        assert np.array_equal(flags, flags_ref)
        assert np.array_equal(_bits(rows), _bits(R.feature_rows_reference(off, it2, r2, item_tab, None))), name
        assert np.abs(q.astype(np.float64) - q_ref).max() <= Q_TOL
        clean_q = _launch(hist, Vd, row_of_d, _dev(mu), 4, 1, 1.0, tab_d, None)[0]
        assert name == "id" or not np.array_equal(q[8], clean_q[8])                      # the entries did leave the sum
        with pytest.raises(ValueError, match="rating outside|item id < 0"):
            fold_in_users_device(bad, Vd, row_of_d, _dev(mu), 4, "rating", 1.0, tab_d)


def test_kernel_arguments():
    """nq = 0 is a no-op; anything out of range is RIHIP_ERR_ARG and launches nothing"""
    from recommendit_amd import _lib as L
    from recommendit_amd.coldstart import UserHistories, fold_in_users_launch
    lib = L.lib()
    V, row_of, mu = _dev(np.eye(4, dtype=np.float32)), _dev(np.arange(4, dtype=np.int32)), _dev(np.zeros(4))
    q, rows, flags, err = fold_in_users_launch(UserHistories.from_lists([]), V, row_of, mu)
    assert q.shape == (0, 4) and rows.shape == (0, 24) and flags.shape == (0,) and int(err.item()) == 0
    hist = UserHistories.from_lists([[(1, 5)]])
    off, items, ratings = hist.device_tensors()
    out_q = torch.full((1, 4), 7.0, dtype=torch.float32, device="cuda")
    out_rows = torch.full((1, 24), 7.0, dtype=torch.float64, device="cuda")
    out_flags = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    tab = torch.zeros((3, 23), dtype=torch.float64, device="cuda")

    def call(**kw):
        a = dict(off=off.data_ptr(), items=items.data_ptr(), ratings=ratings.data_ptr(), nq=1, n_entries=1, V=V.data_ptr(),
                 n_rows=4, ldv=4, d=4, row_of=row_of.data_ptr(), n_ids=4, mu=mu.data_ptr(), min_rating=4, weighting=0,
                 beta=1.0, tab=tab.data_ptr(), n_item_rows=3, meta=None, q=out_q.data_ptr(), rows=out_rows.data_ptr(),
                 flags=out_flags.data_ptr(), err=err.data_ptr())
        a.update(kw)
        return lib.rihip_fold_in_users(a["off"], a["items"], a["ratings"], a["nq"], a["n_entries"], a["V"], a["n_rows"],
                                       a["ldv"], a["d"], a["row_of"], a["n_ids"], a["mu"], a["min_rating"], a["weighting"],
                                       a["beta"], a["tab"], a["n_item_rows"], a["meta"], a["q"], a["rows"], a["flags"],
                                       a["err"], L.stream_ptr())
    bad = [dict(d=0), dict(d=257), dict(ldv=3), dict(nq=-1), dict(n_entries=-1), dict(n_rows=-1), dict(n_ids=-1),
           dict(n_item_rows=-1), dict(min_rating=0), dict(min_rating=6), dict(weighting=2), dict(weighting=-1),
           dict(beta=-0.1), dict(beta=1.5), dict(beta=float("nan")), dict(err=None), dict(off=None), dict(items=None),
           dict(ratings=None), dict(V=None), dict(row_of=None), dict(mu=None), dict(tab=None), dict(q=None),
           dict(rows=None), dict(flags=None)]
    for kw in bad:
        assert call(**kw) == 1, kw                                  # RIHIP_ERR_ARG
        assert b"fold_in_users" in lib.rihip_last_error(), kw
    torch.cuda.synchronize()
    assert (out_q == 7).all() and (out_rows == 7).all() and (out_flags == 7).all()       # nothing was launched
    assert call() == 0 and call(tab=None, n_item_rows=0) == 0
    torch.cuda.synchronize()
    assert out_flags.item() == 0 and out_q.cpu().numpy().tolist() == [[0.0, 1.0, 0.0, 0.0]]
    for bad_kw in (dict(weighting="popular"), dict(min_rating=0), dict(beta=2.0)):
        with pytest.raises(ValueError):
            fold_in_users_launch(hist, V, row_of, mu, **bad_kw)


# ---- 2. cancellation ----------------------------------------------------------------------------------------------------
def test_cancelling_history_is_flagged():
    from recommendit_amd.coldstart import UserHistories, fold_in_users_device
    V = np.zeros((2, 8), np.float32)
    V[0, 0], V[1, 0] = 1.0, -1.0
    hist = UserHistories.from_lists([[(0, 5), (1, 5)], [(0, 5)]])
    q, rows, flags = _host(fold_in_users_device(hist, _dev(V), _dev(np.array([0, 1], np.int32)), _dev(np.zeros(8)),
                                                beta=0.0))
    assert flags.tolist() == [1, 0] and not q[0].any() and np.isfinite(q).all() and np.isfinite(rows).all()
    assert q[1].tolist() == [1.0] + [0.0] * 7 and rows[0, 0] == 5.0
    # the same in one dimension (d = 1)
    q, _, flags = _host(fold_in_users_device(UserHistories.from_lists([[(0, 5), (1, 5)], [(1, 4)]]), _dev(V[:, :1].copy()),
                                             _dev(np.array([0, 1], np.int32)), _dev(np.zeros(1)), beta=0.0))
    assert flags.tolist() == [1, 0] and q.tolist() == [[0.0], [-1.0]]


# ---- 3. the feature row against the training-set builder -------------------------------------------------------------------
def test_feature_row_equals_the_ltr_tables():
    """columns 0, 1 and 6..23 of the slot's row are those rihip_ltr_stats + rihip_ltr_finalize give the same user (every
    rated item of this set is in the catalogue, where the two definitions of the liked count coincide)"""
    import pandas as pd
    from recommendit_amd import synthetic
    from recommendit_amd.coldstart import UserHistories, fold_in_users_device
    from recommendit_amd.feature_engineering import FeatureEngineer
    n_users = 60
    r, m, _ = synthetic.ml1m_like(n_users=n_users, n_item_ids=400, n_catalog=380, n_ratings=3000, seed=3)
    users = pd.DataFrame({"user_id": np.arange(1, n_users + 1), "gender": np.where(np.arange(n_users) % 2, "F", "M"),
                          "age": np.array([1, 18, 25, 35, 45, 50, 56])[np.arange(n_users) % 7],
                          "occupation": np.arange(n_users) % 21, "zip_code": "12345"})
    fe = FeatureEngineer("unused")
    fe.set_data(r, users, m)
    ut, it = fe.build_tables_device()
    sub = r[r["user_id"] <= 50]
    hist = UserHistories.from_pairs(sub["user_id"].to_numpy() - 1, sub["item_id"].to_numpy(), sub["rating"].to_numpy(), n=50)
    assert hist.counts.min() >= 20
    _, rows, _ = fold_in_users_device(hist, _dev(np.ones((1, 4), np.float32)), _dev(np.zeros(1, np.int32)),
                                      _dev(np.zeros(4)), item_table=it)
    rows, ut = rows.cpu().numpy(), ut.cpu().numpy()
    cols = [0, 1] + list(range(6, 24))
    assert np.array_equal(_bits(rows[:, cols]), _bits(ut[1:51][:, cols]))
    assert (np.abs(rows[:, 6:]).sum(1) > 0).all()
    assert np.array_equal(_bits(rows), _bits(R.feature_rows_reference(*hist.host, it.cpu().numpy())))


# ---- 4. behaviour: a clustered corpus -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clusters():
    return R.cluster_case()


@pytest.mark.parametrize("kind", ["exact", "ivf"])
def test_folded_in_query_retrieves_its_own_cluster(clusters, kind):
    from recommendit_amd import FAISSIndex
    from recommendit_amd.coldstart import UserHistories, fold_in_users_device
    X, item_ids, cluster, hists = clusters
    index = FAISSIndex(embed_dim=R.D_CLUSTER, exact=True) if kind == "exact" else FAISSIndex(R.D_CLUSTER, 8, 2)
    index.build_ivf_index(X, item_ids.tolist())
    hist = UserHistories.from_lists(hists)
    V, row_of, mu = index.item_vectors_device()
    assert index.item_vectors_device()[0] is V                                           # cached
    assert np.array_equal(V.cpu().numpy(), index.reconstruct()) and row_of[0].item() == -1
    assert np.array_equal(row_of.cpu().numpy()[1:], np.arange(len(item_ids)))
    assert np.array_equal(mu.cpu().numpy(), V.double().mean(0).cpu().numpy())
    for beta in (0.0, 1.0):
        q, _, flags = fold_in_users_device(hist, V, row_of, mu, beta=beta)
        assert not flags.any()
        _, ids = index.batch_search_device(q, k=50, normalized=True, exclude=hist.as_seen(), user_ids=list(range(hist.n)))
        ids = ids.cpu().numpy()
        for s in range(hist.n):
            assert (ids[s] >= 1).all() and (cluster[ids[s] - 1] == s).all(), (kind, beta, s)
            assert not np.isin(ids[s], hist.history_of(s)[0]).any()


# ---- 5. the pipeline -------------------------------------------------------------------------------------------------------
NU, NI, D, KC = 50, 3000, 64, 200


@pytest.fixture(scope="module")
def parts(tmp_path_factory):
    """model, exact index with genre tags, ranker and feature store of a small catalogue"""
    from recommendit_amd import FAISSIndex, LightGBMRanker, TwoTowerModel
    from recommendit_amd.recommender import GpuFeatureStore, feature_columns
    sd = fx.make_state(NU, NI, D, 128, seed=21)
    model = TwoTowerModel(NU, NI, D, 128)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    rng = np.random.RandomState(2)
    item_ids = list(range(1, NI + 1))
    genres = (rng.rand(NI, 18) < 0.15).astype(np.float32)
    E = model.get_item_embeddings(item_ids, genres)
    index = FAISSIndex(embed_dim=D, exact=True)
    index.build_ivf_index(E, item_ids)
    forest = G.random_forest_model(60, 31, 50, seed=5, names=feature_columns())
    p = tmp_path_factory.mktemp("cold") / "r.lgbm"
    p.write_text(G.write_text_model(forest))
    ranker = LightGBMRanker.load(str(p))
    store = GpuFeatureStore(NU, NI)
    ut = store.user.copy(); it = store.item.copy()
    ut[1:, :6] = rng.rand(NU, 6) * [5, 8, 1, 1, 1, 1]; ut[1:, 6:] = rng.rand(NU, 18)
    it[1:, :5] = rng.rand(NI, 5) * [5, 9, 1, 1.5, 1]; it[1:, 5:] = genres
    it[1:, 1] = np.round(it[1:, 1], 1)                          # ties in log_rating_count: the lower id goes first
    store.load_arrays(ut, it)
    index.set_item_tags(store.item_genre_tags(item_ids))
    return dict(model=model, index=index, ranker=ranker, store=store, item=it, item_ids=item_ids)


def _pipe(parts, **kw):
    from recommendit_amd.recommender import GpuRecommendationPipeline
    return GpuRecommendationPipeline(parts["model"], parts["index"], parts["ranker"], parts["store"], top_k_candidates=KC,
                                     top_k_results=20, **kw)


def _histories(seed, lengths):
    """histories over item ids 1..NI; a length < 0 gives a history of -length items none of which is rated above 3"""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        items = rng.choice(np.arange(1, NI + 1), abs(n), replace=False)
        ratings = rng.integers(1, 4, abs(n)) if n < 0 else rng.integers(1, 6, n)
        if n > 0:
            ratings[0] = 5
        out.append([(int(i), int(r)) for i, r in zip(items, ratings)])
    return out


def _by_hand(parts, hist, k, exclude=True, item_filter=None, div=None, slots=None, **fold):
    """the stages of the cold chain, run one by one from the kernel's own q and rows"""
    from recommendit_amd import _lib as L
    from recommendit_amd import rerank as RR
    from recommendit_amd.coldstart import fold_in_users_device
    from recommendit_amd.recommender import feature_columns
    from recommendit_amd.seen import overfetch_k
    index, store, ranker = parts["index"], parts["store"], parts["ranker"]
    lib = L.lib()
    V, row_of, mu = index.item_vectors_device()
    ut, it = store.device_tables()
    q, rows, flags = fold_in_users_device(hist, V, row_of, mu, item_table=it, **fold)
    slots = np.arange(hist.n) if slots is None else np.asarray(slots)
    uid = _dev(slots.astype(np.int64))
    q = q[uid].contiguous()
    nq = len(slots)
    most = int(hist.counts[slots].max()) if exclude else 0
    kw = {} if item_filter is None else dict(item_filter=item_filter)
    if most:
        k_eff = overfetch_k(KC, most, NI, int(lib.rihip_ip_index_max_k()))
        s0, c0 = index.batch_search_device(q, k=k_eff, normalized=True, **kw)
        rs = torch.empty((nq, KC), dtype=torch.float32, device="cuda")
        cand = torch.empty((nq, KC), dtype=torch.int64, device="cuda")
        index.filter_excluded(s0, c0, KC, hist.as_seen(), uid, rs, cand)
    else:
        rs, cand = index.batch_search_device(q, k=KC, normalized=True, **kw)
    names = ranker.feature_names
    canon = {n: i for i, n in enumerate(feature_columns())}
    col_map = torch.tensor([canon.get(n, -1) for n in names], dtype=torch.int32, device="cuda")
    X = torch.empty((nq * KC, len(names)), dtype=torch.float32, device="cuda")
    L.check(lib.rihip_rank_features_build(rows.data_ptr(), rows.shape[0], it.data_ptr(), it.shape[0], uid.data_ptr(),
                                          cand.data_ptr(), nq, KC, col_map.data_ptr(), len(names), X.data_ptr(),
                                          L.stream_ptr()), "rank_features_build")
    scores = ranker.predict_device(X)
    if div is not None:
        out = RR.launch(scores, cand, rs, k, div, it, 5, 18)
    else:
        out = tuple(torch.empty((nq, k), dtype=t, device="cuda") for t in (torch.int64, torch.float64, torch.float32))
        L.check(lib.rihip_rank_topk(scores.data_ptr(), cand.data_ptr(), rs.data_ptr(), nq, KC, k, out[0].data_ptr(),
                                    out[1].data_ptr(), out[2].data_ptr(), L.stream_ptr()), "rank_topk")
    return _host(out), flags.cpu().numpy(), (X, uid, cand)


def _same(got, exp, what=""):
    assert np.array_equal(got[0], exp[0]), (what, np.argwhere(got[0] != exp[0])[:5])
    assert np.array_equal(_bits(got[1]), _bits(exp[1])), what
    assert np.array_equal(_bits(got[2]), _bits(exp[2])), what


WARM_LENGTHS = [1, 3, 20, 64, 150, 7, 33, 300]


def test_pipeline_equals_its_stages(parts):
    from recommendit_amd.coldstart import UserHistories
    pipe = _pipe(parts)
    hist = UserHistories.from_lists(_histories(1, WARM_LENGTHS))
    exp, flags, _ = _by_hand(parts, hist, 20)
    assert not flags.any()
    got = _host(pipe.recommend_cold_batch(hist, k=20))
    _same(got[:3], exp, "default")
    assert got[3].dtype == np.bool_ and not got[3].any() and (got[0] >= 1).all()
    for s in range(hist.n):
        assert not np.isin(got[0][s], hist.history_of(s)[0]).any()
    # the history left in: no over-fetch
    exp_in, _, _ = _by_hand(parts, hist, 20, exclude=False)
    _same(_host(pipe.recommend_cold_batch(hist, k=20, exclude_history=False))[:3], exp_in, "exclude_history=False")
    everything = _host(pipe.recommend_cold_batch(hist, k=KC, exclude_history=False))[0]
    assert hist.history_of(0)[0][0] in everything[0]                  # slot 0's one liked item is retrieved for it
    # an item filter: genre 0 or 3, not genre 5
    flt = (0b1001, 0, 0b100000)
    _same(_host(pipe.recommend_cold_batch(hist, k=20, item_filter=flt))[:3], _by_hand(parts, hist, 20, item_filter=flt)[0],
          "item_filter")
    g = parts["item"][_host(pipe.recommend_cold_batch(hist, k=20, item_filter=flt))[0], 5:]
    assert ((g[..., 0] + g[..., 3]) > 0).all() and (g[..., 5] == 0).all()
    # the diversified last stage on the staged inputs
    exp_div, _, _ = _by_hand(parts, hist, 20, div=0.3)
    _same(_host(pipe.recommend_cold_batch(hist, k=20, diversity=0.3))[:3], exp_div, "diversity")
    assert not np.array_equal(exp_div[0], exp[0])
    # the fold-in's parameters reach the kernel
    for fold in (dict(beta=0.0), dict(weighting="rating"), dict(min_rating=3)):
        _same(_host(pipe.recommend_cold_batch(hist, k=20, **fold))[:3], _by_hand(parts, hist, 20, **fold)[0], str(fold))
    # a second call is bitwise the first; the warm path is untouched by the cold one
    _same(_host(pipe.recommend_cold_batch(hist, k=20))[:3], got[:3])
    warm = _host(_pipe(parts).recommend_batch(list(range(1, 9)), k=20))
    _same(_host(pipe.recommend_batch(list(range(1, 9)), k=20)), warm)
    with pytest.raises(ValueError):
        pipe.recommend_cold_batch(_histories(1, [3]), k=20)
    with pytest.raises(ValueError):
        pipe.recommend_cold_batch(hist, k=20, labels=[1, 2])
    empty = _host(pipe.recommend_cold_batch(UserHistories.from_lists([]), k=20))
    assert empty[0].shape == (0, 20) and empty[3].shape == (0,)


def test_pipeline_mixed_batch_and_fallback(parts):
    """flagged slots (no history, nothing liked, an unstored item only) get the popularity list; the others are what
    they are without them"""
    from recommendit_amd.coldstart import UserHistories
    pipe = _pipe(parts)
    lists = _histories(4, [12, 0, 40, -9, 5, 0, 90])
    lists.append([(NI + 50, 5)])                                                  # liked, but not in the index
    hist = UserHistories.from_lists(lists)
    warm, cold = [0, 2, 4, 6], [1, 3, 5, 7]
    tags = dict(zip(parts["item_ids"], parts["index"].item_tags().tolist()))
    pop = R.default_popularity(parts["item"], parts["item_ids"])
    assert pipe.popularity_order().cpu().numpy().tolist() == pop
    assert len(set(parts["item"][pop[:200], 1])) < 150                             # ties there: the order has to break them
    for kw, ref_kw in ((dict(), dict()), (dict(exclude_history=False), dict(exclude=False)),
                       (dict(item_filter=(0b11, 0, 0)), dict(item_filter=(0b11, 0, 0))), (dict(diversity=0.5), dict(div=0.5))):
        ids, sc, rs, fb = _host(pipe.recommend_cold_batch(hist, k=20, **kw))
        assert fb.tolist() == [s in cold for s in range(hist.n)], kw
        exp_warm, _, _ = _by_hand(parts, hist, 20, slots=warm, **ref_kw)
        _same((ids[warm], sc[warm], rs[warm]), exp_warm, str(kw))
        alone = _host(pipe.recommend_cold_batch(UserHistories.from_lists([lists[s] for s in warm]), k=20, **kw))
        _same((ids[warm], sc[warm], rs[warm]), alone[:3], str(kw))
        for s in cold:
            e = R.popularity_reference(pop, 20, 20, hist.history_of(s)[0] if kw.get("exclude_history", True) else None,
                                       tags, kw.get("item_filter"))
            _same((ids[s], sc[s], rs[s]), e, f"{kw} slot {s}")
    # slot 3 with its history excluded skips its own items
    pipe.set_popularity([lists[3][0][0], 5, 9, lists[3][1][0], 2])
    ids, sc, rs, fb = _host(pipe.recommend_cold_batch(hist, k=4))
    assert ids[3].tolist() == [5, 9, 2, -1] and ids[1].tolist() == [lists[3][0][0], 5, 9, lists[3][1][0]]
    assert sc[3].tolist() == [1 - 1 / 5, 1 - 2 / 5, 1 - 3 / 5, -math.inf] and rs[3].tolist() == [0, 0, 0, -math.inf]
    # a list shorter than k: -1 padded
    ids, sc, rs, fb = _host(pipe.recommend_cold_batch(hist, k=20))
    for s in cold:
        e = R.popularity_reference([lists[3][0][0], 5, 9, lists[3][1][0], 2], 20, 20, hist.history_of(s)[0])
        _same((ids[s], sc[s], rs[s]), e)
        assert (ids[s][5:] == -1).all()
    pipe.set_popularity(None)
    assert pipe.popularity_order().cpu().numpy().tolist() == pop
    with pytest.raises(ValueError):
        pipe.set_popularity([3, -1])
    # every slot flagged: the chain is not run at all
    ids, sc, rs, fb = _host(pipe.recommend_cold_batch(UserHistories.from_lists([[], []]), k=20))
    assert fb.all() and ids[0].tolist() == pop[:20] and ids[1].tolist() == pop[:20]


def test_pipeline_feature_log_records_the_labels(parts):
    from recommendit_amd.coldstart import UserHistories
    hist = UserHistories.from_lists(_histories(6, [10, 0, 25]))
    pipe = _pipe(parts, feature_log_rows=4 * KC)
    pipe.recommend_cold_batch(hist, k=20)
    df = pipe.serving_features()
    assert len(df) == 2 * KC and (df["user_id"] == -1).all()                       # the fallback slot logs nothing
    pipe.reset_feature_log()
    pipe.recommend_cold_batch(hist, k=20, labels=[901, 902, 903])
    df = pipe.serving_features()
    assert df["user_id"].tolist() == [901] * KC + [903] * KC
    _, _, (X, uid, cand) = _by_hand(parts, hist, 20, slots=[0, 2])
    assert np.array_equal(df[list(parts["ranker"].feature_names)].to_numpy(dtype=np.float32), X.cpu().numpy())
    assert np.array_equal(df["item_id"].to_numpy(), cand.cpu().numpy().reshape(-1))


# ---- 6. live catalogue ------------------------------------------------------------------------------------------------------
def test_live_catalogue_reaches_the_fold_in(parts):
    from recommendit_amd import FAISSIndex
    from recommendit_amd.coldstart import UserHistories, fold_in_users_device
    from recommendit_amd.recommender import GpuRecommendationPipeline
    rng = np.random.default_rng(8)
    X = rng.standard_normal((500, D)).astype(np.float32)
    index = FAISSIndex(embed_dim=D, exact=True)
    index.build_ivf_index(X, list(range(1, 501)))
    pipe = GpuRecommendationPipeline(parts["model"], index, parts["ranker"], parts["store"], top_k_candidates=100)
    hist = UserHistories.from_lists([[(77, 5), (12, 2)], [(300, 4), (301, 5)]])
    ids, _, _, fb = _host(pipe.recommend_cold_batch(hist, k=10))
    assert fb.tolist() == [False, False]
    V0 = index.item_vectors_device()[0]
    assert index.remove_items([77]) == 1
    V1, row_of, mu = index.item_vectors_device()
    assert V1 is not V0 and V1.shape[0] == 499 and row_of[77].item() == -1
    ids2, _, _, fb2 = _host(pipe.recommend_cold_batch(hist, k=10))
    assert fb2.tolist() == [True, False]                                           # its only liked item is gone
    assert ids2[0].tolist() == pipe.popularity_order().cpu().numpy()[:11][~np.isin(
        pipe.popularity_order().cpu().numpy()[:11], [12])][:10].tolist()
    assert 77 not in pipe.popularity_order().cpu().numpy()
    # a replaced vector is the one folded in
    new = np.zeros((1, D), np.float32)
    new[0, 3] = 2.0
    assert index.update_items(new, [300]) == (1, 0)
    V2, row_of, mu = index.item_vectors_device()
    one = UserHistories.from_lists([[(300, 5)]])
    q, _, flags = _host(fold_in_users_device(one, V2, row_of, mu, beta=0.0))
    assert flags.tolist() == [0] and q[0].tolist() == [0.0] * 3 + [1.0] + [0.0] * (D - 4)
    q_ref, _, _ = R.fold_in_reference(*hist.host, index.reconstruct(), row_of.cpu().numpy(), mu.cpu().numpy(), 4, 0, 1.0)
    q, _, _ = _host(fold_in_users_device(hist, V2, row_of, mu))
    assert np.abs(q.astype(np.float64) - q_ref).max() <= Q_TOL


# ---- 7. the single request ----------------------------------------------------------------------------------------------------
def test_single_request_with_a_history(parts, monkeypatch):
    from recommendit_amd.coldstart import UserHistories
    pipe = _pipe(parts)
    history = _histories(9, [30])[0]
    ids, sc, rs, fb = _host(pipe.recommend_cold_batch(UserHistories.from_lists([history]), k=15))
    one = pipe.get_recommendations(10 ** 9, k=15, history=history)                 # the id is a label only
    assert [d["item_id"] for d in one] == ids[0].tolist() and [d["rank"] for d in one] == list(range(1, 16))
    assert [d["score"] for d in one] == sc[0].tolist() and all(d["cold"] is True and d["fallback"] is False for d in one)
    kept = pipe.get_recommendations(1, k=15, history=history, exclude_seen=False)
    assert [d["item_id"] for d in kept] == _host(pipe.recommend_cold_batch(UserHistories.from_lists([history]), k=15,
                                                                           exclude_history=False))[0][0].tolist()
    nothing = pipe.get_recommendations(1, k=5, history=[])
    assert [d["item_id"] for d in nothing] == pipe.popularity_order()[:5].tolist() and all(d["fallback"] for d in nothing)
    assert "cold" not in pipe.get_recommendations(3, k=5)[0]
    with pytest.raises(ValueError):
        pipe.get_recommendations(1, k=5, history=history, graph=True)
    from recommendit_amd import two_tower
    monkeypatch.setattr(two_tower, "_CHECK_IDS", True)                             # (the device-side id check is opt-in)
    with pytest.raises(IndexError):                                                # an unknown user without a history
        pipe.get_recommendations(NU + 1000, k=5)
