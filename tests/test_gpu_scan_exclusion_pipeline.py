"""GPU: the serve chain with seen-item exclusion inside retrieval's scan (GpuRecommendationPipeline(exclusion="scan")):
one chain over the whole batch, equal to its stages run by hand and, bit for bit, to the over-fetch pipeline on a batch
that over-fetch has to split into groups; the cold-start chain; graph=True refused."""
import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import gbdt_np as G

pytestmark = pytest.mark.gpu

NU, NI, D, H, KC = 120, 3000, 64, 128, 100


@pytest.fixture(scope="module", params=["exact", "ivf"])
def served(request, tmp_path_factory):
    from recommendit_amd import FAISSIndex, LightGBMRanker, SeenItems, TwoTowerModel
    from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns
    sd = fx.make_state(NU, NI, D, H, seed=21)
    model = TwoTowerModel(NU, NI, D, H)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    rng = np.random.RandomState(2)
    item_ids = list(range(1, NI + 1))
    genres = (rng.rand(NI, 18) < 0.15).astype(np.float32)
    E = model.get_item_embeddings(item_ids, genres)
    index = FAISSIndex(embed_dim=D, exact=True) if request.param == "exact" else FAISSIndex(embed_dim=D, n_lists=8, n_probe=4)
    index.build_ivf_index(E, item_ids)
    forest = G.random_forest_model(60, 31, 50, seed=5, names=feature_columns())
    p = tmp_path_factory.mktemp("ranker") / "r.lgbm"
    p.write_text(G.write_text_model(forest))
    ranker = LightGBMRanker.load(str(p))
    store = GpuFeatureStore(NU, NI)
    ut, it = store.user.copy(), store.item.copy()
    ut[1:, :6] = rng.rand(NU, 6) * [5, 8, 1, 1, 1, 1]
    ut[1:, 6:] = rng.rand(NU, 18)
    it[1:, :5] = rng.rand(NI, 5) * [5, 9, 1, 1.5, 1]
    it[1:, 5:] = genres
    store.load_arrays(ut, it)
    users = list(range(1, NU + 1))
    uid = torch.tensor(users, device="cuda")
    q = model.get_user_embeddings(uid, as_tensor=True)
    _, unf = index.batch_search_device(q, k=2048, normalized=True)          # each user's own unexcluded order
    unf = unf.cpu().numpy()
    seen = {}
    for qi, u in enumerate(users):
        row = unf[qi][unf[qi] >= 0]
        n = (0, 30, 200, 900)[qi % 4] if u != 42 else 1200                   # several over-fetch classes and a heavy user
        seen[u] = row[:min(n, row.size - KC)].tolist()
    seen_store = SeenItems.from_dict(seen, n_users=NU + 1)
    mk = lambda **kw: GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=KC, top_k_results=20,
                                                seen=seen_store, **kw)
    return dict(model=model, index=index, ranker=ranker, store=store, users=users, uid=uid, seen=seen, seen_store=seen_store,
                over=mk(), scan=mk(exclusion="scan"), mk=mk, item_ids=item_ids)


def _equal(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y)


def test_scan_pipeline_equals_the_overfetch_pipeline_and_its_stages(served, monkeypatch):
    import recommendit_amd.seen as seen_mod
    from recommendit_amd.recommender import build_ranking_features_device
    monkeypatch.setattr(seen_mod, "MIN_GROUP", 8)
    s = served
    users, uid = s["users"], s["uid"]
    plan = seen_mod.plan_overfetch(s["seen_store"].counts_of(users), KC, NI, 16384)
    assert len(plan) >= 3                                            # over-fetch serves this batch in several groups
    over = [t.clone() for t in s["over"].recommend_batch(users)]
    d0 = s["over"].exclusion_deficit()
    x0 = s["index"].exclusion_stats()
    scan = [t.clone() for t in s["scan"].recommend_batch(users)]
    x1 = s["index"].exclusion_stats()
    assert x1["queries"] - x0["queries"] == NU and x1["chunks"] - x0["chunks"] == 1      # one search of the whole batch
    _equal(scan, over)
    ids = scan[0].cpu().numpy()
    for qi, u in enumerate(users):
        assert (ids[qi] >= 0).all() and not np.isin(ids[qi], s["seen"][u]).any()
    _equal(s["scan"].recommend_batch(uid), scan)                     # device ids take the same path
    assert s["scan"].exclusion_deficit() == d0 == 0                  # nothing is added to the deficit
    # the stages by hand: tower -> excluded search -> features -> ranker -> stable top-k by ranker score
    q = s["model"].get_user_embeddings(uid, as_tensor=True)
    rs, cand = s["index"].batch_search_device(q, k=KC, normalized=True, exclude=s["seen_store"], user_ids=uid, exclusion="scan")
    X = build_ranking_features_device(s["store"], uid, cand, s["ranker"].feature_names)
    sc = s["ranker"].predict_device(X).view(NU, KC)
    top, order = torch.sort(sc, dim=1, descending=True, stable=True)
    _equal(scan, (torch.gather(cand, 1, order[:, :20]), top[:, :20].contiguous(), torch.gather(rs, 1, order[:, :20])))
    # single requests
    for qi in (0, 41, 119):
        one = s["scan"].get_recommendations(users[qi])
        assert [r["item_id"] for r in one] == ids[qi].tolist()
        assert [r["score"] for r in one] == scan[1][qi].tolist()
    # exclude_seen=False ignores the store under either implementation
    _equal(s["scan"].recommend_batch(users, exclude_seen=False), s["over"].recommend_batch(users, exclude_seen=False))
    # the over-fetch pipeline after scan calls on the same index: the bytes it gave before
    _equal(s["over"].recommend_batch(users), over)
    assert s["over"].exclusion_deficit() == 0


def test_scan_pipeline_with_an_item_filter(served):
    s = served
    rng = np.random.RandomState(3)
    s["index"].set_item_tags(rng.randint(0, 16, NI).astype(np.uint32))
    try:
        for flt in ((1, 0, 0), rng.randint(0, 4, (NU, 3)).astype(np.uint32) * np.array([1, 0, 4], np.uint32)):
            _equal(s["scan"].recommend_batch(s["users"], item_filter=flt), s["over"].recommend_batch(s["users"], item_filter=flt))
    finally:
        s["index"].clear_item_tags()


def test_graph_is_refused_under_scan(served):
    s = served
    with pytest.raises(ValueError, match="graph"):
        s["scan"].recommend_batch(s["users"][:4], graph=True)
    with pytest.raises(ValueError, match="graph"):
        s["scan"].get_recommendations(7, graph=True)
    with pytest.raises(ValueError, match="exclusion"):
        s["mk"](exclusion="mask")
    # without a store in play the scan pipeline captures as ever
    g = s["scan"].recommend_batch(s["users"][:4], graph=True, exclude_seen=False)
    _equal(g, s["over"].recommend_batch(s["users"][:4], exclude_seen=False))


def test_cold_batch_gives_the_same_bytes(served):
    from recommendit_amd.coldstart import UserHistories
    s = served
    rng = np.random.RandomState(9)
    hist = []
    for n in (0, 3, 40, 400, 25, 1):
        items = rng.choice(np.arange(1, NI + 1), n, replace=False)
        hist.append([(int(i), int(r)) for i, r in zip(items, rng.randint(3, 6, n))])
    hist.append([(NI + 500, 5), (2, 1)])                             # nothing usable: the popularity fallback
    H_ = UserHistories.from_lists(hist)
    a = s["scan"].recommend_cold_batch(H_, exclude_history=True)
    b = s["over"].recommend_cold_batch(H_, exclude_history=True)
    _equal(a, b)
    ids = a[0].cpu().numpy()
    for q, h in enumerate(hist):
        assert not np.isin(ids[q][ids[q] >= 0], [i for i, _ in h]).any()
    assert a[3].cpu().numpy().tolist() == b[3].cpu().numpy().tolist() and a[3][0] and a[3][-1]
    _equal(s["scan"].recommend_cold_batch(H_, exclude_history=False), s["over"].recommend_cold_batch(H_, exclude_history=False))
    one = s["scan"].get_recommendations(5, history=hist[3])
    assert [r["item_id"] for r in one] == [i for i in ids[3].tolist() if i >= 0]
