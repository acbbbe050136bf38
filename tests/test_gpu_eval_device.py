"""GPU: the device evaluation report (recommendit_amd.eval_device, csrc/eval.hip) against the reference's own outputs
(G10) and against the host evaluate_model: ranking keys to 1e-12, coverage exact, diversity to 1e-6 relative (the
reference's pair arithmetic is float32), per-user values, run-to-run bit equality, hipGraph replay, and argument
errors surfacing as RuntimeError."""
import json
import math

import numpy as np
import pytest
import torch

from recommendit_amd import metrics as M

pytestmark = pytest.mark.gpu

RANK = ("ndcg", "recall", "precision", "mrr", "ap")


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def pad_rows(rows, K=None, holes=False, seed=0):
    """lists of ids -> int64 [n, K] with -1 padding at the tail (and, with holes, inside the rows)"""
    rng = np.random.default_rng(seed)
    out = []
    for r in rows:
        r = list(r)
        if holes:
            for _ in range(int(rng.integers(0, 4))):
                r.insert(int(rng.integers(0, len(r) + 1)), -1)
        out.append(r)
    K = K or max(1, max((len(r) for r in out), default=1))
    a = np.full((len(out), K), -1, np.int64)
    for i, r in enumerate(out):
        a[i, :len(r)] = r[:K]
    return a


def assert_report_close(got, ref, div_rel=1e-6):
    """ref: dict or list of (key, value) pairs"""
    ref = list(ref.items()) if isinstance(ref, dict) else ref
    assert list(got.keys()) == [k for k, _ in ref]
    for key, want in ref:
        v = got[key]
        if key in ("n_users", "k_values", "error"):
            assert v == want, key
        elif key == "avg_diversity":
            assert abs(v - want) <= div_rel * max(abs(want), 1e-30), (key, v, want)
        elif key == "coverage":
            assert v == want, (key, v, want)
        else:
            assert abs(v - want) <= 1e-12, (key, v, want)


def test_g10_cases_on_device(golden_dir):
    from recommendit_amd.eval_device import GroundTruth, evaluate_topk_device, vectors_from_dict
    cases = json.loads((golden_dir / "g10_evaluate_model.json").read_text())
    for ci, case in enumerate(cases):
        users = [u for u, _ in case["recs"]]
        truth = {u: t for u, t in case["truth"]}
        rec = torch.from_numpy(pad_rows([r for _, r in case["recs"]], holes=ci % 2 == 1, seed=ci)).to(_dev())
        vec = pres = None
        if case["vectors"]:
            vec, pres = vectors_from_dict({i: np.asarray(v, dtype=np.float32) for i, v in case["vectors"]})
        got = evaluate_topk_device(rec, GroundTruth.from_dict(truth, users), list(case["k_values"]),
                                   catalog_size=case["catalog_size"], item_vectors=vec, item_present=pres,
                                   n_id_space=64)
        assert_report_close(got, case["report"])


def _random_case(n, K, n_items, seed):
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, n_items, (n, K)).astype(np.int64)
    rec[:, 1::7] = rec[:, 0:1]                                    # duplicate recommendations
    tail = rng.integers(0, K // 3, n)
    for i in np.nonzero(rng.random(n) < 0.5)[0]:
        rec[i, K - tail[i]:] = -1                                 # padded tails
    rec[rng.random((n, K)) < 0.02] = -1                           # holes inside rows
    truth, users = {}, list(range(1000, 1000 + n))
    for i, u in enumerate(users):
        m = int(rng.integers(0, 41))
        if m == 0 and i % 2:
            continue                                              # missing (vs. empty) ground truth
        t = [int(x) for x in rng.integers(0, n_items, m)]
        if m > 2:
            t += t[:2]                                            # duplicates in the truth
        # some truth drawn from the user's own list so that hits are frequent
        row = rec[i][rec[i] >= 0]
        if m and row.size:
            t += [int(x) for x in rng.choice(row, min(m, 5))]
        truth[u] = t
    return rec, users, truth


def _host_recs(rec, users):
    return {u: [int(x) for x in row if x >= 0] for u, row in zip(users, rec)}


@pytest.fixture(scope="module")
def big_case():
    n, K, n_items = 20000, 500, 3000
    rec, users, truth = _random_case(n, K, n_items, seed=5)
    rng = np.random.default_rng(6)
    genres = {}
    for i in range(n_items):
        r = rng.random()
        if r < 0.1:
            continue                                              # no vector
        genres[i] = np.zeros(18, np.float32) if r < 0.15 else (rng.random(18) < 0.2).astype(np.float32)
    return rec, users, truth, genres, n_items


def test_random_report_matches_host(big_case):
    from recommendit_amd.eval_device import GroundTruth, evaluate_topk_device, vectors_from_dict
    rec, users, truth, genres, n_items = big_case
    ks = [20, 1, 500, 700, 10]
    recs = _host_recs(rec, users)
    host = M.evaluate_model(recs, truth, ks, catalog_size=n_items, item_genre_vectors=genres)
    vec, pres = vectors_from_dict(genres, n_rows=n_items)
    gt = GroundTruth.from_dict(truth, users)
    dev = evaluate_topk_device(torch.from_numpy(rec).to(_dev()), gt, ks, catalog_size=n_items, item_vectors=vec,
                               item_present=pres, n_id_space=n_items)
    assert_report_close(dev, host)
    assert 0.0 < dev["ndcg@20"] < 1.0 and dev["recall@700"] > 0


def test_embedding_diversity_vs_float64():
    """g = 128, L = 100 (4 x 4 tiles of the MFMA Gram) against a float64 numpy reference"""
    from recommendit_amd.eval_device import GroundTruth, evaluate_topk_device
    n, K, n_items, L, g = 2000, 160, 5000, 100, 128
    rec, users, truth = _random_case(n, K, n_items, seed=9)
    rng = np.random.default_rng(10)
    E = rng.standard_normal((n_items, g)).astype(np.float32)
    E[::97] = 0.0                                                 # zero vectors: their pairs are not counted
    dev = evaluate_topk_device(torch.from_numpy(rec).to(_dev()), GroundTruth.from_dict(truth, users), [5, L],
                               item_vectors=torch.from_numpy(E).to(_dev()), per_user=True)
    E64 = E.astype(np.float64)
    divs = []
    per = dev["per_user"]["diversity"].cpu().numpy()
    for i, u in enumerate(users):
        if not truth.get(u):
            continue
        row = rec[i][rec[i] >= 0][:L]
        X = E64[row]
        nr = np.linalg.norm(X, axis=1)
        ok = nr > 0
        X, nr = X[ok], nr[ok]
        if len(row) < 2 or X.shape[0] < 2:
            d = 0.0
        else:
            C = (X @ X.T) / np.outer(nr, nr)
            iu = np.triu_indices(X.shape[0], 1)
            d = float(np.mean(1.0 - C[iu]))
        assert abs(per[i] - d) <= 1e-5 * max(abs(d), 1.0), (i, per[i], d)
        divs.append(d)
    want = float(np.mean(divs))
    assert abs(dev["avg_diversity"] - want) <= 1e-5 * abs(want), (dev["avg_diversity"], want)


def test_bitwise_repeatable_and_per_user_values(big_case):
    from recommendit_amd.eval_device import GroundTruth, evaluate_topk_device, vectors_from_dict
    rec, users, truth, genres, n_items = big_case
    ks = [20, 1, 500, 700, 10]
    vec, pres = vectors_from_dict(genres, n_rows=n_items)
    gt = GroundTruth.from_dict(truth, users)
    r = torch.from_numpy(rec).to(_dev())
    a = evaluate_topk_device(r, gt, ks, catalog_size=n_items, item_vectors=vec, item_present=pres,
                             n_id_space=n_items, per_user=True)
    b = evaluate_topk_device(r, gt, ks, catalog_size=n_items, item_vectors=vec, item_present=pres,
                             n_id_space=n_items, per_user=True)
    pa, pb = a.pop("per_user"), b.pop("per_user")
    assert a == b                                                 # same floats, bit for bit
    for key in pa:
        assert torch.equal(pa[key], pb[key]), key
    vals, rr = pa["vals"].cpu().numpy(), pa["mrr"].cpu().numpy()
    scored, div = pa["scored"].cpu().numpy(), pa["diversity"].cpu().numpy()
    recs = _host_recs(rec, users)
    for i in range(0, len(users), 7):
        u = users[i]
        rel = truth.get(u, [])
        assert scored[i] == (1 if rel else 0)
        if not rel:
            assert (vals[i] == 0).all() and rr[i] == 0 and div[i] == 0
            continue
        for j, k in enumerate(ks):                                # distinct k in order: here all of them
            assert vals[i, j, 0] == M.ndcg_at_k(recs[u], rel, k), (i, k)
            assert vals[i, j, 1] == M.recall_at_k(recs[u], rel, k), (i, k)
            assert vals[i, j, 2] == M.precision_at_k(recs[u], rel, k), (i, k)
        assert rr[i] == M.mrr(recs[u], rel)
        want = float(M.intra_list_diversity(recs[u][:ks[-1]], genres))
        assert abs(div[i] - want) <= 1e-5 * max(abs(want), 1e-3), (i, div[i], want)


def _serving_setup(tmp_path):
    from oracle import gbdt_np as G
    from recommendit_amd import FAISSIndex, LightGBMRanker, TwoTowerModel
    from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns
    from recommendit_amd.synthetic import ml1m_like
    ratings, movies, gm = ml1m_like(n_users=300, n_item_ids=420, n_catalog=400, n_ratings=30000, seed=2)
    nu, ni, d = 300, 420, 64
    torch.manual_seed(0)
    model = TwoTowerModel(nu, ni, d, 128)
    item_ids = sorted(movies["item_id"].unique().tolist())
    E = model.get_item_embeddings(item_ids, gm[item_ids])
    index = FAISSIndex(embed_dim=d, n_lists=8, n_probe=3)
    index.build_ivf_index(E, item_ids)
    forest = G.random_forest_model(30, 15, 50, seed=9, names=feature_columns())
    p = tmp_path / "r.lgbm"
    p.write_text(G.write_text_model(forest))
    ranker = LightGBMRanker.load(str(p))
    rng = np.random.RandomState(1)
    store = GpuFeatureStore(nu, ni)
    ut = store.user.copy(); it = store.item.copy()
    ut[1:, :6] = rng.rand(nu, 6); ut[1:, 6:] = rng.rand(nu, 18)
    it[1:, :5] = rng.rand(ni, 5); it[1:, 5:] = gm[1:]
    store.load_arrays(ut, it)
    pipe = GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=100, top_k_results=20)
    return ratings, movies, gm, model, index, pipe, item_ids


def test_run_evaluate_and_retrieval_ndcg_on_device(tmp_path):
    from recommendit_amd.evaluate import run_evaluate
    from recommendit_amd.train_embeddings import evaluate_retrieval_all_users, retrieval_ndcg
    from recommendit_amd.eval_device import vectors_from_dict
    ratings, movies, gm, model, index, pipe, item_ids = _serving_setup(tmp_path)
    host = run_evaluate(pipe, ratings, movies, n_eval_users=120, batch_size=50)
    dev = run_evaluate(pipe, ratings, movies, n_eval_users=120, batch_size=50, on_device=True)
    assert "precision@20" in host and "coverage" in host and host["n_eval_users"] > 50
    assert_report_close(dev, host)
    genres = {int(i): gm[i] for i in item_ids}
    host = run_evaluate(pipe, ratings, movies, n_eval_users=120, batch_size=50, item_genre_vectors=genres)
    dev = run_evaluate(pipe, ratings, movies, n_eval_users=120, batch_size=50, on_device=True,
                       item_genre_vectors=genres)
    assert "avg_diversity" in host
    assert_report_close(dev, host)
    for n_eval in (200, None):
        h = retrieval_ndcg(model, ratings, movies, n_eval_users=n_eval)
        d = retrieval_ndcg(model, ratings, movies, n_eval_users=n_eval, on_device=True)
        assert_report_close(d, h)
    # whole population: the device evaluator on the retrieval tensor vs the host report of the same ids
    rs = ratings.sort_values("timestamp")
    test = rs.groupby("user_id").tail(3)
    test = test[test["rating"] >= 4]
    got = evaluate_retrieval_all_users(model, index, test, k_candidates=100, top=20, batch=64, catalog_size=400)
    _, first = np.unique(test["user_id"].to_numpy(), return_index=True)
    users = test["user_id"].to_numpy()[np.sort(first)]
    U = model.get_user_embeddings(torch.from_numpy(users.astype(np.int64)), as_tensor=True)
    _, ids = index.batch_search_device(U, k=100)
    recs = _host_recs(ids[:, :20].cpu().numpy(), [int(u) for u in users])
    truth = {int(u): g["item_id"].tolist() for u, g in test.groupby("user_id")}
    assert_report_close(got, M.evaluate_model(recs, truth, [5, 10, 20], catalog_size=400))


def test_graph_capture_replays_same_report(big_case):
    from recommendit_amd.eval_device import GroundTruth, TopKEvaluator, vectors_from_dict
    rec, users, truth, genres, n_items = big_case
    ks = [20, 1, 500, 700, 10]
    vec, pres = vectors_from_dict(genres, n_rows=n_items)
    r = torch.from_numpy(rec).to(_dev())
    ev = TopKEvaluator(GroundTruth.from_dict(truth, users), r.shape[0], r.shape[1], ks, catalog_size=n_items,
                       item_vectors=vec, item_present=pres, n_id_space=n_items)
    ev.enqueue(r)
    eager = ev.result()
    ev.out.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev.enqueue(r)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev.enqueue(r)
    ev.out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert ev.result() == eager
    r.copy_(torch.flip(r, dims=[0]))                              # new contents, same buffers: the replay follows
    g.replay()
    torch.cuda.synchronize()
    flipped = ev.result()
    assert flipped != eager and flipped["n_users"] == eager["n_users"]


def test_errors_raise_runtime_error():
    from recommendit_amd.eval_device import GroundTruth, evaluate_topk_device
    users = [1, 2]
    gt = GroundTruth.from_dict({1: [3], 2: [4]}, users)
    rec = torch.tensor([[3, 5], [4, 100]], dtype=torch.int64, device=_dev())
    with pytest.raises(RuntimeError, match="n_id_space"):
        evaluate_topk_device(rec, gt, [1, 2], catalog_size=10, n_id_space=50)
    ok = evaluate_topk_device(rec, gt, [1, 2], catalog_size=10, n_id_space=101)
    assert ok["coverage"] == 0.4 and ok["ndcg@1"] == 1.0
    with pytest.raises(RuntimeError, match="K="):
        evaluate_topk_device(torch.zeros((2, 16385), dtype=torch.int64, device=_dev()), gt, [5])
    with pytest.raises(RuntimeError):
        evaluate_topk_device(rec.cpu(), gt, [5])
    with pytest.raises(RuntimeError):
        evaluate_topk_device(rec, gt, [5], item_vectors=torch.zeros((200, 4)))
    with pytest.raises(RuntimeError, match="k="):
        evaluate_topk_device(rec, gt, [5, -1])
    with pytest.raises(RuntimeError, match="L="):
        evaluate_topk_device(rec, gt, [5, 600], item_vectors=torch.zeros((200, 4), device=_dev()))
    assert evaluate_topk_device(rec[:0], GroundTruth.from_dict({}, []), [5]) == {"error": "No users to evaluate",
                                                                                 "n_users": 0}
