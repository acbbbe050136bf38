"""GPU: training-serving skew on the device (recommendit_amd.skew_device, csrc/skew.hip) and the serving feature log
of GpuRecommendationPipeline: the reference's own outputs (G11), edges equal to np.linspace bit for bit, counts equal
to np.histogram exactly, KL against the host to 1e-12, run-to-run bit equality, hipGraph replay, the logged rows of
served batches (wrap-around, graph replay, the deferred exactness re-do) and argument errors."""
import ctypes as C
import json
import math
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import fixtures as fx
from oracle import gbdt_np as G
from recommendit_amd import metrics as M

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def load_g11(golden_dir):
    z = np.load(golden_dir / "g11_skew.npz")
    cases = json.loads(str(z["meta"]))
    for i, c in enumerate(cases):
        if c["kind"] == "detect":
            c["train"] = pd.DataFrame({n: z[f"c{i}_a_{j}"] for j, n in enumerate(c["a_cols"])})
            c["serving"] = pd.DataFrame({n: z[f"c{i}_b_{j}"] for j, n in enumerate(c["b_cols"])})
        else:
            c["p"], c["q"] = z[f"c{i}_a_0"], z[f"c{i}_b_0"]
    return cases


def rel_close(got, want, rel):
    if want is None or (isinstance(want, float) and math.isnan(want)):
        return math.isnan(got)
    return abs(got - want) <= rel * max(abs(want), 1e-300)


def assert_skew_dict(got, ref, raw):
    """equal keys / order / flags / counts; a rounded KL may differ by 1e-6 only on a rounding boundary"""
    ref = dict(ref) if not isinstance(ref, dict) else ref
    assert list(got) == list(ref)
    assert list(got["feature_kl"]) == list(ref["feature_kl"])
    for col, want in ref["feature_kl"].items():
        v = got["feature_kl"][col]
        if isinstance(want, float) and math.isnan(want):
            assert math.isnan(v), col
        elif v != want:
            assert abs(v - want) <= 1.0000001e-6, (col, v, want)
            r = raw[col]
            assert abs(r * 1e6 - math.floor(r * 1e6) - 0.5) < 1e-6, (col, r, v, want)
    for key in ("flagged_features", "skew_detected", "n_features_checked", "threshold"):
        assert got[key] == ref[key], key
    wk = ref["max_kl"]
    assert (isinstance(wk, float) and math.isnan(wk) and math.isnan(got["max_kl"])) or \
        abs(got["max_kl"] - wk) <= 1.0000001e-6


def host_counts(x, edges):
    """np.histogram's array-bin rule without a sort (same result): bin i holds e[i] <= x < e[i+1], the last bin also
    x == e[-1]"""
    x = x[~np.isnan(x)]
    nb = len(edges) - 1
    idx = np.searchsorted(edges, x, side="right") - 1
    idx[x == edges[-1]] = nb - 1
    idx = idx[(idx >= 0) & (idx < nb)]
    return np.bincount(idx, minlength=nb)


def test_g11_cases_on_device(golden_dir):
    from recommendit_amd.skew_device import detect_training_serving_skew_device, kl_divergence_bins_device
    dev = _dev()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in load_g11(golden_dir):
            if c["kind"] == "kl":
                got = kl_divergence_bins_device(torch.from_numpy(c["p"]).to(dev), torch.from_numpy(c["q"]).to(dev),
                                                n_bins=c["n_bins"], epsilon=c["epsilon"])
                assert rel_close(got, c["kl"], 1e-12), (c["name"], got, c["kl"])
                continue
            raw = dict(c["raw_kl"])
            for col, want in raw.items():
                a = c["train"][col].dropna().values.astype(float)
                b = c["serving"][col].dropna().values.astype(float)
                got = kl_divergence_bins_device(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
                assert rel_close(got, want, 1e-12), (c["name"], col, got, want)
            res = detect_training_serving_skew_device(c["train"], c["serving"], threshold=c["threshold"],
                                                      numeric_cols=c["numeric_cols"])
            assert_skew_dict(res, c["result"], raw)


def _check_against_host(A, B, ca, cb, ia, ib, nb, r, kl_rel=1e-12):
    counts, edges, valid, kl = (t.cpu().numpy() for t in (r.counts, r.edges, r.valid, r.kl))
    for c in range(len(ca)):
        a = A[ia >= 0, ca[c]].astype(np.float64) if ia is not None else A[:, ca[c]].astype(np.float64)
        b = B[ib >= 0, cb[c]].astype(np.float64) if ib is not None else B[:, cb[c]].astype(np.float64)
        a, b = a[~np.isnan(a)], b[~np.isnan(b)]
        assert valid[c].tolist() == [len(a), len(b)], c
        comb = np.concatenate([a, b])
        e = np.linspace(comb.min(), comb.max(), nb + 1)
        assert np.array_equal(edges[c].view(np.int64), e.view(np.int64)), (c, edges[c], e)
        if len(a) + len(b) < 200_000:
            ha, hb = np.histogram(a, bins=e)[0], np.histogram(b, bins=e)[0]
        else:
            ha, hb = host_counts(a, e), host_counts(b, e)
        np.testing.assert_array_equal(counts[c, 0], ha)
        np.testing.assert_array_equal(counts[c, 1], hb)
        want = M.kl_divergence_bins(a, b, n_bins=nb)
        assert rel_close(float(kl[c]), want, kl_rel), (c, kl[c], want)


@pytest.mark.parametrize("nb", [1, 20, 128])
def test_edges_and_counts_match_numpy(nb):
    from recommendit_amd.skew_device import feature_histograms_device
    dev = _dev()
    rng = np.random.default_rng(nb)
    A = rng.standard_normal((3000, 13)).astype(np.float32)
    B = (rng.standard_normal((2100, 9)) * 1.3 + 0.2)
    A[rng.random(A.shape) < 0.05] = np.nan
    B[rng.random(B.shape) < 0.03] = np.nan
    # values on every edge of linspace(0, nb, nb + 1), the max repeated
    A[:, 2] = rng.integers(0, nb + 1, 3000)
    B[:, 8] = rng.integers(0, nb + 1, 2100)
    A[:7, 2] = nb
    B[:5, 8] = nb
    # a subnormal range: step = 5e-324 / nb underflows to 0 for nb >= 3
    Bd = B.copy()
    A64 = A.astype(np.float64)
    A64[:, 5] = np.where(rng.random(3000) < 0.5, 0.0, 5e-324)
    Bd[:, 6] = np.where(rng.random(2100) < 0.3, 0.0, 5e-324)
    ca, cb = [11, 2, 7, 0, 5], [3, 8, 1, 0, 6]
    ia = np.where(rng.random(3000) < 0.1, -1, np.arange(3000)).astype(np.int64)
    ib = np.where(rng.random(2100) < 0.2, -1, 5).astype(np.int64)
    # f32 train with ld > nc and row skipping
    r = feature_histograms_device(torch.from_numpy(A).to(dev), torch.from_numpy(Bd).to(dev), ca, cb,
                                  torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev), n_bins=nb)
    _check_against_host(A, Bd, ca, cb, ia, ib, nb, r)
    # f64 train (holds the subnormal column) without ids
    r = feature_histograms_device(torch.from_numpy(A64).to(dev), torch.from_numpy(Bd).to(dev), ca, cb, n_bins=nb)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        counts, edges = r.counts.cpu().numpy(), r.edges.cpu().numpy()
        for c in range(len(ca)):
            a, b = A64[:, ca[c]], Bd[:, cb[c]]
            a, b = a[~np.isnan(a)], b[~np.isnan(b)]
            comb = np.concatenate([a, b])
            e = np.linspace(comb.min(), comb.max(), nb + 1)
            assert np.array_equal(edges[c].view(np.int64), e.view(np.int64)), (c, edges[c], e)
            np.testing.assert_array_equal(counts[c, 0], np.histogram(a, bins=e)[0])
            np.testing.assert_array_equal(counts[c, 1], np.histogram(b, bins=e)[0])
            want = M.kl_divergence_bins(a, b, n_bins=nb)
            assert rel_close(float(r.kl[c]), want, 1e-12), (c, float(r.kl[c]), want)


def _full_size(dev, seed=11):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    A = torch.randn((2_390_000, 50), generator=g, device=dev, dtype=torch.float32)
    B = torch.randn((1_000_000, 50), generator=g, device=dev, dtype=torch.float32)
    shift = torch.linspace(0.0, 1.5, 50, device=dev, dtype=torch.float32)
    B = B * (1.0 + shift / 3) + shift
    A[:, 7] = torch.round(A[:, 7] * 4)          # a column of repeated values (edge hits, near-constant runs)
    B[:, 7] = torch.round(B[:, 7] * 4)
    return A, B.contiguous()


def test_full_size_counts_exact_and_kl_matches_host():
    from recommendit_amd.skew_device import feature_histograms_device
    dev = _dev()
    A, B = _full_size(dev)
    r = feature_histograms_device(A, B)
    torch.cuda.synchronize()
    An, Bn = A.cpu().numpy(), B.cpu().numpy()
    cols = list(range(50))
    _check_against_host(An, Bn, cols, cols, None, None, 20, r)


def test_bitwise_repeatable_and_graph_replay():
    from recommendit_amd import _lib as L
    from recommendit_amd.skew_device import feature_histograms_device
    dev = _dev()
    A, B = _full_size(dev, seed=3)
    A, B = A[:400_000].contiguous(), B[:300_000].contiguous()
    r1 = feature_histograms_device(A, B, n_bins=37)
    r2 = feature_histograms_device(A, B, n_bins=37)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)
    # the raw entry point inside a captured graph, on buffers allocated outside it
    lib = L.lib()
    nc, nb = 50, 37
    cols = torch.arange(nc, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.rihip_skew_workspace_bytes(nc))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    counts = torch.full((nc, 2, nb), -7, dtype=torch.int64, device=dev)
    edges = torch.empty((nc, nb + 1), dtype=torch.float64, device=dev)
    valid = torch.empty((nc, 2), dtype=torch.int64, device=dev)
    kl = torch.empty((nc,), dtype=torch.float64, device=dev)
    status = torch.empty((nc,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        L.check(lib.rihip_skew_compute(A.data_ptr(), 0, A.shape[0], 50, cols.data_ptr(), None, B.data_ptr(), 0,
                                       B.shape[0], 50, cols.data_ptr(), None, nc, nb, 1e-10, 0, 1, ws.data_ptr(),
                                       ws_bytes, counts.data_ptr(), edges.data_ptr(), valid.data_ptr(), kl.data_ptr(),
                                       status.data_ptr(), L.stream_ptr()), "skew_compute")
    for _ in range(2):
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(counts, r1.counts) and torch.equal(edges, r1.edges) and torch.equal(kl, r1.kl)
        assert torch.equal(valid, r1.valid)


def test_errors_raise_without_fault():
    from recommendit_amd import _lib as L
    from recommendit_amd.skew_device import (detect_training_serving_skew_device, feature_histograms_device,
                                             kl_divergence_bins_device)
    dev = _dev()
    a = torch.randn(100, 4, device=dev)
    b = torch.randn(80, 4, device=dev)
    with pytest.raises(ValueError):
        feature_histograms_device(a.cpu(), b)
    with pytest.raises(ValueError):
        feature_histograms_device(a, b.to(torch.int32))
    with pytest.raises(ValueError):
        feature_histograms_device(a.half(), b)
    for nb in (0, 129, -3, 2.5, True):
        with pytest.raises(ValueError):
            feature_histograms_device(a, b, n_bins=nb)
    with pytest.raises(ValueError):
        feature_histograms_device(a, b[:, :3])                       # column-count mismatch
    with pytest.raises(ValueError):
        feature_histograms_device(a, b, [0, 1], [0, 1, 2])
    with pytest.raises(ValueError):
        feature_histograms_device(a, b, [0, 4], [0, 1])               # column outside the row
    with pytest.raises(ValueError):
        feature_histograms_device(a, b, ids_train=torch.zeros(99, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        kl_divergence_bins_device(a[:0, 0], b[:0, 0])
    with pytest.raises(ValueError):
        kl_divergence_bins_device(a, b)
    with pytest.raises(ValueError):
        kl_divergence_bins_device(a[:, 0], b[:, 0], n_bins=200)
    with pytest.raises(ValueError):
        detect_training_serving_skew_device(a, b)                    # a tensor without column names
    with pytest.raises(ValueError):
        detect_training_serving_skew_device(a, b, columns=["x", "y"])
    # the C entry point rejects before any launch
    lib = L.lib()
    ws = torch.empty((int(lib.rihip_skew_workspace_bytes(4)),), dtype=torch.uint8, device=dev)
    out = [torch.empty(64, dtype=torch.float64, device=dev) for _ in range(5)]
    for nb in (0, 129):
        rc = lib.rihip_skew_compute(a.data_ptr(), 0, 100, 4, out[0].data_ptr(), None, b.data_ptr(), 0, 80, 4,
                                    out[0].data_ptr(), None, 4, nb, 1e-10, 0, 0, ws.data_ptr(), ws.numel(),
                                    *(o.data_ptr() for o in out), L.stream_ptr())
        assert rc != 0
    rc = lib.rihip_skew_compute(a.data_ptr(), 0, 100, 4, out[0].data_ptr(), None, b.data_ptr(), 0, 80, 4,
                                out[0].data_ptr(), None, 4, 20, 1e-10, 0, 0, ws.data_ptr(), 16,
                                *(o.data_ptr() for o in out), L.stream_ptr())
    assert rc != 0
    with pytest.raises(L.RihipError):
        L.check(rc, "skew")
    # the device is still healthy
    r = feature_histograms_device(a, b)
    torch.cuda.synchronize()
    assert (r.status.cpu().numpy() == 0).all()
    # tensor inputs with names equal the DataFrame path
    names = ["w", "x", "y", "z"]
    dfa = pd.DataFrame(a.double().cpu().numpy(), columns=names)
    dfb = pd.DataFrame(b.double().cpu().numpy(), columns=names)
    assert detect_training_serving_skew_device(a, b, columns=names) == M.detect_training_serving_skew(dfa, dfb)


# ---- serving feature log --------------------------------------------------------------------------------------------

def _pipeline_parts(tmp_path):
    from recommendit_amd import FAISSIndex, LightGBMRanker, TwoTowerModel
    from recommendit_amd.recommender import GpuFeatureStore, feature_columns
    nu, ni, d, H = 400, 6000, 64, 128
    sd = fx.make_state(nu, ni, d, H, seed=3)
    model = TwoTowerModel(nu, ni, d, H)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    rng = np.random.RandomState(4)
    item_ids = list(range(1, ni + 1))
    genres = (rng.rand(ni, 18) < 0.15).astype(np.float32)
    E = model.get_item_embeddings(item_ids, genres)
    index = FAISSIndex(embed_dim=d, n_lists=16, n_probe=4)
    index.build_ivf_index(E, item_ids)
    forest = G.random_forest_model(80, 31, 50, seed=6, names=feature_columns())
    p = tmp_path / "r.lgbm"
    p.write_text(G.write_text_model(forest))
    ranker = LightGBMRanker.load(str(p))
    store = GpuFeatureStore(nu, ni)
    ut = store.user.copy(); it = store.item.copy()
    ut[1:, :6] = rng.rand(nu, 6); ut[1:, 6:] = rng.rand(nu, 18)
    it[1:, :5] = rng.rand(ni, 5); it[1:, 5:] = genres
    store.load_arrays(ut, it)
    return model, index, ranker, store


def _served_rows(pipe, users):
    """(uid, cand, X) of the chain's ranking stage for these users, from a synchronous search"""
    from recommendit_amd.recommender import build_ranking_features_device
    uid = torch.as_tensor(users, dtype=torch.long, device=_dev())
    q = pipe.model.get_user_embeddings(uid, as_tensor=True)
    _, cand = pipe.index.batch_search_device(q, k=pipe.top_k_candidates, normalized=True)
    X = build_ranking_features_device(pipe.store, uid, cand, pipe.ranker.feature_names)
    kc = cand.shape[1]
    return (uid.repeat_interleave(kc).cpu().numpy(), cand.reshape(-1).cpu().numpy(), X.cpu().numpy())


def _ring(pipe):
    ring, ru, ri, cur = pipe._log
    o = pipe._log_order()
    return ru[o].cpu().numpy(), ri[o].cpu().numpy(), ring[o].cpu().numpy(), int(cur[0].item())


def test_feature_log_outputs_rows_and_wraparound(tmp_path):
    from recommendit_amd.recommender import GpuRecommendationPipeline
    model, index, ranker, store = _pipeline_parts(tmp_path)
    off = GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=300, top_k_results=10)
    on = GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=300, top_k_results=10,
                                   feature_log_rows=100_000)
    assert off.feature_log_rows == 0 and off._log is None
    batches = [list(range(1, 257)), [7], list(range(300, 340)), [3, 5, 5, 9]]
    for users in batches:
        a = off.recommend_batch(users)
        b = on.recommend_batch(users)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    want = [_served_rows(on, u) for u in batches]
    wu, wi, wx = (np.concatenate([w[j] for w in want]) for j in range(3))
    ru, ri, rx, cur = _ring(on)
    assert cur == len(wu) == sum(len(u) for u in batches) * 300
    np.testing.assert_array_equal(ru, wu)
    np.testing.assert_array_equal(ri, wi)
    np.testing.assert_array_equal(rx, wx)
    sf = on.serving_features()
    keep = wi >= 0
    assert list(sf.columns) == ["user_id", "item_id"] + list(ranker.feature_names)
    np.testing.assert_array_equal(sf["item_id"].to_numpy(), wi[keep])
    np.testing.assert_array_equal(sf[list(ranker.feature_names)].to_numpy(), wx[keep])
    # wrap-around: a ring smaller than a batch keeps the newest rows, across batches too
    on.reset_feature_log(1000)
    assert on.feature_log_rows == 1000
    on.recommend_batch(batches[0])
    ru, ri, rx, cur = _ring(on)
    w = _served_rows(on, batches[0])
    np.testing.assert_array_equal(ri, w[1][-1000:])
    np.testing.assert_array_equal(rx, w[2][-1000:])
    on.recommend_batch(batches[3])        # 1 200 rows: wraps again
    on.recommend_batch(batches[1])        # 300 rows
    ru, ri, rx, cur = _ring(on)
    ws = [_served_rows(on, batches[3]), _served_rows(on, batches[1])]
    np.testing.assert_array_equal(ru, np.concatenate([x[0] for x in ws])[-1000:])
    np.testing.assert_array_equal(ri, np.concatenate([x[1] for x in ws])[-1000:])
    np.testing.assert_array_equal(rx, np.concatenate([x[2] for x in ws])[-1000:])
    on.reset_feature_log()
    assert len(on.serving_features()) == 0


def test_feature_log_graph_replay_logs_and_warmups_do_not(tmp_path):
    from recommendit_amd.recommender import GpuRecommendationPipeline
    model, index, ranker, store = _pipeline_parts(tmp_path)
    pipe = GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=300, top_k_results=10,
                                     feature_log_rows=50_000)
    ref = GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=300, top_k_results=10)
    e = ref.get_recommendations(7)
    assert pipe.get_recommendations(7, graph=True) == e          # capture (2 warm-ups + capture) + one replay
    assert pipe.get_recommendations(9, graph=True) == ref.get_recommendations(9)
    ru, ri, rx, cur = _ring(pipe)
    w = [_served_rows(pipe, [7]), _served_rows(pipe, [9])]
    assert cur == 600
    np.testing.assert_array_equal(ru, np.concatenate([x[0] for x in w]))
    np.testing.assert_array_equal(ri, np.concatenate([x[1] for x in w]))
    np.testing.assert_array_equal(rx, np.concatenate([x[2] for x in w]))
    # a resized ring is a new buffer: the graph is captured again and logs into it
    key_state = pipe._graph_state()
    pipe.reset_feature_log(4000)
    assert pipe._graph_state() != key_state
    assert pipe.get_recommendations(7, graph=True) == e
    ru, ri, rx, cur = _ring(pipe)
    assert cur == 300
    np.testing.assert_array_equal(rx, w[0][2])


def test_feature_log_deferred_redo_logs_each_batch_once():
    """A tied-row corpus: 6 000 index rows equal to one user's query overflow the thresholded pass's candidate lists,
    so the deferred exactness check re-does queries and the chain runs again; the batch must be logged once, with
    its final candidates."""
    from recommendit_amd import FAISSIndex, LightGBMRanker, TwoTowerModel
    from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns
    import tempfile
    from pathlib import Path
    nu, N, d, H = 700, 300_000, 128, 128
    sd = fx.make_state(nu, 50, d, H, seed=5)
    model = TwoTowerModel(nu, 50, d, H)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    dev = _dev()
    users = list(range(1, 601))
    U = model.get_user_embeddings(torch.as_tensor(users, device=dev), as_tensor=True).float().cpu().numpy()
    rng = np.random.RandomState(5)
    X = fx.unit_rows(rng, N, d)
    X[:6000] = U[0]
    index = FAISSIndex(embed_dim=d, n_lists=100, n_probe=10)
    index.build_from_device(torch.from_numpy(X).to(dev), np.arange(1, N + 1))
    with tempfile.TemporaryDirectory() as td:
        fp = Path(td) / "r.lgbm"
        fp.write_text(G.write_text_model(G.random_forest_model(40, 15, 50, seed=2, names=feature_columns())))
        ranker = LightGBMRanker.load(str(fp))
    store = GpuFeatureStore(nu, N)
    pipe = GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=500, top_k_results=20,
                                     feature_log_rows=2 * 600 * 500)
    redone = []
    finish = index.finish_search

    def spy():
        n = finish()
        redone.append(n)
        return n
    index.finish_search = spy
    out = pipe.recommend_batch(users)
    index.finish_search = finish
    assert redone and redone[0] > 0, redone              # the re-do path ran
    ru, ri, rx, cur = _ring(pipe)
    assert cur == 600 * 500                               # logged once
    w = _served_rows(pipe, users)                         # synchronous search: the final candidates
    np.testing.assert_array_equal(ri, w[1])
    np.testing.assert_array_equal(rx, w[2])
    ref = GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=500, top_k_results=20)
    for x, y in zip(out, ref.recommend_batch(users)):
        assert torch.equal(x, y)


def test_feature_log_forced_redo_rewinds(tmp_path):
    """the re-do branch on a small corpus: a finish_search that reports re-done queries makes the chain run twice;
    the rewind keeps one copy of the batch"""
    from recommendit_amd.recommender import GpuRecommendationPipeline
    model, index, ranker, store = _pipeline_parts(tmp_path)
    pipe = GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=300, top_k_results=10,
                                     feature_log_rows=10_000)
    finish = index.finish_search
    index.finish_search = lambda: (finish(), 1)[1]
    try:
        pipe.recommend_batch([4, 8])
        pipe.recommend_batch([11])
    finally:
        index.finish_search = finish
    ru, ri, rx, cur = _ring(pipe)
    assert cur == 900
    w = [_served_rows(pipe, [4, 8]), _served_rows(pipe, [11])]
    np.testing.assert_array_equal(ru, np.concatenate([x[0] for x in w]))
    np.testing.assert_array_equal(rx, np.concatenate([x[2] for x in w]))


def test_detect_skew_on_the_ring_equals_host(tmp_path):
    from recommendit_amd.recommender import GpuRecommendationPipeline, build_ranking_features_device
    model, index, ranker, store = _pipeline_parts(tmp_path)
    pipe = GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=300, top_k_results=10,
                                     feature_log_rows=30_000)
    for users in (list(range(1, 65)), list(range(100, 140))):
        pipe.recommend_batch(users)
    # training rows: random (user, item) pairs through the same feature builder, with NaN holes and a shifted column
    rng = np.random.default_rng(1)
    dev = _dev()
    uid = torch.as_tensor(rng.integers(1, 401, 200), device=dev)
    cand = torch.as_tensor(rng.integers(1, 6001, (200, 40)), device=dev)
    Xt = build_ranking_features_device(store, uid, cand, ranker.feature_names).cpu().numpy().astype(np.float64)
    train = pd.DataFrame(Xt, columns=list(ranker.feature_names))
    train.insert(0, "item_id", cand.reshape(-1).cpu().numpy())
    train.insert(0, "user_id", uid.repeat_interleave(40).cpu().numpy())
    train.iloc[::7, 5] = np.nan
    train["genre_affinity"] = train["genre_affinity"] * 1.7 + 0.1
    train["label"] = rng.integers(0, 2, len(train))       # a column serving does not have
    serving = pipe.serving_features()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host = M.detect_training_serving_skew(train, serving)
        raw = {c: M.kl_divergence_bins(train[c].dropna().values.astype(float), serving[c].dropna().values.astype(float))
               for c in host["feature_kl"]}
    got = pipe.detect_skew(train)
    assert host["n_features_checked"] == 52
    assert_skew_dict(got, host, raw)
    sub = ["item_id", "genre_affinity", "avg_rating"]
    assert_skew_dict(pipe.detect_skew(train, threshold=0.05, numeric_cols=sub),
                     M.detect_training_serving_skew(train, serving, threshold=0.05, numeric_cols=sub), raw)
