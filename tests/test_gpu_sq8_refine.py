"""GPU: the SQ8 index's refined search (rihip_sq8_refine_*: attach_vectors, search, the certificate) against its NumPy restatement
(tests/sq8_refine_reference.py).  On inputs whose f32 arithmetic is exact everything is compared bit for bit; on random
unit vectors f itself is compared bit for bit with the header's definition, every certified query with the brute force
over its probed lists, and every score with the float64 product.  tests/test_sq8_refine_host.py shows on the same
inputs that the reference certifies queries, so "every certified query" is not an empty set."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_reference as S  # noqa: E402
import sq8_refine_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

N, NQ, NLIST, NPROBE = 20000, 70, 8, 3
KS, FACTORS = (1, 10, 100), (1, 1.5, 4)
MAX_K = 16384


def _source(X, ivf, seed, ids=None, assign=None):
    from recommendit_amd import FAISSIndex
    ids = np.arange(X.shape[0]) if ids is None else ids
    x_dev = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    if not ivf:
        idx = FAISSIndex(embed_dim=X.shape[1], exact=True)
        idx.build_from_device(x_dev, ids)
        return idx, None, None
    C, a = R.ivf_layout(seed, X.shape[0], X.shape[1], NLIST)
    assign = a if assign is None else assign
    idx = FAISSIndex(embed_dim=X.shape[1], n_lists=NLIST, n_probe=NPROBE)
    idx.build_from_device(x_dev, ids, centroids=C, assign=assign)
    return idx, C, assign


_cases = {}


def _case(kind, d, ivf):
    """one index per (inputs, width, layout), built once: dict(sq, src, X, Q, codes, m, s, allowed, ea)"""
    key = (kind, d, ivf)
    if key not in _cases:
        from recommendit_amd import SQ8Index
        rows = R.dyadic_rows if kind == "exact" else R.unit_rows
        X, Q = rows(100 + d, N, d), rows(200 + d, NQ, d)
        src, C, assign = _source(X, ivf, 300 + d)
        sq = SQ8Index.from_index(src, keep_vectors=True)
        m, s = sq.quantizer()
        codes = sq.codes()
        allowed = R.probe_mask(Q, C, assign, NPROBE) if ivf else None
        _cases[key] = dict(sq=sq, src=src, X=X, Q=Q, qd=torch.from_numpy(Q).cuda(), codes=codes, m=m, s=s, allowed=allowed,
                           ea=R.ranges(X, codes, m, s))
    return _cases[key]


def _k_scan(k, factor):
    return min(max(k, int(math.ceil(factor * k))), MAX_K)


def _refined(sq, qd, k, factor, mode="auto"):
    out = sq.search_rows_device(qd, k, mode=mode, refine=factor, return_cert=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


GRID = [(d, ivf) for d in (40, 128) for ivf in (False, True)]
GRID_IDS = [f"d{d}-{'ivf' if ivf else 'flat'}" for d, ivf in GRID]


# ---- 1. exact inputs: bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ivf", GRID, ids=GRID_IDS)
def test_exact_inputs_bit_for_bit(d, ivf):
    c = _case("exact", d, ivf)
    sq = c["sq"]
    assert sq.has_vectors and sq.stats()["has_vectors"] is True and sq.stats()["refine"] is None
    e, a = sq.refine_ranges()
    np.testing.assert_array_equal(e, c["ea"][0])
    np.testing.assert_array_equal(a, c["ea"][1])
    some_cert = 0
    for k in KS:
        for factor in FACTORS:
            want = R.refine(c["Q"], c["X"], c["codes"], c["m"], c["s"], k, _k_scan(k, factor), c["allowed"], c["ea"])
            # on these inputs f is the float64 product, exactly
            ok = want["rows"] >= 0
            qi = np.nonzero(ok)[0]
            prod = np.einsum("ij,ij->i", c["Q"][qi].astype(np.float64), c["X"][want["rows"][ok]].astype(np.float64))
            np.testing.assert_array_equal(want["scores"][ok].astype(np.float64), prod)
            for mode in ("dense", "thresholded"):
                gs, gr, gc, gb = _refined(sq, c["qd"], k, factor, mode)
                assert gs.dtype == np.float32 and gr.dtype == np.int64 and gc.dtype == np.uint8 and gb.dtype == np.float64
                np.testing.assert_array_equal(gr, want["rows"])
                np.testing.assert_array_equal(gs.view(np.uint32), want["scores"].view(np.uint32))
                np.testing.assert_array_equal(gc, want["cert"])
                np.testing.assert_allclose(gb, want["bound"], rtol=1e-12, atol=0)
            some_cert += int(want["cert"].sum())
    assert some_cert > 0


# ---- 2. soundness on random unit vectors ---------------------------------------------------------------------------
@pytest.mark.parametrize("d,ivf", GRID, ids=GRID_IDS)
def test_certified_queries_equal_the_brute_force(d, ivf):
    c = _case("unit", d, ivf)
    sq, Q, X = c["sq"], c["Q"], c["X"]
    P, AP = R.f64(Q, X), R.abs_dot(Q, X)
    certified = 0
    for k in KS:
        bf_rows, bf_scores = R.brute_force(Q, X, k, c["allowed"])
        for factor in FACTORS:
            gs, gr, gc, gb = _refined(sq, c["qd"], k, factor)
            ok = gc == 1
            certified += int(ok.sum())
            print(f"d={d} ivf={ivf} k={k} factor={factor}: certified {int(ok.sum())}/{NQ}, mean bound {gb.mean():.3e}")
            np.testing.assert_array_equal(gr[ok], bf_rows[ok])
            np.testing.assert_array_equal(gs[ok].view(np.uint32), bf_scores[ok].view(np.uint32))
            valid = gr >= 0
            assert valid.all()
            qi = np.broadcast_to(np.arange(NQ)[:, None], gr.shape)
            err = np.abs(gs.astype(np.float64) - P[qi, gr])
            assert (err <= R.gamma(d) * AP[qi, gr]).all()
            # f, the select and the certificate as the header states them, for every query
            want = R.refine(Q, X, c["codes"], c["m"], c["s"], k, _k_scan(k, factor), c["allowed"], c["ea"])
            np.testing.assert_array_equal(gr, want["rows"])
            np.testing.assert_array_equal(gs.view(np.uint32), want["scores"].view(np.uint32))
            np.testing.assert_array_equal(gc, want["cert"])
            np.testing.assert_allclose(gb, want["bound"], rtol=1e-12, atol=0)
    assert certified > 0


# ---- 3. the two ends of the factor ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ivf", [(40, True), (128, False)], ids=["d40-ivf", "d128-flat"])
def test_factor_one_reorders_the_plain_search(d, ivf):
    c = _case("unit", d, ivf)
    sq = c["sq"]
    for k in KS:
        ps, pr = [t.cpu().numpy() for t in sq.search_rows_device(c["qd"], k, refine=None)]
        gs, gr, gc, _ = _refined(sq, c["qd"], k, 1)
        np.testing.assert_array_equal(np.sort(gr, axis=1), np.sort(pr, axis=1))
        for q in range(NQ):
            f = R.f32_exact(np.broadcast_to(c["Q"][q], (k, d)), c["X"][pr[q]])
            order = np.lexsort((pr[q], -f))
            np.testing.assert_array_equal(gr[q], pr[q][order])
            np.testing.assert_array_equal(gs[q], f[order])


def test_k_scan_beyond_the_probed_rows_certifies_everything():
    c = _case("unit", 40, True)
    probed = c["allowed"].sum(axis=1)
    assert probed.max() < MAX_K and probed.min() > 100
    gs, gr, gc, _ = _refined(c["sq"], c["qd"], 100, 1000.0)          # k_scan = the select buffer: more than any query probes
    assert (gc == 1).all()
    bf_rows, bf_scores = R.brute_force(c["Q"], c["X"], 100, c["allowed"])
    np.testing.assert_array_equal(gr, bf_rows)
    np.testing.assert_array_equal(gs, bf_scores)
    # fewer rows than k: padding
    from recommendit_amd import SQ8Index
    X = R.unit_rows(7, 50, 40)
    src, _, _ = _source(X, False, 0)
    small = SQ8Index.from_index(src, keep_vectors=True)
    for factor in (1, 3):
        gs, gr, gc, _ = _refined(small, c["qd"], 100, factor)
        bf_rows, bf_scores = R.brute_force(c["Q"], X, 50)
        np.testing.assert_array_equal(gr[:, :50], bf_rows)
        np.testing.assert_array_equal(gs[:, :50], bf_scores)
        assert (gr[:, 50:] == -1).all() and np.isneginf(gs[:, 50:]).all() and (gc == 1).all()


# ---- 4. recall never below the plain search's ----------------------------------------------------------------------
@pytest.mark.parametrize("d,ivf", GRID, ids=GRID_IDS)
def test_recall_against_the_f32_index(d, ivf):
    c = _case("exact", d, ivf)
    sq, src = c["sq"], c["src"]
    for k in (10, 100):
        ts, truth = [t.cpu().numpy() for t in src.batch_search_device(c["qd"], k, normalized=True)]
        src.finish_search()
        for factor in FACTORS:
            k_scan = _k_scan(k, factor)
            _, cand = [t.cpu().numpy() for t in sq.batch_search_device(c["qd"], k_scan, normalized=True, refine=None)]
            _, ref = [t.cpu().numpy() for t in sq.batch_search_device(c["qd"], k, normalized=True, refine=factor)]
            for q in range(NQ):
                t = set(truth[q].tolist())
                assert set(ref[q].tolist()) & t == set(cand[q].tolist()) & t          # the identity
                assert len(set(ref[q].tolist()) & t) >= len(set(cand[q, :k].tolist()) & t)


# ---- 5. attach / drop / persistence --------------------------------------------------------------------------------
def test_attach_refusals_drop_and_persistence(tmp_path):
    from recommendit_amd import SQ8Index
    n, d = 3000, 40
    X, Q = R.dyadic_rows(11, n, d), R.dyadic_rows(12, 20, d)
    qd = torch.from_numpy(Q).cuda()
    src, C, assign = _source(X, True, 13)
    sq = SQ8Index.from_index(src, keep_vectors=True)
    plain = SQ8Index.from_index(src)
    assert plain.has_vectors is False and plain.stats()["has_vectors"] is False
    extra = 4 * n * 64 + 2 * 8 * 64
    assert sq.stats()["device_bytes"] == plain.stats()["device_bytes"] + extra
    want = _refined(sq, qd, 10, 2)
    e0 = sq.refine_ranges()

    # the same list lengths with other rows in the lists: only the device comparison of the row ids can see it
    other_assign = np.roll(assign, 1)
    assert (np.bincount(other_assign, minlength=NLIST) == np.bincount(assign, minlength=NLIST)).all()
    other_order, _, _ = _source(X, True, 13, assign=other_assign)
    flat, _, _ = _source(X, False, 0)                                               # one list instead of eight
    shorter, _, _ = _source(X[:-1], True, 13, assign=assign[:-1])                   # another size
    wider, _, _ = _source(R.dyadic_rows(11, n, 64), True, 13, assign=assign)        # another width
    updated, _, _ = _source(X, True, 13)
    updated.add_items(R.unit_rows(14, 3, d), [n + 5, n + 6, n + 7])
    for bad in (other_order, flat, shorter, wider, updated):
        with pytest.raises(RuntimeError, match="attach_vectors"):
            sq.attach_vectors(bad)
        assert sq.has_vectors
        for a, b in zip(want, _refined(sq, qd, 10, 2)):                             # the handle is as it was
            np.testing.assert_array_equal(a, b)
        with pytest.raises(RuntimeError, match="attach_vectors"):
            plain.attach_vectors(bad)
        assert plain.has_vectors is False
    # a flat index takes its flat source
    flat_sq = SQ8Index.from_index(flat)
    flat_sq.attach_vectors(flat)
    assert flat_sq.has_vectors
    np.testing.assert_array_equal(flat_sq.refine_ranges()[1], np.abs(X).max(axis=0).astype(np.float64))

    # drop: refine raises again, the plain search is untouched
    sq.set_refine(2)
    assert sq.stats()["refine"] == 2.0
    sq.drop_vectors()
    assert sq.has_vectors is False and sq.stats()["device_bytes"] == plain.stats()["device_bytes"]
    for call in (lambda: sq.batch_search_device(qd, 10, normalized=True), lambda: sq.search_rows_device(qd, 10, refine=1.5),
                 lambda: sq.search_certified(qd, 10), sq.refine_ranges):
        with pytest.raises(RuntimeError, match="vectors"):
            call()
    sq.set_refine(None)
    for a, b in zip(sq.batch_search_device(qd, 10, normalized=True, return_int=True),
                    plain.batch_search_device(qd, 10, normalized=True, return_int=True)):
        assert torch.equal(a, b)
    sq.attach_vectors(src)
    for a, b in zip(want, _refined(sq, qd, 10, 2)):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(e0, sq.refine_ranges()):
        np.testing.assert_array_equal(a, b)

    # save / load: the file is the plain index's, byte for byte, and loads without vectors
    pa, pb = tmp_path / "with.sq8", tmp_path / "without.sq8"
    sq.save(str(pa))
    plain.save(str(pb))
    raw = pa.read_bytes()
    assert raw == pb.read_bytes()
    hdr = np.frombuffer(raw[8:72], dtype=np.int64)
    Np = int(hdr[5])
    assert raw[:8] == b"RIHIPSQ8" and hdr[0] == 1 and len(raw) == 72 + 8 * 64 + 4 * NLIST * 64 + 8 * NLIST + 8 * Np + Np * 64
    back = SQ8Index.load(str(pa))
    assert back.has_vectors is False and back.stats()["refine"] is None
    with pytest.raises(RuntimeError, match="vectors"):
        back.search_rows_device(qd, 10, refine=2)
    back.attach_vectors(src)
    for a, b in zip(want, _refined(back, qd, 10, 2)):
        np.testing.assert_array_equal(a, b)

    # argument errors at the search
    for bad in (0.5, float("nan"), float("inf"), "2"):
        with pytest.raises(ValueError, match="refine"):
            sq.search_rows_device(qd, 10, refine=bad)
    with pytest.raises(ValueError, match="return_cert"):
        sq.search_rows_device(qd, 10, refine=None, return_cert=True)
    with pytest.raises(ValueError, match="return_int"):
        sq.search_rows_device(qd, 10, refine=2, return_int=True)


# ---- 6. opt-in: nothing changes without it; the serve chain --------------------------------------------------------
def test_unrefined_bytes_are_the_plain_index_s():
    from recommendit_amd import SQ8Index
    c = _case("unit", 40, True)
    plain = SQ8Index.from_index(c["src"])
    kept = c["sq"]
    kept.set_refine(3)
    kept.set_refine(None)
    for mode in ("auto", "dense", "thresholded"):
        a = plain.batch_search_device(c["qd"], 100, normalized=True, mode=mode, return_int=True)
        b = kept.batch_search_device(c["qd"], 100, normalized=True, mode=mode, return_int=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    hs, hi = kept.batch_search(c["Q"], k=10)
    ps, pi = plain.batch_search(c["Q"], k=10)
    np.testing.assert_array_equal(hs, ps)
    np.testing.assert_array_equal(hi, pi)
    # the host entries take refine= too
    rs, ri, rc, rb = kept.batch_search(c["Q"], k=10, refine=4, return_cert=True)
    Qn = c["Q"] / np.maximum(np.linalg.norm(c["Q"], axis=1, keepdims=True), 1e-8)   # as batch_search normalises
    out = kept.batch_search_device(torch.from_numpy(np.ascontiguousarray(Qn)).cuda(), 10, normalized=True, refine=4, return_cert=True)
    for x, y in zip((rs, ri, rc, rb), out):
        np.testing.assert_array_equal(x, y.cpu().numpy())
    assert rc.dtype == np.uint8 and rb.dtype == np.float64 and rs.shape == (NQ, 10)
    one_s, one_i = kept.search(c["Q"][3], k=10, refine=4)
    np.testing.assert_array_equal(one_i, ri[3])


def test_pipeline_over_a_refining_sq8_index_equals_its_stages_run_by_hand(tmp_path):
    from oracle import fixtures as fx
    from oracle import gbdt_np as G
    from recommendit_amd import FAISSIndex, LightGBMRanker, SQ8Index, TwoTowerModel
    from recommendit_amd import _lib as L
    from recommendit_amd.recommender import (GpuFeatureStore, GpuRecommendationPipeline, build_ranking_features_device,
                                             feature_columns)
    nu, ni, d, H, kc, k = 120, 900, 64, 128, 100, 10
    sd = fx.make_state(nu, ni, d, H, seed=21)
    model = TwoTowerModel(nu, ni, d, H)
    model.load_state_dict({key: torch.from_numpy(v.copy()) for key, v in sd.items()})
    rng = np.random.RandomState(2)
    item_ids = list(range(1, ni + 1))
    genres = (rng.rand(ni, 18) < 0.15).astype(np.float32)
    E = model.get_item_embeddings(item_ids, genres)
    src = FAISSIndex(embed_dim=d, n_lists=6, n_probe=2)
    src.build_ivf_index(E, item_ids)
    sq = SQ8Index.from_index(src, keep_vectors=True)
    del src
    sq.set_refine(2.0)
    forest = G.random_forest_model(30, 15, 50, seed=5, names=feature_columns())
    p = tmp_path / "r.lgbm"
    p.write_text(G.write_text_model(forest))
    ranker = LightGBMRanker.load(str(p))
    store = GpuFeatureStore(nu, ni)
    ut, it = store.user.copy(), store.item.copy()
    ut[1:, :6] = rng.rand(nu, 6) * [5, 8, 1, 1, 1, 1]; ut[1:, 6:] = rng.rand(nu, 18)
    it[1:, :5] = rng.rand(ni, 5) * [5, 9, 1, 1.5, 1]; it[1:, 5:] = genres
    store.load_arrays(ut, it)
    pipe = GpuRecommendationPipeline(model, sq, ranker, store, top_k_candidates=kc, top_k_results=k)
    users = [1, 7, 120, 42, 3]
    ids, sc, rs = pipe.recommend_batch(users)
    uid = torch.tensor(users, dtype=torch.long, device="cuda")
    q = model.get_user_embeddings(uid, as_tensor=True)
    r_s, cand = sq.batch_search_device(q, k=kc, normalized=True, refine=2.0)       # what the sticky factor stands for
    p_s, _ = sq.batch_search_device(q, k=kc, normalized=True, refine=None)
    assert not torch.equal(r_s, p_s)                                               # f32 scores, not quantised ones
    rows = torch.clamp(cand - 1, min=0)
    exact = (q[:, None, :].double() * torch.from_numpy(E / np.linalg.norm(E, axis=1, keepdims=True)).cuda()[rows].double()).sum(-1)
    assert ((r_s.double() - exact).abs()[cand >= 0] < 1e-5).all()
    Xf = build_ranking_features_device(store, uid, cand, ranker.feature_names)
    scores = ranker.predict_device(Xf)
    h_ids = torch.empty((len(users), k), dtype=torch.int64, device="cuda")
    h_top = torch.empty((len(users), k), dtype=torch.float64, device="cuda")
    h_rs = torch.empty((len(users), k), dtype=torch.float32, device="cuda")
    L.check(L.lib().rihip_rank_topk(scores.data_ptr(), cand.data_ptr(), r_s.data_ptr(), len(users), kc, k, h_ids.data_ptr(),
                                    h_top.data_ptr(), h_rs.data_ptr(), L.stream_ptr()), "rank_topk")
    torch.cuda.synchronize()
    assert torch.equal(ids, h_ids) and torch.equal(sc, h_top) and torch.equal(rs, h_rs)
    with pytest.raises(ValueError, match="SQ8"):                                   # the refusals stay
        pipe.recommend_batch(users, graph=True)


# ---- 7. search_certified -------------------------------------------------------------------------------------------
def test_search_certified_ends_certified_and_exact():
    from recommendit_amd import SQ8Index
    X, Q = R.unit_rows(0, 20000, 64), R.unit_rows(1, 64, 64)
    src, _, _ = _source(X, False, 0)
    sq = SQ8Index.from_index(src, keep_vectors=True)
    qd = torch.from_numpy(Q).cuda()
    _, _, c1, _ = _refined(sq, qd, 10, 1)
    assert (c1 == 0).all()                                   # factor 1 certifies nothing here: the loop has work to do
    s, ids, cert = sq.search_certified(qd, 10, start=1.0, normalized=True)
    torch.cuda.synchronize()
    assert cert.dtype == torch.uint8 and bool((cert == 1).all())
    bf_rows, bf_scores = R.brute_force(Q, X, 10)
    np.testing.assert_array_equal(ids.cpu().numpy(), bf_rows)
    np.testing.assert_array_equal(s.cpu().numpy(), bf_scores)
    with pytest.raises(ValueError, match="refine"):
        sq.search_certified(qd, 10, start=0.5)
