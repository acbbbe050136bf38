"""Host: the diversified top-k (greedy MMR) -- properties of the definition on its NumPy reference (tests/mmr_reference.py),
the reference's two forms against each other, and the argument checks of the Python layer that need no device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmr_reference as M  # noqa: E402


def _mixed_case(rng, nq, kc, w, n_rows, ld, col0):
    """scores with repeats, signed zeros, NaN and infinities; ids with padding inside and at the tail, some beyond the
    table; vectors with zero rows and duplicates"""
    V = np.zeros((n_rows, ld), dtype=np.float64)
    V[:, col0:col0 + w] = rng.standard_normal((n_rows, w)) * (rng.random((n_rows, w)) < 0.6)
    V[::7, col0:col0 + w] = 0.0
    V[3::11, col0:col0 + w] = V[5, col0:col0 + w]
    V[:, :col0] = 9.0
    V[:, col0 + w:] = -9.0
    s = np.round(rng.standard_normal((nq, kc)), 1)
    s[rng.random((nq, kc)) < 0.05] = np.nan
    s[rng.random((nq, kc)) < 0.03] = -0.0
    s[rng.random((nq, kc)) < 0.03] = 0.0
    s[rng.random((nq, kc)) < 0.02] = np.inf
    s[rng.random((nq, kc)) < 0.02] = -np.inf
    c = np.stack([rng.permutation(n_rows + 20)[:kc] for _ in range(nq)]).astype(np.int64)
    c[rng.random((nq, kc)) < 0.08] = -1
    for q in range(nq):
        c[q, kc - q % 4:] = -1
    r = rng.standard_normal((nq, kc)).astype(np.float32)
    return s, c, r, V


def test_delta_zero_is_the_sort():
    rng = np.random.default_rng(1)
    for kc, k in ((1, 1), (17, 5), (64, 64), (90, 120)):
        s, c, r, V = _mixed_case(rng, 6, kc, 18, 300, 25, 4)
        got = M.mmr_reference(s, c, r, k, 0.0, V, 4, 18)
        exp = M.plain_topk(s, c, r, k)
        for g, e in zip(got, exp):
            np.testing.assert_array_equal(g, e)          # NaN == NaN here, and the bit patterns of +-0 are checked next
        assert np.array_equal(np.signbit(got[1]), np.signbit(exp[1]))
    # normalisation collapses neighbouring doubles: the raw score still decides
    s = np.array([[1.0, np.nextafter(1.0, 2.0), 0.0, 1e300]])
    c = np.arange(4, dtype=np.int64)[None]
    ids, _, _ = M.mmr_reference(s, c, np.zeros((1, 4), np.float32), 4, 0.0, np.ones((4, 2)))
    assert ids.tolist() == [[3, 1, 0, 2]]


def test_delta_one_first_pick_is_the_best_score():
    rng = np.random.default_rng(2)
    s, c, r, V = _mixed_case(rng, 8, 50, 18, 200, 18, 0)
    ids, sc, _ = M.mmr_reference(s, c, r, 10, 1.0, V)
    plain = M.plain_topk(s, c, r, 10)
    assert np.array_equal(ids[:, 0], plain[0][:, 0])
    assert np.array_equal(sc[:, 0], plain[1][:, 0], equal_nan=True)


def test_nan_and_padding_come_last_in_retrieval_order():
    s = np.array([[0.5, np.nan, 0.1, 0.9, np.nan, 0.2, 0.3]])
    c = np.array([[4, 5, -1, 6, 7, -1, 8]], dtype=np.int64)
    r = np.arange(7, dtype=np.float32)[None]
    V = np.eye(10)
    for delta in (0.0, 0.4, 1.0):
        ids, sc, rs = M.mmr_reference(s, c, r, 9, delta, V)
        assert sorted(ids[0, :3].tolist()) == [4, 6, 8] and ids[0, 0] == 6
        assert ids[0, 3:].tolist() == [5, 7, -1, -1, -1, -1]
        assert np.isnan(sc[0, 3:5]).all() and (sc[0, 5:] == -np.inf).all()
        assert rs[0, 3:7].tolist() == [1.0, 4.0, 2.0, 5.0] and (rs[0, 7:] == -np.inf).all()


def test_vectorised_reference_equals_the_scalar_loops():
    rng = np.random.default_rng(3)
    for (nq, kc, k, w, n_rows, ld, col0) in ((4, 1, 1, 18, 40, 18, 0), (4, 37, 12, 18, 60, 23, 5), (2, 64, 64, 7, 50, 9, 1),
                                             (2, 70, 20, 128, 90, 130, 2)):
        s, c, r, V = _mixed_case(rng, nq, kc, w, n_rows, ld, col0)
        for delta in (0.0, 0.3, 0.7, 1.0):
            a = M.mmr_reference(s, c, r, k, delta, V, col0, w, row=M.mmr_row_scalar)
            b = M.mmr_reference(s, c, r, k, delta, V, col0, w)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
    s = np.zeros((1, 6)); c = np.arange(6, dtype=np.int64)[None]; r = np.zeros((1, 6), np.float32)   # everything ties
    for row in (M.mmr_row, M.mmr_row_scalar):
        assert M.mmr_reference(s, c, r, 6, 0.5, np.zeros((6, 3)), row=row)[0].tolist() == [[0, 1, 2, 3, 4, 5]]


def _taste_case(seed=0, n_items=6000, n_genres=18, kc=200, nq=32):
    """the fixed synthetic case: binary genre vectors with 1-3 genres per item; per request a random candidate set and
    score = affinity to a Dirichlet(0.3) taste vector + 0.1 N(0, 1)"""
    rng = np.random.default_rng(seed)
    G = np.zeros((n_items, n_genres))
    for i in range(n_items):
        G[i, rng.choice(n_genres, size=rng.integers(1, 4), replace=False)] = 1.0
    cand = np.stack([rng.choice(n_items, size=kc, replace=False) for _ in range(nq)]).astype(np.int64)
    taste = rng.dirichlet(np.full(n_genres, 0.3), size=nq)
    scores = np.einsum("qcg,qg->qc", G[cand], taste) + 0.1 * rng.standard_normal((nq, kc))
    rs = rng.random((nq, kc)).astype(np.float32)
    return scores, cand, rs, G


def test_diversity_changes_every_list_and_raises_the_metric():
    scores, cand, rs, G = _taste_case()
    plain = M.plain_topk(scores, cand, rs, 20)[0]
    assert np.array_equal(M.mmr_reference(scores, cand, rs, 20, 0.0, G)[0], plain)
    base = np.mean([M.intra_list_diversity(row, G) for row in plain])
    prev = base
    for delta in (0.1, 0.3, 0.5):
        ids = M.mmr_reference(scores, cand, rs, 20, delta, G)[0]
        assert all(not np.array_equal(ids[q], plain[q]) for q in range(ids.shape[0])), delta
        assert (ids[:, 0] == plain[:, 0]).all()
        div = np.mean([M.intra_list_diversity(row, G) for row in ids])
        print(f"delta {delta}: mean intra-list diversity {base:.3f} -> {div:.3f}")
        assert div > prev, (delta, div, prev)            # rises with the weight, from the plain top-20 on
        prev = div


def test_project_metric_agrees_with_the_helper():
    from recommendit_amd.metrics import intra_list_diversity
    scores, cand, rs, G = _taste_case(nq=2)
    ids = M.plain_topk(scores, cand, rs, 20)[0]
    vecs = {i: G[i] for i in range(G.shape[0])}
    for row in ids:
        assert abs(intra_list_diversity(row.tolist(), vecs) - M.intra_list_diversity(row, G)) < 1e-12


# ---- argument checks of the Python layer: nothing here reaches the device ------------------------------------------------
def test_value_errors_without_a_device():
    from recommendit_amd import mmr_rerank_device
    from recommendit_amd import rerank as RR
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            RR.check_diversity(bad)
    assert RR.check_diversity(0) == 0.0 and RR.check_diversity(1) == 1.0 and RR.check_diversity(np.float32(0.5)) == 0.5
    for kc, k, w in ((0, 1, 18), (4097, 1, 18), (10, 0, 18), (10, -3, 18), (10, 1, 0), (10, 1, 257)):
        with pytest.raises(ValueError):
            RR.check_shape(kc, k, w)
    RR.check_shape(1, 1, 1)
    RR.check_shape(4096, 10 ** 6, 256)

    def call(kc=8, k=3, d=0.3, vec=None, col0=0, width=None, rs_cols=None):
        s = torch.zeros((2, kc), dtype=torch.float64)
        c = torch.zeros((2, kc), dtype=torch.int64)
        r = torch.zeros((2, kc if rs_cols is None else rs_cols), dtype=torch.float32)
        v = torch.zeros((5, 18), dtype=torch.float64) if vec is None else vec
        return mmr_rerank_device(s, c, r, k, d, v, col0, width)

    for kw in (dict(d=1.5), dict(d=float("nan")), dict(d=-1), dict(k=0), dict(kc=4097), dict(kc=0),
               dict(vec=torch.zeros((5, 257), dtype=torch.float64)), dict(vec=torch.zeros((5, 18))),
               dict(vec=torch.zeros((18,), dtype=torch.float64)), dict(col0=18), dict(col0=-1), dict(col0=4, width=15),
               dict(width=0), dict(vec=torch.zeros((5, 36), dtype=torch.float64)[:, ::2]), dict(rs_cols=7)):
        with pytest.raises(ValueError):
            call(**kw)


def test_pipeline_constructor_checks_diversity():
    from recommendit_amd.recommender import GpuRecommendationPipeline
    for bad in (2.0, float("nan"), -0.5):
        with pytest.raises(ValueError):
            GpuRecommendationPipeline(None, None, None, None, diversity=bad)
    with pytest.raises(ValueError):
        GpuRecommendationPipeline(None, None, None, None, diversity=0.2, diversity_vectors=torch.zeros((4, 8)))
    pipe = GpuRecommendationPipeline(None, None, None, None, diversity=0.25)
    assert pipe.diversity == 0.25 and pipe.diversity_vectors is None
    assert GpuRecommendationPipeline(None, None, None, None).diversity is None
