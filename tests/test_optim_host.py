"""CPU: oracle/optim_np.py (the reference the optimiser / row-sparse / sampler GPU tests compare against) pinned to
stock torch and NumPy, so that a mistake in the reference cannot hide the same mistake in a kernel."""
import math

import numpy as np
import pytest
import torch

from oracle import optim_np as R


def _ulps32(a, ref):
    """distance of float32 a from ref in units of the float32 spacing at ref"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("wd", [0.0, 1e-5])
@pytest.mark.parametrize("coef", [None, 0.37])
def test_adam_f64_equals_torch_adam(wd, coef):
    """Five steps of adam_f64 + adam_hyper against torch.optim.Adam(weight_decay) on float64 CPU tensors, with the
    clipping coefficient applied to the gradient first (as clip_grad_norm_ does before optimizer.step)."""
    rng = np.random.default_rng(11)
    n = 257
    lr, b1, b2, eps = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8))
    wd32 = float(np.float32(wd))
    p = rng.standard_normal(n)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd32, foreach=False)
    m, v = np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)
        c = None if coef is None else float(np.float32(coef))
        tp.grad = torch.tensor(g if c is None else g * c, dtype=torch.float64)
        opt.step()
        out = R.adam_f64(p, g, m, v, R.adam_hyper(lr, b1, b2, t), b1, b2, eps, wd, coef)
        p, m, v = out.p, out.m, out.v
        st = opt.state[tp]
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)


def test_adam_hyper_uses_the_float32_inputs_and_survives_large_t():
    lr, b1, b2 = np.float32(1e-3), np.float32(0.9), np.float32(0.999)
    h1 = R.adam_hyper(lr, b1, b2, 1)
    assert h1[0] == float(lr) / (1.0 - float(b1)) and h1[1] == math.sqrt(1.0 - float(b2))   # exact at t = 1
    assert abs(h1[1] - math.sqrt(1.0 - 0.999)) > 1e-9      # float32(0.999) is not 0.999
    for t in (2, 7, 1000, 10 ** 5):
        h = R.adam_hyper(lr, b1, b2, t)
        assert abs(h[0] - float(lr) / (1.0 - float(b1) ** t)) <= 1e-12 * h[0]
        assert abs(h[1] - math.sqrt(1.0 - float(b2) ** t)) <= 1e-12 * h[1]
    assert R.adam_hyper(lr, b1, b2, 10 ** 6) == (float(lr), 1.0)


@pytest.mark.parametrize("scale", [1e-3, 0.125, 1.0, 40.0])
def test_clip_coef_f32_equals_clip_grad_norm(scale):
    """Returned norm and the scaling actually applied, against torch.nn.utils.clip_grad_norm_ on float32 tensors
    (64 elements in all, so that torch's float32 accumulation of the norm stays inside the 2-ulp allowance)."""
    rng = np.random.default_rng(5)
    gs = [(rng.standard_normal(k) * scale).astype(np.float32) for k in (7, 33, 24)]
    params = [torch.zeros(g.shape[0], dtype=torch.float32, requires_grad=True) for g in gs]
    for p, g in zip(params, gs):
        p.grad = torch.from_numpy(g.copy())
    tn = torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=False)
    coef, norm = R.clip_coef_f32(sum(R.sumsq_f64(g) for g in gs), 1.0)
    assert coef.dtype == np.float32 and norm.dtype == np.float32
    assert _ulps32(norm, float(tn)) <= 2
    assert (coef == 1.0) == (float(norm) + 1e-6 <= 1.0)
    applied = torch.clamp(1.0 / (tn + 1e-6), max=1.0)      # the coefficient torch multiplied the gradients by
    for p, g in zip(params, gs):
        assert torch.equal(p.grad, torch.from_numpy(g) * applied)
    assert _ulps32(coef, float(applied)) <= 2


def test_clip_coef_of_zero_gradient_is_one():
    coef, norm = R.clip_coef_f32(0.0, 1.0)
    assert coef == np.float32(1.0) and norm == np.float32(0.0)


@pytest.mark.parametrize("n_rows", [0, 50])
def test_group_and_reduce_rows_equal_unique_and_add_at(n_rows):
    rng = np.random.default_rng(3)
    B, d = 700, 5
    ids = rng.integers(0, 50, size=B).astype(np.int64)
    ids[[3, 9, 200]] = [-2, 57, (1 << 40) + 5]
    ids[[4, 5]] = 0
    dX = rng.standard_normal((B, d)).astype(np.float32)
    key = np.where(ids < 0, 0, ids)
    if n_rows > 0:
        key = np.where(key >= n_rows, 0, key)
    uniq, pos = R.group_rows(ids, n_rows)
    ref_u, inv, ref_c = np.unique(key, return_inverse=True, return_counts=True)
    np.testing.assert_array_equal(uniq, ref_u)
    assert (np.diff(uniq) > 0).all()
    for k, p_ in enumerate(pos):
        np.testing.assert_array_equal(p_, np.flatnonzero(key == uniq[k]))
    G, A, cnt = R.reduce_rows_f64(dX, uniq, pos)
    np.testing.assert_array_equal(cnt, ref_c)
    ref_G = np.zeros((ref_u.size, d)); ref_A = np.zeros((ref_u.size, d))
    np.add.at(ref_G, inv, dX.astype(np.float64))
    np.add.at(ref_A, inv, np.abs(dX.astype(np.float64)))
    ref_G[ref_u == 0] = 0; ref_A[ref_u == 0] = 0
    np.testing.assert_allclose(G, ref_G, rtol=0, atol=1e-13)
    np.testing.assert_allclose(A, ref_A, rtol=1e-13, atol=0)
    assert (G[uniq == 0] == 0).all()


def _catalogue(rng):
    return np.sort(rng.choice(np.arange(1, 700), size=480, replace=False)).astype(np.int64)


def test_sampler_reference_never_returns_a_rated_item_unless_it_gave_up():
    rng = np.random.default_rng(2)
    cat = _catalogue(rng)
    M = 700
    users = rng.integers(1, 601, size=20000).astype(np.int64)
    ru, ri = rng.integers(1, 601, size=60000), rng.choice(cat, size=60000)
    rated = np.unique(ru * M + ri)
    neg, gave_up = R.sample_negatives_np(users, cat, rated, M, seed=12345, max_attempts=1000)
    assert gave_up == 0 and np.isin(neg, cat).all() and not np.isin(users * M + neg, rated).any()
    # one attempt: every sample whose first draw is rated gives up and keeps that draw
    neg1, gave1 = R.sample_negatives_np(users, cat, rated, M, seed=12345, max_attempts=1)
    hit = np.isin(users * M + neg1, rated)
    assert gave1 == int(hit.sum()) > 0
    np.testing.assert_array_equal(neg1[~hit], neg[~hit])     # attempt 0 is the same draw in both runs


@pytest.mark.parametrize("max_attempts", [1, 50])
def test_sampler_reference_gave_up_count_is_exact(max_attempts):
    cat = np.array([3, 8, 9, 20], dtype=np.int64)
    M = 32
    rated = np.sort(np.concatenate([7 * M + cat, [5 * M + 8]])).astype(np.int64)   # user 7 rated the whole catalogue
    users = np.array([7, 5, 7, 6, 7, 5] * 50, dtype=np.int64)
    neg, gave_up = R.sample_negatives_np(users, cat, rated, M, seed=9, max_attempts=max_attempts)
    hit = np.isin(users * M + neg, rated)
    if max_attempts == 50:       # P(user 5 draws item 8 fifty times) = 4^-50
        assert gave_up == int((users == 7).sum()) and (hit == (users == 7)).all()
    else:
        assert gave_up == int(hit.sum()) >= int((users == 7).sum())
    assert np.isin(neg, cat).all()


def test_sampler_reference_is_uniform_and_keyed_by_sample_index():
    rng = np.random.default_rng(7)
    cat = _catalogue(rng)
    users = np.ones(200_000, dtype=np.int64)
    neg, gave_up = R.sample_negatives_np(users, cat, np.zeros(0, np.int64), 700, seed=2024, max_attempts=1000)
    assert gave_up == 0
    counts = np.bincount(np.searchsorted(cat, neg), minlength=480)
    exp = 200_000 / 480
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    print("chi2", chi2)
    assert chi2 < 479 + 5 * math.sqrt(958)       # mean + 5 sigma of chi^2(479)
    # the draw depends on (seed, i), not on the batch length
    short, _ = R.sample_negatives_np(users[:777], cat, np.zeros(0, np.int64), 700, seed=2024, max_attempts=1000)
    np.testing.assert_array_equal(short, neg[:777])
    other, _ = R.sample_negatives_np(users[:777], cat, np.zeros(0, np.int64), 700, seed=2025, max_attempts=1000)
    assert (other != short).mean() > 0.9
