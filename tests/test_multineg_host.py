"""CPU: the references of the K-negative sampled step prove themselves, the alias table meets its bound, and the
argument checks that need no device refuse what they should."""
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multineg_reference as M  # noqa: E402
from oracle import optim_np as R  # noqa: E402

SEED = 12345          # fixed: every score below was inside |z| <= 4 with it when the test was written


def test_reference_gradients_are_the_derivatives_of_the_reference_loss():
    """central finite differences in float64, B = 5, K = 3, d = 8"""
    rng = np.random.default_rng(3)
    B, K, d = 5, 3, 8
    U, P, N = rng.standard_normal((B, d)), rng.standard_normal((B, d)), rng.standard_normal((K, B, d))
    ref = M.loss_and_grads_f64(U, P, N)
    assert abs(ref.loss - M.loss_f64(U, P, N)) < 1e-15
    h = 1e-6
    for name, arr, grad in (("dU", U, ref.dU), ("dP", P, ref.dP), ("dN", N, ref.dN)):
        fd = np.zeros_like(arr)
        for idx in np.ndindex(*arr.shape):
            keep = arr[idx]
            arr[idx] = keep + h
            up = M.loss_f64(U, P, N)
            arr[idx] = keep - h
            dn = M.loss_f64(U, P, N)
            arr[idx] = keep
            fd[idx] = (up - dn) / (2 * h)
        assert np.abs(fd - grad).max() < 1e-9, name
    # the tolerances are positive, finite and small against the values
    for name in ("dU", "dP", "dN"):
        e = getattr(ref, "e_" + name)
        assert np.isfinite(e).all() and (e > 0).all() and e.max() < 1e-4 * np.abs(getattr(ref, name)).max(), name
    # K = 1 is the pair loss of the staged step reference
    import step_reference as S
    one = M.loss_and_grads_f64(U, P, N[:1])
    pair = S.stage_loss(U, np.concatenate([P, N[0]]))
    assert np.allclose(one.dU, pair.dU, rtol=1e-14, atol=0) and abs(one.loss - pair.loss) < 1e-15
    assert np.allclose(np.concatenate([one.dP, one.dN[0]]), pair.dI, rtol=1e-14, atol=0)


def _zipf_counts(n):
    c = (3000.0 / (1.0 + np.arange(n))).astype(np.int64)
    c[::7] = 0
    return c


@pytest.mark.parametrize("n", [1, 2, 50, 3706])
@pytest.mark.parametrize("zeros", [False, True], ids=["count_plus_one", "zero_weights"])
def test_alias_table_is_within_its_quantisation_of_the_weights(n, zeros):
    """q_j implied by the integer arrays against w_j / sum w: every column is quantised to 2^-32 / n and an item collects
    from at most n columns, so 2^-31 has a factor two to spare; an item of weight zero is never drawn"""
    from recommendit_amd.negative_sampling import alias_probabilities, alias_table, popularity_weights
    counts = _zipf_counts(n)
    w = popularity_weights(counts, 0.75)
    assert (w >= 1.0).all()                       # the + 1: a count of zero stays drawable
    if zeros:
        w = np.where(counts == 0, 0.0, w)
        if not w.any():
            w[-1] = 2.5
    prob, alias = alias_table(w)
    assert prob.dtype == np.uint32 and alias.dtype == np.int32 and prob.shape == alias.shape == (n,)
    assert ((alias >= 0) & (alias < n)).all()
    # q from the integers alone, written out here (not the package's helper)
    keep = np.where(alias == np.arange(n), 1.0, prob.astype(np.float64) / 2.0 ** 32)
    q = keep.copy()
    np.add.at(q, alias, 1.0 - keep)
    q /= n
    assert np.abs(q - w / w.sum()).max() <= 2.0 ** -31
    assert (q[w == 0] == 0.0).all()
    assert np.array_equal(q, alias_probabilities(prob, alias))


@pytest.mark.parametrize("n", [50, 1000, 3706])
@pytest.mark.parametrize("weighted", [True, False], ids=["alias", "uniform"])
def test_restated_sampler_draws_the_distribution_it_is_given(n, weighted):
    """2^20 slots, empty rated set: Pearson's chi-square against w / sum w, as a Wilson-Hilferty normal score"""
    from recommendit_amd.negative_sampling import alias_table, popularity_weights
    catalog = np.arange(1, n + 1, dtype=np.int64) * 3
    if weighted:
        w = popularity_weights(_zipf_counts(n), 0.75)
        w[5::11] = 0.0
        prob, alias = alias_table(w)
    else:
        w, prob, alias = np.ones(n), None, None
    ns = 1 << 20
    neg, gave_up = M.sample_negatives_multi_np(np.zeros(ns // 4, np.int64), 4, catalog, prob, alias, np.zeros(0, np.int64),
                                               10 ** 6, SEED, 1000)
    assert gave_up == 0 and neg.shape == (ns,)
    counts = np.bincount(neg // 3 - 1, minlength=n)
    z = M.chi2_score(counts, w)
    print(f"[score] n={n} weighted={weighted}: z = {z:.2f}")
    assert abs(z) <= 4.0


def test_restated_sampler_renormalises_over_the_unrated_items():
    """one user who rated 30 % of a 50-item catalogue: the draws follow the weights renormalised over the other items"""
    from recommendit_amd.negative_sampling import alias_table, popularity_weights
    n, stride = 50, 1000
    catalog = np.arange(1, n + 1, dtype=np.int64)
    w = popularity_weights(_zipf_counts(n), 0.75)
    prob, alias = alias_table(w)
    rated_items = catalog[np.random.default_rng(1).permutation(n)[:15]]
    rated = np.sort(7 * stride + rated_items)
    ns = 1 << 20
    neg, gave_up = M.sample_negatives_multi_np(np.full(ns // 2, 7, np.int64), 2, catalog, prob, alias, rated, stride, SEED,
                                               1000)
    assert gave_up == 0
    counts = np.bincount(neg - 1, minlength=n)
    w_left = w.copy()
    w_left[rated_items - 1] = 0.0
    z = M.chi2_score(counts, w_left)            # (asserts that no rated item was drawn)
    print(f"[score] rated 30 %: z = {z:.2f}")
    assert abs(z) <= 4.0


@pytest.mark.parametrize("max_attempts", [1, 2, 1000])
def test_uniform_k1_restatement_is_the_existing_sampler_reference(max_attempts):
    rng = np.random.default_rng(5)
    n, nc, stride = 3001, 3706, 4000
    catalog = np.sort(rng.permutation(stride - 1)[:nc] + 1).astype(np.int64)
    users = rng.integers(1, 60, size=n).astype(np.int64)
    users[:40] = 3
    rated = np.unique(np.concatenate([3 * stride + catalog[2:],                       # user 3 rated all but two items
                                      rng.integers(1, 60, 5000) * stride + catalog[rng.integers(0, nc, 5000)]]))
    ref, ref_gu = R.sample_negatives_np(users, catalog, rated, stride, SEED, max_attempts)
    got, gu = M.sample_negatives_multi_np(users, 1, catalog, None, None, rated, stride, SEED, max_attempts)
    assert np.array_equal(got, ref) and gu == ref_gu
    if max_attempts < 1000:
        assert gu > 0


def test_alias_table_refuses_bad_weights():
    from recommendit_amd.negative_sampling import alias_table, popularity_weights
    for bad in ([], [0.0, 0.0], [1.0, -1.0], [1.0, np.nan], [1.0, np.inf], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            alias_table(bad)
    with pytest.raises(ValueError):
        popularity_weights([1, 2], np.nan)
    with pytest.raises(ValueError):
        popularity_weights([1, -2], 0.75)
    prob, alias = alias_table([0.0, 3.0, 0.0])
    assert prob.tolist() == [0, 2 ** 32 - 1, 0] and alias.tolist() == [1, 1, 1]


def _dataset():
    from recommendit_amd.train_embeddings import UserItemDataset
    ratings = pd.DataFrame({"user_id": [1, 1, 2, 2, 3, 3, 3], "item_id": [10, 20, 10, 30, 10, 20, 50],
                            "rating": [5, 4, 5, 2, 4, 1, 5], "timestamp": range(7)})
    return UserItemDataset(ratings, {}, [10, 20, 30, 40, 50])


def test_set_negative_sampling_builds_the_table_from_the_positives():
    from recommendit_amd.negative_sampling import alias_probabilities
    ds = _dataset()
    assert ds._alias_host is None
    assert ds.catalog_counts().tolist() == [3, 1, 0, 0, 1]           # ratings >= 4 per catalogue position
    ds.set_negative_sampling(alpha=0.75)
    w = np.array([4.0, 2.0, 1.0, 1.0, 2.0]) ** 0.75                    # (count + 1)^alpha: never-liked items stay drawable
    assert np.abs(alias_probabilities(*ds._alias_host) - w / w.sum()).max() <= 2.0 ** -31
    ds.set_negative_sampling(weights=[0, 1, 1, 0, 2])
    assert np.abs(alias_probabilities(*ds._alias_host) - np.array([0, .25, .25, 0, .5])).max() <= 2.0 ** -31
    ds.set_negative_sampling()                                         # alpha = 0, no weights: uniform again
    assert ds._alias_host is None
    for kw in (dict(weights=[1, 1, 1]), dict(weights=[0, 0, 0, 0, 0]), dict(weights=[1, 1, 1, 1, -1]),
               dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            ds.set_negative_sampling(**kw)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="n_negatives"):
            ds.sample_negatives(None, None, n_negatives=bad)
        with pytest.raises(ValueError, match="n_negatives"):
            next(ds.epoch_batches(2, None, n_negatives=bad))


def test_trainer_argument_checks_need_no_device():
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.train_embeddings import EmbeddingTrainer
    from recommendit_amd.trainer import HipBPRTrainer
    m = TwoTowerModel(10, 20, 32, 64)
    for mode in ("inbatch", "softmax", "hard", "mixed"):
        with pytest.raises(ValueError, match="loss_mode='sampled'"):
            HipBPRTrainer(m, 8, loss_mode=mode, n_negatives=2)
        with pytest.raises(ValueError, match="loss_mode='sampled'"):
            EmbeddingTrainer(loss_mode=mode, n_negatives=2)
        with pytest.raises(ValueError, match="loss_mode='sampled'"):
            EmbeddingTrainer(loss_mode=mode, negative_alpha=0.75)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="n_negatives"):
            HipBPRTrainer(m, 8, n_negatives=bad)
        with pytest.raises(ValueError, match="n_negatives"):
            EmbeddingTrainer(n_negatives=bad)
    with pytest.raises(ValueError, match="negative_alpha"):
        EmbeddingTrainer(negative_alpha=float("inf"))
    with pytest.raises(ValueError, match="persistent"):
        HipBPRTrainer(m, 8, n_negatives=2, persistent=True)
    with pytest.raises(ValueError, match="single-GPU for now"):
        HipBPRTrainer(m, 8, n_negatives=2, distributed=True)
    with pytest.raises(ValueError, match="single-GPU for now"):
        HipBPRTrainer(m, 8, n_negatives=2, process_group=object())


def test_trainer_cases_are_what_the_gpu_test_says_they_are():
    for name, (K, B, sparse) in zip(M.CASE_NAMES, ((3, 96, False), (2, 70, False), (4, 128, True))):
        c = M.make_case(name)
        assert (c.K, c.B, c.sparse) == (K, B, sparse)
        for u, it, g in c.batches:
            assert u.shape == (B,) and it.shape == ((1 + K) * B,) and g.shape == ((1 + K) * B, 18)
            assert (it[2 * B + 5] == it[B + 5]) and it[B] == it[0] == it[K * B + 1]
            assert sparse == bool(u.min() > 0 and it.min() > 0)      # the padding id is in the dense cases only
