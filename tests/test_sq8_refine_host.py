"""CPU: the refined SQ8 search's reference (tests/sq8_refine_reference.py) against its own brute force, and the argument
errors SQ8Index raises before it touches the device.  The soundness claim -- a certified query's list is the top k by
(f, row) over every probed row -- is checked here on the reference, at the shapes the GPU tests use, and the reference is
shown to certify most queries at factor 4 and none at factor 1: the GPU test's "for every certified query" is then not a
statement about an empty set."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_reference as S  # noqa: E402
import sq8_refine_reference as R  # noqa: E402

F = np.float32


# ---- the reference's own arithmetic ------------------------------------------------------------------------------------
def _is_correctly_rounded(r, exact):
    r = F(r)
    lo, hi = np.nextafter(r, F(-np.inf)), np.nextafter(r, F(np.inf))
    d = abs(Fraction(float(r)) - exact)
    for nb in (lo, hi):
        dn = abs(Fraction(float(nb)) - exact)
        if dn < d or (dn == d and (r.view(np.uint32) & 1)):
            return False
    return True


def test_fma32_is_correctly_rounded():
    # the sum is just below a tie of f32 that float64 rounds ONTO the tie: rounding twice gives 2^24 + 4
    a, b, c = F(1 + 2.0 ** -20), F(1 - 2.0 ** -20), F(2.0 ** 24 + 2)
    assert R._fma32(np.array([a]), np.array([b]), np.array([c]))[0] == F(2.0 ** 24 + 2)
    assert F(np.float64(a) * np.float64(b) + np.float64(c)) == F(2.0 ** 24 + 4)
    rng = np.random.default_rng(8)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(F)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(F)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(F)
    c[::7] = -(a[::7] * b[::7])                      # cancellation: the residual of the product is the whole result
    got = R._fma32(a, b, c)
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert _is_correctly_rounded(got[i], exact), (a[i], b[i], c[i], got[i])


@pytest.mark.parametrize("d", [40, 64, 128])
def test_f_on_exact_inputs_is_the_f64_product_and_within_gamma_otherwise(d):
    X, Q = R.dyadic_rows(1, 300, d), R.dyadic_rows(2, 300, d)
    f = R.f32_exact(Q, X)
    np.testing.assert_array_equal(f.astype(np.float64), np.einsum("ij,ij->i", Q.astype(np.float64), X.astype(np.float64)))
    X, Q = R.unit_rows(3, 300, d), R.unit_rows(4, 300, d)
    f = R.f32_exact(Q, X).astype(np.float64)
    ref = np.einsum("ij,ij->i", Q.astype(np.float64), X.astype(np.float64))
    lim = R.gamma(d) * np.einsum("ij,ij->i", np.abs(Q).astype(np.float64), np.abs(X).astype(np.float64))
    assert (np.abs(f - ref) <= lim).all() and (f != ref).any()
    z = R.f32_exact(np.array([[-1.0, 0, 0]], dtype=F), np.array([[0.0, 5, 5]], dtype=F))       # -0 + 0 = +0
    assert z[0] == 0 and not np.signbit(z[0])


def test_ranges_read_the_stored_codes():
    X = R.unit_rows(5, 500, 40)
    m, s = S.train_quantizer(X)
    c = S.encode(X, m, s)
    e, a = R.ranges(X, c, m, s)
    assert e.dtype == np.float64 and (e <= 0.5 * s.astype(np.float64) * (1 + 1e-3)).all() and (e > 0).all()
    np.testing.assert_array_equal(a, np.abs(X).max(axis=0).astype(np.float64))
    s2 = np.full(40, 1e-4, dtype=F)                  # an injected quantiser that clamps: the error is the clamp's
    c2 = S.encode(X, m, s2)
    assert (np.abs(c2) == 127).mean() > 0.5
    e2, _ = R.ranges(X, c2, m, s2)
    assert (e2 > 10 * e).all()
    want = np.abs(X.astype(np.float64) - S.decode(c2, m, s2).astype(np.float64)).max(axis=0)
    np.testing.assert_allclose(e2, want, rtol=1e-6)


def test_bound_terms():
    d = 40
    X, Q = R.unit_rows(6, 400, d), R.unit_rows(7, 9, d)
    Q[3] = 0
    m, s = S.train_quantizer(X)
    c = S.encode(X, m, s)
    n, t, b = S.encode_queries(Q, m, s)
    e, a = R.ranges(X, c, m, s)
    bd = R.bound(Q, m, s, n, t, e, a)
    q64 = np.abs(Q.astype(np.float64))
    E1 = q64 @ e
    E2 = 127.0 * np.abs(Q.astype(np.float64) * s.astype(np.float64) - t.astype(np.float64)[:, None] * n).sum(axis=1)
    E3 = R.gamma(d) * (q64 @ a)
    assert R.gamma(d) == 64 * 2.0 ** -24 / (1 - 64 * 2.0 ** -24)
    assert (bd >= E1 + E2 + E3).all() and (bd <= (E1 + E2 + E3) * (1 + 1e-9) + 1e-30).all()
    assert bd[3] == 64 * 2.0 ** -126                                     # the zero query: only the underflow term
    # the bound does bound: every row's f is within it of b + t S
    Sc = S.int_scores(n, c)
    approx = b[:, None] + t.astype(np.float64)[:, None] * Sc
    for q in range(Q.shape[0]):
        f = R.f32_exact(np.broadcast_to(Q[q], X.shape), X).astype(np.float64)
        assert (np.abs(f - approx[q]) <= bd[q]).all()


# ---- soundness of the certificate on the reference, at the GPU tests' shapes ---------------------------------------------
N, NQ = 20000, 70


def _case(d, ivf):
    X, Q = R.unit_rows(100 + d, N, d), R.unit_rows(200 + d, NQ, d)
    m, s = S.train_quantizer(X)
    c = S.encode(X, m, s)
    allowed = None
    if ivf:
        C, assign = R.ivf_layout(300 + d, N, d)
        allowed = R.probe_mask(Q, C, assign, 3)
    return X, Q, c, m, s, allowed


@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
@pytest.mark.parametrize("d", [40, 128])
def test_no_certified_query_differs_from_the_brute_force(d, ivf):
    X, Q, c, m, s, allowed = _case(d, ivf)
    ea = R.ranges(X, c, m, s)
    certified = 0
    for k in (1, 10, 100):
        bf_rows, bf_scores = R.brute_force(Q, X, k, allowed)
        for factor in (1, 1.5, 4):
            k_scan = max(k, int(math.ceil(factor * k)))
            r = R.refine(Q, X, c, m, s, k, k_scan, allowed, ea)
            ok = r["cert"] == 1
            certified += int(ok.sum())
            np.testing.assert_array_equal(r["rows"][ok], bf_rows[ok])
            np.testing.assert_array_equal(r["scores"][ok], bf_scores[ok])
            # refined recall is the candidates' recall: never below the plain search's
            plain = r["stage1"][:, :k]
            for q in range(NQ):
                truth = set(bf_rows[q].tolist())
                assert len(truth & set(r["rows"][q].tolist())) >= len(truth & set(plain[q].tolist()))
    assert certified > 0


def test_reference_certifies_at_factor_4_and_not_at_factor_1():
    """the issue's simulation: 20 000 unit rows, one list, d = 64, 64 queries, k = 10"""
    X, Q = R.unit_rows(0, 20000, 64), R.unit_rows(1, 64, 64)
    m, s = S.train_quantizer(X)
    c = S.encode(X, m, s)
    ea = R.ranges(X, c, m, s)
    bf_rows, _ = R.brute_force(Q, X, 10)
    r1 = R.refine(Q, X, c, m, s, 10, 10, None, ea)
    r4 = R.refine(Q, X, c, m, s, 10, 40, None, ea)
    assert int(r1["cert"].sum()) == 0
    assert int(r4["cert"].sum()) >= 48
    ok = r4["cert"] == 1
    np.testing.assert_array_equal(r4["rows"][ok], bf_rows[ok])
    assert 0.005 < r4["bound"].mean() < 0.03
    np.testing.assert_array_equal(r1["bound"], r4["bound"])              # the bound does not depend on stage 1
    # too few probed rows for k_scan: every probed row is re-scored, certified whatever the scores
    few = np.zeros((64, 20000), dtype=bool)
    few[:, 100:125] = True
    rf = R.refine(Q, X, c, m, s, 10, 40, few, ea)
    assert (rf["cert"] == 1).all() and (rf["n_valid"] == 25).all()
    np.testing.assert_array_equal(rf["rows"], R.brute_force(Q, X, 10, few)[0])


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors():
    from recommendit_amd import SQ8Index
    from recommendit_amd.sq8_index import _factor
    for bad in (0.5, 0, -1, float("nan"), float("inf"), "2", True, [2]):
        with pytest.raises(ValueError, match="refine"):
            _factor(bad)
    assert _factor(None) is None and _factor(1) == 1.0 and _factor(np.float32(2.5)) == 2.5
    sq = SQ8Index(embed_dim=64)
    assert sq.has_vectors is False and sq.stats() == {"status": "not built"}
    sq.set_refine(None)                                                   # nothing to refuse: the plain search
    for bad in (0.99, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="refine"):
            sq.set_refine(bad)
    with pytest.raises(RuntimeError, match="no vectors attached"):
        sq.set_refine(2.0)
    for call in (lambda: sq.attach_vectors(None), sq.drop_vectors, sq.refine_ranges,
                 lambda: sq.search_certified(None, 10)):
        with pytest.raises(RuntimeError, match="not built"):
            call()
    with pytest.raises(ValueError, match="FAISSIndex"):
        SQ8Index.from_index(object(), keep_vectors=True)
