"""NumPy restatement of the SQ8 index's refined search, written from the specification (recommendit_hip.h at
rihip_sq8_refine_search), not from the kernels.  Stage 1 is sq8_reference's integer search, unchanged.  The
bound and the certificate are float64 in the order the header gives.  f exists twice: f64() is the plain float64 inner
product (what f approximates, and equal to it bit for bit on inputs whose f32 products and sums are exact), f32_exact()
is the header's f operation by operation, with a correctly rounded fmaf."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_reference as S  # noqa: E402

F = np.float32
D = np.float64


def kernel_width(d):
    """dk: the width rows are zero-padded to (32 / 64 / 128)"""
    return 32 if d <= 32 else (64 if d <= 64 else 128)


def gamma(d):
    u = D(kernel_width(d)) * D(2.0) ** -24
    return u / (D(1.0) - u)


# ---- f ---------------------------------------------------------------------------------------------------------------
def f64(Q, X):
    """float64 inner products [nq, N]"""
    return np.asarray(Q, dtype=D) @ np.asarray(X, dtype=D).T


def abs_dot(Q, X):
    """sum_j |q_j x_j| in float64 [nq, N]: what f's rounding error is relative to"""
    return np.abs(np.asarray(Q, dtype=D)) @ np.abs(np.asarray(X, dtype=D)).T


def _fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded.  The product is exact in float64; the sum is rounded to odd
    there (TwoSum gives the exact residual: where it is not zero and the sum's last bit is even, the neighbour on the
    residual's side is the odd one), and a round-to-odd result with two spare bits rounds to float32 as the exact one."""
    p = a.astype(D) * b.astype(D)
    c = c.astype(D)
    t = p + c
    bb = t - p
    err = (p - (t - bb)) + (c - bb)
    fix = (err != 0) & ((t.view(np.int64) & 1) == 0)
    t = np.where(fix, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
    return t.astype(F)


def f32_exact(Qr, Xr):
    """f of the header for PAIRS of rows: Qr, Xr f32 [n, d] -> f32 [n].  16 lanes, lane l an fmaf chain over its dk / 16
    contiguous columns from 0.f, then s_l += s_(l xor o) for o = 8, 4, 2, 1, then + 0.f"""
    Qr, Xr = np.asarray(Qr, dtype=F), np.asarray(Xr, dtype=F)
    n, d = Qr.shape
    dk = kernel_width(d)
    P = dk // 16
    q = np.zeros((n, dk), dtype=F)
    x = np.zeros((n, dk), dtype=F)
    q[:, :d], x[:, :d] = Qr, Xr
    q, x = q.reshape(n, 16, P), x.reshape(n, 16, P)
    s = np.zeros((n, 16), dtype=F)
    for j in range(P):
        s = _fma32(q[:, :, j], x[:, :, j], s)
    lanes = np.arange(16)
    for o in (8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
        assert s.dtype == F
    return s[:, 0] + F(0.0)


# ---- attach: e and a -------------------------------------------------------------------------------------------------
def ranges(X, c, m, s):
    """(e, a) f64 [d]: e_j = max_i |x_ij - (m_j + s_j c_ij)| over the STORED codes c, a_j = max_i |x_ij|"""
    x = np.asarray(X, dtype=D)
    prod = np.asarray(s, dtype=D)[None, :] * c.astype(D)          # exact
    dec = np.asarray(m, dtype=D)[None, :] + prod
    return np.abs(x - dec).max(axis=0), np.abs(x).max(axis=0)


# ---- the bound -------------------------------------------------------------------------------------------------------
def bound(Q, m, s, n, t, e, a):
    """f64 [nq]: ((E1 + E2) + E3) + slack, every sum in ascending j"""
    Q = np.asarray(Q, dtype=F)
    nq, d = Q.shape
    dk = kernel_width(d)
    t64 = t.astype(D)
    s1, s2, sa, sm, sw = (np.zeros(nq, dtype=D) for _ in range(5))
    for j in range(d):
        x = Q[:, j].astype(D)
        ax = np.abs(x)
        tn = t64 * n[:, j].astype(D)                              # exact
        s1 = s1 + ax * D(e[j])
        s2 = s2 + np.abs(x * D(s[j]) - tn)
        sa = sa + ax * D(a[j])
        sm = sm + np.abs(x * D(m[j]))
        sw = sw + np.abs(tn)
    E1, E2, E3, W = s1, D(127.0) * s2, gamma(d) * sa, D(127.0) * sw
    mag = (((sm + W) + sa) + E1) + E2
    slack = D(2.0) ** -44 * mag + D(dk) * D(2.0) ** -126
    return ((E1 + E2) + E3) + slack


# ---- the refined search ----------------------------------------------------------------------------------------------
def probe_mask(Q, C, assign, nprobe):
    """bool [nq, N]: the rows of each query's probed lists"""
    probes = S.probed_lists(Q, C, nprobe)
    return (np.asarray(assign)[None, None, :] == probes[:, :, None]).any(axis=1)


def _select(rows, f, k):
    """top k of one query's (row, f) pairs by (f descending, row ascending), -1 / -inf padded"""
    order = np.lexsort((rows, -(f + F(0.0))))[:k]
    out_r = np.full(k, -1, dtype=np.int64)
    out_s = np.full(k, -np.inf, dtype=F)
    out_r[:len(order)], out_s[:len(order)] = rows[order], f[order]
    return out_r, out_s


def refine(Q, X, c, m, s, k, k_scan, allowed=None, ea=None):
    """-> dict(rows i64 [nq, k], scores f32 [nq, k], cert u8 [nq], bound f64 [nq], stage1 rows [nq, k_scan], n_valid,
    s_cut).  c: the stored codes; ea: (e, a), computed from X and c when left out"""
    Q, X = np.asarray(Q, dtype=F), np.asarray(X, dtype=F)
    nq = Q.shape[0]
    n, t, b = S.encode_queries(Q, m, s)
    rows1, sc1 = S.topk_fast(S.int_scores_blas(n, c), k_scan, allowed)
    e, a = ranges(X, c, m, s) if ea is None else ea
    bnd = bound(Q, m, s, n, t, e, a)
    out_r = np.empty((nq, k), dtype=np.int64)
    out_s = np.empty((nq, k), dtype=F)
    n_valid = (rows1 >= 0).sum(axis=1)
    s_cut = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        cand = rows1[q, :n_valid[q]]
        f = f32_exact(np.broadcast_to(Q[q], (len(cand), Q.shape[1])), X[cand]) if len(cand) else np.zeros(0, dtype=F)
        out_r[q], out_s[q] = _select(cand, f, k)
        if n_valid[q]:
            s_cut[q] = sc1[q, :n_valid[q]].min()
    U = (b + t.astype(D) * s_cut.astype(D)) + bnd
    cert = (n_valid < k_scan) | (out_s[:, k - 1].astype(D) > U)
    return dict(rows=out_r, scores=out_s, cert=cert.astype(np.uint8), bound=bnd, stage1=rows1, n_valid=n_valid, s_cut=s_cut)


def brute_force(Q, X, k, allowed=None):
    """the claim's right-hand side: the top k by (f, row) over ALL allowed rows, f the header's f32 function.
    f32_exact runs only where it can matter: |f - <q, x>| <= gamma * sum_j |q_j x_j| =: delta, so a row of the top k by f
    has a float64 product of at least (the k-th largest float64 product) - 2 max delta."""
    Q, X = np.asarray(Q, dtype=F), np.asarray(X, dtype=F)
    nq, N = Q.shape[0], X.shape[0]
    P = f64(Q, X)
    delta = gamma(Q.shape[1]) * abs_dot(Q, X) + D(kernel_width(Q.shape[1])) * D(2.0) ** -126
    out_r = np.empty((nq, k), dtype=np.int64)
    out_s = np.empty((nq, k), dtype=F)
    for q in range(nq):
        rows = np.arange(N) if allowed is None else np.nonzero(allowed[q])[0]
        if len(rows) > k:
            p = P[q, rows]
            kth = np.partition(p, len(p) - k)[len(p) - k]
            rows = rows[p >= kth - 2.0 * delta[q, rows].max()]
        f = f32_exact(np.broadcast_to(Q[q], (len(rows), Q.shape[1])), X[rows]) if len(rows) else np.zeros(0, dtype=F)
        out_r[q], out_s[q] = _select(rows, f, k)
    return out_r, out_s


# ---- inputs shared by the host and the GPU tests ---------------------------------------------------------------------
def unit_rows(seed, n, d):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(F)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(F)


def dyadic_rows(seed, n, d):
    """multiples of 1/64 in [-1, 1]: every f32 product and every sum of up to 128 of them is exact"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-64, 65, (n, d)) / 64.0).astype(F)


def ivf_layout(seed, N, d, nlist=8):
    """(centroids f32 [nlist, d] with entries +-1/2 and 0, assign int32 [N]): uneven lists, list 5 empty"""
    rng = np.random.default_rng(seed)
    C = (rng.integers(-1, 2, (nlist, d)) / 2.0).astype(F)
    assign = rng.integers(0, nlist, N).astype(np.int32)
    assign[assign == 5] = 1
    return C, assign
