"""NumPy restatement of the residual product quantiser, written from the specification (recommendit_hip.h at
rihip_pq_index_from_ip_index_residual), not from the kernels.  The quantiser itself is tests/pq_reference.py's, run on the
residuals; the search expectations are tests/sq8_reference.py's over the int16 decoded matrix; the refined search is
tests/sq8_refine_reference.py's with the certificate's code bound 254 in place of 127.

Inputs: c int8 [N, dpad], the rows' SQ8 codes in ORIGINAL row order (padding columns 0); assign int [N], the list of
every row; C f32 [nlist, du], the centroids; (m, s) the SQ8 quantiser."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_reference as P  # noqa: E402
import sq8_reference as S  # noqa: E402
import sq8_refine_reference as R  # noqa: E402

CODE_BOUND = 254          # |K + entry| <= 127 + 127
SCORE_BOUND = 32512 * 254 * 128


def list_codes(C, m, s, dpad):
    """int8 [nlist, dpad]: the centroids on the SQ8 grid, padding columns 0"""
    return P.pad_codes(S.encode(np.asarray(C, dtype=np.float32), m, s), dpad)


def residuals(c, K, assign):
    """(r int8 [N, dpad], clamped int): clamp(c - K[list], +-127) and the number of values the clamp changed"""
    r = c.astype(np.int32) - K[np.asarray(assign)].astype(np.int32)
    clamped = int((np.abs(r) > 127).sum())
    return np.clip(r, -127, 127).astype(np.int8), clamped


def train(c, K, assign, dsub, n_iter):
    """(book int8 [M, 256, dsub], codes uint8 [N, M], trace int64 [n_iter + 1], clamped): pq_reference.train on the residuals"""
    r, clamped = residuals(c, K, assign)
    book, codes, trace = P.train(r, dsub, n_iter)
    return book, codes, trace, clamped


def assign_with(c, K, assign, book):
    """(codes, distortion, clamped) under injected residual codebooks"""
    r, clamped = residuals(c, K, assign)
    codes, dist = P.assign(r, book)
    return codes, dist, clamped


def decode(codes, book, K, assign):
    """int16 [N, dpad]: K[list] + entry, not clamped"""
    return K[np.asarray(assign)].astype(np.int16) + P.decode(codes, book).astype(np.int16)


def reconstruct(dec16, m, s):
    """f32 [N, du]: m + s * c^ (two f32 roundings), sq8_reference.decode on the int16 codes"""
    return S.decode(dec16[:, :len(m)], m, s)


def pair_offsets(n, K, probes):
    """int64 [nq, nprobe]: T[q, p] = sum_j n_j K[probes[q, p]][j]"""
    du = n.shape[1]
    full = n.astype(np.int64) @ K[:, :du].astype(np.int64).T          # [nq, nlist]
    return np.take_along_axis(full, np.asarray(probes, dtype=np.int64), axis=1)


def int_scores(n, dec16):
    """int64 [nq, N]: S = sum_j n_j c^_ij, checked against the bound 32512 * 254 * dpad"""
    Sc = S.int_scores_blas(n, dec16[:, :n.shape[1]])
    assert np.abs(Sc).max() <= SCORE_BOUND
    return Sc


def split_scores(n, codes, book, K, assign):
    """the same scores the way the scan forms them: T of the row's list + the gathered dot product over the entries"""
    du = n.shape[1]
    gathered = S.int_scores_blas(n, P.decode(codes, book)[:, :du])
    T = n.astype(np.int64) @ K[:, :du].astype(np.int64).T
    return T[:, np.asarray(assign)] + gathered


def bound(Q, m, s, n, t, e, a, cmax=CODE_BOUND):
    """sq8_refine_reference.bound with the code bound cmax in E2 and W"""
    Q = np.asarray(Q, dtype=np.float32)
    D = np.float64
    nq, d = Q.shape
    dk = R.kernel_width(d)
    t64 = t.astype(D)
    s1, s2, sa, sm, sw = (np.zeros(nq, dtype=D) for _ in range(5))
    for j in range(d):
        x = Q[:, j].astype(D)
        ax = np.abs(x)
        tn = t64 * n[:, j].astype(D)
        s1 = s1 + ax * D(e[j])
        s2 = s2 + np.abs(x * D(s[j]) - tn)
        sa = sa + ax * D(a[j])
        sm = sm + np.abs(x * D(m[j]))
        sw = sw + np.abs(tn)
    E1, E2, E3, W = s1, D(cmax) * s2, R.gamma(d) * sa, D(cmax) * sw
    mag = (((sm + W) + sa) + E1) + E2
    slack = D(2.0) ** -44 * mag + D(dk) * D(2.0) ** -126
    return ((E1 + E2) + E3) + slack


def refine(Q, X, dec16, m, s, k, k_scan, allowed=None, ea=None, cmax=CODE_BOUND):
    """sq8_refine_reference.refine over the int16 decoded codes; the bound and the certificate with cmax"""
    dec = dec16[:, :np.asarray(Q).shape[1]]
    ea = R.ranges(X, dec, m, s) if ea is None else ea
    out = R.refine(Q, X, dec, m, s, k, k_scan, allowed, ea)
    n, t, b = S.encode_queries(Q, m, s)
    bnd = bound(Q, m, s, n, t, ea[0], ea[1], cmax)
    U = (b + t.astype(np.float64) * out["s_cut"].astype(np.float64)) + bnd
    cert = (out["n_valid"] < k_scan) | (out["scores"][:, k - 1].astype(np.float64) > U)
    out.update(bound=bnd, cert=cert.astype(np.uint8))
    return out


# ---- a fixed clustered fixture shared by the host and the GPU tests ----------------------------------------------------
def clustered(seed, n, du, nlist, spread=0.08):
    """(X f32 [n, du] unit rows around nlist centres, C f32 [nlist, du] the centres, assign int32 [n] the true cluster)"""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((nlist, du)).astype(np.float32)
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    assign = rng.integers(0, nlist, n).astype(np.int32)
    X = C[assign] + spread * rng.standard_normal((n, du)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X.astype(np.float32), C.astype(np.float32), assign
