"""NumPy restatement of the 8-bit scalar quantiser and its integer search, written from the specification
(recommendit_hip.h at rihip_sq8_index_*), not from the kernels: f32 where the specification says f32, int64 for the
scores.  NumPy's float32 subtraction, multiplication and division are single correctly rounded operations and np.rint
rounds half to even, so every function here is bit for bit what the specification asks for."""
import numpy as np

F = np.float32
QMAX = 32512          # largest |n_j| = 127 * 256


def train_quantizer(X):
    """X f32 [N, d] -> (centre, scale) f32 [d]"""
    X = np.asarray(X, dtype=F)
    lo, hi = X.min(axis=0), X.max(axis=0)
    m = F(0.5) * (lo + hi)
    s = (hi - lo) / F(254.0)
    s[hi == lo] = F(1.0)
    return m.astype(F), s.astype(F)


def encode(X, m, s):
    """int8 [N, d]: clamp(rint((x - m) / s), -127, 127)"""
    X, m, s = np.asarray(X, dtype=F), np.asarray(m, dtype=F), np.asarray(s, dtype=F)
    v = np.rint((X - m[None, :]) / s[None, :])
    assert v.dtype == F
    return np.clip(v, -127, 127).astype(np.int8)


def decode(c, m, s):
    """f32 [N, d]: m + s * c, two f32 roundings"""
    prod = np.asarray(s, dtype=F)[None, :] * c.astype(F)
    out = np.asarray(m, dtype=F)[None, :] + prod
    assert out.dtype == F
    return out


def encode_queries(Q, m, s):
    """Q f32 [nq, d] -> (n int32 [nq, d], t f32 [nq], b f64 [nq])"""
    Q, m, s = np.asarray(Q, dtype=F), np.asarray(m, dtype=F), np.asarray(s, dtype=F)
    w = Q * s[None, :]
    A = np.abs(w).max(axis=1)
    t = (A / F(QMAX)).astype(F)
    n = np.zeros(Q.shape, dtype=np.int32)
    nz = A != 0
    if nz.any():
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.rint(w[nz] / t[nz, None])
        assert v.dtype == F
        n[nz] = np.clip(v, -QMAX, QMAX).astype(np.int32)
    t[~nz] = 0
    b = np.zeros(Q.shape[0], dtype=np.float64)
    for j in range(Q.shape[1]):                       # ascending j
        b = b + Q[:, j].astype(np.float64) * np.float64(m[j])
    return n, t, b


def limbs(n):
    """(hi, lo) with n == 256 * hi + lo, both in int8 range"""
    n = np.asarray(n, dtype=np.int32)
    hi = (n + 128) >> 8
    lo = n - 256 * hi
    return hi, lo


def int_scores(n, c):
    """int64 [nq, N]: S = sum_j n_j c_ij"""
    return n.astype(np.int64) @ c.astype(np.int64).T


def float_scores64(b, t, S):
    """the reported score before its cast to f32: b + t * S in f64"""
    return b[:, None] + t.astype(np.float64)[:, None] * S.astype(np.float64)


def topk(S, k, allowed=None):
    """rows int64 [nq, k] (-1 padded) and their scores int64 [nq, k] (0 where padded): by S descending, ties to the
    lower row; allowed bool [nq, N] restricts a query to some rows"""
    nq, N = S.shape
    rows = np.full((nq, k), -1, dtype=np.int64)
    sc = np.zeros((nq, k), dtype=np.int64)
    for q in range(nq):
        cand = np.arange(N) if allowed is None else np.nonzero(allowed[q])[0]
        order = cand[np.lexsort((cand, -S[q, cand]))][:k]
        rows[q, :len(order)] = order
        sc[q, :len(order)] = S[q, order]
    return rows, sc


def probed_lists(Q, C, nprobe):
    """int64 [nq, nprobe]: lists by coarse score <q, c> descending, ties to the lower list (exact in f64 for the dyadic
    inputs the tests use)"""
    cs = np.asarray(Q, dtype=np.float64) @ np.asarray(C, dtype=np.float64).T
    out = np.empty((cs.shape[0], nprobe), dtype=np.int64)
    ids = np.arange(cs.shape[1])
    for q in range(cs.shape[0]):
        out[q] = ids[np.lexsort((ids, -cs[q]))][:nprobe]
    return out
