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


# ---- additions for tests/test_gpu_sq8_paths.py: a faster exact reference and the driver's arithmetic --------------------
def int_scores_blas(n, c):
    """int_scores through a float64 matmul: every product is an integer below 2^22 and every partial sum below
    32512 * 127 * 128 < 2^29, far inside the 2^53 of a double, so the result is exact in any summation order"""
    out = n.astype(np.float64) @ c.astype(np.float64).T
    r = np.rint(out)
    assert (r == out).all()
    return r.astype(np.int64)


def topk_fast(S, k, allowed=None, chunk=256):
    """topk() for large S: one int64 sort key per score (-S in the high bits, the row in the low 24), partition + sort"""
    nq, N = S.shape
    assert N < 2 ** 24 and np.abs(S).max() < 2 ** 38
    rows = np.full((nq, k), -1, dtype=np.int64)
    sc = np.zeros((nq, k), dtype=np.int64)
    kk = min(k, N)
    ar = np.arange(N, dtype=np.int64)
    big = np.int64(2 ** 62)
    for q0 in range(0, nq, chunk):
        s = S[q0:q0 + chunk]
        key = (-s) * (1 << 24) + ar[None, :]
        if allowed is not None:
            key = np.where(allowed[q0:q0 + chunk], key, big)
        if kk < N:
            key = np.partition(key, kk - 1, axis=1)[:, :kk]
        key = np.sort(key, axis=1)
        ok = key < big
        r = np.where(ok, key & ((1 << 24) - 1), -1)
        rows[q0:q0 + chunk, :kk] = r
        sc[q0:q0 + chunk, :kk] = np.where(ok, np.take_along_axis(s, np.maximum(r, 0), axis=1), 0)
    return rows, sc


GRANULE = 64          # rows a list is padded to (TR)
TILE = 32             # rows per scanned tile (TRS)
SAMPLE_STEP = 16      # the threshold sample takes every 16th tile of a list (SQ8_SS)
PASS_QUERIES = 4096   # queries per internal pass (SQ8_CH)


def _tiles(list_len):
    return (int(list_len) + GRANULE - 1) // GRANULE * (GRANULE // TILE)


def plan(list_lens, probes_per_list, tile_step, target=4096):     # 4096: SQ8_TARGET = 16 * RIHIP_NCU in csrc/sq8.hip
    """the work plan as the rule above ivf_plan_body states it: (tpi, n_seq per list, splits per list).  A wave takes one
    list, 32 of the queries probing it and tpi consecutive sampled tiles; tpi = ceil(total_tiles / target)"""
    n_seq = [(_tiles(l) + tile_step - 1) // tile_step for l in list_lens]
    total = sum((int(p) + 31) // 32 * s for p, s in zip(probes_per_list, n_seq))
    tpi = max(1, (total + target - 1) // target)
    return tpi, n_seq, [(s + tpi - 1) // tpi for s in n_seq]


def geometry(list_lens, nprobe):
    """(nprobe used, cap_full, cap_lf, cap_df): rows of the nprobe longest lists; dense slots per (query, list) pair =
    the longest list padded; dense slots per query"""
    ll = sorted((int(l) for l in list_lens), reverse=True)
    npr = min(int(nprobe), len(ll))
    cap_full = max(1, sum(ll[:npr]))
    cap_lf = max(_tiles(ll[0]) * TILE, TILE)
    return npr, cap_full, cap_lf, cap_lf * npr


def auto_is_thresholded(nq, k, list_lens, nprobe):
    """the rule at SQ8_DENSE_AUTO: dense while the batch's dense slots stay within 2^23, or the probed rows within 16 384,
    or the sample is too short for k (4 k > cap_full / 16)"""
    _, cap_full, _, cap_df = geometry(list_lens, nprobe)
    return not (nq * cap_df <= 2 ** 23 or cap_full <= 16384 or 4.0 * k > cap_full / SAMPLE_STEP)


def dense_chunk(list_lens, nprobe):
    """queries per dense pass, the rule at SQ8_DENSE_BUDGET: 2^26 dense slots at most, 4 096 queries at most"""
    _, _, _, cap_df = geometry(list_lens, nprobe)
    return max(1, min(PASS_QUERIES, 2 ** 26 // cap_df))


def threshold_rank(k):
    """the sampled score that becomes the threshold: the rank-th best, rank = ceil(m + 4 sqrt(m) + 4), m = k / 16"""
    m = k / SAMPLE_STEP
    return int(np.ceil(m + 4.0 * np.sqrt(m) + 4.0))


def threshold_cap(k, list_lens, nprobe):
    """candidate slots per query of the thresholded pass: the power of two from 4 096 up that holds 2.5 * rank * 16,
    at most cap_full"""
    cap = 4096
    while cap < 2.5 * threshold_rank(k) * SAMPLE_STEP:
        cap *= 2
    return min(cap, geometry(list_lens, nprobe)[1])


def flat_sample_rows(N):
    """rows of a one-list index that the threshold sample scores: tiles 0, 16, 32, ..."""
    r = np.arange(N)
    return r[(r // TILE) % SAMPLE_STEP == 0]


REDO, KEPT, EITHER = 1, 0, -1


def _redo_state(scores, samp, rank, cap, k):
    """one query: scores int64 [rows it probes], samp int64 [its sampled rows].  The rule above sq8_thresholded: the
    threshold is the rank-th best sampled score, every probed row with S >= threshold becomes a candidate, and the query is
    re-done when the candidates overflow its cap slots or are fewer than k under a real threshold.  A sample shorter than
    rank gives no threshold: every probed row is a candidate and only overflow fails.

    What the rule leaves open: the select that finds the threshold (finalize_kernel, mode 1) may stop its radix passes as
    soon as exactly rank sampled keys remain above its prefix, so the threshold it hands on is SOME value t with
    #{sampled >= t} == rank: anything above the (rank+1)-th best sampled score up to the rank-th best (only the rank-th
    best itself when the two tie).  The candidate count is monotone in t, so the verdict is REDO / KEPT when both ends of
    that interval agree and EITHER when they do not."""
    if len(samp) < rank:
        return REDO if len(scores) > cap else KEPT
    top = -np.sort(-samp)[:rank + 1]
    a = top[rank - 1]
    lo = None if len(samp) == rank else (a if top[rank] == a else top[rank] + 1)
    cnt_min = int((scores >= a).sum())
    cnt_max = len(scores) if lo is None else int((scores >= lo).sum())
    fail_hi, fail_lo = cnt_min > cap or cnt_min < k, cnt_max > cap or cnt_max < k
    if cnt_min <= cap < cnt_max or cnt_min < k <= cnt_max:      # the verdict changes somewhere inside the interval
        return EITHER
    return REDO if fail_hi and fail_lo else (KEPT if not fail_hi and not fail_lo else EITHER)


def redo_bounds(state):
    """(fewest, most) queries a thresholded pass may re-do, from the states of its queries"""
    state = np.asarray(state)
    return int((state == REDO).sum()), int((state != KEPT).sum())


def flat_thresholded_redo(S, k):
    """int8 [nq] of REDO / KEPT / EITHER for a ONE-LIST index: the sample is every 16th tile of the list"""
    nq, N = S.shape
    rank, cap = threshold_rank(k), threshold_cap(k, [N], 1)
    samp = flat_sample_rows(N)
    return np.array([_redo_state(S[q], S[q, samp], rank, cap, k) for q in range(nq)], dtype=np.int8)


def ivf_thresholded_redo(S, k, assign, probes, nlist):
    """flat_thresholded_redo for an IVF index: assign int [N] (the list of every row; rows ascend inside a list, as
    ip_index.h states), probes int [nq, nprobe].  The sample of a query is every 16th tile of each list it probes"""
    nq, N = S.shape
    list_lens = np.bincount(assign, minlength=nlist)
    rank, cap = threshold_rank(k), threshold_cap(k, list_lens, probes.shape[1])
    rows_of = [np.nonzero(assign == l)[0] for l in range(nlist)]
    samp_of = [r[(np.arange(len(r)) // TILE) % SAMPLE_STEP == 0] for r in rows_of]
    out = np.empty(nq, dtype=np.int8)
    for q in range(nq):
        probed = np.concatenate([rows_of[l] for l in probes[q]])
        samp = np.concatenate([samp_of[l] for l in probes[q]])
        out[q] = _redo_state(S[q, probed], S[q, samp], rank, cap, k)
    return out
