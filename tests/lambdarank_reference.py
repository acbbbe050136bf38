"""Independent reference of the lambdarank gradients and of NDCG@k (TEST INFRASTRUCTURE).

Written from LightGBM's published ``LambdarankNDCG::GetGradientsForOneQuery`` (rank_objective.hpp), not from the HIP
kernel and not from oracle/lambdamart_np.py:

    sort the query's documents by score, descending, stable
    for i < min(cnt - 1, truncation_level), for j > i, labels different:
        high / low = the document with the larger / smaller label
        delta      = score[high] - score[low]
        pair_ndcg  = (gain[high] - gain[low]) * |discount[rank high] - discount[rank low]| * inverse_max_dcg
        if norm and best score != worst score:  pair_ndcg /= 0.01 + |delta|
        rho        = 1 / (1 + exp(sigmoid * delta))
        p_lambda   = -sigmoid * pair_ndcg * rho;   p_hessian = sigmoid^2 * pair_ndcg * rho * (1 - rho)
        lambda[high] += p_lambda; lambda[low] -= p_lambda; both hessians += p_hessian; sum_lambdas -= 2 * p_lambda
    if norm and sum_lambdas > 0:  everything *= log2(1 + sum_lambdas) / sum_lambdas

with discount[r] = 1 / log2(r + 2) and max_dcg the DCG at the truncation level of the documents taken from the highest
LABEL down (so ``label_gain`` must not decrease: a decreasing one is refused).

Every pair term is computed in ``np.longdouble`` (64-bit mantissa on x86-64: callers check ``LONGDOUBLE_OK``) and the
terms of a document are added EXACTLY: each long double is split into two doubles (high part + remainder, both exact)
and ``math.fsum`` adds those without any rounding; the one rounding left is that of the final sum.  The outer loop over
i is a Python loop; the inner loop over j runs as long-double array operations (a 16 384-document query has 524 000
pairs).  ``lambdarank_query_plain`` is the same pseudo-code as a scalar double loop, and the two are held together to
a few long-double roundings (2^-58 of the magnitude) by tests/test_lambdamart_oracle_host.py.

Besides lambda and hessian, per document: the number of pairs P it is in, and the UN-CANCELLED magnitudes an error bound
has to be relative to:

    M_lam = nf * sum over its pairs of sigmoid * |gain_i - gain_j| * (disc_i + disc_j) * inv * [1 / (0.01 + |delta|)] * rho
    M_hes = sigmoid * M_lam

-- the SUM of the discounts (|disc_i - disc_j| cancels for neighbouring ranks) and rho instead of rho * (1 - rho)
(1 - rho cancels when rho -> 1).  Per query (repeated for each of its documents): X = max over the pairs of
|sigmoid * delta| * (1 - rho), the factor by which a relative error of the exponent's argument grows in rho, and S =
sum_lambdas (a rounding of 1 + S grows by 1 / ln(1 + S) in log2(1 + S))."""
from __future__ import annotations

import math
from typing import Dict, Sequence

import numpy as np

LD = np.longdouble
LONGDOUBLE_OK = np.finfo(LD).nmant >= 63
LONGDOUBLE_WHY = f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa here: no headroom over float64"


def _exact_sum(terms) -> LD:
    """the long doubles of `terms` added without rounding (fsum of their exact double halves), rounded once"""
    t = np.asarray(terms, dtype=LD).ravel()
    if t.size == 0:
        return LD(0)
    hi = t.astype(np.float64)
    lo = (t - hi.astype(LD)).astype(np.float64)     # exact: the remainder of a 64-bit mantissa has <= 11 bits
    parts = np.concatenate([hi, lo]).tolist()
    s = math.fsum(parts)                              # correctly rounded double of the exact sum
    r = math.fsum(parts + [-s])                       # what that rounding dropped
    return LD(s) + LD(r)


def _check_gain(gain: np.ndarray) -> None:
    if not np.all(np.diff(gain) >= 0):
        raise ValueError("label_gain decreases: the ideal DCG is taken in label order")


def _ideal_dcg(labels: np.ndarray, k: int, gain: np.ndarray) -> LD:
    """documents from the highest label down, the first k of them"""
    top = np.sort(labels)[::-1][:k]
    pos = np.arange(top.size).astype(LD)
    return _exact_sum(gain.astype(LD)[top] / np.log2(pos + LD(2)))


def stable_order(scores: np.ndarray) -> np.ndarray:
    """ranks by descending score; equal scores (+0.0 == -0.0) keep their order"""
    idx = list(range(len(scores)))
    idx.sort(key=lambda d: -float(scores[d]) if scores[d] != 0 else 0.0)   # list.sort is stable
    return np.asarray(idx, dtype=np.int64)


def lambdarank_reference(scores: np.ndarray, labels: np.ndarray, groups: Sequence[int], label_gain: Sequence[float],
                         sigmoid: float, truncation_level: int, norm: bool) -> Dict[str, np.ndarray]:
    """-> dict of per-document arrays in document order: lam, hes (longdouble), P (int64), M_lam, M_hes (longdouble),
    X, S (longdouble, per query), cnt (int64, the size of the document's query), and sorted (int64: the row at each
    rank position, query after query).  `labels` are integers inside 0 .. len(label_gain) - 1."""
    gain = np.asarray(label_gain, dtype=np.float64)
    _check_gain(gain)
    labels = np.asarray(labels).astype(np.int64)
    assert labels.min() >= 0 and labels.max() < gain.size
    n = len(scores)
    sig, T = LD(sigmoid), int(truncation_level)
    out = dict(lam=np.zeros(n, LD), hes=np.zeros(n, LD), P=np.zeros(n, np.int64), M_lam=np.zeros(n, LD),
               M_hes=np.zeros(n, LD), X=np.zeros(n, LD), S=np.zeros(n, LD), cnt=np.zeros(n, np.int64),
               sorted=np.zeros(n, np.int64))
    b = 0
    for cnt in groups:
        cnt = int(cnt)
        s = np.asarray(scores[b:b + cnt], dtype=np.float64)
        lab = labels[b:b + cnt]
        order = stable_order(s)
        out["sorted"][b:b + cnt] = b + order
        out["cnt"][b:b + cnt] = cnt
        ss, ll = s[order].astype(LD), lab[order]
        gg = gain.astype(LD)[ll]
        mx = _ideal_dcg(lab, T, gain)
        inv = LD(1) / mx if mx > 0 else LD(0)
        disc = LD(1) / np.log2(np.arange(cnt).astype(LD) + LD(2))
        do_norm = bool(norm) and cnt > 0 and ss[0] != ss[-1]
        ni = min(cnt - 1, T)
        # signed lambda terms, hessian terms and magnitude terms of every pair (i, j): row i, column j; 0 = no pair
        tl = np.zeros((max(ni, 0), cnt), LD)
        th = np.zeros_like(tl)
        tm = np.zeros_like(tl)
        pair = np.zeros(tl.shape, bool)
        xq = LD(0)
        for i in range(ni):
            j = np.arange(i + 1, cnt)
            j = j[ll[j] != ll[i]]
            if j.size == 0:
                continue
            i_high = ll[i] > ll[j]
            delta = np.where(i_high, ss[i] - ss[j], ss[j] - ss[i])
            dgain = np.abs(gg[i] - gg[j])
            scale = inv / (LD(0.01) + np.abs(delta)) if do_norm else np.full(j.size, inv, LD)
            rho = LD(1) / (LD(1) + np.exp(sig * delta))
            p_lambda = -sig * (dgain * np.abs(disc[i] - disc[j]) * scale) * rho
            p_hess = sig * sig * (dgain * np.abs(disc[i] - disc[j]) * scale) * rho * (LD(1) - rho)
            # tl[i, j] = what document j (the partner) receives; document i receives the opposite
            tl[i, j] = np.where(i_high, -p_lambda, p_lambda)
            th[i, j] = p_hess
            tm[i, j] = sig * dgain * (disc[i] + disc[j]) * scale * rho
            pair[i, j] = True
            xq = max(xq, LD(np.max(np.abs(sig * delta) * (LD(1) - rho))))
        l_r, h_r, m_r = np.zeros(cnt, LD), np.zeros(cnt, LD), np.zeros(cnt, LD)
        P = np.zeros(cnt, np.int64)
        if ni > 0:
            P += pair.sum(0)
            P[:ni] += pair.sum(1)
            for r in range(cnt):
                k = min(r, ni)                      # as the partner of positions 0 .. k-1
                own = r < ni
                if not (P[r] > 0):
                    continue
                l_r[r] = _exact_sum(np.concatenate([tl[:k, r], -tl[r, r + 1:] if own else []]))
                h_r[r] = _exact_sum(np.concatenate([th[:k, r], th[r, r + 1:] if own else []]))
                m_r[r] = _exact_sum(np.concatenate([tm[:k, r], tm[r, r + 1:] if own else []]))
        # sum_lambdas = sum of -2 * p_lambda = 2 * sum |lambda term|
        S = LD(2) * _exact_sum(np.abs(tl))
        nf = np.log2(LD(1) + S) / S if (norm and S > 0) else LD(1)
        rows = b + order
        out["lam"][rows] = l_r * nf
        out["hes"][rows] = h_r * nf
        out["M_lam"][rows] = m_r * nf
        out["M_hes"][rows] = m_r * nf * sig
        out["P"][rows] = P
        out["X"][b:b + cnt] = xq
        out["S"][b:b + cnt] = S
        b += cnt
    assert b == n
    return out


def lambdarank_query_plain(scores, labels, label_gain, sigmoid, truncation_level, norm):
    """One query, the pseudo-code of the module docstring as a plain double loop over scalar long doubles -- no array
    operation takes part.  -> (lam, hes, P) in document order."""
    gain = [LD(g) for g in label_gain]
    cnt = len(scores)
    order = sorted(range(cnt), key=lambda d: -float(scores[d]))
    s = [LD(float(scores[d])) for d in order]
    lab = [int(labels[d]) for d in order]
    disc = [LD(1) / np.log2(LD(r) + LD(2)) for r in range(cnt)]
    top = sorted(lab, reverse=True)[:truncation_level]
    mx = _exact_sum([gain[l] / np.log2(LD(pos) + LD(2)) for pos, l in enumerate(top)])
    inv = LD(1) / mx if mx > 0 else LD(0)
    sig = LD(sigmoid)
    tl = [[] for _ in range(cnt)]
    th = [[] for _ in range(cnt)]
    all_l = []
    for i in range(min(cnt - 1, truncation_level)):
        for j in range(i + 1, cnt):
            if lab[i] == lab[j]:
                continue
            high, low = (i, j) if lab[i] > lab[j] else (j, i)
            delta = s[high] - s[low]
            pair = (gain[lab[high]] - gain[lab[low]]) * abs(disc[high] - disc[low]) * inv
            if norm and s[0] != s[-1]:
                pair = pair / (LD(0.01) + abs(delta))
            rho = LD(1) / (LD(1) + np.exp(sig * delta))
            p_lambda = -sig * pair * rho
            p_hess = sig * sig * pair * rho * (LD(1) - rho)
            tl[high].append(p_lambda); tl[low].append(-p_lambda)
            th[high].append(p_hess); th[low].append(p_hess)
            all_l.append(-p_lambda)
    S = LD(2) * _exact_sum(all_l)
    nf = np.log2(LD(1) + S) / S if (norm and S > 0) else LD(1)
    lam, hes, P = np.zeros(cnt, LD), np.zeros(cnt, LD), np.zeros(cnt, np.int64)
    for r, d in enumerate(order):
        lam[d], hes[d], P[d] = _exact_sum(tl[r]) * nf, _exact_sum(th[r]) * nf, len(tl[r])
    return lam, hes, P


def ndcg_reference(scores: np.ndarray, labels: np.ndarray, groups: Sequence[int], ks: Sequence[int],
                   label_gain: Sequence[float]):
    """mean NDCG@k over the queries for every k: DCG of the first min(k, cnt) documents of the stable descending order
    over the label-order ideal DCG; a query whose ideal DCG is not positive counts 1 (LightGBM's NDCGMetric)"""
    gain = np.asarray(label_gain, dtype=np.float64)
    _check_gain(gain)
    labels = np.asarray(labels).astype(np.int64)
    per_k = [[] for _ in ks]
    b = 0
    for cnt in groups:
        cnt = int(cnt)
        lab = labels[b:b + cnt]
        order = stable_order(np.asarray(scores[b:b + cnt], dtype=np.float64))
        for t, k in enumerate(ks):
            kk = min(int(k), cnt)
            mx = _ideal_dcg(lab, kk, gain)
            if mx > 0:
                dcg = _exact_sum(gain.astype(LD)[lab[order[:kk]]] / np.log2(np.arange(kk).astype(LD) + LD(2)))
                per_k[t].append(dcg / mx)
            else:
                per_k[t].append(LD(1))
        b += cnt
    return [float(_exact_sum(v) / LD(len(groups))) for v in per_k]


U = 2.0 ** -53


def gradient_bound(ref: Dict[str, np.ndarray], truncation_level: int, nf_adds: np.ndarray, norm: bool):
    """|computed - ref| allowed for an implementation that evaluates the published formula in float64, operation by
    operation (each +, -, x, / rounds once: relative error <= u = 2^-53; exp and log2 within 1 ulp <= 2u, the documented
    HIP double-precision bounds, which glibc meets as well).  Per pair term, relative to its un-cancelled magnitude:

      gain difference 1 | the two discounts 1/log2(r+2): (2 + 1) each, their difference 1 -> 4 relative to the SUM
      x discount, x inv: 2 | inv = 1/max_dcg: max_dcg is <= T terms of (2 + 1) added in sequence, then one division: T + 3
      delta 1, 0.01 + |delta| 1, the division 1: 3 | exp 2, 1 + e 1, 1 / (..) 1: 4 | -sigmoid x, x rho: 2
      => T + 19 for a lambda term; a hessian term has sigmoid x sigmoid, 1 - rho and one more product: T + 22
      the exponent's argument sigmoid * delta carries 2 roundings, which exp turns into 2 |sigmoid delta| (1 - rho) <= 2 X

    The terms of a document are then added: at most P - 1 additions in a thread and 10 in the fixed tree (6 wave levels,
    3 across the waves, 1 onto the partner sum) -> P + 9, and the product with nf: 1.
      => c = (T + 22) + 10 + 2 X = T + 32 + 2 X      |got - ref| <= (P + c) u M

    nf = log2(1 + S) / S: S is `nf_adds` additions of positive terms that each carry T + 19 + 2 X; |S nf'/nf| <= 1 passes
    that on at most unchanged; 1 + S rounds once, which log2 turns into 1 / ln(1 + S); log2 2, the division 1.
      => c_nf = T + 22 + 2 X + 1 / ln(1 + S)         + (nf_adds + c_nf) u |ref|

    and P 2^-1012 absolutely: rho = 1 / (1 + exp(x)) is 0 in float64 once exp(x) overflows (rho < 2^-1022), where the
    long double still holds it; the other factors of a term are <= 2 * 2 * 1 * 100 * 1.4427 < 2^10 (sigmoid^2, discount
    difference, |gain difference| * inv <= 1, 1 / 0.01, nf <= 1 / ln 2).
    -> (bound_lam, bound_hes, c, c_nf) per document."""
    T = int(truncation_level)
    X = ref["X"].astype(np.float64)
    c = T + 32 + 2.0 * X
    tiny = ref["P"] * 2.0 ** -1012
    if norm:
        S = ref["S"].astype(np.float64)
        with np.errstate(divide="ignore"):
            amp = np.where(S > 0, 1.0 / np.log1p(np.maximum(S, 1e-300)), 0.0)
        c_nf = np.where(S > 0, T + 22 + 2.0 * X + amp, 0.0)
        nf_part = np.where(S > 0, nf_adds + c_nf, 0.0) * U
    else:
        c_nf = np.zeros(len(X))
        nf_part = np.zeros(len(X))
    P = ref["P"].astype(np.float64)
    bl = (P + c) * U * ref["M_lam"].astype(np.float64) + nf_part * np.abs(ref["lam"].astype(np.float64)) + tiny
    bh = (P + c) * U * ref["M_hes"].astype(np.float64) + nf_part * np.abs(ref["hes"].astype(np.float64)) + tiny
    return bl, bh, c, c_nf
