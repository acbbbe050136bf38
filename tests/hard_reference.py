"""Host side of the in-batch hard-negative tests (TEST INFRASTRUCTURE; NumPy f64, no GPU, no torch).

Written from the contract in include/recommendit_hip.h (rihip_inbatch_hard_*), not from the kernel:

    global index of user i: gu = user_goff + i, of item j: gi = item_goff + j; user i's partner is the item with gi == gu
    s_ij = <u_i, y_j>;  item j is eligible for user i iff gi != gu and (no ids or item_ids[j] != user_pos_ids[i])
    eligible items ordered by (score descending, global item index ascending); N_i = ranks skip .. skip+m-1, c_i = |N_i|
    loss = (1/n_global) sum_i [c_i > 0] (1/c_i) sum_{j in N_i} softplus(s_ij - s_ii)
    w_ij = sigma(s_ij - s_ii) / (n_global c_i),  W_i = sum_j w_ij
    dU_i = sum_{j in N_i} w_ij y_j - W_i y_partner,  dI_j = sum_{i: j in N_i} w_ij u_i - [j partner of i] W_i u_i

``select`` is the selection, ``reference`` the loss and gradients of a given selection with the un-cancelled magnitudes
the bounds are relative to, ``bounds`` derives the error bounds (BOUNDS_DOC), ``one_pair_ratios`` sizes the cases.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from softmax_reference import (TINY, U32, USER_SHAPES, WIDTHS, cdiv, make_ids, partner_of_items,  # noqa: F401
                               partner_of_users, rows_of_norm, worst_ratio)

OWN = 128                 # users per loss part
M_MAX, SKIP_M_MAX = 32, 64


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def grid_rows(rng: np.random.RandomState, n: int, d: int) -> np.ndarray:
    """entries are multiples of 2^-6 in [-1, 1]: with d <= 256 every product (12 bits) and every partial sum of a score
    (<= 256, steps of 2^-12: 20 bits) is exact in f32 in any order, and equal scores are plentiful"""
    return (rng.randint(-64, 65, size=(n, d)) / 64.0).astype(np.float32)


def make_grid_case(seed: int, nu: int, ni: int, user_goff: int, item_goff: int, d: int, with_ids: bool) -> Dict[str, object]:
    rng = np.random.RandomState(seed)
    users, items = grid_rows(rng, nu, d), grid_rows(rng, ni, d)
    upos, iids = make_ids(rng, nu, ni, user_goff, item_goff) if with_ids else (None, None)
    return dict(users=users, items=items, user_goff=user_goff, item_goff=item_goff, user_pos_ids=upos, item_ids=iids)


def make_unit_case(seed: int, nu: int, ni: int, user_goff: int, item_goff: int, d: int, with_ids: bool) -> Dict[str, object]:
    rng = np.random.RandomState(seed)
    users, items = rows_of_norm(rng, nu, d, 1.0), rows_of_norm(rng, ni, d, 1.0)
    upos, iids = make_ids(rng, nu, ni, user_goff, item_goff) if with_ids else (None, None)
    return dict(users=users, items=items, user_goff=user_goff, item_goff=item_goff, user_pos_ids=upos, item_ids=iids)


# ---------------------------------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------------------------------
def eligible(nu: int, ni: int, user_goff: int, item_goff: int, user_pos_ids=None, item_ids=None) -> np.ndarray:
    assert (user_pos_ids is None) == (item_ids is None)
    gu, gi = user_goff + np.arange(nu, dtype=np.int64), item_goff + np.arange(ni, dtype=np.int64)
    el = gu[:, None] != gi[None, :]
    if item_ids is not None:
        el &= np.asarray(item_ids)[None, :] != np.asarray(user_pos_ids)[:, None]
    return el


def select(users: np.ndarray, items: np.ndarray, user_goff: int, item_goff: int, m: int, skip: int = 0,
           user_pos_ids: Optional[np.ndarray] = None, item_ids: Optional[np.ndarray] = None,
           scores: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """neg_idx int32 [nu, m] (local item indices in rank order, -1 in empty slots), neg_score f64 [nu, m] (0 in empty
    slots), pos_score f64 [nu], c [nu], and the full f64 score matrix.  ``scores`` overrides <u_i, y_j>."""
    assert 1 <= m <= M_MAX and skip >= 0 and skip + m <= SKIP_M_MAX
    nu, ni = users.shape[0], items.shape[0]
    S = users.astype(np.float64) @ items.astype(np.float64).T if scores is None else np.asarray(scores, np.float64)
    drow, ok = partner_of_users(nu, user_goff, ni, item_goff)
    assert ok.all(), "every user's partner must lie inside the items"
    el = eligible(nu, ni, user_goff, item_goff, user_pos_ids, item_ids)
    gi = item_goff + np.arange(ni, dtype=np.int64)
    neg_idx = np.full((nu, m), -1, np.int32)
    neg_score = np.zeros((nu, m), np.float64)
    for i in range(nu):
        cand = np.flatnonzero(el[i])
        order = cand[np.lexsort((gi[cand], -S[i, cand]))]     # last key first: -score, then the global index
        take = order[skip:skip + m]
        neg_idx[i, :take.size] = take
        neg_score[i, :take.size] = S[i, take]
    return dict(neg_idx=neg_idx, neg_score=neg_score, pos_score=S[np.arange(nu), drow], c=(neg_idx >= 0).sum(axis=1), S=S)


def selection_margin(sel: Dict[str, np.ndarray], el: np.ndarray, m: int, skip: int) -> float:
    """smallest score gap across the two edges of any row's window (rank skip-1 | skip and skip+m-1 | skip+m): a
    selection computed with score errors below half of it is the same set in the same order only if, in addition, the
    gaps inside the window hold; returns the smallest gap between any two consecutive ranks up to skip+m"""
    best = np.inf
    for i in range(el.shape[0]):
        s = np.sort(sel["S"][i, el[i]])[::-1][:skip + m + 1]
        if s.size > 1:
            best = min(best, float(np.min(s[:-1] - s[1:])))
    return best


# ---------------------------------------------------------------------------------------------------------------------
# expected values of the gradient entry
# ---------------------------------------------------------------------------------------------------------------------
def softplus(z):
    return np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def reference(users: np.ndarray, items: np.ndarray, user_goff: int, item_goff: int, m: int, n_global: int,
              neg_idx: np.ndarray, neg_score: Optional[np.ndarray] = None, pos_score: Optional[np.ndarray] = None
              ) -> Dict[str, object]:
    """f64 values of everything rihip_inbatch_hard_grads writes for the selection ``neg_idx`` [nu, m].  ``neg_score`` /
    ``pos_score`` are the arrays the entry is given (f32); None = the f64 scores of the rows.

    ok [nu, m], c, z, sp = softplus(z), sg = sigma(z), w, W;  a_neg [nu, m] / a_pos [nu] = sum_k |u_k y_k| of the
    scores;  loss_rows, loss_part (sums over 128 users), loss;  dU with M_dU = sum_j w |y_j|, C_dU = W |y_partner|;
    dI with M_dI = sum_i w |u_i|, C_dI = W |u_partner| and run [ni] = number of terms that land in the item."""
    U, Y = users.astype(np.float64), items.astype(np.float64)
    nu, ni, d = U.shape[0], Y.shape[0], U.shape[1]
    neg_idx = np.asarray(neg_idx)
    assert neg_idx.shape == (nu, m)
    ok = (neg_idx >= 0) & (neg_idx < ni)
    jj = np.where(ok, neg_idx, 0)
    drow, inside = partner_of_users(nu, user_goff, ni, item_goff)
    assert inside.all()
    c = ok.sum(axis=1)
    s_neg = np.einsum("ik,isk->is", U, Y[jj]) if neg_score is None else np.asarray(neg_score).astype(np.float64)
    s_pos = np.einsum("ik,ik->i", U, Y[drow]) if pos_score is None else np.asarray(pos_score).astype(np.float64)
    a_neg = np.einsum("ik,isk->is", np.abs(U), np.abs(Y[jj])) * ok
    a_pos = np.einsum("ik,ik->i", np.abs(U), np.abs(Y[drow]))
    z = np.where(ok, s_neg - s_pos[:, None], 0.0)
    sp, sg = softplus(z) * ok, sigmoid(z) * ok
    csafe = np.maximum(c, 1)
    w = sg / (float(n_global) * csafe)[:, None]
    W = w.sum(axis=1)
    loss_rows = sp.sum(axis=1) / csafe
    dU = np.einsum("is,isk->ik", w, Y[jj]) - W[:, None] * Y[drow]
    M_dU = np.einsum("is,isk->ik", w, np.abs(Y[jj]))
    C_dU = W[:, None] * np.abs(Y[drow])
    dI, M_dI, C_dI = np.zeros((ni, d)), np.zeros((ni, d)), np.zeros((ni, d))
    run = np.zeros(ni, np.int64)
    for i in range(nu):
        for s in range(m):
            if ok[i, s]:
                dI[jj[i, s]] += w[i, s] * U[i]
                M_dI[jj[i, s]] += w[i, s] * np.abs(U[i])
                run[jj[i, s]] += 1
        if c[i] > 0:
            dI[drow[i]] -= W[i] * U[i]
            C_dI[drow[i]] += W[i] * np.abs(U[i])
            run[drow[i]] += 1
    return dict(ok=ok, jj=jj, drow=drow, c=c, z=z, sp=sp, sg=sg, w=w, W=W, a_neg=a_neg, a_pos=a_pos, loss_rows=loss_rows,
                loss_part=np.array([loss_rows[b:b + OWN].sum() for b in range(0, nu, OWN)]),
                loss=loss_rows.sum() / n_global, dU=dU, M_dU=M_dU, C_dU=C_dU, dI=dI, M_dI=M_dI, C_dI=C_dI, run=run,
                n_users=nu, n_items=ni, m=m, n_global=n_global)


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
BOUNDS_DOC = """Bounds on |device - ref|, in units of u = 2^-24, derived (nothing here comes from a device run).  The
ulp figures of the device functions are the ones tests/softmax_reference.py records: v_exp_f32 1 ulp = 2 u, v_rcp 2 u;
log1pf is taken at 2 ulp = 4 u of its value.  c = c_i <= m is the row's number of negatives.

    score:  the entry is GIVEN its scores.  Where the reference computes them itself from the rows, a device score is a
            chain of d fused multiply-adds: d roundings relative to a = sum_k |u_k y_k| (k_neg = k_pos = d).  Where the
            test rounds an f64 score to f32, that is one rounding (k = 1); where both sides get the same array, none.
    z = fl(s_ij - s_ii):  |dz| <= (|z| + k_neg a_ij + k_pos a_ii) u =: E u.
    e = __expf(-z) = exp2(fl(-z fl(log2 e))):  the product and the rounded constant cost 2 |z| u in the argument, taken
            as 3 |z| u with one to spare, relative in e; v_exp_f32 2 u:  e (1 + (3 |z| + 2) u).
    sigma = 1 / (1 + e):  the error of e enters 1 + e with weight e / (1 + e) = 1 - sigma; the add rounds once; the
            division 2 u; dz enters with sigma' / sigma = 1 - sigma:
                relative error of sigma:  ((1 - sigma) (E + 3 |z| + 2) + 3) u.
    w = fl(sigma * scale), scale = fl(1 / (n_global c)) formed in double and rounded once:  2 u more:
                relative error of w_ij:   d_ij = ((1 - sigma) (E + 3 |z| + 2) + 5) u.
    W_i = sum_j w_ij:  a plain f32 sum of c positive terms in slot order, the recursive-sum bound (c - 1) u sum |w|:
                |dW_i| <= sum_j w_ij d_ij + (c - 1) W_i u.
    dU_ik = sum_j w_ij y_jk - W_i y_pk:  one chain of c + 1 fused multiply-adds, each rounding relative to a partial
            sum that is at most M + C (M = sum_j w |y_jk|, C = W |y_pk|): (c + 1) (M + C) u; every term carries its
            weight's error:
                |d dU| <= [ sum_j w_ij d_ij |y_jk| + (sum_j w_ij d_ij + (c - 1) W_i) |y_pk| + (c + 1) (M + C) ] u.
    dI_jk:  the same chain over the R_j terms that land in item j (in ascending pair order), the partner terms -W_i u_ik
            among them:
                |d dI| <= [ sum_i w_ij d_ij |u_ik| + sum_{i: partner} (sum_j w_ij d_ij + (c_i - 1) W_i) |u_ik|
                            + R_j (M + C) ] u.
    softplus = fmaxf(z, 0) + log1pf(e'), e' = __expf(-|z|):  dz enters with softplus' = sigma; the error of e' enters
            log1p with weight e' / (1 + e') = sigma(-|z|); log1pf 4 u of its value; the add rounds once:
                |d sp_ij| <= [ sigma E + sigma(-|z|) (3 |z| + 2) + 4 log1p(e') + sp ] u.
    loss row = (1/c) sum_j sp_ij in double (2^-52, ignored):  (1/c) sum_j |d sp_ij|; a part is a double sum of <= 128
            rows.
    second order:  every bound is multiplied by 1 + 2 D u, D the largest relative coefficient above.
    underflow:  a product below 2^-126 may be flushed to 0: + (terms) 2^-126 absolute on dU and dI."""


def bounds(ref: Dict[str, object], users: np.ndarray, items: np.ndarray, k_neg: int = 0, k_pos: int = 0
           ) -> Dict[str, np.ndarray]:
    """bounds of loss_rows, loss_part, dU, dI (BOUNDS_DOC)"""
    nu, ni, m = ref["n_users"], ref["n_items"], ref["m"]
    absU, absY = np.abs(users.astype(np.float64)), np.abs(items.astype(np.float64))
    ok, jj, drow, c, z, w, W = (ref[k] for k in ("ok", "jj", "drow", "c", "z", "w", "W"))
    az = np.abs(z)
    E = (az + k_neg * ref["a_neg"] + k_pos * ref["a_pos"][:, None]) * ok
    sg = sigmoid(z)
    dij = ((1 - sg) * (E + 3 * az + 2) + 5) * ok
    wd = (w * dij).sum(axis=1)                                   # sum_j w_ij d_ij
    dW = wd + np.maximum(c - 1, 0) * W
    second = 1.0 + 2.0 * float(max(dij.max() if dij.size else 0.0, m + 1, ref["run"].max())) * U32
    b_dU = (np.einsum("is,isk->ik", w * dij, absY[jj]) + dW[:, None] * absY[drow]
            + (c + 1)[:, None] * (ref["M_dU"] + ref["C_dU"])) * U32 * second + (m + 1) * TINY
    t_dI = np.zeros((ni, users.shape[1]))
    for i in range(nu):
        for s in range(m):
            if ok[i, s]:
                t_dI[jj[i, s]] += w[i, s] * dij[i, s] * absU[i]
        if c[i] > 0:
            t_dI[drow[i]] += dW[i] * absU[i]
    b_dI = (t_dI + ref["run"][:, None] * (ref["M_dI"] + ref["C_dI"])) * U32 * second + (ref["run"][:, None] + 1) * TINY
    e1 = np.exp(-az)
    b_sp = (sg * E + sigmoid(-az) * (3 * az + 2) + 4 * np.log1p(e1) + ref["sp"]) * ok * U32 * second
    b_rows = b_sp.sum(axis=1) / np.maximum(c, 1)
    return dict(loss_rows=b_rows, loss_part=np.array([b_rows[b:b + OWN].sum() for b in range(0, nu, OWN)]), dU=b_dU,
                dI=b_dI)


def one_pair_ratios(ref, bnd, users, items) -> Dict[str, float]:
    """smallest ratio of one selected pair's contribution to the bound of the output it lands in: w_ij |y_jk| against
    dU_ik's bound and w_ij |u_ik| against dI_jk's, in the most sensitive of the d elements; softplus_ij / c_i against
    the bound of the loss part that holds row i.  inf when no pair is selected."""
    absU, absY = np.abs(users.astype(np.float64)), np.abs(items.astype(np.float64))
    ok, jj, w, c = ref["ok"], ref["jj"], ref["w"], ref["c"]
    du = di = ls = np.inf
    for i in range(ref["n_users"]):
        for s in range(ref["m"]):
            if ok[i, s]:
                du = min(du, float((w[i, s] * absY[jj[i, s]] / bnd["dU"][i]).max()))
                di = min(di, float((w[i, s] * absU[i] / bnd["dI"][jj[i, s]]).max()))
                ls = min(ls, float(ref["sp"][i, s] / c[i] / bnd["loss_part"][i // OWN]))
    return dict(dU=du, dI=di, loss_part=ls)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_hard_negatives.py
# ---------------------------------------------------------------------------------------------------------------------
M_SKIP = [(1, 0), (8, 0), (8, 3), (32, 32)]
# (n_users, n_items, user_goff, item_goff): softmax_reference.USER_SHAPES puts the 32-owner group, the 128-owner
# workgroup and the 128-row tile each at -1 / 0 / +1, has more than four tiles and a slice of the items
SHAPES = list(USER_SHAPES)
# gradient cases: every shape and width, (m, skip, with_ids) cycling so that each shape and each width meets each
GRAD_M = [(8, 0, True), (32, 32, False), (1, 0, True), (8, 3, False)]


def grad_cases():
    """(d, shape, m, skip, with_ids) of the gradient tests"""
    out = []
    for a, d in enumerate(WIDTHS):
        for b, shape in enumerate(SHAPES):
            m, skip, with_ids = GRAD_M[(a + b) % len(GRAD_M)]
            out.append((d, shape, m, skip, with_ids))
    return out


def make_grad_case(d: int, shape: Tuple[int, int, int, int], m: int, skip: int, with_ids: bool):
    """unit rows; the selection and the f32 scores the gradient entry is given (the reference's own, rounded once)"""
    nu, ni, ug, ig = shape
    cs = make_unit_case(3000 + d + nu + m, nu, ni, ug, ig, d, with_ids)
    sel = select(cs["users"], cs["items"], ug, ig, m, skip, cs["user_pos_ids"], cs["item_ids"])
    cs["neg_idx"] = sel["neg_idx"]
    cs["neg_score"] = sel["neg_score"].astype(np.float32)
    cs["pos_score"] = sel["pos_score"].astype(np.float32)
    cs["m"], cs["skip"] = m, skip
    return cs
