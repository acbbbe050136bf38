"""Host side of the in-batch sampled-softmax tests (TEST INFRASTRUCTURE; NumPy f64, no GPU, no torch).

Written from the contract in include/recommendit_hip.h (rihip_inbatch_softmax_*), not from the kernel:

    global index of user i: gu = user_goff + i, of item j: gi = item_goff + j; user i's partner is the item with gi == gu
    l_ij  = inv_temp <u_i, y_j> - logq_j                        (logq None = 0; the diagonal is corrected too)
    pair (i, j) dropped iff ids are given, gi != gu and item_ids[j] == user_pos_ids[i]
    lse_i = log sum_{j kept} exp(l_ij),  p_ij = exp(l_ij - lse_i) (0 where dropped),  loss = (1/n_global) sum_i (lse_i - l_ii)
    dU_i  = c (sum_j p_ij y_j - y_partner),  dI_j = c (sum_i p_ij u_i - u_partner),  c = inv_temp / n_global
    item mode takes lse as an INPUT (f32, one per swept user) and gives an item whose partner user is outside the swept
    users no -u_partner term.

``reference`` returns the expectations with the un-cancelled magnitudes the bounds are relative to; ``bounds`` derives the
error bounds (BOUNDS_DOC); ``REALISTIC_CASES`` / ``one_pair_ratios`` / ``choose_rung`` size the realistic cases.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of f32
OWN, SWT = 128, 128       # users per loss part; swept rows per tile (a rescale step per tile)
TINY = 2.0 ** -126        # smallest normal f32: results below it may be flushed to 0


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def rows_of_norm(rng: np.random.RandomState, n: int, d: int, norm: float) -> np.ndarray:
    x = rng.standard_normal((n, d))
    return (x * (norm / np.linalg.norm(x, axis=1, keepdims=True))).astype(np.float32)


def zipf_logq(rng: np.random.RandomState, n: int) -> np.ndarray:
    """log of sampling probabilities proportional to Zipf counts floor(10000 / rank), ranks in random order"""
    cnt = np.floor(10000.0 / rng.permutation(np.arange(1, n + 1))).clip(min=1)
    return np.log(cnt / cnt.sum()).astype(np.float32)


def partner_of_users(nu: int, user_goff: int, ni: int, item_goff: int) -> Tuple[np.ndarray, np.ndarray]:
    """(local item index of each user's partner (0 where outside), inside flag)"""
    drow = user_goff + np.arange(nu, dtype=np.int64) - item_goff
    ok = (drow >= 0) & (drow < ni)
    return np.where(ok, drow, 0), ok


def partner_of_items(ni: int, item_goff: int, nu: int, user_goff: int) -> Tuple[np.ndarray, np.ndarray]:
    drow = item_goff + np.arange(ni, dtype=np.int64) - user_goff
    ok = (drow >= 0) & (drow < nu)
    return np.where(ok, drow, 0), ok


def make_ids(rng: np.random.RandomState, nu: int, ni: int, user_goff: int, item_goff: int, dup: float = 0.1
             ) -> Tuple[np.ndarray, np.ndarray]:
    """(user_pos_ids [nu], item_ids [ni]) int64: distinct item ids, then about `dup` of the items take another item's
    id.  user_pos_ids[i] is the id of i's partner; a user whose partner is outside the items gets a fresh id, or (with
    probability `dup`) the id of a random item: a duplicate of its positive sits in the set."""
    item_ids = rng.permutation(10 * ni + 10)[:ni].astype(np.int64) + 1
    if ni > 1:
        for j in np.flatnonzero(rng.rand(ni) < dup):
            item_ids[j] = item_ids[(j + 1 + rng.randint(ni - 1)) % ni]
    drow, ok = partner_of_users(nu, user_goff, ni, item_goff)
    fresh = -1 - np.arange(nu, dtype=np.int64)
    stray = np.where(rng.rand(nu) < dup, item_ids[rng.randint(ni, size=nu)], fresh)
    return np.where(ok, item_ids[drow], stray).astype(np.int64), item_ids


def make_case(seed: int, nu: int, ni: int, user_goff: int, item_goff: int, d: int, with_logq: bool = True,
              with_ids: bool = True, norm: float = 1.0) -> Dict[str, object]:
    rng = np.random.RandomState(seed)
    users, items = rows_of_norm(rng, nu, d, norm), rows_of_norm(rng, ni, d, norm)
    logq = zipf_logq(rng, ni) if with_logq else None
    upos, iids = make_ids(rng, nu, ni, user_goff, item_goff) if with_ids else (None, None)
    return dict(users=users, items=items, user_goff=user_goff, item_goff=item_goff, logq=logq, user_pos_ids=upos,
                item_ids=iids)


# ---------------------------------------------------------------------------------------------------------------------
# expected values
# ---------------------------------------------------------------------------------------------------------------------
def reference(users: np.ndarray, items: np.ndarray, user_goff: int, item_goff: int, inv_temp: float, n_global: int,
              logq: Optional[np.ndarray] = None, user_pos_ids: Optional[np.ndarray] = None,
              item_ids: Optional[np.ndarray] = None, lse_in: Optional[np.ndarray] = None) -> Dict[str, object]:
    """f64 values of everything the two sweeps write, from the f32 inputs as given.

    l, a = sum_k |u_k y_k|, dropped [user, item]; lse, p (user mode: normalised by the row's own lse); dU with
    M_dU = c sum_j p |y_j| and C_dU = c |y_partner|; loss_rows = lse_i - l_ii and loss_part (sums over 128 users);
    item mode: lse_used = ``lse_in`` (default: lse rounded to f32, what a caller passes on), p_item = exp(l - lse_used),
    dI with M_dI = c sum_i p_item |u_i| and C_dI = c |u_partner| (0 where the partner user is outside).
    ``user_ok``: every user's partner is inside the items (else the user-mode entries are None)."""
    assert (user_pos_ids is None) == (item_ids is None)
    U, Y = users.astype(np.float64), items.astype(np.float64)
    nu, ni = U.shape[0], Y.shape[0]
    c = float(inv_temp) / float(n_global)
    lq = np.zeros(ni) if logq is None else logq.astype(np.float64)
    l = float(inv_temp) * (U @ Y.T) - lq[None, :]
    a = np.abs(U) @ np.abs(Y).T
    diag = (user_goff + np.arange(nu))[:, None] == (item_goff + np.arange(ni))[None, :]
    dropped = np.zeros((nu, ni), dtype=bool)
    if item_ids is not None:
        dropped = (~diag) & (np.asarray(item_ids)[None, :] == np.asarray(user_pos_ids)[:, None])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lm = np.where(dropped, -np.inf, l)
        m = lm.max(axis=1)
        msafe = np.where(np.isfinite(m), m, 0.0)
        wsum = np.exp(lm - msafe[:, None]).sum(axis=1)
        lse = msafe + np.log(wsum)                       # -inf for a row with every pair dropped (item mode only)
        p = np.where(dropped, 0.0, np.exp(lm - np.where(np.isfinite(lse), lse, 0.0)[:, None]))
    out: Dict[str, object] = dict(c=c, l=l, a=a, dropped=dropped, diag=diag, m=m, lse=lse, p=p, n_users=nu, n_items=ni)
    drow, ok = partner_of_users(nu, user_goff, ni, item_goff)
    out["user_ok"] = bool(ok.all())
    if out["user_ok"]:
        out["dU"] = c * (p @ Y - Y[drow])
        out["M_dU"], out["C_dU"] = c * (p @ np.abs(Y)), c * np.abs(Y[drow])
        out["l_diag"] = l[np.arange(nu), drow]
        out["loss_rows"] = lse - out["l_diag"]
        out["loss_part"] = np.array([out["loss_rows"][b:b + OWN].sum() for b in range(0, nu, OWN)])
        out["loss"] = out["loss_rows"].sum() / n_global
    lse_used = (lse.astype(np.float32) if lse_in is None else np.asarray(lse_in, dtype=np.float32)).astype(np.float64)
    with np.errstate(over="ignore"):
        p_item = np.where(dropped, 0.0, np.exp(l - lse_used[:, None]))
    irow, iok = partner_of_items(ni, item_goff, nu, user_goff)
    out["lse_used"], out["p_item"] = lse_used, p_item
    out["dI"] = c * (p_item.T @ U - np.where(iok[:, None], U[irow], 0.0))
    out["M_dI"] = c * (p_item.T @ np.abs(U))
    out["C_dI"] = c * np.where(iok[:, None], np.abs(U[irow]), 0.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
BOUNDS_DOC = """Bounds on |device - ref|, in units of u = 2^-24, derived (nothing here comes from a device run).
T = ceil(n_swept / 128) tiles.  First order in u, then multiplied by (1 + 2 E_max u) for exp(x) - 1 <= x (1 + x).

    logit:  s_ij is a chain of d fused multiply-adds (d roundings relative to a_ij = sum_k |u_k y_k|); the product with
            inv_temp rounds once more (relative to inv_temp |s| <= inv_temp a), one to spare; the subtraction of logq
            rounds once relative to |l|:        |dl_ij| <= (inv_temp (d + 2) a_ij + |l_ij|) u  =: E_ij u.
    weight (user mode):  an item enters at the running maximum m_t of its tile, w = exp(l - m_t), and is then multiplied
            by exp(m_old - m_new) once per later tile.  Each factor is exp2(fl(x log2 e)) with x = fl(difference): the
            subtraction, the product and the rounded constant cost 3 |x| u in the argument = 3 |x| u relative; v_exp_f32
            is 1 ulp = 2 u, the product with the factor 1 u, 2 to spare: 5 u per factor, at most T + 1 factors.  The
            exponents telescope: sum |x| = m_i - l_ij =: X_ij (the running maximum only rises; a factor exp(0) = 1 is
            exact).  The maximum itself is exact given the logits and cancels in p = w / L:
                relative error of w_ij:  d_ij = (E_ij + 3 X_ij + 5 (T + 1)) u.
    L_i = sum_j w_ij:  a lane adds one term per tile (T), five shuffle levels and three adds across the waves (8):
                relative error of L_i:   dL_i = sum_j p_ij d_ij + (T + 8) u       (p-weighted mean, not the maximum)
    lse_i = m_i + log L_i:  logf 1 ulp of |log L| (2 |log L| u) and 2 u absolute to spare, the final add |lse| u:
                |d lse_i| <= dL_i + (2 |log L_i| + 2 + |lse_i|) u.
    loss row = lse_i - l_ii:  |d| <= |d lse_i| + E_ii u + (|lse_i| + |l_ii|) u; a part is an exact (double) sum of <= 128
            rows, converted once: + 2^-52 relative, ignored.
    dU_ik = c (sum_j p_ij y_jk - y_partner,k):  every term carries d_ij + dL_i and its place in the MFMA chain over the
            n_items swept rows plus one rescale product per tile (n_items + T); then 1 / L (v_rcp, 2 u), the product, the
            subtraction, the product with c and c's own rounding (6, taken as 8) relative to the un-cancelled
            M = c sum_j p |y_j| and C = c |y_partner|:
                |d dU| <= c sum_j p_ij |y_jk| (d_ij + dL_i + (n_items + T) u) + 8 (M + C) u.
    item mode:  p_ij = exp(l_ij - lse_i) with the f32 lse given: x = l - lse, relative error (E_ij + 3 |x_ij| + 5) u;
            on the diagonal p - 1 rounds once more (relative to p + 1).  The partner's -u term is a TERM OF THE CHAIN
            here (weight p_ii - 1 in the same product), so every later accumulation rounds relative to a partial sum
            that holds it: the recursive-sum bound n_users u sum_k |x_k| runs over M + C, not over M alone:
                |d dI| <= c sum_i p_ij |u_ik| (E_ij + 3 |x_ij| + 5) u + (n_users + 8) (M + C) u.
    underflow:  a weight below 2^-126 may be flushed to 0: + c n 2^-126 max|row| absolute on dU and dI, + n 2^-126 on L
            (relative to L >= 1: absolute on lse)."""


def logit_E(ref, d: int, inv_temp: float) -> np.ndarray:
    return float(inv_temp) * (d + 2) * ref["a"] + np.abs(ref["l"])


def bounds(ref: Dict[str, object], users: np.ndarray, items: np.ndarray, d: int, inv_temp: float) -> Dict[str, np.ndarray]:
    """bounds of lse [user], loss_rows, loss_part, dU, dI (see BOUNDS_DOC); the user-mode ones only when ref['user_ok']"""
    nu, ni = ref["n_users"], ref["n_items"]
    E = logit_E(ref, d, inv_temp)
    second = 1.0 + 2.0 * float(E.max()) * U32
    out: Dict[str, np.ndarray] = {}
    absU, absY = np.abs(users.astype(np.float64)), np.abs(items.astype(np.float64))
    c = ref["c"]
    if ref["user_ok"]:
        T = cdiv(ni, SWT)
        p = ref["p"]
        X = np.where(ref["dropped"], 0.0, ref["m"][:, None] - ref["l"])
        dij = E + 3.0 * X + 5.0 * (T + 1)
        dL = (p * dij).sum(axis=1) + (T + 8)
        logL = ref["lse"] - ref["m"]
        b_lse = (dL + 2 * np.abs(logL) + 2 + np.abs(ref["lse"])) * U32 + ni * TINY
        drow = ref["diag"].argmax(axis=1)     # the partner's local index
        b_rows = b_lse + (E[np.arange(nu), drow] + np.abs(ref["lse"]) + np.abs(ref["l_diag"])) * U32
        out["lse"] = b_lse * second
        out["loss_rows"] = b_rows * second
        out["loss_part"] = np.array([out["loss_rows"][b:b + OWN].sum() for b in range(0, nu, OWN)])
        out["dU"] = (c * ((p * (dij + dL[:, None] + ni + T)) @ absY) + 8 * (ref["M_dU"] + ref["C_dU"])) * U32 * second \
            + c * ni * TINY * absY.max()
    pi = ref["p_item"]
    x = np.where(ref["dropped"], 0.0, np.abs(ref["l"] - ref["lse_used"][:, None]))
    out["dI"] = (c * ((pi * (E + 3.0 * x + 5)).T @ absU) + (nu + 8) * (ref["M_dI"] + ref["C_dI"])) * U32 * second \
        + c * nu * TINY * absU.max()
    return out


def worst_ratio(got: np.ndarray, exp: np.ndarray, bound: np.ndarray) -> float:
    """max |got - exp| / bound (inf when something is not finite); 0 / 0 counts as 0"""
    got, exp, bound = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64), np.asarray(bound)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - exp)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_softmax.py
# ---------------------------------------------------------------------------------------------------------------------
WIDTHS = (16, 48, 64, 128, 144, 256)
INV_TEMPS = (1.0, 20.0)
# (n_users, n_items, user_goff, item_goff): the 32-owner group, the 128-owner workgroup and the 128-row swept tile each
# at -1 / 0 / +1, more than four tiles, a slice of the items
USER_SHAPES = [
    (1, 1, 0, 0), (1, 33, 17, 0), (31, 32, 0, 0), (32, 33, 1, 0), (33, 127, 94, 0), (127, 129, 1, 0), (128, 128, 0, 0),
    (129, 300, 77, 0), (129, 200, 300, 250), (130, 517, 200, 0),
]
# (n_items, n_users, item_goff, user_goff): the mirrored shapes, then partners partly outside the swept users
ITEM_SHAPES = [(ni, nu, ig, ug) for (nu, ni, ug, ig) in USER_SHAPES] + [(97, 131, 0, 64), (257, 161, 0, 0)]

# realistic sizes: d -> (n_users, n_items) at inv_temp = 1, the largest rung of LADDER at which one pair's contribution is
# >= 100 x the derived bound of the output it lands in (lse, dU, dI); tests/test_softmax_host.py re-derives the table.
# At inv_temp = 20 NO rung qualifies: the least likely pair of a sharp softmax (p_min ~ e^-8 / n and below) is smaller
# than the rounding of the likely ones at any size, so one dropped pair of that kind cannot be seen by any bound.  The
# inv_temp = 20 checks are the shape cases against their bounds; the one-pair sensitivity is claimed at inv_temp = 1.
LADDER = [(2, 8), (4, 16), (5, 33), (7, 33), (12, 45), (20, 70), (33, 97), (70, 161), (130, 300)]
REALISTIC_INV_TEMP = 1.0
REALISTIC_CASES = {16: (12, 45), 64: (12, 45), 144: (12, 45), 256: (7, 33)}


def make_realistic_case(d: int, inv_temp: float, shape: Optional[Tuple[int, int]] = None) -> Dict[str, object]:
    """unit rows, Zipf logq, no ids (a dropped pair has no contribution to measure); users in the middle of the items"""
    nu, ni = REALISTIC_CASES[d] if shape is None else shape
    return make_case(1, nu, ni, (ni - nu) // 2, 0, d, with_logq=True, with_ids=False)


def one_pair_ratios(ref, bnd, users, items) -> Dict[str, float]:
    """smallest ratio of one pair's contribution to the bound of the output it lands in: p_ij against lse_i's bound (a
    pair missing from the row sum moves lse by p_ij to first order); c p_ij |y_j| / c p_ij |u_i| against dU / dI, in the
    most sensitive of the d elements"""
    p, pi, c = ref["p"], ref["p_item"], ref["c"]
    absU, absY = np.abs(users.astype(np.float64)), np.abs(items.astype(np.float64))
    lse = (p / bnd["lse"][:, None]).min()
    du = (c * p[:, :, None] * absY[None, :, :] / bnd["dU"][:, None, :]).max(axis=2).min()
    di = (c * pi[:, :, None] * absU[:, None, :] / bnd["dI"][None, :, :]).max(axis=2).min()
    return dict(lse=float(lse), dU=float(du), dI=float(di))


def rung_ratios(d: int, inv_temp: float, shape: Tuple[int, int]) -> Dict[str, float]:
    cs = make_realistic_case(d, inv_temp, shape)
    ref = reference(cs["users"], cs["items"], cs["user_goff"], 0, inv_temp, shape[1], logq=cs["logq"])
    return one_pair_ratios(ref, bounds(ref, cs["users"], cs["items"], d, inv_temp), cs["users"], cs["items"])


def choose_rung(d: int, inv_temp: float) -> Optional[Tuple[int, int]]:
    best = None
    for shape in LADDER:
        if min(rung_ratios(d, inv_temp, shape).values()) >= 100:
            best = shape
    return best
