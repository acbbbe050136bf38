"""Host side of the mixed in-batch objective tests (TEST INFRASTRUCTURE; NumPy only, no GPU, no torch).

Written from the contract in include/recommendit_hip.h (rihip_inbatch_gmat_mine / rihip_inbatch_mixed_apply), not from
the kernels:

    sigma_ij = the f32 stored in gmat for (item j, user i);  n = n_global;  c = 1 / (n (n - 1))
    eligible: j is not i's partner and (no ids or item_ids[j] != user_pos_ids[i]) -- by index, never by value
    order: (sigma + 0.f descending, global item index ascending);  N_i = ranks skip .. skip+m-1, c_i = |N_i|
    f_i = f32(1 + f64(f32 hard_weight) (n - 1) / c_i);  sigma' = fl32(sigma f_i), in place for j in N_i
    D_ij = fl32(sigma' - sigma), S_i = sum_j D_ij;  r_i += c S_i;  dU_i += c (sum_j D_ij y_j - S_i y_partner)
    z_ij = <u_i, y_j> - pos_i;  part[b] = hard_weight (n - 1) sum_{i in block b} [c_i > 0] (1/c_i) sum_j softplus(z_ij)

``mine`` restates the selection sequentially, ``apply_reference`` gives the exact f32 gmat and the f64 values of r, dU
and the loss parts with the un-cancelled magnitudes, ``apply_bounds`` derives the bounds (BOUNDS_DOC),
``chain_reference`` / ``chain_bounds`` do the same for the whole mixed_loss_and_grads chain against the definition
L_inbatch + hard_weight L_hard with the selection by f64 score.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

import hard_reference as H
import inbatch_reference as IB
from hard_reference import TINY, U32, cdiv, partner_of_users, rows_of_norm, worst_ratio  # noqa: F401

OWN = 128                 # users per loss part
MAX_SPLIT = 16            # rihip_inbatch_gmat_mine_max_nsplit = min(ceil(n_items / 64), 16)
M_SKIP = [(1, 0), (8, 0), (8, 3), (32, 32)]
# (n_users, n_items, user_goff); item_goff = 0
MINE_SHAPES = [(1, 2, 0), (31, 33, 0), (33, 33, 0), (130, 517, 200), (257, 1100, 300), (300, 300, 0)]
APPLY_SHAPES = [(33, 97, 30), (130, 300, 85)]
CHAIN_SHAPES = [(130, 517, 200), (300, 300, 0)]
HARD_WEIGHTS = (0.0, 0.1, 1.0, 50.0)


def max_nsplit(n_items: int) -> int:
    return min(cdiv(n_items, 64), MAX_SPLIT)


# ---------------------------------------------------------------------------------------------------------------------
# 1. mining
# ---------------------------------------------------------------------------------------------------------------------
def make_weights(kind: str, seed: int, nu: int, ni: int, user_goff: int, item_goff: int = 0) -> np.ndarray:
    """weights f32 [item, user] with 0 on the diagonal.  'random': uniform in [0, 1]; 'ternary': {0, 0.5, 1}, so that
    the index order decides nearly every rank.  User 0's column is all zeros in both (eligible zeros are candidates)."""
    rng = np.random.RandomState(seed)
    if kind == "random":
        w = rng.random_sample((ni, nu)).astype(np.float32)
    else:
        w = (rng.randint(0, 3, size=(ni, nu)) * 0.5).astype(np.float32)
    w[:, 0] = 0
    gi = item_goff + np.arange(ni, dtype=np.int64)[:, None]
    gu = user_goff + np.arange(nu, dtype=np.int64)[None, :]
    w[gi == gu] = 0
    return w


def make_mine_ids(mode: str, seed: int, nu: int, ni: int, user_goff: int, m: int, skip: int, item_goff: int = 0
                  ) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """(user_pos_ids, item_ids).  'none': no arrays.  'dups': distinct ids, then one item in ten carries the id of some
    row's positive.  'below' / 'between': all items but K carry one id Z, which is also the positive id of the first and
    the last user, whose eligible counts are then K or K - 1: K = skip ('below': skip - 1 < skip and skip itself both
    select nothing) or skip + ceil(m / 2) ('between': a partly filled row)."""
    if mode == "none":
        return None, None
    rng = np.random.RandomState(seed)
    iids = 1000 + item_goff + np.arange(ni, dtype=np.int64)
    upos = 1000 + user_goff + np.arange(nu, dtype=np.int64)
    if mode == "dups":
        pick = rng.choice(ni, size=max(1, ni // 10), replace=False)
        iids[pick] = upos[rng.randint(0, nu, size=pick.size)]
        return upos, iids
    K = skip if mode == "below" else skip + (m + 1) // 2
    K = min(K, ni)
    keep = rng.choice(ni, size=K, replace=False)
    z = np.int64(7)
    iids[:] = z
    iids[keep] = 1000 + item_goff + keep
    upos[0] = z
    upos[-1] = z
    return upos, iids


def mine(weights: np.ndarray, user_goff: int, item_goff: int, m: int, skip: int, user_pos_ids=None, item_ids=None
         ) -> Dict[str, np.ndarray]:
    """sequential restatement of the selection: neg_idx int32 [nu, m] (-1 in empty slots), neg_w f32 [nu, m] (0 there)"""
    ni, nu = weights.shape
    el = H.eligible(nu, ni, user_goff, item_goff, user_pos_ids, item_ids)
    neg_idx = np.full((nu, m), -1, np.int32)
    neg_w = np.zeros((nu, m), np.float32)
    for i in range(nu):
        cand = [j for j in range(ni) if el[i, j]]
        cand.sort(key=lambda j: (-float(weights[j, i] + np.float32(0)), item_goff + j))
        take = cand[skip:skip + m]
        for s, j in enumerate(take):
            neg_idx[i, s] = j
            neg_w[i, s] = weights[j, i]
    return dict(neg_idx=neg_idx, neg_w=neg_w, c=(neg_idx >= 0).sum(axis=1), eligible_count=el.sum(axis=1))


def blocked_gmat(weights: np.ndarray, nu: int, ni: int) -> np.ndarray:
    """blocked gmat around `weights` [item, user]: NaN outside the blocks that hold an in-range element (never read), 0
    in the ragged slots of those blocks"""
    ub, ib = IB.g_ub(nu), IB.g_ub(ni)
    full = np.full((ib * 32, ub * 32), np.nan, dtype=np.float32)
    full[:cdiv(ni, 32) * 32, :cdiv(nu, 32) * 32] = 0
    full[:ni, :nu] = weights
    return IB.encode_gmat(full, nu, ni)



# ---------------------------------------------------------------------------------------------------------------------
# 2. apply
# ---------------------------------------------------------------------------------------------------------------------
def boost_factors(c: np.ndarray, hard_weight: float, n_global: int) -> np.ndarray:
    hw = float(np.float32(hard_weight))
    return (1.0 + hw * float(n_global - 1) / np.maximum(c, 1).astype(np.float64)).astype(np.float32)


def apply_reference(weights: np.ndarray, users: np.ndarray, items: np.ndarray, pos: np.ndarray, user_goff: int,
                    item_goff: int, m: int, neg_idx: np.ndarray, neg_w: np.ndarray, hard_weight: float, n_global: int,
                    dU_in: np.ndarray, r_in: np.ndarray) -> Dict[str, object]:
    """weights_out f32 [item, user]: exact.  D [nu, m] = fl32(sigma' - sigma): exact f32 operations, so the f64 sums
    below are sums of the device's own terms.  r, dU, loss_part in f64; A_dU = sum_j D |y_j| + S |y_partner| and
    a [nu, m] = sum_k |u_k y_k| are the un-cancelled magnitudes."""
    U, Y = users.astype(np.float64), items.astype(np.float64)
    nu, ni = U.shape[0], Y.shape[0]
    neg_idx = np.asarray(neg_idx)
    ok = (neg_idx >= 0) & (neg_idx < ni)
    jj = np.where(ok, neg_idx, 0)
    c = ok.sum(axis=1)
    drow, inside = partner_of_users(nu, user_goff, ni, item_goff)
    assert inside.all()
    hw = float(np.float32(hard_weight))
    live = (c > 0) & (hw != 0.0)
    f = boost_factors(c, hard_weight, n_global)
    sg = np.asarray(neg_w, np.float32)
    sb = (sg * f[:, None]).astype(np.float32)                        # one rounded f32 multiply
    D32 = np.where(ok & live[:, None], (sb - sg).astype(np.float32), np.float32(0))
    wout = weights.copy()
    for i in range(nu):
        if live[i]:
            for s in range(m):
                if ok[i, s]:
                    wout[jj[i, s], i] = sb[i, s]
    D = D32.astype(np.float64)
    S = D.sum(axis=1)
    cc = 1.0 / (float(n_global) * (n_global - 1.0))
    r = r_in.astype(np.float64) + cc * S
    dU = dU_in.astype(np.float64) + cc * (np.einsum("is,isk->ik", D, Y[jj]) - S[:, None] * Y[drow])
    A = np.einsum("is,isk->ik", D, np.abs(Y[jj])) + S[:, None] * np.abs(Y[drow])
    z = (np.einsum("ik,isk->is", U, Y[jj]) - pos.astype(np.float64)[:, None]) * ok
    a = np.einsum("ik,isk->is", np.abs(U), np.abs(Y[jj])) * ok
    sp = H.softplus(z) * (ok & live[:, None])
    rows = sp.sum(axis=1) / np.maximum(c, 1)
    scale = hw * (n_global - 1.0)
    return dict(weights=wout, ok=ok, jj=jj, c=c, live=live, drow=drow, D=D, S=S, r=r, dU=dU, A_dU=A, z=z, a=a, sp=sp,
                loss_part=np.array([scale * rows[b:b + OWN].sum() for b in range(0, nu, OWN)]), scale=scale, cc=cc,
                f=f, r_in=r_in.astype(np.float64), dU_in=dU_in.astype(np.float64), n_users=nu, n_items=ni, m=m, d=U.shape[1])


BOUNDS_DOC = """Bounds on |device - ref|, in units of u = 2^-24, derived (nothing here comes from a device run).  sigma,
sigma' and D_ij = fl(sigma' - sigma) are exact f32 values that the reference forms with the same three operations, so
the errors below are those of the sums alone.  c_i <= m is the row's number of negatives, cf = fl(c) (one rounding).

    S_i = sum_j D_ij:   a plain f32 sum of c_i non-negative terms in slot order: (c_i - 1) S_i u.
    r_i' = fma(cf, S_i, r_i):  S's error and cf's rounding scale c S_i: c_i c S_i u; the fused multiply-add rounds once,
            relative to the result:                |dr| <= (c_i c S_i + |r_i'|) u.
    dU_ik' = fma(cf, acc, dU_ik), acc = a chain of c_i + 1 fused multiply-adds (the partner term -S_i y_pk last), each
            rounding relative to a partial sum of at most A = sum_j D_ij |y_jk| + S_i |y_pk|: (c_i + 1) A u; S's own
            error enters through the partner term: (c_i - 1) S_i |y_pk| u <= (c_i - 1) A u; cf: A u; the last rounding
            is relative to the result, at most |dU_ik| + c A:
                                                   |d dU| <= (c (2 c_i + 1) A + |dU_ik| + c A) u.
    z_ij = fl(p - pos_i):  p is, per lane, a chain of ceil(d / 64) fused multiply-adds and then six levels of the wave
            sum: ceil(d / 64) + 6 roundings relative to a_ij = sum_k |u_k y_k|; the subtraction one, relative to |z|:
                                                   |dz| <= ((ceil(d / 64) + 6) a_ij + |z|) u =: E u.
    softplus = fmaxf(z, 0) + log1pf(__expf(-|z|)):  as tests/hard_reference.py derives it:
                |d sp| <= [ sigma(z) E + sigma(-|z|) (3 |z| + 2) + 4 log1p(e^-|z|) + sp ] u.
    loss part = hard_weight (n - 1) sum_i (1 / c_i) sum_j sp_ij in double (2^-52, ignored): the same sum of |d sp|.
    second order:  every bound is multiplied by 1 + 2 (2 m + 8) u.
    underflow:  a product below 2^-126 may be flushed to 0: + (m + 2) 2^-126 absolute on r and dU."""


def apply_bounds(ref: Dict[str, object]) -> Dict[str, np.ndarray]:
    c, cc, S, A = ref["c"], ref["cc"], ref["S"], ref["A_dU"]
    second = 1.0 + 2.0 * (2 * ref["m"] + 8) * U32
    tiny = (ref["m"] + 2) * TINY
    b_r = (c * cc * S + np.abs(ref["r"])) * U32 * second + tiny
    b_dU = (cc * (2 * c + 1)[:, None] * A + np.abs(ref["dU_in"]) + cc * A) * U32 * second + tiny
    az = np.abs(ref["z"])
    E = ((cdiv(ref["d"], 64) + 6) * ref["a"] + az) * ref["ok"]
    b_sp = (H.sigmoid(ref["z"]) * E + H.sigmoid(-az) * (3 * az + 2) + 4 * np.log1p(np.exp(-az)) + ref["sp"]) \
        * (ref["ok"] & ref["live"][:, None]) * U32 * second
    rows = b_sp.sum(axis=1) / np.maximum(c, 1)
    nu = ref["n_users"]
    return dict(r=np.where(ref["live"], b_r, 0.0), dU=np.where(ref["live"][:, None], b_dU, 0.0),
                loss_part=np.array([ref["scale"] * rows[b:b + OWN].sum() for b in range(0, nu, OWN)]))


def one_pair_ratios(ref, bnd, items: np.ndarray) -> Dict[str, float]:
    """smallest ratio of one selected pair's contribution to the bound of the output it lands in: c D_ij against r_i's,
    c D_ij |y_jk| against dU_ik's in the most sensitive element, scale softplus_ij / c_i against its loss part's"""
    absY = np.abs(items.astype(np.float64))
    out = dict(r=np.inf, dU=np.inf, loss_part=np.inf)
    for i in range(ref["n_users"]):
        if not ref["live"][i]:
            continue
        for s in range(ref["m"]):
            if ref["ok"][i, s] and ref["D"][i, s] > 0:
                cd = ref["cc"] * ref["D"][i, s]
                out["r"] = min(out["r"], float(cd / bnd["r"][i]))
                out["dU"] = min(out["dU"], float((cd * absY[ref["jj"][i, s]] / bnd["dU"][i]).max()))
                out["loss_part"] = min(out["loss_part"], float(ref["scale"] * ref["sp"][i, s] / ref["c"][i]
                                                               / bnd["loss_part"][i // OWN]))
    return out


def make_apply_case(seed: int, shape: Tuple[int, int, int], d: int, m: int, skip: int) -> Dict[str, object]:
    """unit rows; weights = the f32 rounding of the f64 sigma(s - pos) with 0 on the diagonal (what the user pass
    stores, up to its own error, which this test does not look at); r_in, dU_in = the in-batch values in f32"""
    nu, ni, ug = shape
    rng = np.random.RandomState(seed)
    users, items = rows_of_norm(rng, nu, d, 1.0), rows_of_norm(rng, ni, d, 1.0)
    pos = np.einsum("ij,ij->i", users.astype(np.float64), items[ug:ug + nu].astype(np.float64)).astype(np.float32)
    ref = IB.realistic_reference(users, items, pos, ug, 0, ni)
    weights = ref["g"].astype(np.float32)
    sel = mine(weights, ug, 0, m, skip)
    return dict(users=users, items=items, pos=pos, user_goff=ug, weights=weights, neg_idx=sel["neg_idx"],
                neg_w=sel["neg_w"], r_in=ref["r"].astype(np.float32), dU_in=ref["dU"].astype(np.float32), n_global=ni,
                m=m, skip=skip)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the chain against the definition
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_DOC = """rowdot, user pass, mine, apply, item pass and the sum of both part arrays against the definition
L_inbatch + hard_weight L_hard, everything in f64 from the f32 rows (item_goff = 0, n_global = n_items).

pos:    the device's pos is rihip_rowdot's f32 value, the reference's the f64 dot: at most d + 2 roundings relative to
        a_ii = sum_k |u_k y_partner,k| more in every score difference of user i.  inbatch_reference's
        E_ij = K a_ij + 2 |pos| + |z| becomes K a_ij + (d + 2) a_ii + 2 |pos| + |z| (passed in as an inflated a_ij).
select: the device orders by its stored weight, at most bound_gmat away from the f64 weight: a row ENTERS the selection
        comparison only if every gap between consecutive f64 weights at ranks 0 .. skip + m exceeds the sum of the two
        entries' bounds; for the other rows the reference takes the device's own selection.
With g' = g f_i on the selected pairs (f_i in f64), D = g' - g, S_i = sum_j D_ij and r' = c sum_j g'_ij the reference is
in-batch BPR on the boosted weights.  emax = max E_ij + 5 is the relative error of one stored weight in u
(inbatch_reference.BOUNDS_DOC), k = K_CONST = 32.
    D:      |dD_ij| <= (D_ij emax + g'_ij + D_ij) u: the weight's error times f_i - 1, the boost's one rounding relative
            to g', the subtraction's relative to D.
    dU:     the user pass's own bound on the un-boosted sums ((P n + emax + k) M0 + (n + emax + k) C0) u, plus
            c sum_j |dD_ij| (|y_jk| + |y_pk|), plus apply's sums (BOUNDS_DOC above): (c (2 c_i + 2) A + |dU_ik|) u.
    r':     relative (n + 2 emax + k + m + 4) u: r's own (n + emax + k), c sum_j |dD_ij| <= (emax + 2) r' u, apply's
            (c_i c S + r') u <= (m + 1) r' u, one to spare.
    dI:     the item pass on the boosted weights, each with relative error (emax + 1) u:
            ((P n_u + emax + 1 + k) M' + (n + 2 emax + k + m + 4) C') u,  M' = c sum_i g'_ij |u_ik|, C' = r' |u_pk|.
    loss:   c (sum of the user pass's part bounds + the hard parts' bound) + 2 |loss| u for the f32 result; the hard
            parts as in BOUNDS_DOC with E = (ceil(d / 64) + 6) a_ij + (d + 2) a_ii + |z|."""


def chain_reference(users, items, user_goff: int, hard_weight: float, m: int, skip: int, user_pos_ids, item_ids,
                    precision: int, device_neg_idx: Optional[np.ndarray] = None) -> Dict[str, object]:
    nu, d = users.shape
    ni = items.shape[0]
    U, Y = users.astype(np.float64), items.astype(np.float64)
    drow, inside = partner_of_users(nu, user_goff, ni, 0)
    assert inside.all()
    pos64 = np.einsum("ij,ij->i", U, Y[drow])
    # realistic_reference takes pos as given: hand it the f64 value (a float64 array passes through astype unchanged)
    ref = IB.realistic_reference(users, items, pos64, user_goff, 0, ni)
    a_ii = np.einsum("ij,ij->i", np.abs(U), np.abs(Y[drow]))
    K = IB.score_factor(d, precision)
    ref["a"] = ref["a"] + (d + 2) / K * a_ii[None, :]                # (d + 2) a_ii more in every E_ij (CHAIN_DOC)
    gx, nsplit = cdiv(nu, IB.OW), ref["nsplit"]
    off = (np.arange(ni)[:, None]) != (user_goff + np.arange(nu)[None, :])
    for by in range(nsplit):
        t0, t1 = IB.split_range(ni, nsplit, by)
        for bx in range(gx):
            blk = (slice(t0 * IB.TSW, min(t1 * IB.TSW, ni)), slice(bx * IB.OW, min((bx + 1) * IB.OW, nu)))
            ref["A_loss"][by * gx + bx] = (ref["a"] * off)[blk].sum()
    bg = IB.bound_gmat(ref, pos64, d, precision)                     # [item, user]
    g = ref["g"]
    sel = H.select(users, items, user_goff, 0, m, skip, user_pos_ids, item_ids)
    el = H.eligible(nu, ni, user_goff, 0, user_pos_ids, item_ids)
    entered = np.zeros(nu, dtype=bool)
    for i in range(nu):
        cand = np.flatnonzero(el[i])
        order = cand[np.lexsort((cand, -sel["S"][i, cand]))][:skip + m + 1]
        gw, gb = g[order, i], bg[order, i]
        entered[i] = bool(np.all(gw[:-1] - gw[1:] > gb[:-1] + gb[1:])) if order.size > 1 else True
    neg_idx = sel["neg_idx"].copy()
    if device_neg_idx is not None:
        neg_idx[~entered] = np.asarray(device_neg_idx)[~entered]
    ok = neg_idx >= 0
    jj = np.where(ok, neg_idx, 0)
    c = ok.sum(axis=1)
    hw = float(np.float32(hard_weight))
    f = 1.0 + hw * (ni - 1.0) / np.maximum(c, 1)
    gp = g.copy()
    Dm, gsel = np.zeros((nu, m)), np.zeros((nu, m))
    for i in range(nu):
        for s in range(m):
            if ok[i, s]:
                Dm[i, s] = g[jj[i, s], i] * (f[i] - 1.0)
                gsel[i, s] = g[jj[i, s], i] * f[i]
                gp[jj[i, s], i] = gsel[i, s]
    cc = ref["c"]
    S = Dm.sum(axis=1)
    rp = cc * gp.sum(axis=0)
    dU = cc * (gp.T @ Y) - rp[:, None] * Y[drow]
    A = np.einsum("is,isk->ik", Dm, np.abs(Y[jj])) + S[:, None] * np.abs(Y[drow])
    irow, iok = IB._partner(ni, 0, user_goff, nu)
    dI = cc * (gp @ U) - np.where(iok[:, None], rp[irow][:, None] * U[irow], 0.0)
    M_dI = cc * (gp @ np.abs(U))
    C_dI = np.where(iok[:, None], rp[irow][:, None] * np.abs(U[irow]), 0.0)
    z = np.where(ok, np.einsum("ik,isk->is", U, Y[jj]) - pos64[:, None], 0.0)
    a = np.einsum("ik,isk->is", np.abs(U), np.abs(Y[jj])) * ok
    sp = H.softplus(z) * ok
    rows = sp.sum(axis=1) / np.maximum(c, 1)
    scale = hw * (ni - 1.0)
    hard_parts = np.array([scale * rows[b:b + OWN].sum() for b in range(0, nu, OWN)])
    loss = cc * (ref["loss_part"].sum() + hard_parts.sum())
    return dict(inb=ref, bg=bg, entered=entered, neg_idx=neg_idx, ref_neg_idx=sel["neg_idx"], ok=ok, jj=jj, c=c, f=f, D=Dm,
                gsel=gsel, S=S, A=A, gp=gp, r=rp, dU=dU, dI=dI, M_dI=M_dI, C_dI=C_dI, z=z, a=a, a_ii=a_ii, sp=sp,
                drow=drow, hard_parts=hard_parts, scale=scale, loss=loss, cc=cc, d=d, m=m, nu=nu, ni=ni,
                precision=precision, pos64=pos64, absY=np.abs(Y))


def chain_bounds(cr: Dict[str, object]) -> Dict[str, np.ndarray]:
    """bounds of loss, dU and dI of the chain (CHAIN_DOC)"""
    ref, d, precision, nu, ni, m, cc = cr["inb"], cr["d"], cr["precision"], cr["nu"], cr["ni"], cr["m"], cr["cc"]
    E = IB.elementwise_E(ref, cr["pos64"], d, precision)
    P = 1 if precision == 0 else 6
    emax = float(E.max()) + 5
    k, c, absY = IB.K_CONST, cr["c"], cr["absY"]
    dD = (cr["D"] * emax + cr["gsel"] + cr["D"]) * cr["ok"]                                  # in units of u
    b_dU = ((P * ni + emax + k) * ref["M_dU"] + (ni + emax + k) * ref["C_dU"]
            + cc * (np.einsum("is,isk->ik", dD, absY[cr["jj"]]) + dD.sum(axis=1)[:, None] * absY[cr["drow"]])
            + cc * (2 * c + 2)[:, None] * cr["A"] + np.abs(cr["dU"])) * U32
    b_dI = ((P * nu + emax + 1 + k) * cr["M_dI"] + (ni + 2 * emax + k + m + 4) * cr["C_dI"]) * U32
    K = IB.score_factor(d, precision)
    b_in = ((18 * ref["loss_tiles"] + 6 + IB.K_LOSS) * ref["M_loss"] + K * ref["A_loss"] + ref["Z_loss"]) * U32
    az = np.abs(cr["z"])
    Eh = ((cdiv(d, 64) + 6) * cr["a"] + (d + 2) * cr["a_ii"][:, None] + az) * cr["ok"]
    b_sp = (H.sigmoid(cr["z"]) * Eh + H.sigmoid(-az) * (3 * az + 2) + 4 * np.log1p(np.exp(-az)) + cr["sp"]) * cr["ok"] * U32
    b_hard = cr["scale"] * (b_sp.sum(axis=1) / np.maximum(c, 1)).sum()
    b_loss = cc * (b_in.sum() + b_hard) + 2 * abs(cr["loss"]) * U32
    return dict(dU=b_dU, dI=b_dI, loss=b_loss)


def make_chain_case(seed: int, shape: Tuple[int, int, int], d: int):
    """unit rows; ids with duplicates (user_pos_ids[i] = the id of i's partner)"""
    nu, ni, ug = shape
    rng = np.random.RandomState(seed)
    users, items = rows_of_norm(rng, nu, d, 1.0), rows_of_norm(rng, ni, d, 1.0)
    iids = 1000 + np.arange(ni, dtype=np.int64)
    pick = rng.choice(ni, size=max(1, ni // 10), replace=False)
    iids[pick] = iids[rng.randint(0, ni, size=pick.size)]
    return users, items, iids[ug:ug + nu].copy(), iids


CHAIN_SEED = 11
CHAIN_CASES = [(32, 0), (32, 2), (64, 0), (64, 2), (128, 0), (128, 2)]     # (d, precision)


def chain_m_skip(d: int, precision: int) -> Tuple[int, int]:
    """(8, 3) wherever the reference alone leaves at most a tenth of the rows out of the selection comparison
    (tests/test_mixed_host.py asserts it); at d = 128 with bf16x6 the stored weights' bounds are six times wider and
    (8, 3) leaves out 14 to 20 %, (4, 1) 3 to 5 %"""
    return (4, 1) if (d, precision) == (128, 2) else (8, 3)
