"""Staged float64 reference of the sampled-negative training step with the dense optimiser (TEST INFRASTRUCTURE).

Used by tests/test_gpu_step_phases.py (GPU, both the one-launch and the seven-launch step) and proven against stock torch
in tests/test_step_host.py (CPU).  Written from the definitions in oracle/two_tower_np.py (tower_forward, bpr_loss,
tower_backward, embedding_scatter_add, clip_coef, adam_step) and oracle/optim_np.py (clip_coef_f32, adam_hyper, adam_f64),
not from the kernels.

Stages
------
A step is checked stage by stage.  Every stage takes the float32 arrays the previous stage STORED (the trainer's public
buffers) and evaluates its own definition in float64, so an error does not travel: the stage that is red is the stage
that is wrong.

    A1  hid          from the parameters before the step, the ids, the genres and the keep mask
    A2  den, out     from the stored hid (y = hid W2^T + b2 is not stored; the kernels normalise the y they formed from
                     the hid they stored)
    B1  dU, dI, loss from the stored U and I
    B2  dX           from the stored dU / dI, U / I, den, hid and the weights
    C1  MLP grads    the same inputs, with the float64 gy / dPre of B2
    C2  table grads  from the stored dX and the ids (row 0 and ids outside the table get nothing)
    C3  gnorm, coef  from the stored MLP gradients and C2's table gradients
    D   m, v         adam_f64 on the parameters and moments before the step, the stored MLP gradients / C2's table
                     gradients, the stored coef
        p            p0 - lr' m / (sqrt(v) / sqrt_bc2 + eps) from the m and v the step itself stored: no eps region

Bounds (u = 2^-24; first order, SECOND_ORDER = 1.01 covers the (n u)^2 terms and the rounding of the reference)
------
A float32 sum of n products in any order, with or without FMA, is within n u S of the exact value, S = the sum of the
absolute values of the terms; a bias added to it counts as one more term.
    pre   = x W1^T + b1                  (K1 + 1) u S_pre,  S_pre = |x| |W1|^T + |b1|
    hid   = keep ? relu(pre) scale : 0   relu is 1-Lipschitz, one product:  scale (K1 + 1) u S_pre + u |hid|
    y     = hid W2^T + b2                e_y = (H + 1) u S_y
    ss    = sum y^2                      e_ss = sum 2 |y| e_y + (D + 1) u ss
    den   = max(sqrt(ss), 1e-12)         e_den = e_ss / (2 sqrt(ss)) + SQRT_ULPS ulp
    out   = y / den                      e_out = e_y / den + |out| e_den / den + DIV_ULPS ulp
    delta = sum U (P - N)                e_delta = (2 D + 2) u S_delta,  S_delta = sum |U| (|P| + |N|)  (covers both
                                         u (p - n) and u p - u n)
    w     = -1 / (1 + exp(delta)) / B    the fast exponential is within EXP_ULPS(x) = 2 + 1.16 |x| ulp (the figure the
                                         CUDA and HIP programming guides state for __expf); d ln w / d ln e = sigma(delta):
                                         e_w = |w| (sigma(delta) (e_delta + EXP_ULPS ulp) + W_ROUNDINGS u)
                                         (W_ROUNDINGS = 8: 1 + e, the reciprocal at 2 ulp, 1 / B and the product with it)
    dU    = w (P - N)                    e_w |P - N| + 2 u |w| (|P| + |N|)
    dI    = +-w U                        e_w |U| + u |w U|
    loss  = mean softplus(-delta)        softplus' = sigma(-delta); t = exp(-|delta|):
                                         per row sigma(-delta) e_delta + EXP_ULPS ulp t / (1 + t) + LOG1P_ULPS ulp log1p(t)
                                         + u softplus;  the mean is taken in float64 and rounded once: + 2 u |loss|
    gy, dh, dPre, dX, dW1, db1, dW2, db2  the derivation of tests/tower_reference.py (backward_with_bounds) with
                                         depth = the number of batch rows (any order of the batch sum)
    table gradient row                   hits u sum |dX rows|   (hits = samples of the row)
    gnorm = sqrt(sum g^2)                the squares are summed in float64 from float32 gradients: the table part differs
                                         from the reference's by e_G:  sum |G| e_G / gnorm + NORM_ULPS ulp
    coef  = min(1, max_norm / (gnorm + 1e-6))   coef e_gnorm / gnorm + NORM_ULPS ulp
    m     = b1 m0 + (1 - b1) g'          M_U u S_m + (1 - b1) coef e_G          g' = coef g + wd p,  A = |coef g| + |wd p|
                                         S_m = |b1 m0| + (1 - b1) A   (coef g and wd p may cancel in g')
    v     = b2 v0 + (1 - b2) g'^2        V_U u S_v + (1 - b2) (2 A + coef e_G) coef e_G,  S_v = b2 v0 + (1 - b2) A^2
    p     = p0 - lr' m / denom           P_ULPS ulp(|p|) + UPD_ULPS ulp(|upd|)
1 ulp(x) is taken as 2 u |x|.  The worst-case rounding counts of the element-wise Adam chains are 6 for m (coef g, wd p,
their sum, the two products with b1 and 1 - b1, the sum) and 10 for v (g' to 3 u A, doubled by the square, the square,
the two products, the sum); a plain float32 evaluation comes within about half of them, so M_U = 15 and V_U = 25 are
2.5 times the counts: the factor four of the cap condition below, taken from the reference's own error.  P_ULPS = 2 and
UPD_ULPS = 8 (sqrt, two divisions, + eps, the product, the two float32 step constants; then the final subtraction) on
the same grounds: the final subtraction alone rounds by up to u |p|.  No constant is fitted to a kernel.

Cap
---
No tolerance exceeds CAP = 2^-12 times the largest |reference| of its tensor; where the derived bound is larger (the
n u bound of a 4096-term batch sum is), the tolerance is the cap.  tests/test_step_host.py runs a plain float32 step
with every sum taken sequentially (f32_step below) through the same check with slack = 1/4: a case whose tolerance the
reference alone cannot meet with a factor four to spare fails on the CPU when it is built.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

from oracle import fixtures as fx
from oracle import optim_np as R
from oracle import two_tower_np as O

import tower_reference as T

F32, F64, I64 = np.float32, np.float64, np.int64
U = 2.0 ** -24
ULP = 2.0 * U
CAP = 2.0 ** -12
SECOND_ORDER = 1.01
SQRT_ULPS, DIV_ULPS, LOG1P_ULPS, NORM_ULPS = 1.0, 1.5, 2.0, 2.0
W_ROUNDINGS = 8.0
M_U, V_U, P_ULPS, UPD_ULPS = 15.0, 25.0, 2.0, 8.0
B1, B2, EPS = 0.9, 0.999, 1e-8
EPS32 = float(F32(1e-12))
N_GENRES = 18
NWG, SCAT_LIST, GTM = 256, 4096, 32          # workgroups of the one-launch step, its scatter list, rows per tower tile

TOWERS = ("user_tower", "item_tower")
MLP = ("mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias")
MLP_KEYS = tuple(f"{t}.{k}" for t in TOWERS for k in MLP)                  # the trainer's flat-buffer order
TAB_KEYS = tuple(f"{t}.embedding.weight" for t in TOWERS)
ALL_KEYS = MLP_KEYS + TAB_KEYS


def exp_ulps(x):
    return 2.0 + 1.16 * np.abs(x)


# ------------------------------------------------------------------------------------------------------------------- #
# Cases                                                                                                                #
# ------------------------------------------------------------------------------------------------------------------- #
#        name          d    H    B     p    train  wd    max_norm
_CASES = (
    ("one_row",        32,  64,  1,    0.5, True,  1e-2, 1e-3),
    ("tile_boundary",  48,  96,  33,   0.5, True,  0.0,  1.0),
    ("min_width",      16,  16,  40,   0.5, False, 0.0,  1.0),
    ("odd_widths",     240, 208, 70,   0.5, True,  1e-2, 1e-3),
    ("second_wgrad",   256, 256, 96,   0.5, False, 0.0,  1.0),
    ("max_batch",      32,  32,  2048, 0.0, True,  1e-2, 1.0),
    ("full_list",      32,  32,  2048, 0.0, True,  0.0,  1e-3),
)
CASE_NAMES = tuple(c[0] for c in _CASES)
HOST_CASES = (("host_a", 16, 32, 5, 0.5, True, 0.0, 1e-3), ("host_b", 32, 16, 37, 0.0, True, 1e-2, 1.0))
NU, NI = 300, 200
LRS = (5e-3, 2e-3, 2e-3)                     # the lr changes before step 2
SEED = 5


def trainer_seed(seed):
    """s0 of trainer.py (single GPU: rank 0)"""
    return (seed * 1000003) & ((1 << 62) - 1)


def _batches(name, B, rng):
    out = []
    for k in range(3):
        u = rng.integers(1, NU + 1, size=B).astype(I64)
        it = rng.integers(1, NI + 1, size=2 * B).astype(I64)
        if name in ("max_batch", "full_list"):
            # users: rows 1 and 257 have the same owner (id % 256) and alternate with a third row of that owner and with
            # rows of other owners; positions that are equal mod 256 hold different rows
            u[0::3] = 1
            u[1::3] = 257
            u[5::7] = 1 + 256 * (k % 2)
            it = rng.integers(1, 4, size=2 * B).astype(I64) if name == "max_batch" else np.full(2 * B, 5, dtype=I64)
        else:
            if B > 1:
                u[B // 2] = u[0]                                   # duplicates
                it[B - 1] = it[0]; it[B] = it[0]                   # the same item as positive and as negative
            # the padding row at a user, a positive and a negative position (one of them per step when B = 1)
            if B == 1:
                if k == 1:
                    u[0] = 0
                if k == 2:
                    it[1] = 0
            else:
                u[(3 + k) % B] = 0
                it[(1 + 2 * k) % B] = 0
                it[B + (2 + k) % B] = 0
        # positives carry genres of the first half, negatives of the second: the pos and neg halves of the item tower's
        # batch sums (gradients +w U and -w U) do not cancel each other, so the sums stay well conditioned
        g = np.zeros((2 * B, N_GENRES), dtype=F32)
        g[:B, :9] = rng.random((B, 9)) < 0.4
        g[B:, 9:] = rng.random((B, 9)) < 0.4
        out.append((u, it, g))
    return out


@functools.lru_cache(maxsize=None)
def make_case(name):
    row = next(c for c in _CASES + HOST_CASES if c[0] == name)
    _, d, H, B, p, train, wd, max_norm = row
    rng = np.random.default_rng(1000 + (CASE_NAMES + tuple(c[0] for c in HOST_CASES)).index(name))
    sd = fx.make_state(NU, NI, d, H, seed=11)
    assert np.abs(sd[TAB_KEYS[0]][0]).min() > 0 and np.abs(sd[TAB_KEYS[1]][0]).min() > 0      # the padding rows are visible
    c = SimpleNamespace(name=name, d=d, H=H, B=B, p=p, train=train, wd=wd, max_norm=max_norm, lrs=LRS, seed=SEED,
                        sd=sd, batches=_batches(name, B, rng), nu1=NU + 1, ni1=NI + 1)
    c.dropout = bool(train and p > 0)
    c.scale = float(F32(1.0) / (F32(1.0) - F32(p))) if c.dropout else 1.0
    return c


def initial_state(c):
    P = {k: c.sd[k].copy() for k in ALL_KEYS}
    return SimpleNamespace(p=P, m={k: np.zeros_like(v) for k, v in P.items()}, v={k: np.zeros_like(v) for k, v in P.items()})


def keep_masks(c, t):
    """(user [B, H], item [2B, H]) keep masks of the step whose clock reads t, or (None, None)"""
    if not c.dropout:
        return None, None
    out = []
    for seed, rows in ((trainer_seed(c.seed), c.B), (trainer_seed(c.seed) + 1, 2 * c.B)):
        s = SimpleNamespace(seed=seed, step=t)
        out.append(O.dropout_keep_mask(T.seed_eff(s), 0, rows, c.H, c.p))
    return tuple(out)


def schedule(c):
    """tile and iteration counts of the one-launch step for this case"""
    d, H, B = c.d, c.H, c.B
    wt = lambda K1: -(-H // 32) * (-(-(K1 + 1) // 32)) + -(-d // 32) * (-(-(H + 1) // 32))
    nw = wt(d) + wt(d + N_GENRES)
    own = lambda ids, n: np.bincount(ids[(ids >= 1) & (ids < n)] % NWG, minlength=NWG)
    lists = [max(int(own(u, c.nu1).max()), int(own(it, c.ni1).max())) for u, it, _ in c.batches]
    return dict(user_tiles=-(-B // GTM), item_tiles=-(-2 * B // GTM), wgrad_tiles=nw,
                wgrad_second=max(0, nw - NWG), longest_list=max(lists))


# ------------------------------------------------------------------------------------------------------------------- #
# Stages (float64 on whatever they are given)                                                                          #
# ------------------------------------------------------------------------------------------------------------------- #
def _x(table, ids, genres):
    ids = np.asarray(ids)
    table = np.asarray(table, dtype=F64)
    x = table[np.where((ids < 0) | (ids >= table.shape[0]), 0, ids)]
    return x if genres is None else np.concatenate([x, np.asarray(genres, dtype=F64)], axis=1)


def stage_hid(table, ids, genres, W1, b1, keep, scale):
    x = _x(table, ids, genres)
    W1, b1 = np.asarray(W1, dtype=F64), np.asarray(b1, dtype=F64)
    pre = x @ W1.T + b1
    S = np.abs(x) @ np.abs(W1).T + np.abs(b1)
    hid = np.maximum(pre, 0.0)
    e = (x.shape[1] + 1) * U * S
    if keep is not None:
        hid, e = np.where(keep, hid * scale, 0.0), np.where(keep, e * scale, 0.0)
    return SimpleNamespace(x=x, hid=hid, e_hid=SECOND_ORDER * (e + U * np.abs(hid)))


def stage_out(hid, W2, b2):
    hid, W2, b2 = (np.asarray(a, dtype=F64) for a in (hid, W2, b2))
    y = hid @ W2.T + b2
    e_y = (hid.shape[1] + 1) * U * (np.abs(hid) @ np.abs(W2).T + np.abs(b2))
    ss = (y * y).sum(1)
    e_ss = (2.0 * np.abs(y) * e_y).sum(1) + (y.shape[1] + 1) * U * ss
    root = np.sqrt(ss)
    assert root.min() > 1e-6, "a row in the clamp branch of the normalisation: its bound is not derived here"
    den = np.maximum(root, EPS32)
    e_den = e_ss / (2.0 * root) + SQRT_ULPS * ULP * den
    out = y / den[:, None]
    e_out = e_y / den[:, None] + np.abs(out) * (e_den / den)[:, None] + DIV_ULPS * ULP * np.abs(out)
    return SimpleNamespace(den=den, e_den=SECOND_ORDER * e_den, out=out, e_out=SECOND_ORDER * e_out)


def stage_loss(Uo, Io):
    Uo, Io = np.asarray(Uo, dtype=F64), np.asarray(Io, dtype=F64)
    B, D = Uo.shape
    P, N = Io[:B], Io[B:]
    delta = (Uo * (P - N)).sum(1)
    e_delta = (2 * D + 2) * U * (np.abs(Uo) * (np.abs(P) + np.abs(N))).sum(1)
    w = -O.sigmoid(-delta) / B                              # dL / d delta
    e_w = np.abs(w) * (O.sigmoid(delta) * (e_delta + exp_ulps(delta) * ULP) + W_ROUNDINGS * U)
    w, e_w = w[:, None], e_w[:, None]
    dU = w * (P - N)
    e_dU = e_w * np.abs(P - N) + 2 * U * np.abs(w) * (np.abs(P) + np.abs(N))
    dI = np.concatenate([w * Uo, -w * Uo])
    e_dI = np.tile(e_w * np.abs(Uo) + U * np.abs(w * Uo), (2, 1))
    sp = O.softplus(-delta)
    t = np.exp(-np.abs(delta))
    e_sp = O.sigmoid(-delta) * e_delta + exp_ulps(delta) * ULP * t / (1 + t) + LOG1P_ULPS * ULP * np.log1p(t) + U * sp
    loss = sp.mean()
    return SimpleNamespace(delta=delta, dU=dU, e_dU=SECOND_ORDER * e_dU, dI=dI, e_dI=SECOND_ORDER * e_dI, loss=loss,
                           e_loss=SECOND_ORDER * (e_sp.mean() + 2 * U * abs(loss)))


def stage_backward(x, W1, W2, gout, out, den, hid, scale, d):
    """B2 + C1 of one tower: tests/tower_reference.py's float64 backward with depth = the number of batch rows"""
    return T.backward_with_bounds(x, W1, W2, gout, out, den, hid, scale, d, depth=np.asarray(gout).shape[0])


def stage_scatter(n_rows, ids, dX):
    ids, dX = np.asarray(ids), np.asarray(dX, dtype=F64)
    ok = (ids >= 1) & (ids < n_rows)
    G, A = np.zeros((n_rows, dX.shape[1])), np.zeros((n_rows, dX.shape[1]))
    np.add.at(G, ids[ok], dX[ok])
    np.add.at(A, ids[ok], np.abs(dX[ok]))
    hits = np.bincount(ids[ok], minlength=n_rows).astype(F64)[:, None]
    return SimpleNamespace(G=G, e_G=SECOND_ORDER * hits * U * A)


def stage_norm(mlp_grads, tabs, max_norm, exact=False):
    """tabs: the stage_scatter results.  exact: float64 throughout (the comparison with torch), else clip_coef_f32"""
    ss = sum(R.sumsq_f64(g) for g in mlp_grads) + sum(R.sumsq_f64(t.G) for t in tabs)
    if exact:
        tn = math.sqrt(ss)
        return SimpleNamespace(gnorm=tn, coef=min(1.0, max_norm / (tn + 1e-6)), e_gnorm=0.0, e_coef=0.0)
    coef, tn = R.clip_coef_f32(ss, max_norm)
    coef, tn = float(coef), float(tn)
    e_tn = sum(float((np.abs(t.G) * t.e_G).sum()) for t in tabs) / max(tn, 1e-300) + NORM_ULPS * ULP * tn
    e_coef = (coef * e_tn / max(tn, 1e-300) + NORM_ULPS * ULP * coef) if coef < 1.0 else \
        (0.0 if max_norm / (tn + e_tn + 1e-6) >= 1.0 else coef * e_tn / tn + NORM_ULPS * ULP)
    return SimpleNamespace(gnorm=tn, coef=coef, e_gnorm=SECOND_ORDER * e_tn, e_coef=SECOND_ORDER * e_coef)


def stage_adam_mv(p0, g, m0, v0, hyper, wd, coef, e_G=None):
    a = R.adam_f64(p0, g, m0, v0, hyper, F32(B1), F32(B2), F32(EPS), F32(wd), coef)
    e_G = 0.0 if e_G is None else float(F32(coef)) * e_G
    b1, b2 = float(F32(B1)), float(F32(B2))
    # A >= |g'|: coef g and wd p may cancel in g', and their roundings are relative to each of them
    A = np.abs(np.asarray(g, dtype=F64)) * float(F32(coef)) + float(F32(wd)) * np.abs(np.asarray(p0, dtype=F64))
    S_m = b1 * np.abs(np.asarray(m0, dtype=F64)) + (1 - b1) * A
    S_v = b2 * np.abs(np.asarray(v0, dtype=F64)) + (1 - b2) * A * A
    e_m = M_U * U * S_m + (1 - b1) * e_G
    e_v = V_U * U * S_v + (1 - b2) * (2 * A + e_G) * e_G
    return SimpleNamespace(m=a.m, e_m=SECOND_ORDER * e_m, v=a.v, e_v=SECOND_ORDER * e_v, p=a.p)


def stage_adam_p(p0, m, v, hyper, eps=float(F32(EPS))):
    p0, m, v = (np.asarray(a, dtype=F64) for a in (p0, m, v))
    upd = float(hyper[0]) * m / (np.sqrt(v) / float(hyper[1]) + eps)
    p = p0 - upd
    return SimpleNamespace(p=p, upd=upd, e_p=P_ULPS * ULP * np.abs(p) + UPD_ULPS * ULP * np.abs(upd))


# ------------------------------------------------------------------------------------------------------------------- #
# The check: every stage of one step                                                                                   #
# ------------------------------------------------------------------------------------------------------------------- #
def _ratio(got, ref, bound):
    """worst error / tolerance over the elements; tolerance = min(bound, CAP max|ref|); an element whose tolerance is
    zero must be exact"""
    got, ref = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64)
    bound = np.broadcast_to(np.asarray(bound, dtype=F64), ref.shape)
    if got.size == ref.size == 1:
        got = got.reshape(ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return math.inf
    cap = CAP * float(np.abs(ref).max()) if ref.size else 0.0
    tol = np.minimum(bound, cap)
    err = np.abs(got - ref)
    r = np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)
    return float(r.max()) if r.size else 0.0


def tower_params(P, tower):
    return [P[f"{tower}.{k}"] for k in ("embedding.weight",) + MLP]


def check_step(c, k, prev, got, slack=1.0):
    """All stages of step k (0-based) of case c.  prev: the state (p, m, v: float32) before the step; got: what the step
    stored.  Returns {tensor: worst error / tolerance}; raises if one exceeds slack."""
    t = k + 1
    u, it, g = c.batches[k]
    keep = keep_masks(c, t)
    hyper = R.adam_hyper(F32(c.lrs[k]), F32(B1), F32(B2), t)
    r = {}
    tabs = []
    for ti, (tower, ids, gen, sfx, gout_name) in enumerate((("user_tower", u, None, "U", "dU"), ("item_tower", it, g, "I", "dI"))):
        table, W1, b1, W2, b2 = tower_params(prev.p, tower)
        a1 = stage_hid(table, ids, gen, W1, b1, keep[ti], c.scale)
        r["hid" + sfx] = _ratio(got["hid" + sfx], a1.hid, a1.e_hid)
        a2 = stage_out(got["hid" + sfx], W2, b2)
        r["den" + sfx] = _ratio(got["den" + sfx], a2.den, a2.e_den)
        r[sfx] = _ratio(got[sfx], a2.out, a2.e_out)
        if ti == 1:
            b1s = stage_loss(got["U"], got["I"])
            r["dU"] = _ratio(got["dU"], b1s.dU, b1s.e_dU)
            r["dI"] = _ratio(got["dI"], b1s.dI, b1s.e_dI)
            r["loss"] = _ratio(got["loss"], b1s.loss, b1s.e_loss)
    for tower, ids, gen, sfx, gout_name in (("user_tower", u, None, "U", "dU"), ("item_tower", it, g, "I", "dI")):
        table, W1, b1, W2, b2 = tower_params(prev.p, tower)
        bw = stage_backward(_x(table, ids, gen), W1, W2, got[gout_name], got[sfx], got["den" + sfx], got["hid" + sfx],
                            c.scale, c.d)
        r["dX" + sfx.lower()] = _ratio(got["dX" + sfx.lower()], bw.ref.dX, bw.e_dX)
        for key, n in zip(MLP, ("dW1", "db1", "dW2", "db2")):
            r[f"g.{tower}.{key}"] = _ratio(got["g"][f"{tower}.{key}"], bw.grads[n], bw.bounds[n])
        tabs.append(stage_scatter(table.shape[0], ids, got["dX" + sfx.lower()]))
    nrm = stage_norm([got["g"][key] for key in MLP_KEYS], tabs, c.max_norm)
    r["gnorm"] = _ratio(got["gnorm"], nrm.gnorm, nrm.e_gnorm)
    r["coef"] = _ratio(got["coef"], nrm.coef, nrm.e_coef)
    coef = float(got["coef"])
    for key in ALL_KEYS:
        tab = tabs[TAB_KEYS.index(key)] if key in TAB_KEYS else None
        gk = tab.G if tab is not None else got["g"][key]
        mv = stage_adam_mv(prev.p[key], gk, prev.m[key], prev.v[key], hyper, c.wd, coef, None if tab is None else tab.e_G)
        r["m." + key] = _ratio(got["m"][key], mv.m, mv.e_m)
        r["v." + key] = _ratio(got["v"][key], mv.v, mv.e_v)
        pp = stage_adam_p(prev.p[key], got["m"][key], got["v"][key], hyper)
        r["p." + key] = _ratio(got["p"][key], pp.p, pp.e_p)
    r["hyper"] = max(abs(float(got["hyper"][i]) - hyper[i]) / (2 * ULP * hyper[i]) for i in (0, 1))     # 2 ulps
    bad = {n: v for n, v in r.items() if not v <= slack}
    if bad:
        raise AssertionError(f"case {c.name}, step {t}: error / tolerance above {slack}: " +
                             ", ".join(f"{n} {v:.3g}" for n, v in sorted(bad.items(), key=lambda kv: -kv[1])))
    return r


def touched_rows(c):
    """(user rows, item rows) that appear in any of the three batches (row 0 never counts: it gets no gradient)"""
    us = np.unique(np.concatenate([b[0] for b in c.batches]))
    its = np.unique(np.concatenate([b[1] for b in c.batches]))
    return us[(us >= 1) & (us < c.nu1)], its[(its >= 1) & (its < c.ni1)]


# ------------------------------------------------------------------------------------------------------------------- #
# The same step in float64 from end to end (compared with torch in tests/test_step_host.py)                            #
# ------------------------------------------------------------------------------------------------------------------- #
def f64_step(c, k, prev):
    t = k + 1
    u, it, g = c.batches[k]
    keep = keep_masks(c, t)
    hyper = (c.lrs[k] / (1 - B1 ** t), math.sqrt(1 - B2 ** t))
    got = dict(g={}, p={}, m={}, v={})
    for ti, (tower, ids, gen, sfx) in enumerate((("user_tower", u, None, "U"), ("item_tower", it, g, "I"))):
        table, W1, b1, W2, b2 = tower_params(prev.p, tower)
        a1 = stage_hid(table, ids, gen, W1, b1, keep[ti], c.scale)
        a2 = stage_out(a1.hid, W2, b2)
        got["hid" + sfx], got["den" + sfx], got[sfx] = a1.hid, a2.den, a2.out
    ls = stage_loss(got["U"], got["I"])
    got.update(dU=ls.dU, dI=ls.dI, loss=ls.loss)
    tabs = []
    for tower, ids, gen, sfx in (("user_tower", u, None, "U"), ("item_tower", it, g, "I")):
        table, W1, b1, W2, b2 = tower_params(prev.p, tower)
        bw = stage_backward(_x(table, ids, gen), W1, W2, got["d" + sfx], got[sfx], got["den" + sfx], got["hid" + sfx],
                            c.scale, c.d)
        got["dX" + sfx.lower()] = bw.ref.dX
        for key, n in zip(MLP, ("dW1", "db1", "dW2", "db2")):
            got["g"][f"{tower}.{key}"] = bw.grads[n]
        tabs.append(stage_scatter(table.shape[0], ids, bw.ref.dX))
    nrm = stage_norm([got["g"][key] for key in MLP_KEYS], tabs, c.max_norm, exact=True)
    got.update(gnorm=nrm.gnorm, coef=nrm.coef, hyper=hyper, gtab=[tb.G for tb in tabs])
    for key in ALL_KEYS:
        gk = tabs[TAB_KEYS.index(key)].G if key in TAB_KEYS else got["g"][key]
        p0, m0, v0 = (np.asarray(x[key], dtype=F64) for x in (prev.p, prev.m, prev.v))
        gp = gk * nrm.coef + (c.wd * p0 if c.wd != 0 else 0.0)
        got["m"][key] = B1 * m0 + (1 - B1) * gp
        got["v"][key] = B2 * v0 + (1 - B2) * gp * gp
        got["p"][key] = stage_adam_p(p0, got["m"][key], got["v"][key], hyper, eps=EPS).p
    return got


# ------------------------------------------------------------------------------------------------------------------- #
# A plain float32 step, every sum in sequential order (the cap condition)                                              #
# ------------------------------------------------------------------------------------------------------------------- #
def seq_mm32(A, Bm):
    """A [M, K] @ B [K, N] in float32, the K products of an element added one after the other"""
    A, Bm = np.asarray(A, dtype=F32), np.asarray(Bm, dtype=F32)
    acc = np.zeros((A.shape[0], Bm.shape[1]), dtype=F32)
    for kk in range(A.shape[1]):
        acc += A[:, kk:kk + 1] * Bm[kk:kk + 1, :]
    return acc


def seq_sum32(a, axis):
    a = np.moveaxis(np.asarray(a, dtype=F32), axis, 0)
    acc = np.zeros(a.shape[1:], dtype=F32)
    for row in a:
        acc = acc + row
    return acc


def f32_step(c, k, prev):
    t = k + 1
    u, it, g = c.batches[k]
    keep = keep_masks(c, t)
    h64 = R.adam_hyper(F32(c.lrs[k]), F32(B1), F32(B2), t)
    hyper = (F32(h64[0]), F32(h64[1]))
    scale = F32(c.scale)
    got, xs = dict(g={}, p={}, m={}, v={}), {}
    for ti, (tower, ids, gen, sfx) in enumerate((("user_tower", u, None, "U"), ("item_tower", it, g, "I"))):
        table, W1, b1, W2, b2 = tower_params(prev.p, tower)
        x = _x(table, ids, gen).astype(F32)
        hid = np.maximum(seq_mm32(x, W1.T) + b1, F32(0))
        if keep[ti] is not None:
            hid = np.where(keep[ti], hid * scale, F32(0)).astype(F32)
        y = seq_mm32(hid, W2.T) + b2
        den = np.maximum(np.sqrt(seq_sum32(y * y, 1)), F32(1e-12))
        xs[sfx] = x
        got["hid" + sfx], got["den" + sfx], got[sfx] = hid, den, (y / den[:, None]).astype(F32)
    B = c.B
    Uo, P, N = got["U"], got["I"][:B], got["I"][B:]
    delta = seq_sum32(Uo * (P - N), 1)
    w = (F32(-1) / (F32(1) + np.exp(delta, dtype=F32)) * (F32(1) / F32(B))).astype(F32)[:, None]
    got["dU"], got["dI"] = w * (P - N), np.concatenate([w * Uo, -w * Uo])
    sp = np.maximum(-delta, F32(0)) + np.log1p(np.exp(-np.abs(delta), dtype=F32), dtype=F32)
    got["loss"] = F32(sp.astype(F64).sum() / B)
    gtab = []
    for tower, ids, gen, sfx in (("user_tower", u, None, "U"), ("item_tower", it, g, "I")):
        table, W1, b1, W2, b2 = tower_params(prev.p, tower)
        gout, out, den, hid, x = got["d" + sfx], got[sfx], got["den" + sfx], got["hid" + sfx], xs[sfx]
        dot = seq_sum32(gout * out, 1)[:, None]
        gy = ((gout - out * dot) / den[:, None]).astype(F32)
        dpre = np.where(hid > 0, seq_mm32(gy, W2) * scale, F32(0)).astype(F32)
        dX = seq_mm32(dpre, W1)[:, :c.d]
        got["dX" + sfx.lower()] = dX
        for key, val in zip(MLP, (seq_mm32(dpre.T, x), seq_sum32(dpre, 0), seq_mm32(gy.T, hid), seq_sum32(gy, 0))):
            got["g"][f"{tower}.{key}"] = val
        G = np.zeros_like(table)
        for pos, i in enumerate(ids.tolist()):
            if 1 <= i < table.shape[0]:
                G[i] += dX[pos]
        gtab.append(G)
    coef, tn = R.clip_coef_f32(sum(R.sumsq_f64(got["g"][key]) for key in MLP_KEYS) + sum(R.sumsq_f64(G) for G in gtab),
                               c.max_norm)
    got.update(gnorm=tn, coef=coef, hyper=hyper)
    for key in ALL_KEYS:
        gk = gtab[TAB_KEYS.index(key)] if key in TAB_KEYS else got["g"][key]
        p, m, v = prev.p[key].copy(), prev.m[key].copy(), prev.v[key].copy()
        gp = (gk * coef).astype(F32)
        if c.wd != 0.0:
            gp = gp + F32(c.wd) * p
        m = F32(B1) * m + (F32(1) - F32(B1)) * gp
        v = F32(B2) * v + (F32(1) - F32(B2)) * gp * gp
        p = p - hyper[0] * (m / (np.sqrt(v) / hyper[1] + F32(EPS)))
        got["p"][key], got["m"][key], got["v"][key] = p.astype(F32), m.astype(F32), v.astype(F32)
    return got


def next_state(got):
    return SimpleNamespace(p=got["p"], m=got["m"], v=got["v"])
