"""References of the K-negative sampled step (TEST INFRASTRUCTURE; NumPy only, never imports the package).

loss_and_grads_f64          float64 loss and gradients of rihip_bpr_multi_loss from its definition, with a per-element
                            tolerance derived from the operation order the header states
sample_negatives_multi_np   exact integer restatement of rihip_sample_negatives_multi
check_step                  the staged check of tests/step_reference.py with the K-negative loss stage in place of B1
                            (the K-independent stages are imported from there), for the dense and the row-sparse optimiser

Bounds of the loss stage (u = 2^-24, 1 ulp(x) = 2 u |x|; the constants are those of tests/step_reference.py)
------
The header fixes: float32 dot products of d terms in a fixed tree (any order of n products, fused or not, is within
n u S of the exact sum, S = the sum of the absolute products); z = fl(u.p - u.n_k), one rounding; e = expf(-|z|),
sigma(-z) = e / (1 + e) or 1 / (1 + e), g = sigma(-z) * fl(1 / (B K)); k ascending; dN_k = g_k u; s and a are K
sequential float32 additions from 0; dP = -s u; dU = -a.
    z_k    e_z = d u (S_p + S_nk) + u |z_k|
    g_k    d ln sigma(-z) / d ln e = sigma(z), the exponential within exp_ulps(z) ulp of exp(argument):
           e_g = g (sigma(z) (e_z + exp_ulps(z) ulp) + W_ROUNDINGS u)   (1 + e, the quotient, 1 / (B K), the product)
    dN_k   e_g |u| + u |g u|
    s      sum_k e_g + K u s            (K additions, every partial sum at most s)
    dP     e_s |u| + u |s u|
    a      sum_k (e_g |p - n_k| + 2 u g (|p| + |n_k|)) + K u sum_k |g (p - n_k)|
           (the difference and the product round once each, or the product is fused; K additions whose partial sums are
           at most the sum of the absolute terms)
    loss   per pair sigma(-z) e_z + exp_ulps ulp t / (1 + t) + LOG1P_ULPS ulp log1p(t) + u softplus, t = exp(-|z|);
           the mean is taken in float64 and rounded once: + 2 u |loss|
Everything is multiplied by SECOND_ORDER.  Nothing is fitted to a kernel: the tolerance is a function of the inputs."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

import step_reference as S
from oracle import fixtures as fx
from oracle import optim_np as R

F32, F64, I64 = np.float32, np.float64, np.int64
U = S.U
ULP = S.ULP


def _sigmoid(x):
    x = np.asarray(x, dtype=F64)
    t = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + t), t / (1.0 + t))


def _softplus(x):
    x = np.asarray(x, dtype=F64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def loss_f64(Uo, P, N) -> float:
    """L = 1/(B K) sum_ik softplus(-(u_i.p_i - u_i.n_ik)); N is [K, B, d]"""
    Uo, P, N = (np.asarray(a, dtype=F64) for a in (Uo, P, N))
    z = (Uo * P).sum(1)[None, :] - np.einsum("bd,kbd->kb", Uo, N)
    return float(_softplus(-z).mean())


def loss_and_grads_f64(Uo, P, N):
    """Uo, P [B, d]; N [K, B, d].  loss, dU, dP [B, d], dN [K, B, d] and their tolerances e_*."""
    Uo, P, N = (np.asarray(a, dtype=F64) for a in (Uo, P, N))
    K, B, d = N.shape
    assert Uo.shape == P.shape == (B, d)
    inv = 1.0 / (B * K)
    aU, aP, aN = np.abs(Uo), np.abs(P), np.abs(N)
    sp, S_p = (Uo * P).sum(1), (aU * aP).sum(1)
    sn, S_n = np.einsum("bd,kbd->kb", Uo, N), np.einsum("bd,kbd->kb", aU, aN)
    z = sp[None, :] - sn                                          # [K, B]
    e_z = d * U * (S_p[None, :] + S_n) + U * np.abs(z)
    g = _sigmoid(-z) * inv
    e_g = g * (_sigmoid(z) * (e_z + S.exp_ulps(z) * ULP) + S.W_ROUNDINGS * U)
    dN = g[:, :, None] * Uo[None]
    e_dN = e_g[:, :, None] * aU[None] + U * np.abs(dN)
    s = g.sum(0)
    e_s = e_g.sum(0) + K * U * s
    dP = -s[:, None] * Uo
    e_dP = e_s[:, None] * aU + U * np.abs(dP)
    diff = P[None] - N
    term = g[:, :, None] * diff
    dU = -term.sum(0)
    e_dU = (e_g[:, :, None] * np.abs(diff) + 2 * U * g[:, :, None] * (aP[None] + aN)).sum(0) + K * U * np.abs(term).sum(0)
    spl = _softplus(-z)
    t = np.exp(-np.abs(z))
    e_sp = _sigmoid(-z) * e_z + S.exp_ulps(z) * ULP * t / (1 + t) + S.LOG1P_ULPS * ULP * np.log1p(t) + U * spl
    loss = spl.mean()
    so = S.SECOND_ORDER
    return SimpleNamespace(z=z, loss=loss, e_loss=so * (e_sp.mean() + 2 * U * abs(loss)), dU=dU, e_dU=so * e_dU,
                           dP=dP, e_dP=so * e_dP, dN=dN, e_dN=so * e_dN)


# ------------------------------------------------------------------------------------------------------------------- #
# Sampler                                                                                                              #
# ------------------------------------------------------------------------------------------------------------------- #
_M64 = (1 << 64) - 1


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def sample_negatives_multi_np(users, K, catalog, alias_prob, alias_idx, rated_keys, key_stride, seed, max_attempts):
    """(neg [K n] k-major, gave_up).  Slot s = k n + i, attempt a: r = splitmix64(splitmix64(seed ^ splitmix64(s)) + a),
    column j = ((r >> 32) n_catalog) >> 32; uniform (alias_prob is None): pick = j; weighted: pick = j when
    (uint32) r < alias_prob[j], else alias_idx[j] (read as j when outside [0, n_catalog)).  The slot keeps the first
    catalog[pick] whose key users[i] key_stride + catalog[pick] is not in rated_keys (sorted); after max_attempts it keeps
    the last one and counts as given up."""
    users = np.asarray(users, dtype=I64)
    catalog = np.asarray(catalog, dtype=I64)
    rated = np.asarray(rated_keys, dtype=I64)
    n, nc = users.shape[0], catalog.shape[0]
    assert (alias_prob is None) == (alias_idx is None)
    if alias_prob is not None:
        alias_prob = np.asarray(alias_prob).astype(np.uint64)
        alias_idx = np.asarray(alias_idx).astype(I64)
    ns = K * n
    slot = np.arange(ns, dtype=np.uint64)
    base = splitmix64(np.uint64(seed & _M64) ^ splitmix64(slot))
    usr = users[np.arange(ns) % n] if n else users
    neg = np.full(ns, catalog[0], dtype=I64)
    ok = np.zeros(ns, dtype=bool)
    for a in range(max_attempts):
        live = np.flatnonzero(~ok)
        if live.size == 0:
            break
        with np.errstate(over="ignore"):
            r = splitmix64(base[live] + np.uint64(a))
            j = (((r >> np.uint64(32)) * np.uint64(nc)) >> np.uint64(32)).astype(I64)
        if alias_prob is not None:
            coin = r & np.uint64(0xFFFFFFFF)
            al = alias_idx[j]
            al = np.where((al < 0) | (al >= nc), j, al)
            j = np.where(coin < alias_prob[j], j, al)
        pick = catalog[j]
        key = usr[live] * I64(key_stride) + pick
        if rated.shape[0]:
            at = np.searchsorted(rated, key)
            member = (at < rated.shape[0]) & (rated[np.minimum(at, rated.shape[0] - 1)] == key)
        else:
            member = np.zeros(live.size, dtype=bool)
        neg[live] = pick
        ok[live] = ~member
    return neg, int((~ok).sum())


def wilson_hilferty(chi2: float, dof: int) -> float:
    """normal score of a chi-square value with dof degrees of freedom"""
    v = 2.0 / (9.0 * dof)
    return ((chi2 / dof) ** (1.0 / 3.0) - (1.0 - v)) / math.sqrt(v)


def chi2_score(counts, prob) -> float:
    """Wilson-Hilferty score of Pearson's chi-square of `counts` against `prob` (cells of probability zero must be
    empty and do not count)"""
    counts, prob = np.asarray(counts, dtype=F64), np.asarray(prob, dtype=F64)
    live = prob > 0
    assert not counts[~live].any(), "a draw in a cell of probability zero"
    e = prob[live] / prob[live].sum() * counts.sum()
    chi2 = float(((counts[live] - e) ** 2 / e).sum())
    dof = int(live.sum()) - 1
    return wilson_hilferty(chi2, dof) if dof > 0 else 0.0


# ------------------------------------------------------------------------------------------------------------------- #
# Trainer cases and the staged check                                                                                   #
# ------------------------------------------------------------------------------------------------------------------- #
#        name       d    H    B    K  wd    max_norm  sparse
_CASES = (
    ("k3_dense",    32,  64,  96,  3, 1e-2, 1e-3,     False),
    ("k2_dense",    48,  96,  70,  2, 0.0,  1.0,      False),
    ("k4_sparse",   64,  128, 128, 4, 1e-2, 1.0,      True),
)
CASE_NAMES = tuple(c[0] for c in _CASES)


def _batches(B, K, sparse, rng):
    out = []
    nI = (1 + K) * B
    for k in range(3):
        if sparse:      # rows beyond 150 / 120 stay idle; no padding id: row 0 must not move
            u = rng.integers(1, 151, size=B).astype(I64)
            it = rng.integers(1, 121, size=nI).astype(I64)
        else:
            u = rng.integers(1, S.NU + 1, size=B).astype(I64)
            it = rng.integers(1, S.NI + 1, size=nI).astype(I64)
            u[(3 + k) % B] = 0                                   # the padding row as a user, a positive, a negative
            it[(1 + 2 * k) % B] = 0
            it[B * (1 + k % K) + (2 + k) % B] = 0
        u[B // 2] = u[0]                                         # duplicates
        it[B - 1] = it[0]; it[B] = it[0]; it[K * B + 1] = it[0]  # one item as a positive and as negatives 0 and K-1
        it[2 * B + 5] = it[B + 5]                                # a sample with the same negative twice
        # positives carry genres of the first half, negatives of the second (step_reference._batches: the halves of the
        # item tower's batch sums then do not cancel)
        g = np.zeros((nI, S.N_GENRES), dtype=F32)
        g[:B, :9] = rng.random((B, 9)) < 0.4
        g[B:, 9:] = rng.random((nI - B, 9)) < 0.4
        out.append((u, it, g))
    return out


@functools.lru_cache(maxsize=None)
def make_case(name):
    _, d, H, B, K, wd, max_norm, sparse = next(c for c in _CASES if c[0] == name)
    rng = np.random.default_rng(7000 + CASE_NAMES.index(name))
    sd = fx.make_state(S.NU, S.NI, d, H, seed=11)
    c = SimpleNamespace(name=name, d=d, H=H, B=B, K=K, p=0.0, train=True, wd=wd, max_norm=max_norm, sparse=sparse,
                        lrs=S.LRS, seed=S.SEED, sd=sd, batches=_batches(B, K, sparse, rng), nu1=S.NU + 1, ni1=S.NI + 1,
                        dropout=False, scale=1.0)
    return c


def stage_loss(Uo, Io, K):
    """B1 with K negatives: I = pos || neg_0 || ... || neg_(K-1)"""
    Uo, Io = np.asarray(Uo, dtype=F64), np.asarray(Io, dtype=F64)
    B, d = Uo.shape
    r = loss_and_grads_f64(Uo, Io[:B], Io[B:].reshape(K, B, d))
    return SimpleNamespace(dU=r.dU, e_dU=r.e_dU, dI=np.concatenate([r.dP, r.dN.reshape(K * B, d)]),
                           e_dI=np.concatenate([r.e_dP, r.e_dN.reshape(K * B, d)]), loss=r.loss, e_loss=r.e_loss)


def check_step(c, k, prev, got, slack=1.0):
    """tests/step_reference.check_step with stage_loss above; c.sparse: the row-sparse optimiser, whose tables move in
    the rows of the batch only (those rows are checked against the same Adam stage, the others must hold prev's bits)."""
    t = k + 1
    u, it, g = c.batches[k]
    hyper = R.adam_hyper(F32(c.lrs[k]), F32(S.B1), F32(S.B2), t)
    r, tabs = {}, []
    towers = (("user_tower", u, None, "U", "dU"), ("item_tower", it, g, "I", "dI"))
    for tower, ids, gen, sfx, _ in towers:
        table, W1, b1, W2, b2 = S.tower_params(prev.p, tower)
        a1 = S.stage_hid(table, ids, gen, W1, b1, None, 1.0)
        r["hid" + sfx] = S._ratio(got["hid" + sfx], a1.hid, a1.e_hid)
        a2 = S.stage_out(got["hid" + sfx], W2, b2)
        r["den" + sfx] = S._ratio(got["den" + sfx], a2.den, a2.e_den)
        r[sfx] = S._ratio(got[sfx], a2.out, a2.e_out)
    ls = stage_loss(got["U"], got["I"], c.K)
    r["dU"] = S._ratio(got["dU"], ls.dU, ls.e_dU)
    r["dI"] = S._ratio(got["dI"], ls.dI, ls.e_dI)
    r["loss"] = S._ratio(got["loss"], ls.loss, ls.e_loss)
    for tower, ids, gen, sfx, gout_name in towers:
        table, W1, b1, W2, b2 = S.tower_params(prev.p, tower)
        bw = S.stage_backward(S._x(table, ids, gen), W1, W2, got[gout_name], got[sfx], got["den" + sfx],
                              got["hid" + sfx], 1.0, c.d)
        r["dX" + sfx.lower()] = S._ratio(got["dX" + sfx.lower()], bw.ref.dX, bw.e_dX)
        for key, n in zip(S.MLP, ("dW1", "db1", "dW2", "db2")):
            r[f"g.{tower}.{key}"] = S._ratio(got["g"][f"{tower}.{key}"], bw.grads[n], bw.bounds[n])
        tabs.append(S.stage_scatter(table.shape[0], ids, got["dX" + sfx.lower()]))
    nrm = S.stage_norm([got["g"][key] for key in S.MLP_KEYS], tabs, c.max_norm)
    r["gnorm"] = S._ratio(got["gnorm"], nrm.gnorm, nrm.e_gnorm)
    r["coef"] = S._ratio(got["coef"], nrm.coef, nrm.e_coef)
    coef = float(got["coef"])
    for key in S.ALL_KEYS:
        tab = tabs[S.TAB_KEYS.index(key)] if key in S.TAB_KEYS else None
        gk = tab.G if tab is not None else got["g"][key]
        rows = slice(None)
        if tab is not None and c.sparse:
            ids = (u, it)[S.TAB_KEYS.index(key)]
            rows = np.unique(ids[(ids >= 1) & (ids < gk.shape[0])])
            idle = np.setdiff1d(np.arange(gk.shape[0]), rows)
            for grp in ("p", "m", "v"):
                same = np.array_equal(got[grp][key][idle].view(np.uint32), getattr(prev, grp)[key][idle].view(np.uint32))
                r[f"idle.{grp}.{key}"] = 0.0 if same else math.inf
        e_G = None if tab is None else tab.e_G[rows]
        mv = S.stage_adam_mv(prev.p[key][rows], gk[rows], prev.m[key][rows], prev.v[key][rows], hyper, c.wd, coef, e_G)
        r["m." + key] = S._ratio(got["m"][key][rows], mv.m, mv.e_m)
        r["v." + key] = S._ratio(got["v"][key][rows], mv.v, mv.e_v)
        pp = S.stage_adam_p(prev.p[key][rows], got["m"][key][rows], got["v"][key][rows], hyper)
        r["p." + key] = S._ratio(got["p"][key][rows], pp.p, pp.e_p)
    r["hyper"] = max(abs(float(got["hyper"][i]) - hyper[i]) / (2 * ULP * hyper[i]) for i in (0, 1))
    bad = {n: v for n, v in r.items() if not v <= slack}
    if bad:
        raise AssertionError(f"case {c.name}, step {t}: error / tolerance above {slack}: " +
                             ", ".join(f"{n} {v:.3g}" for n, v in sorted(bad.items(), key=lambda kv: -kv[1])))
    return r

