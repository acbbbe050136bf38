"""Host side of the in-batch BPR pass tests (TEST INFRASTRUCTURE; NumPy only, no GPU, no torch).

Four things.  The inputs, the expectations, the semantics and the bounds (1, 2, 4) are written from
include/recommendit_hip.h and the comments of recommendit_amd/csrc/loss_sweep_args.h.  The schedule mirror (3) is a
deliberate line-by-line restatement of the tile loops of recommendit_amd/csrc/loss.hip (same names: s_lim, band_lo,
rel, the `end` expression): it is not independent of them, and tests/test_inbatch_host.py holds it to brute-force
invariants that are.

1.  EXACT INPUTS ("ternary G").  ``pos`` is an input pointer of the passes, so the tests pass ``pos = 0`` and choose
    rows whose every score is a multiple of 256: the "hot" side (the users) has rows 16 s1 e_a + 16 s2 e_b (a != b,
    s = +-1), the "ternary" side (the items) has entries in {-16, 0, 16}.  Then s_ij in {0, +-256, +-512}; in the
    kernels' log2 units the products are 0 or +-P with P = fl(16 log2 e) * 16 (an exact scaling of one rounded
    number), so the chain gives exactly 0, +-P or about +-2P in any order, for the exact-f32 MFMA and for the
    split-bf16 forms (the pieces h, h + m, h + m + l of P are prefixes of its mantissa: every partial sum is
    representable).  exp2 of -+369 is +inf / 0, so the weight sigma(z) is exactly 0.5, 0 or 1 -- provided
    rcp(2) == 0.5 on the device, which the first GPU test pins.  With ``n_global = 2`` the scale c = 1/(B(B-1)) is 1/2
    and every partial sum of G.Y, G^T.U, r and the -r.y correction is a multiple of 1/8 far below 2^24: exact in f32
    in any order and under any swept-range split.  The loss overflows by design at such scores and is not looked at.

2.  THE SEMANTICS PINNED (``ExactCase`` / ``expected_*``).  A row's global index is its offset argument plus its local
    index; the header says only that the offsets "place a rank's local rows inside the all-gathered batch".
      * a pair (owner o, swept s) is "diagonal" iff o_goff + o == s_goff + s.  User mode: weight 0, not in r, not in
        the loss.  mode_user=0 sweep: the pair's weight is replaced by -r_in[s] / c (so that d_owner gets -r_s y_s).
      * user mode: d_owner[o] = c sum_s w_os y_s - r_o y_drow with drow = o_goff + o - s_goff, the owner's positive
        partner inside the swept set; r_o = c sum_s w_os.  The header is SILENT on a partner outside the swept set
        (drow < 0 or >= n_swept): the code applies no correction and masks nothing, and that is what is pinned here.
      * stored-G item pass: d_items[j] = c sum_i gmat[j][i] u_i - r[drow] u_drow, drow = item_goff + j - user_goff,
        no correction outside [0, n_users) (header: "over the LOCAL users for ALL n_items items").
      * gmat: element (item j, user i) at ((j//32) g_ub + i//32) 1024 + (j%32) 32 + i%32, g_ub = 8 ceil(n_users/256);
        0 on the diagonal and in ragged slots of every block the item pass multiplies (header: "0 on the diagonal").
        The header is silent on which other blocks are written; pinned: nothing but 0 or the caller's prefill.

3.  A MIRROR OF THE TILE SCHEDULE (``sweep_schedule`` / ``gt_schedule`` / ``sweep_nw`` / ``sweep_nsplit`` / ...): per
    workgroup and split, which swept tiles run in the lead-in, the steady trips before the band, the band, the steady
    trips after it, the one-tile "fill" between those, and the tail.  tests/test_inbatch_host.py checks the mirror's own
    invariants by brute force and that the chosen cases reach every region.

4.  REALISTIC VALUES (``realistic_reference`` / ``bound_gmat`` / ``bound_sums``): fp64 weights, r, dU, dI and loss
    parts with the UN-CANCELLED magnitudes the derived bounds are relative to (as tests/lambdarank_reference.py does).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

OW, TSW, NCU = 128, 32, 256          # owners per loss slot, swept rows per tile, RIHIP_NCU
U32 = 2.0 ** -24                     # unit roundoff of f32
C_EXACT = 0.5                        # c = 1/(B(B-1)) at n_global = 2
N_GLOBAL_EXACT = 2


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# 3. mirror of the launch arithmetic and of the tile schedule
# ---------------------------------------------------------------------------------------------------------------------
def sweep_nw(n_owner: int, n_swept: int, forced: Optional[int] = None) -> int:
    """workgroup waves; `forced` = the value of RIHIP_SWEEP_NW (read once per process), None when unset"""
    if forced is not None:
        return 8 if forced == 8 else 4
    return 8 if (n_owner >= 4096 and n_swept >= 16384) else 4


def sweep_nsplit(n_owner: int, n_swept: int, nw: int = 4) -> int:
    tiles, gx4 = cdiv(n_swept, TSW), cdiv(n_owner, OW)
    ns4 = max(1, min(16, tiles, cdiv(2 * NCU, gx4)))
    if nw == 4:
        return ns4
    gx8 = cdiv(n_owner, 2 * OW)
    return max(1, min(ns4, cdiv(NCU, gx8)))


def loss_parts(n_owner: int, n_swept: int, forced: Optional[int] = None) -> int:
    return cdiv(n_owner, OW) * sweep_nsplit(n_owner, n_swept, sweep_nw(n_owner, n_swept, forced))


def workspace_floats(n_owner: int, n_swept: int, d: int) -> int:
    ns = sweep_nsplit(n_owner, n_swept)
    return ns * n_owner * (d + 1) if ns > 1 else 1


def g_ub(n_users: int) -> int:
    return 8 * cdiv(n_users, 2 * OW)


def gmat_floats(n_users: int, n_items: int) -> int:
    return g_ub(n_users) * g_ub(n_items) * 1024


def sweep_steady(d: int, mode_user: bool, gout: bool, nw: int) -> bool:
    return d == 128 and mode_user and gout and nw == 8


def gt_steady(d: int, nw: int) -> bool:
    return d == 128 and nw == 8


def split_range(n_swept: int, nsplit: int, by: int) -> Tuple[int, int]:
    ntiles = cdiv(n_swept, TSW)
    per = cdiv(ntiles, nsplit)
    t0 = by * per
    return t0, min(t0 + per, ntiles)


REGIONS = ("lead", "steady_pre", "fill", "band", "steady_post", "tail")


def sweep_schedule(n_owner: int, o_goff: int, n_swept: int, s_goff: int, nw: int, nsplit: int, bx: int, by: int,
                   steady: bool) -> Dict[str, List[int]]:
    """Tiles of workgroup (bx, by) of the f32 sweep kernel by loop region, in execution order within each region.

    Without a steady loop every tile runs in the one-tile loop ("lead").  With it: three lead-in tiles (one turn of the
    LDS ring), then trips of six steady tiles wherever ring position 0 meets a run of >= 6 tiles that are full, off the
    workgroup's diagonal band and two tiles before the end of the split's full tiles; the band, the ring-alignment
    "fill" and the "tail" go one tile at a time."""
    t0, t1 = split_range(n_swept, nsplit, by)
    out: Dict[str, List[int]] = {k: [] for k in REGIONS}
    if t0 >= t1:
        return out
    lead_end = t0 + 3 if (steady and t0 + 3 < t1) else t1
    out["lead"] = list(range(t0, lead_end))
    if not steady:
        return out
    ntl = t1 - t0

    def rel(t: int) -> int:
        return min(max(t - t0, 0), ntl)

    nfull = n_swept // TSW
    wg_full = (bx + 1) * nw * 32 <= n_owner
    s_lim = rel(min(t1, nfull) - 2) if wg_full else 0
    ddw = o_goff + bx * nw * 32 - s_goff
    band_lo, band_hi = rel(ddw >> 5), rel((ddw + nw * 32 + 31) >> 5)
    rt = lead_end - t0
    general: List[int] = []
    steady_tiles: List[int] = []
    while True:
        n = 0
        if rt % 3 == 0:
            end = min(band_lo, s_lim) if rt < band_lo else (s_lim if rt >= band_hi else rt)
            n = (end - rt) // 6 * 6 if end > rt else 0
        if n > 0:
            steady_tiles += list(range(rt, rt + n))
            rt += n
        if rt >= ntl:
            break
        general.append(rt)
        rt += 1
    last_steady = steady_tiles[-1] if steady_tiles else -1
    for t in steady_tiles:
        out["steady_pre" if t < band_lo else "steady_post"].append(t0 + t)
    for t in general:
        key = "band" if band_lo <= t < band_hi else ("tail" if t > last_steady else "fill")
        out[key].append(t0 + t)
    return out


def gt_schedule(n_owner: int, n_swept: int, nsplit: int, by: int, steady: bool) -> Dict[str, List[int]]:
    """Tiles of split `by` of the f32 stored-G item kernel (the same for every workgroup: it has no band)."""
    t0, t1 = split_range(n_swept, nsplit, by)
    out: Dict[str, List[int]] = {k: [] for k in REGIONS}
    if t0 >= t1:
        return out
    lead_end = t0 + 3 if (steady and t0 + 3 < t1) else t1
    out["lead"] = list(range(t0, lead_end))
    if not steady:
        return out
    s_lim = min(t1, n_swept // TSW) - 2
    s_end = lead_end + (s_lim - lead_end) // 3 * 3 if s_lim > lead_end else lead_end
    out["steady_pre"] = list(range(lead_end, s_end))
    out["tail"] = list(range(s_end, t1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# gmat layout
# ---------------------------------------------------------------------------------------------------------------------
def decode_gmat(flat: np.ndarray, n_users: int, n_items: int) -> np.ndarray:
    """flat blocked G^T -> [g_ub(n_items) * 32, g_ub(n_users) * 32] array indexed [item, user] (a copy)"""
    ub, ib = g_ub(n_users), g_ub(n_items)
    assert flat.shape == (ub * ib * 1024,), (flat.shape, ub, ib)
    return flat.reshape(ib, ub, 32, 32).transpose(0, 2, 1, 3).reshape(ib * 32, ub * 32)


def encode_gmat(full: np.ndarray, n_users: int, n_items: int) -> np.ndarray:
    """inverse of decode_gmat"""
    ub, ib = g_ub(n_users), g_ub(n_items)
    assert full.shape == (ib * 32, ub * 32), (full.shape, ub, ib)
    return np.ascontiguousarray(full.reshape(ib, 32, ub, 32).transpose(0, 2, 1, 3)).reshape(-1)


def check_gmat(flat: np.ndarray, weights: np.ndarray, n_users: int, n_items: int) -> None:
    """`flat` (prefilled with NaN by the caller) against `weights` [n_items, n_users] (diagonal already 0).

    Inside the 32x32 blocks that hold an in-range element (the blocks the item pass multiplies): bit-for-bit the
    expectation, with 0 in the ragged slots.  Everywhere else: 0 or the NaN prefill, never another number."""
    assert weights.shape == (n_items, n_users)
    full = decode_gmat(np.asarray(flat), n_users, n_items)
    ni, nu = cdiv(n_items, 32) * 32, cdiv(n_users, 32) * 32
    exp = np.zeros((ni, nu), dtype=np.float32)
    exp[:n_items, :n_users] = weights
    got = full[:ni, :nu]
    if not np.array_equal(got, exp):
        bad = np.argwhere(~(got == exp))
        j, i = bad[0]
        kind = "ragged slot" if (j >= n_items or i >= n_users) else "element"
        raise AssertionError(f"gmat: {len(bad)} wrong entries; first {kind} (item {j}, user {i}): "
                             f"got {got[j, i]!r}, expected {exp[j, i]!r}")
    rest = np.ones(full.shape, dtype=bool)
    rest[:ni, :nu] = False
    out = full[rest]
    stray = ~(np.isnan(out) | (out == 0))
    if stray.any():
        raise AssertionError(f"gmat: {int(stray.sum())} entries outside the used blocks are neither 0 nor the prefill")


def check_equal(name: str, got: np.ndarray, exp: np.ndarray) -> None:
    """array_equal with a message that names the first wrong element"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (name, got.shape, exp.shape, got.dtype, exp.dtype)
    if not np.array_equal(got, exp):
        bad = np.argwhere(~(got == exp))
        idx = tuple(bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {got.size} elements differ; first at {idx}: "
                             f"got {got[idx]!r}, expected {exp[idx]!r}")


# ---------------------------------------------------------------------------------------------------------------------
# 1 + 2. exact inputs and their expectations
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class ExactCase:
    """users: the two-hot side [n_users, d]; items: the ternary side [n_items, d]; w2[item, user] = 2 * weight in
    {0, 1, 2} (int8) with the diagonal already 0; global index of user i is user_goff + i, of item j item_goff + j"""
    d: int
    users: np.ndarray
    items: np.ndarray
    user_goff: int
    item_goff: int
    w2: np.ndarray

    @property
    def n_users(self) -> int:
        return self.users.shape[0]

    @property
    def n_items(self) -> int:
        return self.items.shape[0]

    def weights(self) -> np.ndarray:
        return self.w2.astype(np.float32) * np.float32(0.5)


def assert_distinguishable(w2: np.ndarray, min_len: int = 16) -> None:
    """No two users share an expected G column of `w2` [item, user] and no two items share a row: otherwise a value
    stored at, or taken from, the wrong owner would compare equal.  Vectors shorter than `min_len` cannot all differ
    (3^len patterns) and are exempt: those shapes are there for the edge handling, the longer ones for placement."""
    n_items, n_users = w2.shape
    head = 64   # vectors that differ in their first 64 entries differ: sufficient, and cheap at the large shapes
    if n_items >= min_len and n_users > 1:
        assert len(np.unique(w2[:head].T, axis=0)) == n_users, "two users share their expected weights"
    if n_users >= min_len and n_items > 1:
        assert len(np.unique(w2[:, :head], axis=0)) == n_items, "two items share their expected weights"


def make_exact_case(seed: int, n_users: int, n_items: int, d: int, user_goff: int = 0,
                    item_goff: int = 0) -> ExactCase:
    rng = np.random.RandomState(seed)
    # two-hot users: distinct (a, b, s1, s2) patterns while the supply lasts (d (d-1) / 2 pairs x 4 signs)
    pairs = np.array([(a, b) for a in range(d) for b in range(a + 1, d)], dtype=np.int64)
    pat = rng.permutation(len(pairs) * 4)
    pat = pat[np.arange(n_users) % len(pat)]
    a, b = pairs[pat // 4, 0], pairs[pat // 4, 1]
    s1 = (1 - 2 * (pat % 2)).astype(np.int8)
    s2 = (1 - 2 * ((pat // 2) % 2)).astype(np.int8)
    users = np.zeros((n_users, d), dtype=np.float32)
    users[np.arange(n_users), a] = 16.0 * s1
    users[np.arange(n_users), b] = 16.0 * s2
    tern = rng.randint(-1, 2, size=(n_items, d)).astype(np.int8)
    items = tern.astype(np.float32) * np.float32(16.0)
    v = s1[None, :] * tern[:, a] + s2[None, :] * tern[:, b]          # score / 256, [item, user], by gather
    w2 = (1 + np.sign(v)).astype(np.int8)
    gi = item_goff + np.arange(n_items, dtype=np.int64)[:, None]
    gu = user_goff + np.arange(n_users, dtype=np.int64)[None, :]
    w2[gi == gu] = 0
    return ExactCase(d, users, items, user_goff, item_goff, w2)


def _partner(n: int, goff_own: int, goff_other: int, n_other: int) -> Tuple[np.ndarray, np.ndarray]:
    drow = goff_own + np.arange(n, dtype=np.int64) - goff_other
    ok = (drow >= 0) & (drow < n_other)
    return np.where(ok, drow, 0), ok


def expected_user_outputs(cs: ExactCase) -> Tuple[np.ndarray, np.ndarray]:
    """(r [n_users], dU [n_users, d]) of the user pass / mode_user=1 sweep at n_global = 2; exact in f32"""
    r = (cs.w2.sum(axis=0, dtype=np.int64) / 4.0).astype(np.float32)
    gy = (cs.w2.T.astype(np.float32) @ cs.items) * np.float32(0.25)     # small integers x +-16: exact in any order
    drow, ok = _partner(cs.n_users, cs.user_goff, cs.item_goff, cs.n_items)
    corr = np.where(ok[:, None], r[:, None] * cs.items[drow], np.float32(0))
    return r, (gy - corr).astype(np.float32)


def expected_item_outputs(weights: np.ndarray, users: np.ndarray, r: np.ndarray, user_goff: int, item_goff: int,
                          c: float = C_EXACT) -> np.ndarray:
    """dI [n_items, d] of the stored-G item pass and of the mode_user=0 sweep, for ANY weights [item, user] whose
    products are exact in f32 (the ternary weights, or the synthetic small integers)"""
    n_items, n_users = weights.shape
    gu = (weights.astype(np.float32) @ users.astype(np.float32)) * np.float32(c)
    drow, ok = _partner(n_items, item_goff, user_goff, n_users)
    corr = np.where(ok[:, None], r.astype(np.float32)[drow][:, None] * users[drow], np.float32(0))
    return (gu - corr).astype(np.float32)


def make_synthetic_item_case(seed: int, n_users: int, n_items: int, d: int, user_goff: int, item_goff: int):
    """(gmat_full uint8-valued f32 expectation inputs) for the item pass alone: integer weights 0..3 (0 on the
    diagonal), integer user rows in [-8, 8], r = k / 8 with k in 0..63.  Returns (weights u8 [item, user], users, r)."""
    rng = np.random.RandomState(seed)
    w = rng.randint(0, 4, size=(n_items, n_users)).astype(np.uint8)
    gi = item_goff + np.arange(n_items, dtype=np.int64)[:, None]
    gu = user_goff + np.arange(n_users, dtype=np.int64)[None, :]
    w[gi == gu] = 0
    users = rng.randint(-8, 9, size=(n_users, d)).astype(np.float32)
    r = (rng.randint(0, 64, size=n_users) / 8.0).astype(np.float32)
    return w, users, r


def synthetic_gmat(weights: np.ndarray, n_users: int, n_items: int) -> np.ndarray:
    """Blocked f32 gmat around `weights` [item, user]: 0 in the ragged user slots of the blocks that hold an in-range
    user (the user pass's contract: the item kernel multiplies them with zero-filled rows, and 0 * NaN is NaN), NaN in
    (a) every user block past the last user -- never read -- and (b) every item row past n_items -- read into rows of
    the product that are never stored."""
    ub, ib = g_ub(n_users), g_ub(n_items)
    full = np.full((ib * 32, ub * 32), np.nan, dtype=np.float32)
    full[:n_items, :cdiv(n_users, 32) * 32] = 0
    full[:n_items, :n_users] = weights
    return encode_gmat(full, n_users, n_items)


# ---------------------------------------------------------------------------------------------------------------------
# 4. realistic values: fp64 reference with un-cancelled magnitudes, and the derived bounds
# ---------------------------------------------------------------------------------------------------------------------
def rows_of_norm(rng: np.random.RandomState, n: int, d: int, norm: float) -> np.ndarray:
    x = rng.standard_normal((n, d))
    return (x * (norm / np.linalg.norm(x, axis=1, keepdims=True))).astype(np.float32)


def realistic_reference(users: np.ndarray, items: np.ndarray, pos: np.ndarray, user_goff: int, item_goff: int,
                        n_global: int, forced_nw: Optional[int] = None) -> Dict[str, np.ndarray]:
    """fp64 values of everything the two stored-G passes write, from the f32 inputs as given (pos included).

    g [item, user] = sigma(s - pos_user), 0 on the diagonal;  a = sum_k |u_k y_k| (the score's un-cancelled size);
    r, dU, dI as in ``expected_*`` with c = 1 / (n_global (n_global - 1)), M_* = c sum g |row| and C_* = r |partner
    row| their un-cancelled sum and correction;  loss_part[split * gx + blk] = sum of
    softplus(z) over the pairs of 128-user block blk and the items of that split (in nats, unscaled), with m_loss the
    same sum of |z| + log(1 + e^-z) -- the two terms the kernel accumulates --, A_loss = sum of a and Z_loss = sum of
    2 |pos| + |z|."""
    U, Y, p = users.astype(np.float64), items.astype(np.float64), pos.astype(np.float64)
    nu, ni = U.shape[0], Y.shape[0]
    c = 1.0 / (n_global * (n_global - 1.0))
    s = Y @ U.T
    a = np.abs(Y) @ np.abs(U).T
    z = s - p[None, :]
    g = 1.0 / (1.0 + np.exp(-z))
    off = (item_goff + np.arange(ni)[:, None]) != (user_goff + np.arange(nu)[None, :])
    g = g * off
    r = c * g.sum(axis=0)
    du, mu = c * (g.T @ Y), c * (g.T @ np.abs(Y))
    drow, ok = _partner(nu, user_goff, item_goff, ni)
    du -= np.where(ok[:, None], r[:, None] * Y[drow], 0.0)
    cu = np.where(ok[:, None], r[:, None] * np.abs(Y[drow]), 0.0)
    di, mi = c * (g @ U), c * (g @ np.abs(U))
    drow, ok = _partner(ni, item_goff, user_goff, nu)
    di -= np.where(ok[:, None], r[drow][:, None] * U[drow], 0.0)
    ci = np.where(ok[:, None], r[drow][:, None] * np.abs(U[drow]), 0.0)
    nsplit = sweep_nsplit(nu, ni, sweep_nw(nu, ni, forced_nw))
    gx = cdiv(nu, OW)
    sp = (np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))) * off
    ms = (np.abs(z) + np.log1p(np.exp(-z))) * off
    zs = (2 * np.abs(p)[None, :] + np.abs(z)) * off
    lp, lm, la, lz, ltiles = (np.zeros(gx * nsplit) for _ in range(5))
    for by in range(nsplit):
        t0, t1 = split_range(ni, nsplit, by)
        for bx in range(gx):
            blk = (slice(t0 * TSW, min(t1 * TSW, ni)), slice(bx * OW, min((bx + 1) * OW, nu)))
            k = by * gx + bx
            lp[k], lm[k], ltiles[k] = sp[blk].sum(), ms[blk].sum(), t1 - t0
            la[k], lz[k] = (a * off)[blk].sum(), zs[blk].sum()
    return dict(c=c, g=g, a=a, z=z, r=r, dU=du, M_dU=mu, C_dU=cu, dI=di, M_dI=mi, C_dI=ci, loss_part=lp, M_loss=lm,
                A_loss=la, Z_loss=lz,
                loss_tiles=ltiles, min_softplus=float(np.where(off, sp, np.inf).min()), nsplit=nsplit)


K_CONST = 32
K_LOSS = 16


def score_factor(d: int, precision: int) -> int:
    """K: roundings of one score relative to a = sum_k |u_k y_k|.  Exact-f32 MFMA: d multiply-adds, the owner row
    pre-scaled by the rounded log2(e) (2 more) and one to spare: d + 3.  bf16x6: six piece products per k, each added
    in f32 (6 d), the dropped pieces (2) and the same pre-scaling: 6 d + 5."""
    return d + 3 if precision == 0 else 6 * d + 5


BOUNDS_DOC = """Bounds on |device - ref|, in units of u = 2^-24, derived (nothing here comes from a device run):

    score:  z2 = fl(s2 - pos2), s2 a chain of K = score_factor roundings relative to a_ij, pos2 = fl(pos * fl(log2 e))
            (2), the subtraction (1):  |dz| <= (K a + 2 |pos| + |z|) u  =: E_ij u  (natural units; the log2 e cancels).
    weight: e = exp2(-z2) and rcp are 1 ulp = 2 u each, 1 + e rounds once; with sigma' = sigma (1 - sigma) <= 1/4:
            |dg| <= sigma (1 - sigma) (E + 2) u + 3 u sigma  <=  (E / 4 + 3.5) u.      No dependence on G.
    r:      (n + E_max + k) u r, n = the number of swept rows (a plain f32 sum in every precision), E_max = max E_ij + 5
            the relative error of one weight (|dg| <= g (E + 5) u because sigma' <= sigma).
    dU, dI: ((P n + E_max + k) M + (n_r + E_max + k) C) u, P = 1 (f32 MFMA: one fused multiply-add per term) or 6
            (bf16x6: six piece products per term, each added in f32; the dropped pieces are 2 of k), M = c sum g |y|
            the un-cancelled sum over the n swept rows, C = r |y_partner| the correction, which carries r's own error
            (r is a sum over n_r = n_items rows in both passes).
            k = 32: c = fl(1 / (B (B - 1))) and the product with it (2), the add of the two half-waves (1), up to 16
            split slabs added in order (16), the correction's product and subtraction (2), r's own three scale
            roundings inside the correction (3), the dropped bf16 pieces (2): 26, rounded up to 32.
    loss_part:  a lane adds, per tile, 16 values z2 and two log2 of products of eight denominators: 18 T roundings
            for T tiles, then 6 levels of the wave sum and doubles.  Per element the denominator carries 3 u (exp2, the
            add) and its place in the product 1 u: an absolute 4 u in the log, at most 6 u of the element's own
            |z| + log(1 + e^-z) >= 0.69; v_log_f32 2 u; 8, doubled: k_loss = 16.  The score error enters through
            softplus' = sigma <= 1 unamplified:   ((18 T + 6 + k_loss) M_loss + sum over the part's pairs of E_ij) u."""


def elementwise_E(ref: Dict[str, np.ndarray], pos: np.ndarray, d: int, precision: int) -> np.ndarray:
    """E_ij of BOUNDS_DOC: (K a_ij + 2 |pos_i| + |z_ij|), [item, user]"""
    K = score_factor(d, precision)
    return K * ref["a"] + 2 * np.abs(pos.astype(np.float64))[None, :] + np.abs(ref["z"])


def bound_gmat(ref, pos, d, precision) -> np.ndarray:
    E = elementwise_E(ref, pos, d, precision)
    g = ref["g"]
    return (g * (1 - g) * (E + 2) + 3 * g) * U32


def bound_sums(ref, pos, d, precision) -> Dict[str, np.ndarray]:
    """bounds of r [user], dU, dI and loss_part (see BOUNDS_DOC)"""
    E = elementwise_E(ref, pos, d, precision)
    P = 1 if precision == 0 else 6
    emax = float(E.max()) + 5
    ni, nu = ref["g"].shape
    K = score_factor(d, precision)
    return dict(r=(ni + emax + K_CONST) * U32 * ref["r"],
                dU=((P * ni + emax + K_CONST) * ref["M_dU"] + (ni + emax + K_CONST) * ref["C_dU"]) * U32,
                dI=((P * nu + emax + K_CONST) * ref["M_dI"] + (ni + emax + K_CONST) * ref["C_dI"]) * U32,
                loss_part=((18 * ref["loss_tiles"] + 6 + K_LOSS) * ref["M_loss"] + K * ref["A_loss"]
                           + ref["Z_loss"]) * U32)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_inbatch_exact.py (tests/test_inbatch_host.py shows which loop regions they reach)
# ---------------------------------------------------------------------------------------------------------------------
# (n_users, n_items, user_goff, item_goff): the counts 1 / 31 / 32 / 33 / 127 / 128 / 129 on either side, offsets 0,
# mid-tile and G - Bl, ragged rectangles, users > items, slices of the item set (item_goff != 0) with partners below,
# inside and above the slice.  With <= 22 swept tiles a split holds one or two tiles, so the last shape has 79: splits
# of five, the only small shape whose workgroups go round the three-buffer LDS ring and prefetch tile + 2.
EXACT_SMALL_SHAPES = [
    (1, 1, 0, 0),
    (1, 33, 17, 0),
    (31, 32, 0, 0),
    (32, 33, 1, 0),
    (33, 127, 94, 0),
    (127, 129, 1, 0),
    (128, 128, 0, 0),
    (129, 300, 77, 0),
    (300, 700, 400, 0),
    (257, 161, 0, 0),
    (129, 200, 300, 250),
    (97, 131, 0, 64),
    (64, 96, 500, 0),
    (130, 2500, 1000, 0),
]
GENERIC_SHAPES = [EXACT_SMALL_SHAPES[k] for k in (1, 3, 4, 6, 7, 9, 10, 11)] + [(130, 300, 170, 0)]
TUNED_D = (32, 64, 128)
GENERIC_D = (16, 48, 144, 256)
# the 8-wave child (RIHIP_SWEEP_NW=8) repeats the ragged ones
CHILD_SHAPES = [EXACT_SMALL_SHAPES[k] for k in (1, 4, 7, 8, 9, 10, 11, 13)]

# 8-wave shapes: 4096 + e owners and 16384 + e swept rows is the minimum for nw = 8 without the environment variable
LARGE_OWNERS, LARGE_SWEPT = 4196, 16400
LARGE_USER_OFFSETS = (77, 12204)       # mid-tile; G - Bl.  test_inbatch_host.py shows what each reaches

# realistic values: (d, precision, row norm) -> (n_users, n_items); the largest rung of a ladder at which one pair's
# contribution is >= 100 x the derived bound of r, dU and dI (asserted on the host)
REALISTIC_CASES = {
    (32, 0, 1): (130, 300), (32, 0, 2): (20, 70), (32, 2, 1): (70, 161), (32, 2, 2): (12, 45),
    (64, 0, 1): (130, 300), (64, 0, 2): (33, 97), (64, 2, 1): (70, 161), (64, 2, 2): (12, 45),
    (128, 0, 1): (130, 300), (128, 0, 2): (33, 97), (128, 2, 1): (70, 161), (128, 2, 2): (7, 33),
}


# the same for the loss parts: a part's bound grows with the number of its pairs (every pair's score error enters it
# unamplified), so one pair stands >= 100 x above it only in parts of a few dozen to a few hundred pairs
LOSS_CASES = {
    (32, 0, 1): (20, 33), (32, 0, 2): (5, 33), (32, 2, 1): (12, 33), (32, 2, 2): (2, 8),
    (64, 0, 1): (20, 33), (64, 0, 2): (5, 33), (64, 2, 1): (7, 33), (64, 2, 2): (2, 8),
    (128, 0, 1): (20, 33), (128, 0, 2): (4, 32), (128, 2, 1): (5, 33), (128, 2, 2): (2, 8),
}


def make_realistic_case(d: int, precision: int, norm: int, table=None):
    """(users, items, pos, user_goff) of one realistic case of `table` (REALISTIC_CASES unless given); pos is the f32
    rounding of the fp64 partner score"""
    nu, ni = (REALISTIC_CASES if table is None else table)[(d, precision, norm)]
    rng = np.random.RandomState(1)
    users, items = rows_of_norm(rng, nu, d, norm), rows_of_norm(rng, ni, d, norm)
    off = (ni - nu) // 2
    pos = np.einsum("ij,ij->i", users.astype(np.float64), items[off:off + nu].astype(np.float64)).astype(np.float32)
    return users, items, pos, off


def one_pair_ratios(ref, bounds, users, items) -> Dict[str, float]:
    """smallest ratio of one pair's contribution to the bound of the output it lands in (for dU / dI: in the most
    sensitive of the d elements); loss: the smallest softplus against the largest part bound"""
    g, c = ref["g"], ref["c"]
    on = g > 0
    r = (np.where(on, c * g, np.inf) / bounds["r"][None, :]).min()
    du = np.where(on[:, :, None], c * g[:, :, None] * np.abs(items)[:, None, :] / bounds["dU"][None, :, :],
                  np.inf).max(axis=2).min()
    di = np.where(on[:, :, None], c * g[:, :, None] * np.abs(users)[None, :, :] / bounds["dI"][:, None, :],
                  np.inf).max(axis=2).min()
    return dict(r=float(r), dU=float(du), dI=float(di), loss_part=ref["min_softplus"] / float(bounds["loss_part"].max()))


def issue_form_bounds(ref, d: int) -> Dict[str, np.ndarray]:
    """The plain form (n + d + k) u M, valid for unit rows at precision 0 only: there a_ij <= |u| |y| = 1, |pos| <= 1 and
    |z| <= 2, so E_max = (d + 3) a + 2 |pos| + |z| + 5 <= d + 12 and BOUNDS_DOC's (n + E_max + 32) is at most
    n + d + 44: k = 44.  (At norm 2 or with bf16x6 the derived coefficient is 1.7 to 13 times this one -- a up to 4,
    six piece products per term -- and this form is not claimed.)"""
    ni, nu = ref["g"].shape
    k = 44
    return dict(r=(ni + d + k) * U32 * ref["r"],
                dU=(ni + d + k) * U32 * (ref["M_dU"] + ref["C_dU"]),
                dI=((nu + d + k) * ref["M_dI"] + (ni + d + k) * ref["C_dI"]) * U32)
