"""Exact inputs, exact references and tile schedules for the tower kernels' multi-tile loops (TEST INFRASTRUCTURE).

Used by tests/test_gpu_tower_loops.py (GPU) and proven by tests/test_tower_host.py (CPU).  Written from the definitions
in oracle/two_tower_np.py (tower_forward / tower_backward / embedding_scatter_add), not from the kernels.

Exactness
---------
Every input is a small integer (or, in the backward, an integer multiple of GRID = 2^-2), so every product the kernels
form is exact in f32 and every partial sum of such products is an integer multiple of GRID whose magnitude is at most
the sum of the absolute values of its terms.  While that sum stays below 2^24 * GRID every partial sum is exactly
representable in f32, *whatever the order of summation*: a correct kernel must reproduce the reference bit for bit, and
the comparison is np.array_equal.  The builders compute those absolute sums on the host and raise if one reaches the
limit, so a case that would lose exactness fails when it is built.

The forward's `denom = max(sqrt(sum y^2), 1e-12)` and `out = y / denom` are not exact.  sum y^2 is (an integer below
2^24, asserted), so the kernels' only roundings are
    sqrtf            <= 1 ulp  = 2u relative          (u = 2^-24)
    y / dn           <= 1 ulp  = 2u      -- 64-row and generic kernels, total 4u
    1 / dn ; y * inv <= 2u + u           -- 32-row kernel, total 5u
so |denom - ref| <= 2u * ref and |out - ref| <= 5u * |ref| to first order; OUT_ULPS = 5.5 and DENOM_ULPS = 2.5 leave
half a unit for the second-order terms and the rounding of the f64 reference to the stored f32.  Where sum y^2 is a
perfect square with a power-of-two root (rows whose hidden layer is all zero: y = b2 and sum b2^2 is built to be a power
of four) sqrt and the division are exact, and equality is required.

Backward: gout and out are small integers, denom is 1, 2 or 4, so gy = (gout - out <gout, out>) / denom is a multiple
of GRID in either form the kernels use (`/ dn` or `* (1 / dn)`).  Rows in the clamp branch have denom = float32(1e-12)
and gout = +-float32(1e-12) * 2^j: float32 division gives +-2^j exactly, and so does the product with fl(1 / 1e-12f)
(checked on the host when the case is built), so those rows are exact too and a kernel that forgets to drop the
<gout, out> term there is off by an integer.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

from oracle import two_tower_np as O

F32, F64, I64 = np.float32, np.float64, np.int64
U = 2.0 ** -24                       # unit roundoff of f32
LIMIT = float(1 << 24)
GRID = 0.25                          # every backward quantity is a multiple of this
EPS32 = np.float32(1e-12)
OUT_ULPS, DENOM_ULPS = 5.5, 2.5      # in units of u (derivation above)
NCU, SLAB_GROUPS = 256, 16           # RIHIP_NCU (common.h), SLAB_GROUPS (tower.hip)
TUNED = ((32, 64), (64, 128), (128, 128), (64, 64), (32, 128))
N_GENRES = 18
P_DROP = 0.5                         # scale = 1 / (1 - p) = 2 exactly
SENTINEL = 7.0                       # what the tests pre-fill outputs with


# ------------------------------------------------------------------------------------------------------------------- #
# Tile schedules: which walker (workgroup, or wave of a workgroup) sees which tiles, in which order; restated from the   #
# launch code of tower.hip / tower2.hip / tower3.hip / tower_generic.hip.                                              #
# ------------------------------------------------------------------------------------------------------------------- #
# kind -> (rows per tile, walkers per workgroup, workgroup cap, rows that size the grid, writes slabs)
_KINDS = {
    "fwd64": (64, 1, 2 * NCU, 64, False),        # tower_fwd_kernel: grid = min(ntiles, 2 NCU)
    "bwd64": (64, 1, NCU, 64, True),             # tower_bwd_kernel: grid = min(ntiles, NCU), slab = workgroup
    "fwd2": (32, 8, NCU, 256, False),            # tower_fwd2_kernel: grid = min(ceil(B / 256), NCU), wave w of wg b
    "bwd_data": (32, 8, NCU, 256, False),        # tower_bwd_data_kernel: starts at tile 8 b + w, stride 8 grid
    "wgrad": (32, 1, NCU, 32, True),             # tower_wgrad_kernel: grid = min(ntiles, NCU), buffer = iteration & 1
    "bwd3": (32, 1, NCU, 32, True),              # tower_bwd3_kernel: grid = min(ntiles, NCU, max_slabs = the same)
    "gen_fwd": (32, 1, 4 * NCU, 32, False),      # tower_fwd_generic_kernel: grid = min(ntiles, 4 NCU)
    "gen_bwd_data": (32, 1, 4 * NCU, 32, False),
}


def gen_wgrad_split(B, d, H, item):
    """(tiles per slab, slabs) of tower_wgrad_generic_kernel: `want = ...` in rihip_launch_tower_bwd_generic."""
    K1 = d + (N_GENRES if item else 0)
    ntiles = (B + 31) // 32
    out_tiles = ((H + 31) // 32) * ((K1 + 1 + 31) // 32) + ((d + 31) // 32) * ((H + 1 + 31) // 32)
    gx = (out_tiles + 3) // 4
    want = (2 * NCU + gx - 1) // gx
    want = max(1, min(want, min(ntiles, NCU), ntiles))
    per = (ntiles + want - 1) // want
    return per, (ntiles + per - 1) // per


class Schedule:
    """tiles_of(w): the tiles walker w handles, in iteration order.  For slab-writing kernels walker = slab."""

    def __init__(self, kind, B, d=None, H=None, item=False):
        self.kind, self.B = kind, int(B)
        if kind == "gen_wgrad":
            self.tile = 32
            self.ntiles = (B + 31) // 32
            self.per, self.nwalkers = gen_wgrad_split(B, d, H, item)
            self.pass_rows = None
            self.slabs = True
        else:
            self.tile, waves, cap, grid_rows, self.slabs = _KINDS[kind]
            self.ntiles = (B + self.tile - 1) // self.tile
            grid = min((B + grid_rows - 1) // grid_rows, cap)
            self.nwalkers = grid * waves
            self.pass_rows = cap * waves * self.tile      # rows per pass of a full grid
            self.per = None
        self.nslab = self.nwalkers if self.slabs else 0

    def tiles_of(self, w):
        if self.kind == "gen_wgrad":
            return list(range(w * self.per, min((w + 1) * self.per, self.ntiles)))
        return list(range(w, self.ntiles, self.nwalkers))

    def where(self, tile):
        """(walker, iteration) of a tile"""
        if self.kind == "gen_wgrad":
            return tile // self.per, tile % self.per
        return tile % self.nwalkers, tile // self.nwalkers

    def rows_of_tile(self, t):
        return np.arange(t * self.tile, min((t + 1) * self.tile, self.B))

    def rows_of_walker(self, w):
        ts = self.tiles_of(w)
        return np.concatenate([self.rows_of_tile(t) for t in ts]) if ts else np.zeros(0, dtype=I64)

    def coverage(self):
        """the loop regions this (kind, B) reaches"""
        its = [len(self.tiles_of(w)) for w in range(self.nwalkers)]
        ragged = self.B % self.tile != 0
        return dict(max_iterations=max(its), second=max(its) >= 2, third=max(its) >= 3,
                    ragged_later=ragged and self.where(self.ntiles - 1)[1] >= 1,
                    idle_last_pass=min(its) < max(its),
                    # tower_wgrad_kernel stages iteration i in buffer i & 1 (other kinds have no staging buffers: None)
                    both_buffers=(len({i & 1 for n in its for i in range(n)}) == 2) if self.kind == "wgrad" else None,
                    nslab_gt16=self.nslab > SLAB_GROUPS)


def slab_groups(nslab):
    """two-level slab reduction (slab_reduce1/2_multi_kernel): group g sums slabs g, g + G, ...; <= 16 slabs: one level"""
    G = min(nslab, SLAB_GROUPS)
    return [list(range(g, nslab, G)) for g in range(G)]


def case_B(kind, which):
    """the two batch sizes used for a kernel with pass size R: R + 3 tile + 5 (second iteration) and 2 R + 9 tile + 17 (third)"""
    tile, waves, cap, _, _ = _KINDS[kind]
    R = cap * waves * tile
    return R + 3 * tile + 5 if which == 0 else 2 * R + 9 * tile + 17


GENERIC = ((48, 96), (144, 80), (256, 256))      # shapes without a tuned instantiation


def forward_cases():
    """(kind, d, H, item, B) of every exact forward the GPU tests run"""
    out = []
    for kind in ("fwd64", "fwd2"):
        out += [(kind, d, H, item, case_B(kind, w)) for d, H in TUNED for w in (0, 1) for item in (False, True)]
    out += [("gen_fwd", d, H, item, case_B("gen_fwd", 0)) for d, H in GENERIC for item in (False, True)]
    return out


def backward_cases():
    """(kind, d, H, item, B) of every exact backward the GPU tests run; kind bwd2 = tower_bwd_data_kernel (rows) +
    tower_wgrad_kernel (slabs)"""
    out = []
    for item in (False, True):
        out += [("bwd64", d, H, item, case_B("bwd64", w)) for d, H in TUNED for w in (0, 1)]
        out += [("bwd2", 128, 128, item, B) for B in (case_B("wgrad", 0), case_B("wgrad", 1), case_B("bwd_data", 0),
                                                      case_B("bwd_data", 1))]
        out += [("bwd3", 128, 128, item, case_B("bwd3", w)) for w in (0, 1)]
        out += [("gen", d, H, item, case_B("gen_bwd_data", 0)) for d, H in GENERIC]
    return out


def backward_schedules(kind, B, d, H, item):
    """(schedule of the per-row outputs, schedule of the slabs) of a backward kind"""
    if kind == "gen":
        return Schedule("gen_bwd_data", B), Schedule("gen_wgrad", B, d, H, item)
    if kind == "bwd2":
        return Schedule("bwd_data", B), Schedule("wgrad", B)
    return Schedule(kind, B), Schedule(kind, B)


# ------------------------------------------------------------------------------------------------------------------- #
# Inputs                                                                                                               #
# ------------------------------------------------------------------------------------------------------------------- #
def _sparse_signs(rng, rows, cols, nnz, col_lo=0):
    """[rows, cols] of {-1, 0, 1} with exactly nnz non-zeros per row at columns >= col_lo"""
    W = np.zeros((rows, cols), dtype=F64)
    for r in range(rows):
        c = col_lo + rng.choice(cols - col_lo, size=nnz, replace=False)
        W[r, c] = rng.choice([-1.0, 1.0], size=nnz)
    return W


def _b2_power_of_four(rng, d):
    """entries in {-2..2} with sum of squares = the smallest power of four >= d (root = a power of two)"""
    target = 4 ** math.ceil(math.log(d, 4) - 1e-12)
    diff = target - d
    a = -(-diff // 3)
    z = 3 * a - diff
    mag = np.ones(d)
    perm = rng.permutation(d)
    mag[perm[:a]] = 2.0
    mag[perm[a:a + z]] = 0.0
    b2 = mag * rng.choice([-1.0, 1.0], size=d)
    assert (b2 ** 2).sum() == target and math.log2(math.isqrt(int(target))) % 1 == 0
    return b2


def _ids(rng, B, n_rows):
    """ids that vary with the row, with adjacent and distant duplicates, id 0 (padding), the zero row 1 and the last row"""
    ids = rng.integers(2, n_rows, size=B).astype(I64)
    ids[3::64] = ids[2::64][: len(ids[3::64])]          # duplicates inside a tile
    r = np.arange(B)
    ids[r % 97 == 0] = 0
    ids[r % 97 == 1] = 1
    ids[r % 197 == 5] = n_rows - 1
    return ids


def _tiles_differ(a, tile, shift_rows):
    """every full tile t of `a` differs from tile t + shift (same row-in-tile positions)"""
    if shift_rows >= a.shape[0]:
        return True
    n = ((a.shape[0] - shift_rows) // tile) * tile
    if n <= 0:
        return True
    diff = (a[:n] != a[shift_rows:shift_rows + n]).reshape(n, -1).any(axis=1)
    return bool(diff.reshape(n // tile, tile).any(axis=1).all())


ALIAS_ROWS = (8192, 16384, 32768, 65536)     # the pass sizes: a stale or misrouted tile comes from one of these away


def _weights(d, H, item, seed):
    rng = np.random.default_rng(1000 * d + H + (7 if item else 0) + seed)
    K1 = d + (N_GENRES if item else 0)
    n_rows = 1021
    table = rng.integers(-2, 3, size=(n_rows, d)).astype(F64)
    table[1] = 0.0                                        # rows with id 1 (and no genre): hidden = 0, y = b2
    if not table[0].any():
        table[0, 0] = 1.0
    W1 = _sparse_signs(rng, H, K1, 8)
    if item:
        W1[:, d:] = 0.0
        W1[:, d:] += _sparse_signs(rng, H, N_GENRES, 3)
    b1 = -rng.integers(0, 3, size=H).astype(F64)          # <= 0: a zero input row gives a zero hidden row
    W2 = _sparse_signs(rng, d, H, 4)
    b2 = _b2_power_of_four(rng, d)
    return SimpleNamespace(d=d, H=H, K1=K1, item=item, n_rows=n_rows, table=table, W1=W1, b1=b1, W2=W2, b2=b2)


@functools.lru_cache(maxsize=3)
def forward_case(d, H, item, B, seed=0):
    """Inputs of an exact forward; raises if the 2^24 condition fails (checked for the all-kept, scale-2 worst case, which
    dominates eval and training)."""
    w = _weights(d, H, item, seed)
    rng = np.random.default_rng(B + 31 * d + H + int(item))
    ids = _ids(rng, B, w.n_rows)
    genres = None
    if item:
        genres = (rng.random((B, N_GENRES)) < 0.25).astype(F64)
        genres[ids == 1] = 0.0
    c = SimpleNamespace(**vars(w), B=B, ids=ids, genres=genres, seed=0x1234567 + B, step=5, row0=12345, p=P_DROP)
    x = np.abs(forward_x(c, np.arange(B)))
    a1 = x @ np.abs(c.W1).T + np.abs(c.b1)
    a2 = (2.0 * a1) @ np.abs(c.W2).T + np.abs(c.b2)
    c.abs_sums = dict(pre=float(a1.max()), y=float(a2.max()), ss=float((a2 * a2).sum(1).max()))
    for k, v in c.abs_sums.items():
        if not v < LIMIT:
            raise AssertionError(f"forward case (d={d}, H={H}, item={item}, B={B}): sum|terms| of {k} = {v} >= 2^24")
    return c


def seed_eff(c, with_step=True):
    """the seed O.dropout_keep_mask must be given to reproduce the kernel's mask: the kernel hashes the counter with
    splitmix64(seed) and, when a step clock is passed, with splitmix64(splitmix64(seed) + step)"""
    if not with_step:
        return c.seed
    sm = int(O.splitmix64(np.array([c.seed], dtype=np.uint64))[0])
    return (sm + c.step) % (1 << 64)


def keep_rows(c, rows, with_step=True):
    """dropout keep mask of the given global batch rows (contiguous runs are hashed together)"""
    rows = np.asarray(rows, dtype=I64)
    out = np.empty((len(rows), c.H), dtype=bool)
    if len(rows) == 0:
        return out
    cuts = np.flatnonzero(np.diff(rows) != 1) + 1
    s = seed_eff(c, with_step)
    for a, b in zip(np.r_[0, cuts], np.r_[cuts, len(rows)]):
        for a2 in range(a, b, 16384):
            b2 = min(b, a2 + 16384)
            out[a2:b2] = O.dropout_keep_mask(s, c.row0 + int(rows[a2]), b2 - a2, c.H, c.p)
    return out


def forward_x(c, rows, ids=None):
    ids = c.ids if ids is None else ids
    idr = ids[rows]
    idr = np.where((idr < 0) | (idr >= c.n_rows), 0, idr)          # the kernels' documented handling: row 0, err_flag
    x = c.table[idr]
    if c.genres is not None:
        x = np.concatenate([x, c.genres[rows]], axis=1)
    return x


def forward_rows(c, rows, train, mask_rows=None, ids=None):
    """Reference forward of batch rows `rows` (f64 arithmetic on integers: exact).  mask_rows: the global rows whose
    dropout counters are used (default: the rows themselves)."""
    rows = np.asarray(rows, dtype=I64)
    x = forward_x(c, rows, ids)
    pre = x @ c.W1.T + c.b1
    h = np.maximum(pre, 0.0)
    if train:
        h = np.where(keep_rows(c, rows if mask_rows is None else mask_rows), h * 2.0, 0.0)
    y = h @ c.W2.T + c.b2
    ss = (y * y).sum(1)
    root = np.sqrt(ss)
    denom = np.maximum(root, float(EPS32))
    iroot = np.rint(root).astype(I64)
    exact = (iroot * iroot == ss) & (iroot > 0) & ((iroot & (iroot - 1)) == 0)
    return SimpleNamespace(x=x, hid=h.astype(F32), y=y, ss=ss, denom=denom, out=y / denom[:, None], exact=exact)


@functools.lru_cache(maxsize=4)
def forward_reference(d, H, item, B, train, seed=0):
    c = forward_case(d, H, item, B, seed)
    r = forward_rows(c, np.arange(B), train)
    assert r.exact.any(), "no row with a power-of-two norm"
    for shift in ALIAS_ROWS:
        for tile in (32, 64):
            assert _tiles_differ(r.hid, tile, shift) and _tiles_differ(r.out, tile, shift), (shift, tile)
    r.x = r.y = None          # (not needed by the comparisons; a case of 131 k rows is large)
    return r


@functools.lru_cache(maxsize=3)
def backward_case(d, H, item, B, seed=0):
    """Synthetic activations for an exact backward through the C ABI (see the module docstring)."""
    rng = np.random.default_rng(77 + B + 31 * d + H + int(item) + seed)
    K1 = d + (N_GENRES if item else 0)
    n_rows = 1021
    table = rng.integers(-2, 3, size=(n_rows, d)).astype(F64)
    ids = _ids(rng, B, n_rows)
    genres = (rng.random((B, N_GENRES)) < 0.25).astype(F64) if item else None
    W1 = rng.integers(-1, 2, size=(H, K1)).astype(F64)
    W2 = _sparse_signs(rng, H, d, 2).T.copy()             # [d, H], two non-zeros per column
    r = np.arange(B)
    # gout: 3 non-zeros per row, out: 3 non-zeros sharing two of gout's columns => |<gout, out>| <= 2
    c0, st = rng.integers(0, d, size=B), 2 * rng.integers(0, 4, size=B) + 1       # odd stride: 4 distinct columns
    cols = (c0[:, None] + st[:, None] * np.arange(4)[None, :]) % d
    gout = np.zeros((B, d)); out = np.zeros((B, d))
    sg = 2.0 * rng.integers(0, 2, size=(B, 4)) - 1.0
    so = 2.0 * rng.integers(0, 2, size=(B, 4)) - 1.0
    for j in range(3):
        gout[r, cols[:, j]] = sg[:, j]
        out[r, cols[:, j + 1]] = so[:, j]
    denom = np.array([1.0, 2.0, 4.0])[(r + r // 32) % 3]
    clamp = r % 53 == 7
    j2 = np.array([1.0, 2.0, 4.0])[(r // 53) % 3]
    e = float(EPS32)
    gout[clamp] = gout[clamp] * e * j2[clamp, None]
    denom[clamp] = e
    g32, inv32 = gout[clamp].astype(F32), F32(1) / EPS32
    want = (gout[clamp] / e)
    assert np.array_equal(g32.astype(F64), gout[clamp]), "clamp-row gout is not representable"
    assert np.array_equal((g32 / EPS32).astype(F64), want) and np.array_equal((g32 * inv32).astype(F64), want), \
        "gout / 1e-12f is not exact in both forms the kernels use"
    hid = np.array([0.0, 0.0, 1.0, 2.0])[rng.integers(0, 4, size=(B, H), dtype=np.int8)]
    c = SimpleNamespace(d=d, H=H, K1=K1, item=item, B=B, n_rows=n_rows, table=table, ids=ids, genres=genres, W1=W1, W2=W2,
                        gout=gout, out=out, denom=denom, hid=hid, scale=2.0, clamp=clamp)
    c.x = table[ids] if genres is None else np.concatenate([table[ids], genres], axis=1)
    c.ref = backward_rows(c.x, W1, W2, gout, out, denom, hid, c.scale, d)
    a = c.ref
    # |gy| is exact by construction; the abs-sum condition for everything summed (in units of GRID)
    agy, adp, ax, ah = np.abs(a.gy), np.abs(a.dpre), np.abs(c.x), hid
    c.abs_sums = dict(dh=float((agy @ np.abs(W2)).max()), dX=float((adp @ np.abs(W1)).max()),
                      dW1=float((adp.T @ ax).max()), db1=float(adp.sum(0).max()),
                      dW2=float((agy.T @ ah).max()), db2=float(agy.sum(0).max()))
    for k, v in c.abs_sums.items():
        if not v / GRID < LIMIT:
            raise AssertionError(f"backward case (d={d}, H={H}, item={item}, B={B}): sum|terms| of {k} = {v} >= 2^24 GRID")
    nc = ~clamp
    assert np.abs(a.dh).max() <= 8.0, np.abs(a.dh).max()
    assert np.array_equal(np.rint(a.gy / GRID) * GRID, a.gy)      # (dh, dPre, dX: integer combinations of gy, times 2)
    assert np.abs((gout[nc] * out[nc]).sum(1)).max() > 0 and (np.abs((gout[clamp] * out[clamp]).sum(1)) > 0).any()
    for shift in ALIAS_ROWS:
        for tile in (32, 64):
            assert _tiles_differ(a.dX, tile, shift) and _tiles_differ(a.gy, tile, shift), (shift, tile)
    return c


# ------------------------------------------------------------------------------------------------------------------- #
# Reference backward (oracle/two_tower_np.py: tower_backward, in f64)                                                   #
# ------------------------------------------------------------------------------------------------------------------- #
def backward_rows(x, W1, W2, gout, out, denom, hid, scale, d):
    """per-row quantities: gy, dh, dPre, dX.  denom holds the f32 values the kernel is given."""
    x, gout, out, denom, hid = (np.asarray(v, dtype=F64) for v in (x, gout, out, denom, hid))
    W1, W2 = np.asarray(W1, dtype=F64), np.asarray(W2, dtype=F64)
    dot = (gout * out).sum(1, keepdims=True)
    clamped = denom[:, None] <= float(EPS32)
    gy = np.where(clamped, gout, gout - out * dot) / denom[:, None]
    dh = gy @ W2
    dpre = np.where(hid > 0, dh * scale, 0.0)
    dX = (dpre @ W1)[:, :d]
    return SimpleNamespace(gy=gy, dh=dh, dpre=dpre, dX=dX)


def weight_grads(ref, hid, x, rows=None):
    """(dW1, db1, dW2, db2) summed over `rows` (default: all)"""
    gy, dp = (ref.gy, ref.dpre) if rows is None else (ref.gy[rows], ref.dpre[rows])
    h, xx = (hid, x) if rows is None else (hid[rows], x[rows])
    return dp.T @ xx, dp.sum(0), gy.T @ np.asarray(h, dtype=F64), gy.sum(0)


def pack_slab(g):
    """slab layout of every backward kernel: [dW1 (H*K1) | db1 (H) | dW2 (D*H) | db2 (D)]"""
    return np.concatenate([np.asarray(v, dtype=F64).ravel() for v in g])


def slab_sections(d, H, K1):
    e = np.cumsum([0, H * K1, H, d * H, d])
    return {n: (int(e[i]), int(e[i + 1])) for i, n in enumerate(("dW1", "db1", "dW2", "db2"))}


def reference_slabs(c, sched, tiles_of=None):
    """[nslab, P]: slab s = the sum over exactly the tiles the schedule gives walker s"""
    out = []
    for s in range(sched.nslab):
        ts = sched.tiles_of(s) if tiles_of is None else tiles_of(s)
        rows = np.concatenate([sched.rows_of_tile(t) for t in ts]) if len(ts) else np.zeros(0, dtype=I64)
        out.append(pack_slab(weight_grads(c.ref, c.hid, c.x, rows)))
    return np.stack(out)


def reduce_slabs(slabs, skip=None):
    """the two-level reduction, in its order (exact inputs: the order is immaterial; it is restated for the defects)"""
    tot = np.zeros(slabs.shape[1])
    for grp in slab_groups(slabs.shape[0]):
        part = np.zeros(slabs.shape[1])
        for s in grp:
            if s != skip:
                part += slabs[s]
        tot += part
    return tot


def split_slab(v, d, H, K1):
    s = slab_sections(d, H, K1)
    return (v[s["dW1"][0]:s["dW1"][1]].reshape(H, K1), v[s["db1"][0]:s["db1"][1]],
            v[s["dW2"][0]:s["dW2"][1]].reshape(d, H), v[s["db2"][0]:s["db2"][1]])


def scatter_reference(preset, n_rows, ids, dX):
    """embedding_scatter_add onto a table gradient preset to `preset`: row 0 and out-of-range ids get nothing"""
    g = np.full((n_rows, dX.shape[1]), float(preset))
    ok = (ids >= 1) & (ids < n_rows)
    np.add.at(g, ids[ok], np.asarray(dX, dtype=F64)[ok])
    return g


# ------------------------------------------------------------------------------------------------------------------- #
# Comparison helpers (each is shown red for every defect it can see in tests/test_tower_host.py)                        #
# ------------------------------------------------------------------------------------------------------------------- #
def _first_bad_row(bad_rows, sched):
    b = int(np.flatnonzero(bad_rows)[0])
    if sched is None:
        return f"first wrong row {b}"
    t = b // sched.tile
    w, it = sched.where(t)
    return f"first wrong row {b} = tile {t} (walker {w}, iteration {it}), {int(bad_rows.sum())} rows wrong"


def check_rows_exact(name, got, ref, sched=None):
    """bitwise equality of a per-row output with an exactly representable reference"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if got.dtype == F32:
        assert np.array_equal(ref.astype(F32).astype(F64), ref.astype(F64)), f"{name}: reference not representable"
    if np.array_equal(got.astype(F64), ref.astype(F64)):
        return
    bad = (got.astype(F64) != ref.astype(F64)).reshape(got.shape[0], -1).any(1)
    raise AssertionError(f"{name}: {_first_bad_row(bad, sched)}")


def check_out_denom(got_out, got_denom, ref, sched=None):
    """out and denom of a forward within the derived bounds; rows with a power-of-two norm bitwise"""
    go, gd = np.asarray(got_out, dtype=F64), np.asarray(got_denom, dtype=F64)
    eo = np.abs(go - ref.out) / U
    ed = np.abs(gd - ref.denom) / U
    bad = (eo > OUT_ULPS * np.abs(ref.out)).any(1) | (ed > DENOM_ULPS * ref.denom) | ~np.isfinite(go).all(1)
    ex = ref.exact
    bad |= ex & ((go != ref.out).any(1) | (gd != ref.denom))
    if bad.any():
        raise AssertionError(f"out/denom: {_first_bad_row(bad, sched)}")
    nz = np.abs(ref.out) > 0
    return float((eo[nz] / np.abs(ref.out[nz])).max()), float((ed / ref.denom).max())


def check_slabs(got, ref, d, H, K1):
    """every slab equals the reference sum over its own tiles; names the first wrong slab and section"""
    got, ref = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if np.array_equal(got, ref):
        return
    s = int(np.flatnonzero((got != ref).any(1))[0])
    secs = [n for n, (a, b) in slab_sections(d, H, K1).items() if not np.array_equal(got[s, a:b], ref[s, a:b])]
    raise AssertionError(f"slab {s} wrong in {secs} ({int((got != ref).any(1).sum())} slabs wrong)")


def check_grads(got, ref, names=("dW1", "db1", "dW2", "db2")):
    for n, g, r in zip(names, got, ref):
        g, r = np.asarray(g, dtype=F64), np.asarray(r, dtype=F64)
        assert g.shape == r.shape, (n, g.shape, r.shape)
        if not np.array_equal(g, r):
            raise AssertionError(f"{n}: {int((g != r).sum())} of {g.size} elements wrong, max |diff| "
                                 f"{float(np.abs(g - r).max())}")


# ------------------------------------------------------------------------------------------------------------------- #
# Realistic values: f64 reference with a running error bound                                                           #
# ------------------------------------------------------------------------------------------------------------------- #
# With arbitrary f32 inputs the kernels round.  Every gradient element is a sum of products; the kernel's error is held
# to (depth + c) * u * S, S = the sum of the absolute values of the terms of the fully expanded expression, computed here
# with absolute-value matrix products.  First-order derivation (u = 2^-24, D = embed_dim), inputs taken as exact:
#   dot   = sum_j g_j o_j              f32 chain of D products, any order:  |err| <= D u Sdot,  Sdot = sum_j |g_j o_j|
#   gy_j  = (g_j - o_j dot) / dn       product, difference, reciprocal (1 ulp = 2u) and product: 5 roundings, plus the
#                                      error of dot times |o_j|:            |err| <= (D + 5) u Agy_j,
#                                      Agy_j = (|g_j| + |o_j| Sdot) / dn  >= |gy_j|
#   dh_h  = sum_j gy_j W2[j, h]        chain of D:                          |err| <= (2 D + 5) u Adh_h,  Adh = Agy |W2|
#   dPre  = [hid > 0] dh * scale       one rounding:                        |err| <= (2 D + 6) u Adp,    Adp = scale [hid > 0] Adh
#   dW1[h, k] = sum_b dPre[b, h] x[b, k],  db1[h] = sum_b dPre[b, h]        c = 2 D + 6,  S = sum_b Adp |x|   (|x| = 1 for db1)
#   dW2[j, h] = sum_b gy[b, j] hid[b, h],  db2[j] = sum_b gy[b, j]          c = D + 5,    S = sum_b Agy |hid|
#   dX[b, k]  = sum_h dPre[b, h] W1[h, k]                                   (2 D + 6 + H) u sum_h Adp |W1|
# depth = the longest chain of f32 additions a term of the batch sum passes through: one per row of every tile of the
# slab (the accumulator persists over the workgroup's tiles), one per tile (the column sums add a tile subtotal),
# 16 slabs per group, 16 groups, one for the final store or accumulation: tiles_per_slab * (tile + 1) + 16 + 16 + 1.
# SECOND_ORDER = 1.01 covers the (n u)^2 terms (n u < 1e-4 here) and the f64 reference's own rounding.
SECOND_ORDER = 1.01


def summation_depth(B, tile, nslab_cap=NCU):
    ntiles = (B + tile - 1) // tile
    per = -(-ntiles // min(ntiles, nslab_cap))
    return per * (tile + 1) + SLAB_GROUPS + SLAB_GROUPS + 1


def model_forward(table, ids, genres, W1, b1, W2, b2, keep, scale):
    """f64 forward of the tower (oracle/two_tower_np.py: tower_forward) on f32-valued inputs"""
    x = np.asarray(table, dtype=F64)[ids]
    if genres is not None:
        x = np.concatenate([x, np.asarray(genres, dtype=F64)], axis=1)
    h = np.maximum(x @ np.asarray(W1, dtype=F64).T + np.asarray(b1, dtype=F64), 0.0)
    if keep is not None:
        h = np.where(keep, h * scale, 0.0)
    y = h @ np.asarray(W2, dtype=F64).T + np.asarray(b2, dtype=F64)
    denom = np.maximum(np.sqrt((y * y).sum(1)), float(EPS32))
    return SimpleNamespace(x=x, hid=h, denom=denom, out=y / denom[:, None])


def backward_with_bounds(x, W1, W2, gout, out, denom, hid, scale, d, depth):
    """reference gradients of one tower call and the bound on |kernel - reference| of each (derivation above)"""
    x, gout, out, denom, hid = (np.asarray(v, dtype=F64) for v in (x, gout, out, denom, hid))
    W1, W2 = np.asarray(W1, dtype=F64), np.asarray(W2, dtype=F64)
    H = W1.shape[0]
    ref = backward_rows(x, W1, W2, gout, out, denom, hid, scale, d)
    sdot = (np.abs(gout) * np.abs(out)).sum(1, keepdims=True)
    agy = (np.abs(gout) + np.abs(out) * sdot) / denom[:, None]
    adp = np.where(hid > 0, (agy @ np.abs(W2)) * scale, 0.0)
    S = dict(dW1=adp.T @ np.abs(x), db1=adp.sum(0), dW2=agy.T @ np.abs(hid), db2=agy.sum(0))
    c = dict(dW1=2 * d + 6, db1=2 * d + 6, dW2=d + 5, db2=d + 5)
    bounds = {k: SECOND_ORDER * (depth + c[k]) * U * S[k] for k in S}
    e_dX = SECOND_ORDER * (2 * d + 6 + H) * U * (adp @ np.abs(W1))[:, :d]
    grads = dict(zip(("dW1", "db1", "dW2", "db2"), weight_grads(ref, hid, x)))
    return SimpleNamespace(ref=ref, grads=grads, bounds=bounds, e_dX=e_dX, hid=hid, x=x)


def scatter_with_bound(n_rows, ids, dX, e_dX):
    """dense embedding gradient and its bound: the per-row errors of dX, plus one rounding per sample added to a row"""
    g = scatter_reference(0.0, n_rows, ids, dX)
    ok = (ids >= 1) & (ids < n_rows)
    b = np.zeros_like(g)
    np.add.at(b, ids[ok], e_dX[ok])
    a = np.zeros_like(g)
    np.add.at(a, ids[ok], np.abs(dX[ok]))
    hits = np.bincount(ids[ok], minlength=n_rows).astype(F64)[:, None]
    return g, b + SECOND_ORDER * (hits + 1) * U * a


def dropped_tile_ratios(bw, tiles, tile=32):
    """for each weight gradient: the smallest, over `tiles`, of  max over elements |that tile's contribution| / bound.
    A result that lacks the tile misses the reference by at least (ratio - 1) bounds somewhere: it is red when ratio > 2."""
    worst = {k: np.inf for k in bw.bounds}
    for t in tiles:
        rows = np.arange(t * tile, (t + 1) * tile)
        con = dict(zip(("dW1", "db1", "dW2", "db2"), weight_grads(bw.ref, bw.hid, bw.x, rows)))
        for k in worst:
            ok = bw.bounds[k] > 0
            worst[k] = min(worst[k], float((np.abs(con[k][ok]) / bw.bounds[k][ok]).max()))
    return worst


def check_within(name, got, ref, bound):
    """|got - ref| <= bound element by element; returns the worst error / bound"""
    got, ref, bound = (np.asarray(v, dtype=F64) for v in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0.0))), err.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.size} elements outside the bound; worst at {i}: "
                             f"error {err[i]:.3e}, bound {bound[i]:.3e}")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


REALISTIC = dict(nu=3000, ni=3000, B=65536 + 3 * 32 + 5, p=0.25, state_seed=9, batch_seed=4)


def realistic_tower_inputs(d, H, seeds=(11, 12, 13)):
    """the three tower calls (user, positive items, negative items) of the realistic-values case, forward in f64"""
    from oracle import fixtures as fx
    r = REALISTIC
    sd = fx.make_state(r["nu"], r["ni"], d, H, r["state_seed"])
    u, p, gp, n, gn = fx.make_batch(r["nu"], r["ni"], r["B"], seed=r["batch_seed"])
    scale = float(F32(1.0) / (F32(1.0) - F32(r["p"])))
    calls = []
    for tower, ids, g, seed in (("user_tower", u, None, seeds[0]), ("item_tower", p, gp, seeds[1]), ("item_tower", n, gn, seeds[2])):
        prm = [sd[f"{tower}.{k}"] for k in ("embedding.weight", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias")]
        keep = np.concatenate([O.dropout_keep_mask(seed, r0, min(16384, r["B"] - r0), H, r["p"])
                               for r0 in range(0, r["B"], 16384)])
        calls.append(SimpleNamespace(tower=tower, ids=ids, genres=g, prm=prm, keep=keep, scale=scale,
                                     fwd=model_forward(prm[0], ids, g, *prm[1:], keep, scale)))
    return sd, calls
