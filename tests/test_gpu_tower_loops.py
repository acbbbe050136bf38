"""The tower kernels' multi-tile loops against exact references (tests/tower_reference.py).

Every tower kernel is persistent: a workgroup (or wave) walks tiles with a stride, and the walks are software-pipelined.
The other tower tests stop at batch sizes where no walker gets a second tile.  Here every kernel runs at
B = R + 3 tile + 5 (a few walkers get a second, ragged, tile; the rest exit after one) and B = 2 R + 9 tile + 17 (a
third iteration: prefetches on both sides of a steady one), R = the rows one pass of the full grid covers.  Inputs are
integers chosen so that every sum is exact in f32 in any order; comparisons are np.array_equal except for out / denom
of the forward, held to the few-ulp bound derived in tower_reference.py.  tests/test_tower_host.py proves the
references, the schedules and that every comparison used here goes red for the defects these loops can have.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tower_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

GENERIC = R.GENERIC
FWD_ENV = {"fwd64": "1", "fwd2": "3"}
BWD_ENV = {"bwd64": "1", "bwd2": "3", "bwd3": "4"}


def _L():
    from recommendit_amd import _lib as L
    return L, L.lib(), L.device()


def _t(a, dtype=torch.float32):
    _, _, dev = _L()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _np(t):
    return t.detach().cpu().numpy()


def _set_env(monkeypatch, var, val):
    if val is None:
        monkeypatch.delenv(var, raising=False)
    else:
        monkeypatch.setenv(var, val)


class FwdDev:
    """device copies of a forward case"""

    def __init__(self, c, ids=None):
        self.c = c
        self.table, self.W1, self.b1, self.W2, self.b2 = (_t(v) for v in (c.table, c.W1, c.b1, c.W2, c.b2))
        self.ids = _t(c.ids if ids is None else ids, torch.int64)
        self.genres = _t(c.genres) if c.genres is not None else None
        _, _, dev = _L()
        self.step = torch.full((1,), c.step, dtype=torch.int64, device=dev)

    def io(self, out, hid, den, fws):
        L, _, _ = _L()
        c, io = self.c, L.TowerIO()
        io.table, io.n_rows, io.ids, io.genres, io.B = self.table.data_ptr(), c.n_rows, self.ids.data_ptr(), L.ptr(self.genres), c.B
        io.W1, io.b1, io.W2, io.b2 = self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr()
        io.seed, io.row0 = c.seed, c.row0
        io.out, io.hid, io.denom, io.fwd_workspace = out.data_ptr(), hid.data_ptr(), den.data_ptr(), L.ptr(fws)
        return io

    def outputs(self):
        _, lib, dev = _L()
        c = self.c
        f32 = dict(dtype=torch.float32, device=dev)
        return (torch.full((c.B, c.d), R.SENTINEL, **f32), torch.full((c.B, c.H), R.SENTINEL, **f32),
                torch.full((c.B,), R.SENTINEL, **f32),
                torch.empty((lib.rihip_tower_forward_workspace_floats(c.d, c.H, int(c.item)),), **f32))

    def run(self, train, workspace=True):
        L, lib, dev = _L()
        c = self.c
        out, hid, den, fws = self.outputs()
        err = torch.zeros((1,), dtype=torch.int32, device=dev)
        L.check(lib.rihip_tower_forward(self.table.data_ptr(), c.n_rows, self.ids.data_ptr(), L.ptr(self.genres), c.B, c.d, c.H,
                                        self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(),
                                        int(train), c.p, c.seed, c.row0, out.data_ptr(), hid.data_ptr(), den.data_ptr(),
                                        err.data_ptr(), fws.data_ptr() if workspace else None, self.step.data_ptr(),
                                        L.stream_ptr()), "tower_forward")
        torch.cuda.synchronize()
        return dict(out=out, hid=hid, den=den, err=int(err.item()))


def _check_forward(res, ref, sched):
    R.check_rows_exact("hid", _np(res["hid"]), ref.hid, sched)
    return R.check_out_denom(_np(res["out"]), _np(res["den"]), ref, sched)


def _same_bits(a, b, what):
    for k in ("hid", "out", "den"):
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


def _auto_kind(B):
    return "fwd2" if B >= 49152 else "fwd64"       # rihip_tower_forward: the wave-per-32-rows kernel from 49 152 rows


# --------------------------------------------------------------------------------------------------------------------
# Forward
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item", [False, True], ids=["user", "item"])
@pytest.mark.parametrize("which", [0, 1], ids=["second", "third"])
@pytest.mark.parametrize("shape", R.TUNED, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["fwd64", "fwd2"])
def test_forward_loops_exact(kind, shape, which, item, monkeypatch):
    """tower_fwd_kernel (64-row tiles, with and without packed weights) and tower_fwd2_kernel (prefetched 32-row tiles) in
    their second and third iterations, eval and training (p = 0.5, step clock, row0 != 0): hid bitwise, out / denom
    within OUT_ULPS / DENOM_ULPS u (rows with a power-of-two norm bitwise); the library's own choice at this B gives the
    bits of the kernel it selects."""
    d, H = shape
    B = R.case_B(kind, which)
    c = R.forward_case(d, H, item, B)
    sched = R.Schedule(kind, B)
    cov = sched.coverage()
    assert cov["second"] and cov["ragged_later"] and cov["idle_last_pass"] and (which == 0 or cov["third"])
    dv = FwdDev(c)
    for train in (False, True):
        ref = R.forward_reference(d, H, item, B, train)
        _set_env(monkeypatch, "RIHIP_TOWER_FWD", FWD_ENV[kind])
        res = dv.run(train)
        assert res["err"] == 0
        ratios = _check_forward(res, ref, sched)
        print(f"{kind} {shape} B={B} item={item} train={train}: worst out / denom error {ratios[0]:.2f}u / {ratios[1]:.2f}u")
        if kind == "fwd64":          # ntiles > 64: the fragment-packed weights; without a workspace: strided loads
            _same_bits(res, dv.run(train, workspace=False), "packed vs unpacked weights")
        forced = res
        if _auto_kind(B) != kind:
            _set_env(monkeypatch, "RIHIP_TOWER_FWD", FWD_ENV[_auto_kind(B)])
            forced = dv.run(train)
            _check_forward(forced, ref, R.Schedule(_auto_kind(B), B))
        _set_env(monkeypatch, "RIHIP_TOWER_FWD", None)
        _same_bits(dv.run(train), forced, f"auto vs forced {_auto_kind(B)}")


@pytest.mark.parametrize("item", [False, True], ids=["user", "item"])
@pytest.mark.parametrize("shape", GENERIC, ids=lambda s: f"{s[0]}x{s[1]}")
def test_generic_forward_loop_exact(shape, item, monkeypatch):
    """tower_fwd_generic_kernel past one pass of its grid (4 NCU workgroups x 32 rows), ragged"""
    d, H = shape
    B = R.case_B("gen_fwd", 0)
    _set_env(monkeypatch, "RIHIP_TOWER_FWD", None)
    c = R.forward_case(d, H, item, B)
    sched = R.Schedule("gen_fwd", B)
    cov = sched.coverage()
    assert cov["second"] and cov["ragged_later"] and cov["idle_last_pass"]
    dv = FwdDev(c)
    for train in (False, True):
        res = dv.run(train)
        assert res["err"] == 0
        ratios = _check_forward(res, R.forward_reference(d, H, item, B, train), sched)
        print(f"generic {shape} B={B} item={item} train={train}: worst out / denom error {ratios[0]:.2f}u / {ratios[1]:.2f}u")


@pytest.mark.parametrize("kind,shape", [("fwd64", (64, 128)), ("fwd2", (128, 128)), ("gen_fwd", (48, 96))])
def test_bad_ids_in_a_later_iteration(kind, shape, monkeypatch):
    """An id >= n_rows and a negative id in rows of the second iteration: err_flag = 1, those rows are computed from
    table row 0 (the documented handling), every other row keeps its bits."""
    d, H = shape
    B = R.case_B(kind, 0)
    _set_env(monkeypatch, "RIHIP_TOWER_FWD", FWD_ENV.get(kind))
    c = R.forward_case(d, H, True, B)
    sched = R.Schedule(kind, B)
    first = sched.pass_rows                                  # first row of the second pass
    rows = np.array([first + 3, first + sched.tile + 9])
    assert all(sched.where(int(r) // sched.tile)[1] == 1 for r in rows) and rows.max() < B
    ids = c.ids.copy()
    ids[rows] = [c.n_rows, -5]
    clean, bad = FwdDev(c).run(True), FwdDev(c, ids).run(True)
    assert clean["err"] == 0 and bad["err"] == 1
    ref = R.forward_rows(c, np.arange(B), True, ids=ids)
    _check_forward(bad, ref, sched)
    keep = np.ones(B, dtype=bool)
    keep[rows] = False
    for k in ("hid", "out", "den"):
        a, b = _np(clean[k]), _np(bad[k])
        assert np.array_equal(a[keep], b[keep]), k
        assert not np.array_equal(a[~keep], b[~keep]), k


# --------------------------------------------------------------------------------------------------------------------
# Backward, through the C ABI with synthetic activations
# --------------------------------------------------------------------------------------------------------------------
class BwdDev:
    def __init__(self, c):
        _, lib, dev = _L()
        self.c = c
        self.table, self.W1, self.W2, self.gout, self.out, self.den, self.hid = (
            _t(v) for v in (c.table, c.W1, c.W2, c.gout, c.out, c.denom, c.hid))
        self.ids = _t(c.ids, torch.int64)
        self.genres = _t(c.genres) if c.genres is not None else None
        self.f32 = dict(dtype=torch.float32, device=dev)
        self.P = c.H * c.K1 + c.H + c.d * c.H + c.d
        self.nws = lib.rihip_tower_backward_workspace_floats(c.B, c.d, c.H, int(c.item))

    def front(self):
        L, c = _L()[0], self.c
        return [self.table.data_ptr(), c.n_rows, self.ids.data_ptr(), L.ptr(self.genres), c.B, c.d, c.H, self.W1.data_ptr(),
                self.W2.data_ptr(), self.gout.data_ptr(), self.out.data_ptr(), self.den.data_ptr(), self.hid.data_ptr(),
                c.scale]

    def grads(self, fill):
        c = self.c
        return [torch.full(s, fill, **self.f32) for s in ((c.H, c.K1), (c.H,), (c.d, c.H), (c.d,))]

    def partial(self):
        L, lib, _ = _L()
        ws = torch.full((self.nws,), R.SENTINEL, **self.f32)
        dX = torch.full((self.c.B, self.c.d), R.SENTINEL, **self.f32)
        n = C.c_int(0)
        L.check(lib.rihip_tower_backward_partial(*self.front(), dX.data_ptr(), ws.data_ptr(), L.stream_ptr(), None,
                                                 C.byref(n)), "tower_backward_partial")
        torch.cuda.synchronize()
        return dX, ws, n.value


def _bwd_sched(kind, c):
    if kind == "gen":
        return R.Schedule("gen_wgrad", c.B, c.d, c.H, c.item)
    return R.Schedule({"bwd64": "bwd64", "bwd2": "wgrad", "bwd3": "bwd3"}[kind], c.B)


def _backward_exact(kind, c):
    L, lib, dev = _L()
    dv = BwdDev(c)
    sched = _bwd_sched(kind, c)
    d, H, K1, B = c.d, c.H, c.K1, c.B
    # ---- partial: dX and every slab
    dX, ws, ns = dv.partial()
    assert ns == sched.nslab, (ns, sched.nslab)
    row_sched = {"bwd64": sched, "bwd2": R.Schedule("bwd_data", B), "bwd3": sched, "gen": R.Schedule("gen_bwd_data", B)}[kind]
    R.check_rows_exact("dX", _np(dX), c.ref.dX, row_sched)
    ref_slabs = R.reference_slabs(c, sched)
    R.check_slabs(_np(ws[: ns * dv.P]).reshape(ns, dv.P), ref_slabs, d, H, K1)
    ref_g = R.split_slab(R.reduce_slabs(ref_slabs), d, H, K1)
    R.check_grads(ref_g, R.weight_grads(c.ref, c.hid, c.x))          # (the slabs add up to the whole batch)
    st = L.stream_ptr()
    # ---- the two-level slab reduction on its own
    g = dv.grads(R.SENTINEL)
    L.check(lib.rihip_tower_backward_reduce2(d, H, ws.data_ptr(), B, int(c.item), ns, *(x.data_ptr() for x in g), None, 0, 0,
                                             0, None, None, None, None, 0, st), "reduce2")
    torch.cuda.synchronize()
    R.check_grads([_np(x) for x in g], ref_g)
    # ---- the reduction inside the scatter launch: integer dX, table gradients preset to a power of two
    rng = np.random.default_rng(B)
    sdx = rng.integers(-3, 4, size=(B, d)).astype(np.float64) + (np.arange(B) // 32 % 3)[:, None]
    ids2 = rng.integers(0, 50, size=100)
    sdx2 = rng.integers(-3, 4, size=(100, d)).astype(np.float64)
    tab, tab2 = torch.full((c.n_rows, d), 4.0, **dv.f32), torch.full((50, d), 4.0, **dv.f32)
    sdx_d, ids2_d, sdx2_d = _t(sdx), _t(ids2, torch.int64), _t(sdx2)
    g = dv.grads(R.SENTINEL)
    L.check(lib.rihip_backward_reduce2_scatter2(d, H, ws.data_ptr(), B, int(c.item), ns, *(x.data_ptr() for x in g), None, 0,
                                                0, 0, None, None, None, None, 0, tab.data_ptr(), c.n_rows,
                                                dv.ids.data_ptr(), sdx_d.data_ptr(), B, tab2.data_ptr(), 50,
                                                ids2_d.data_ptr(), sdx2_d.data_ptr(), 100, st), "reduce2_scatter2")
    torch.cuda.synchronize()
    R.check_grads([_np(x) for x in g], ref_g)
    want = R.scatter_reference(4.0, c.n_rows, c.ids, sdx)
    assert np.abs(want).max() < R.LIMIT
    R.check_rows_exact("scattered table", _np(tab), want)
    R.check_rows_exact("second scattered table", _np(tab2), R.scatter_reference(4.0, 50, ids2, sdx2))
    # ---- the one-call form, accumulating onto a non-zero destination
    g = dv.grads(3.0)
    ws2 = torch.full((dv.nws,), R.SENTINEL, **dv.f32)
    dX2 = torch.full((B, d), R.SENTINEL, **dv.f32)
    L.check(lib.rihip_tower_backward(*dv.front(), dX2.data_ptr(), *(x.data_ptr() for x in g), 1, ws2.data_ptr(), st),
            "tower_backward")
    torch.cuda.synchronize()
    R.check_rows_exact("dX (one call)", _np(dX2), c.ref.dX, row_sched)
    R.check_grads([_np(x) for x in g], [v + 3.0 for v in ref_g])


def _bwd_cases():
    out = []
    for shape in R.TUNED:
        out += [("bwd64", shape, R.case_B("bwd64", w)) for w in (0, 1)]
    out += [("bwd2", (128, 128), B) for B in (R.case_B("wgrad", 0), R.case_B("wgrad", 1), R.case_B("bwd_data", 0),
                                              R.case_B("bwd_data", 1))]
    out += [("bwd3", (128, 128), R.case_B("bwd3", w)) for w in (0, 1)]
    return out


@pytest.mark.parametrize("item", [False, True], ids=["user", "item"])
@pytest.mark.parametrize("kind,shape,B", _bwd_cases(), ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_backward_loops_exact(kind, shape, B, item, monkeypatch):
    """tower_bwd_kernel (all five shapes), tower_bwd_data_kernel + tower_wgrad_kernel and tower_bwd3_kernel in later
    iterations: dX bitwise, every slab equal to the reference sum over exactly its own tiles, the gradients after the
    stand-alone and the fused two-level reduction, and after the accumulating one-call form."""
    d, H = shape
    _set_env(monkeypatch, "RIHIP_TOWER_BWD", BWD_ENV[kind])
    c = R.backward_case(d, H, item, B)
    cov = _bwd_sched(kind, c).coverage()
    assert cov["second"] and cov["ragged_later"] and cov["idle_last_pass"] and cov["nslab_gt16"]
    assert cov["both_buffers"] == (True if kind == "bwd2" else None)
    _backward_exact(kind, c)
    # the library's own choice: the two-kernel form for d = hidden = 128 from 49 152 rows, else the 64-row-tile kernel
    auto = "bwd2" if (shape == (128, 128) and B >= 49152) else "bwd64"
    if auto == kind:
        dv = BwdDev(c)
        forced = dv.partial()
        _set_env(monkeypatch, "RIHIP_TOWER_BWD", None)
        chosen = dv.partial()
        assert forced[2] == chosen[2] and torch.equal(forced[0], chosen[0])
        assert torch.equal(forced[1][: forced[2] * dv.P], chosen[1][: forced[2] * dv.P])


@pytest.mark.parametrize("item", [False, True], ids=["user", "item"])
@pytest.mark.parametrize("shape", GENERIC, ids=lambda s: f"{s[0]}x{s[1]}")
def test_generic_backward_loop_exact(shape, item, monkeypatch):
    """tower_bwd_data_generic_kernel past one pass of its grid and tower_wgrad_generic_kernel with several tiles per
    batch split"""
    d, H = shape
    _set_env(monkeypatch, "RIHIP_TOWER_BWD", None)
    B = R.case_B("gen_bwd_data", 0)
    c = R.backward_case(d, H, item, B)
    assert R.Schedule("gen_bwd_data", B).coverage()["ragged_later"]
    cov = _bwd_sched("gen", c).coverage()
    assert cov["second"] and cov["third"]
    _backward_exact("gen", c)


# --------------------------------------------------------------------------------------------------------------------
# Pair launches: the two towers split one grid unevenly
# --------------------------------------------------------------------------------------------------------------------
def _assert_pair_path(ios, backward):
    """the conditions under which the *_pair entry points launch the pair kernel instead of falling back to two single
    calls (restated from tower.hip), so that the test is known to reach tower_fwd_pair_kernel / tower_bwd_pair_kernel"""
    user, item = ios
    assert user.genres is None and item.genres is not None
    for io in ios:
        assert 0 < io.B < 49152 and io.n_rows > 0
        ptrs = [io.table, io.out, io.hid] + ([io.grad_out] if backward else [io.fwd_workspace])
        assert all(p is not None and p % 16 == 0 for p in ptrs), ptrs
        need = [io.ids, io.W1, io.W2] + ([io.denom, io.dX, io.bwd_workspace] if backward else [io.b1, io.b2])
        assert all(p is not None for p in need)
    if backward:
        assert user.bwd_workspace != item.bwd_workspace


@pytest.mark.parametrize("shape", [(64, 128), (32, 64), (128, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_launches_exact(shape, monkeypatch):
    """rihip_tower_forward_pair / rihip_tower_backward_partial_pair with the user tower below one pass of its share of
    the grid and the item tower above it: both against the reference, not only against the single calls."""
    L, lib, dev = _L()
    d, H = shape
    _set_env(monkeypatch, "RIHIP_TOWER_FWD", None)
    _set_env(monkeypatch, "RIHIP_TOWER_BWD", None)
    st = L.stream_ptr()
    # ---- forward
    Bu, Bi = 5000, R.case_B("fwd64", 0)
    cu, ci = R.forward_case(d, H, False, Bu), R.forward_case(d, H, True, Bi)
    su, si = R.Schedule("fwd64", Bu), R.Schedule("fwd64", Bi)
    assert su.nwalkers < si.nwalkers and su.coverage()["max_iterations"] == 1 and si.coverage()["ragged_later"]
    du, di = FwdDev(cu), FwdDev(ci)
    assert cu.step == ci.step
    for train in (False, True):
        ou, oi = du.outputs(), di.outputs()
        err = torch.zeros((1,), dtype=torch.int32, device=dev)
        iu, ii = du.io(*ou), di.io(*oi)
        _assert_pair_path((iu, ii), backward=False)
        L.check(lib.rihip_tower_forward_pair(C.byref(iu), C.byref(ii), d, H, int(train), R.P_DROP, err.data_ptr(),
                                             du.step.data_ptr(), st), "forward_pair")
        torch.cuda.synchronize()
        assert int(err.item()) == 0
        for c, o, s in ((cu, ou, su), (ci, oi, si)):
            _check_forward(dict(out=o[0], hid=o[1], den=o[2]), R.forward_reference(d, H, c.item, c.B, train), s)
    # ---- backward
    Bu, Bi = 5000, R.case_B("bwd64", 0)
    cu, ci = R.backward_case(d, H, False, Bu), R.backward_case(d, H, True, Bi)
    ios, keep = [], []
    for c in (cu, ci):
        dv = BwdDev(c)
        dX = torch.full((c.B, d), R.SENTINEL, **dv.f32)
        ws = torch.full((dv.nws,), R.SENTINEL, **dv.f32)
        io = L.TowerIO()
        io.table, io.n_rows, io.ids, io.genres, io.B = dv.table.data_ptr(), c.n_rows, dv.ids.data_ptr(), L.ptr(dv.genres), c.B
        io.W1, io.W2 = dv.W1.data_ptr(), dv.W2.data_ptr()
        io.out, io.hid, io.denom = dv.out.data_ptr(), dv.hid.data_ptr(), dv.den.data_ptr()
        io.grad_out, io.dX, io.bwd_workspace = dv.gout.data_ptr(), dX.data_ptr(), ws.data_ptr()
        ios.append(io)
        keep.append((dv, dX, ws))
    _assert_pair_path(ios, backward=True)
    nu, ni = C.c_int(0), C.c_int(0)
    L.check(lib.rihip_tower_backward_partial_pair(C.byref(ios[0]), C.byref(ios[1]), d, H, 2.0, st, None, None, C.byref(nu),
                                                  C.byref(ni)), "backward_partial_pair")
    torch.cuda.synchronize()
    for c, (dv, dX, ws), ns in ((cu, keep[0], nu.value), (ci, keep[1], ni.value)):
        sched = R.Schedule("bwd64", c.B)
        assert ns == sched.nslab
        R.check_rows_exact("dX", _np(dX), c.ref.dX, sched)
        R.check_slabs(_np(ws[: ns * dv.P]).reshape(ns, dv.P), R.reference_slabs(c, sched), d, H, c.K1)
    assert nu.value < ni.value and R.Schedule("bwd64", Bi).coverage()["ragged_later"]


# --------------------------------------------------------------------------------------------------------------------
# Realistic values through the Python layer on the default path
# --------------------------------------------------------------------------------------------------------------------
def _tower_node(t):
    """the autograd node of the tower Function behind an output (its saved tensors: the kernel's own out, hid, denom)"""
    fn = t.grad_fn
    while fn is not None and "_TowerFn" not in type(fn).__name__:
        fn = fn.next_functions[0][0]
    assert fn is not None
    return fn


@pytest.mark.parametrize("shape", [(128, 128), (64, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_default_path_realistic_values(shape, monkeypatch):
    """TwoTowerModel, no kernel selection, B = 65 536 + 3 * 32 + 5, train mode with dropout 0.25, bpr_loss, backward():
    the autograd Function, seed plumbing, workspace sizing and scatter past one pass of every grid.
    Outputs: atol 2e-6 against the f64 forward.  Gradients: each tower call's backward is recomputed in f64 from exactly
    what the kernel was given (its own out, hid, denom and the incoming gradient), and every element is held to
    (depth + c) u sum|terms| (tower_reference.py: backward_with_bounds; depth = summation_depth of the kernel the library
    picks: 32-row tiles for 128/128, 64-row tiles for (64, 128)); the item tower's two calls add one rounding.
    tests/test_tower_host.py shows that a dropped 32-row tile is above twice these bounds, so it would be red here.
    Measured worst error / bound on an MI355X (128x128 | 64x128):  dW1 0.001 | 0.001, db1 < 0.001 | 0.001,
    dW2 0.005 | 0.005, db2 0.003 | 0.003, embedding rows < 0.001 | < 0.001 (worst-case bounds: f32 errors do not line up)."""
    from recommendit_amd import TwoTowerModel
    from oracle import two_tower_np as O
    d, H = shape
    _set_env(monkeypatch, "RIHIP_TOWER_FWD", None)
    _set_env(monkeypatch, "RIHIP_TOWER_BWD", None)
    r = R.REALISTIC
    B = r["B"]
    torch.manual_seed(1234)
    seeds = [int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item()) for _ in range(3)]
    sd, calls = R.realistic_tower_inputs(d, H, seeds)
    m = TwoTowerModel(r["nu"], r["ni"], embed_dim=d, hidden_dim=H, dropout=r["p"])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m.to(_L()[2])
    m.train()
    torch.manual_seed(1234)
    outs = [m.user_tower(_t(calls[0].ids, torch.int64)),
            m.item_tower(_t(calls[1].ids, torch.int64), _t(calls[1].genres)),
            m.item_tower(_t(calls[2].ids, torch.int64), _t(calls[2].genres))]
    for o in outs:
        o.retain_grad()
    saved = []
    for o, c in zip(outs, calls):
        np.testing.assert_allclose(_np(o), c.fwd.out, atol=2e-6, rtol=0)
        st = _tower_node(o).saved_tensors                      # table, W1, W2, ids, genres, out, hid, denom
        assert torch.equal(st[5], o.detach())
        np.testing.assert_allclose(_np(st[6]), c.fwd.hid, atol=1e-5, rtol=0)
        saved.append((_np(st[5]), _np(st[6]), _np(st[7])))
    loss = m.bpr_loss(*outs)
    loss.backward()
    torch.cuda.synchronize()
    lo = O.bpr_loss(*(c.fwd.out.astype(np.float32) for c in calls))[0]
    assert abs(float(loss.detach()) - float(lo)) < 1e-5
    tile = 32 if shape == (128, 128) else 64                    # the two-kernel backward / the 64-row-tile kernel
    depth = R.summation_depth(B, tile)
    bws = [R.backward_with_bounds(c.fwd.x, c.prm[1], c.prm[3], _np(o.grad), so, sden, shid, c.scale, d, depth)
           for c, o, (so, shid, sden) in zip(calls, outs, saved)]
    G = {k: _np(v.grad) for k, v in m.named_parameters()}
    names = dict(dW1="mlp.0.weight", db1="mlp.0.bias", dW2="mlp.3.weight", db2="mlp.3.bias")
    ratios = {}
    for k, pn in names.items():
        ru = R.check_within(f"user {k}", G[f"user_tower.{pn}"], bws[0].grads[k], bws[0].bounds[k])
        ref = bws[1].grads[k] + bws[2].grads[k]
        ri = R.check_within(f"item {k}", G[f"item_tower.{pn}"], ref,
                            bws[1].bounds[k] + bws[2].bounds[k] + R.SECOND_ORDER * R.U * np.abs(ref))
        ratios[k] = max(ru, ri)
    gu, bu = R.scatter_with_bound(r["nu"] + 1, calls[0].ids, bws[0].ref.dX, bws[0].e_dX)
    ratios["emb"] = R.check_within("user embedding", G["user_tower.embedding.weight"], gu, bu)
    gp, bp = R.scatter_with_bound(r["ni"] + 1, calls[1].ids, bws[1].ref.dX, bws[1].e_dX)
    gn, bn = R.scatter_with_bound(r["ni"] + 1, calls[2].ids, bws[2].ref.dX, bws[2].e_dX)
    ratios["emb"] = max(ratios["emb"], R.check_within("item embedding", G["item_tower.embedding.weight"], gp + gn,
                                                      bp + bn + R.SECOND_ORDER * R.U * np.abs(gp + gn)))
    print(f"default path {shape}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
