"""The in-batch BPR passes (csrc/loss.hip, loss_x6.hip, loss_bf16.hip, loss_generic.hip) pair by pair.

EXACT INPUTS (tests/inbatch_reference.py, part 1): every score is a multiple of 256 and pos = 0, so every weight is
exactly 0, 1/2 or 1 and, with n_global = 2 (c = 1/2), every sum the passes form is exact in f32 in any order.  The
stored weights `gmat`, `r_out`, dU and dI (from the stored-G item pass and from the mode_user=0 sweep) are compared with
``array_equal``: one pair dropped, doubled, moved to another owner, or masked at the wrong place is a wrong bit, at any
size -- where the random-unit-row comparison of the older tests sees nothing below 16 dropped rows.  The loss overflows
by design at such scores and is not looked at here.  Semantics pinned: inbatch_reference.py, part 2.
Which loop regions each case reaches: tests/test_inbatch_host.py.

REALISTIC VALUES (unit rows and rows of norm 2): the weights against fp64 sigma, r / dU / dI / every loss part against
bounds derived in inbatch_reference.BOUNDS_DOC; the worst ratio to the bound is printed per case (run with -s).
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import inbatch_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
NG = R.N_GLOBAL_EXACT


# ---------------------------------------------------------------------------------------------------------------------
# plumbing: NumPy in, NumPy out; every output buffer is prefilled with NaN
# ---------------------------------------------------------------------------------------------------------------------
class Dev:
    def __init__(self):
        import torch
        from recommendit_amd import _lib as L
        self.t, self.L, self.lib, self.dev, self.st = torch, L, L.lib(), L.device(), L.stream_ptr()

    def up(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def nan(self, *shape, dtype=None):
        return self.t.full(shape, float("nan"), dtype=dtype or self.t.float32, device=self.dev)

    def user_pass(self, users, items, user_goff, item_goff, pos, n_global, precision):
        """-> dict(gm: device tensor, r, dU, loss_part: NumPy)"""
        nu, d = users.shape
        ni = items.shape[0]
        lib = self.lib
        assert lib.rihip_inbatch_gmat_floats(nu, ni) == R.gmat_floats(nu, ni)
        U, Y, p = self.up(users), self.up(items), self.up(pos)
        gm = self.nan(R.gmat_floats(nu, ni))
        r, dU = self.nan(nu), self.nan(nu, d)
        lp = self.nan(lib.rihip_inbatch_workspace_doubles(nu), dtype=self.t.float64)
        ws = self.nan(lib.rihip_inbatch_workspace_floats(nu, ni, d))
        self.L.check(lib.rihip_inbatch_user_pass(U.data_ptr(), nu, user_goff, Y.data_ptr(), ni, item_goff, d, p.data_ptr(),
                                                 n_global, dU.data_ptr(), r.data_ptr(), lp.data_ptr(), ws.data_ptr(),
                                                 gm.data_ptr(), precision, self.st), "user_pass")
        self.t.cuda.synchronize()
        return dict(gm=gm, r=r.cpu().numpy(), dU=dU.cpu().numpy(),
                    loss_part=lp.cpu().numpy()[:lib.rihip_inbatch_loss_parts(nu, ni)])

    def item_pass(self, gm, users, user_goff, n_items, item_goff, r, n_global, precision):
        nu, d = users.shape
        lib = self.lib
        U, rr = self.up(users), self.up(r)
        dI = self.nan(n_items, d)
        ws = self.nan(lib.rihip_inbatch_workspace_floats(n_items, nu, d))
        assert gm.numel() == R.gmat_floats(nu, n_items)
        self.L.check(lib.rihip_inbatch_item_pass(gm.data_ptr(), U.data_ptr(), nu, user_goff, n_items, item_goff, d,
                                                 rr.data_ptr(), n_global, dI.data_ptr(), ws.data_ptr(), precision,
                                                 self.st), "item_pass")
        self.t.cuda.synchronize()
        return dI.cpu().numpy()

    def sweep(self, mode_user, owners, o_goff, swept, s_goff, pos, r_in, n_global, precision):
        """-> (d_owner, r_out or None)"""
        no, d = owners.shape
        ns = swept.shape[0]
        lib = self.lib
        O, S, p = self.up(owners), self.up(swept), self.up(pos)
        assert pos.shape == ((no,) if mode_user else (ns,))
        rin = self.up(r_in) if r_in is not None else None
        dO, r = self.nan(no, d), self.nan(no)
        lp = self.nan(lib.rihip_inbatch_workspace_doubles(no), dtype=self.t.float64)
        ws = self.nan(lib.rihip_inbatch_workspace_floats(no, ns, d))
        self.L.check(lib.rihip_inbatch_sweep(1 if mode_user else 0, O.data_ptr(), no, o_goff, S.data_ptr(), ns, s_goff, d,
                                             p.data_ptr(), rin.data_ptr() if rin is not None else None, n_global,
                                             dO.data_ptr(), r.data_ptr(), lp.data_ptr(), ws.data_ptr(), precision,
                                             self.st), "sweep")
        self.t.cuda.synchronize()
        return dO.cpu().numpy(), (r.cpu().numpy() if mode_user else None)


@pytest.fixture(scope="module")
def gpu():
    return Dev()


def _zeros(n):
    return np.zeros(n, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 0. the premise: rcp(2) is exactly 1/2 on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_rcp_of_two_is_exactly_half(gpu):
    """v_rcp_f32 is specified to 1 ulp; the ternary weights need rcp(2.0f) == 0.5f exactly.  A 2 x 2 case whose two
    off-diagonal scores are 0: the stored weights must be exactly 0.5 (f32 MFMA and bf16x6 sweeps, which store them),
    and r = c * 0.5 = 0.25 in the bf16x3 and runtime-width kernels.  Measured on an MI355X: exact in every one of them
    (profiles/r16_inbatch_exact_tests.md); were it not, every exact case would have to keep to the weights {0, 1}."""
    d = 32
    users = np.zeros((2, d), np.float32); items = np.zeros((2, d), np.float32)
    users[0, 0] = users[0, 1] = 16; users[1, 2], users[1, 3] = 16, -16
    items[0, 2] = items[0, 3] = 16; items[1, 0], items[1, 1] = 16, -16           # y0.u1 = 0, y1.u0 = 0
    w = np.array([[0, 0.5], [0.5, 0]], np.float32)                               # [item, user], diagonal masked
    got = {}
    for precision in (0, 2):
        out = gpu.user_pass(users, items, 0, 0, _zeros(2), NG, precision)
        full = R.decode_gmat(out["gm"].cpu().numpy(), 2, 2)
        got[f"user pass precision {precision}"] = (full[1, 0], full[0, 1], out["r"][0])
        R.check_gmat(out["gm"].cpu().numpy(), w, 2, 2)
        R.check_equal("r", out["r"], np.array([0.25, 0.25], np.float32))
    for precision in (0, 1, 2):
        _, r = gpu.sweep(True, users, 0, items, 0, _zeros(2), None, NG, precision)
        got[f"sweep precision {precision}"] = tuple(r)
        R.check_equal("r", r, np.array([0.25, 0.25], np.float32))
    u16, i16 = users[:, :16].copy(), items[:, :16].copy()
    _, r = gpu.sweep(True, u16, 0, i16, 0, _zeros(2), None, NG, 0)
    got["runtime-width sweep"] = tuple(r)
    R.check_equal("r", r, np.array([0.25, 0.25], np.float32))
    print("rcp(2) probe:", {k: [float(x).hex() for x in v] for k, v in got.items()})


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact cases, 4-wave kernels (and, in the child process, the 8-wave kernels at the same shapes)
# ---------------------------------------------------------------------------------------------------------------------
def run_exact_tuned(gpu, shape, d, precisions_stored=(0, 2), precisions_sweep=(0, 1, 2)):
    nu, ni, uo, io = shape
    cs = R.make_exact_case(1000 + 7 * nu + ni + d, nu, ni, d, uo, io)
    R.assert_distinguishable(cs.w2)
    w = cs.weights()
    r, dU = R.expected_user_outputs(cs)
    dI = R.expected_item_outputs(w, cs.users, r, uo, io)
    for p in precisions_stored:
        tag = f"stored-G precision {p}: "
        out = gpu.user_pass(cs.users, cs.items, uo, io, _zeros(nu), NG, p)
        R.check_gmat(out["gm"].cpu().numpy(), w, nu, ni)
        R.check_equal(tag + "r", out["r"], r)
        R.check_equal(tag + "dU", out["dU"], dU)
        R.check_equal(tag + "dI", gpu.item_pass(out["gm"], cs.users, uo, ni, io, out["r"], NG, p), dI)
    for p in precisions_sweep:
        tag = f"two-sweep precision {p}: "
        got_dU, got_r = gpu.sweep(True, cs.users, uo, cs.items, io, _zeros(nu), None, NG, p)
        R.check_equal(tag + "r", got_r, r)
        R.check_equal(tag + "dU", got_dU, dU)
        # owners = the items, swept = the local users at their global offset (the multi-GPU two-sweep form)
        got_dI, _ = gpu.sweep(False, cs.items, io, cs.users, uo, _zeros(nu), r, NG, p)
        R.check_equal(tag + "dI", got_dI, dI)


def run_item_synthetic(gpu, shape, d, precisions=(0, 2)):
    """the item pass alone: gmat written by the test (integers 0..3, zeros in the ragged user slots, NaN wherever the
    result must not depend on it) and an r of dyadic values that no user pass produced"""
    nu, ni, uo, io = shape
    w, users, r = R.make_synthetic_item_case(2000 + nu + 3 * ni + d, nu, ni, d, uo, io)
    gm = gpu.up(R.synthetic_gmat(w, nu, ni))
    dI = R.expected_item_outputs(w, users, r, uo, io)
    for p in precisions:
        R.check_equal(f"synthetic item pass precision {p}: dI", gpu.item_pass(gm, users, uo, ni, io, r, NG, p), dI)


@pytest.mark.parametrize("d", R.TUNED_D)
@pytest.mark.parametrize("shape", R.EXACT_SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_tuned_small(gpu, shape, d):
    run_exact_tuned(gpu, shape, d)


@pytest.mark.parametrize("d", R.TUNED_D)
@pytest.mark.parametrize("shape", R.EXACT_SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_item_pass_synthetic_small(gpu, shape, d):
    run_item_synthetic(gpu, shape, d)


@pytest.mark.parametrize("d", R.GENERIC_D)
@pytest.mark.parametrize("shape", R.GENERIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_generic_width(gpu, shape, d):
    """the runtime-width kernel (two-sweep form only, precision 0)"""
    nu, ni, uo, io = shape
    cs = R.make_exact_case(3000 + nu + ni + d, nu, ni, d, uo, io)
    R.assert_distinguishable(cs.w2)
    r, dU = R.expected_user_outputs(cs)
    dI = R.expected_item_outputs(cs.weights(), cs.users, r, uo, io)
    got_dU, got_r = gpu.sweep(True, cs.users, uo, cs.items, io, _zeros(nu), None, NG, 0)
    R.check_equal("r", got_r, r)
    R.check_equal("dU", got_dU, dU)
    got_dI, _ = gpu.sweep(False, cs.items, io, cs.users, uo, _zeros(nu), r, NG, 0)
    R.check_equal("dI", got_dI, dI)


# ---------------------------------------------------------------------------------------------------------------------
# 2. 8-wave kernels at their smallest natural shape: steady loops (d = 128, precision 0) and bf16x6 (d = 64)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", R.LARGE_USER_OFFSETS)
@pytest.mark.parametrize("d,precision", [(128, 0), (64, 2)])
def test_user_pass_8wave_large(gpu, d, precision, off):
    nu, ni = R.LARGE_OWNERS, R.LARGE_SWEPT
    assert R.sweep_nw(nu, ni) == 8
    cs = R.make_exact_case(4000 + off + d, nu, ni, d, off, 0)
    R.assert_distinguishable(cs.w2)
    r, dU = R.expected_user_outputs(cs)
    out = gpu.user_pass(cs.users, cs.items, off, 0, _zeros(nu), NG, precision)
    R.check_equal("r", out["r"], r)
    R.check_equal("dU", out["dU"], dU)
    R.check_gmat(out["gm"].cpu().numpy(), cs.weights(), nu, ni)


@pytest.mark.parametrize("d,precision", [(128, 0), (64, 2)])
def test_item_pass_8wave_large_synthetic(gpu, d, precision):
    ni, nu = R.LARGE_OWNERS, R.LARGE_SWEPT          # owners = items, swept = users
    assert R.sweep_nw(ni, nu) == 8
    run_item_synthetic(gpu, (nu, ni, 123, 0), d, precisions=(precision,))


# ---------------------------------------------------------------------------------------------------------------------
# 3. 8-wave kernels at small shapes: RIHIP_SWEEP_NW is read once per process, so one fresh child runs them
# ---------------------------------------------------------------------------------------------------------------------
def child_main():
    assert os.environ.get("RIHIP_SWEEP_NW") == "8"
    gpu = Dev()
    n = 0
    for d in R.TUNED_D:
        for shape in R.CHILD_SHAPES:
            run_exact_tuned(gpu, shape, d, precisions_stored=(0, 2), precisions_sweep=(0, 2))
            run_item_synthetic(gpu, shape, d)
            n += 1
    print(f"8-wave child ok: {n} cases")


def test_exact_small_shapes_with_8wave_workgroups(gpu):
    """A child that faults, aborts or hangs ends the whole pytest session: nothing more is started on that GPU."""
    gpu.t.cuda.synchronize()
    env = dict(os.environ, RIHIP_SWEEP_NW="8")
    try:
        p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child-8wave"], env=env, cwd=str(ROOT),
                           capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"8-wave child did not finish in 300 s; stopping the session: {str(e.stderr)[-2000:]}", returncode=3)
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:
        pytest.exit(f"8-wave child died (return code {p.returncode}); stopping the session: {p.stderr[-4000:]}",
                    returncode=3)
    assert p.returncode == 0 and "8-wave child ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


# ---------------------------------------------------------------------------------------------------------------------
# 4. element arithmetic at realistic values, against derived bounds
# ---------------------------------------------------------------------------------------------------------------------
def run_realistic(gpu, key, table, what):
    d, precision, norm = key
    users, items, pos, off = R.make_realistic_case(d, precision, norm, table)
    nu, ni = users.shape[0], items.shape[0]
    ref = R.realistic_reference(users, items, pos, off, 0, ni)
    bg, bs = R.bound_gmat(ref, pos, d, precision), R.bound_sums(ref, pos, d, precision)
    out = gpu.user_pass(users, items, off, 0, pos, ni, precision)
    dI = gpu.item_pass(out["gm"], users, off, ni, 0, out["r"], ni, precision)
    g = R.decode_gmat(out["gm"].cpu().numpy(), nu, ni)[:ni, :nu].astype(np.float64)
    on = ref["g"] > 0
    assert np.all(g[~on] == 0)
    assert out["loss_part"].shape == ref["loss_part"].shape
    ratios = {
        "gmat": float((np.abs(g - ref["g"])[on] / bg[on]).max()),
        "r": float((np.abs(out["r"] - ref["r"]) / bs["r"]).max()),
        "dU": float((np.abs(out["dU"] - ref["dU"]) / bs["dU"]).max()),
        "dI": float((np.abs(dI - ref["dI"]) / bs["dI"]).max()),
        "loss_part": float((np.abs(out["loss_part"] - ref["loss_part"]) / bs["loss_part"]).max()),
    }
    print(f"{what} d={d} precision={precision} norm={norm} {nu}x{ni} nsplit={ref['nsplit']}: worst |err| / bound",
          {k: f"{v:.3f}" for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v <= 1.0, (k, v, ratios)
    if precision == 0 and norm == 1:    # where the plain (n + d + k) u M form is valid, hold the sums to it as well
        plain = R.issue_form_bounds(ref, d)
        for k, got in (("r", out["r"]), ("dU", out["dU"]), ("dI", dI)):
            assert np.all(np.abs(got - ref[k]) <= plain[k]), k


@pytest.mark.parametrize("key", sorted(R.REALISTIC_CASES), ids=lambda k: f"d{k[0]}-p{k[1]}-norm{k[2]}")
def test_realistic_values_within_derived_bounds(gpu, key):
    """Bounds: inbatch_reference.BOUNDS_DOC (score chain of d multiply-adds on inputs pre-scaled by log2 e, pos rounded
    once, |sigma'| <= 1/4, 1-ulp exp2 / rcp; sums (P n + E + k) u M on the un-cancelled magnitude, k = 32).  None of it
    is fitted to a device run.  At these shapes one pair stands >= 100 x above the bounds of r, dU and dI (asserted in
    tests/test_inbatch_host.py).  Worst observed ratios on an MI355X: profiles/r16_inbatch_exact_tests.md."""
    run_realistic(gpu, key, R.REALISTIC_CASES, "realistic")


@pytest.mark.parametrize("key", sorted(R.LOSS_CASES), ids=lambda k: f"d{k[0]}-p{k[1]}-norm{k[2]}")
def test_realistic_loss_parts_within_derived_bounds(gpu, key):
    """The same at the shapes of LOSS_CASES, whose loss parts hold so few pairs that one pair's softplus stands >= 100 x
    above each part's bound (asserted in tests/test_inbatch_host.py): every part is checked on its own."""
    run_realistic(gpu, key, R.LOSS_CASES, "loss parts")


if __name__ == "__main__":
    assert sys.argv[1:] == ["--child-8wave"], sys.argv
    child_main()
