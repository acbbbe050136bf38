"""The in-batch sampled-softmax sweeps (csrc/loss_softmax.hip) against the f64 reference of tests/softmax_reference.py,
within the bounds derived there (BOUNDS_DOC; nothing in them comes from a device run).  Every output buffer is prefilled
with NaN and carries guard rows that must stay NaN.  The worst ratio to the bound is printed per case (run with -s)."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import softmax_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 3     # rows past the end of every output that must keep their NaN prefill


class Dev:
    """NumPy in, NumPy out"""

    def __init__(self):
        import torch
        from recommendit_amd import _lib as L
        self.t, self.L, self.lib, self.dev, self.st = torch, L, L.lib(), L.device(), L.stream_ptr()

    def up(self, a):
        return None if a is None else self.t.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def nan(self, *shape, dtype=None):
        return self.t.full(shape, float("nan"), dtype=dtype or self.t.float32, device=self.dev)

    @staticmethod
    def _cut(t, n, what):
        a = t.cpu().numpy()
        assert np.isnan(a[n:]).all(), f"{what}: written outside [0, {n})"
        return a[:n]

    def user_raw(self, users, items, ug, ig, inv_temp, n_global, logq=None, upos=None, iids=None, d=None):
        """-> (status, dict of device tensors); d overrides the width argument (contract tests)"""
        nu, ni = users.shape[0], items.shape[0]
        d = users.shape[1] if d is None else d
        P = self.L.ptr
        U, Y, lq, up_, ii = (self.up(x) for x in (users, items, logq, upos, iids))
        npart = self.lib.rihip_inbatch_softmax_loss_parts(nu)
        assert npart == R.cdiv(nu, R.OWN)
        out = dict(dU=self.nan(nu + GUARD, users.shape[1]), lse=self.nan(nu + GUARD),
                   loss_part=self.nan(npart + GUARD, dtype=self.t.float64))
        rc = self.lib.rihip_inbatch_softmax_user_sweep(U.data_ptr(), nu, ug, Y.data_ptr(), ni, ig, d, inv_temp, P(lq), P(up_),
                                                       P(ii), n_global, out["dU"].data_ptr(), out["lse"].data_ptr(),
                                                       out["loss_part"].data_ptr(), self.st)
        self.t.cuda.synchronize()
        return rc, out

    def user(self, users, items, ug, ig, inv_temp, n_global, logq=None, upos=None, iids=None):
        rc, out = self.user_raw(users, items, ug, ig, inv_temp, n_global, logq, upos, iids)
        self.L.check(rc, "softmax_user_sweep")
        nu = users.shape[0]
        return dict(dU=self._cut(out["dU"], nu, "dU"), lse=self._cut(out["lse"], nu, "lse"),
                    loss_part=self._cut(out["loss_part"], R.cdiv(nu, R.OWN), "loss_part"))

    def item_raw(self, items, users, ig, ug, inv_temp, n_global, lse, logq=None, iids=None, upos=None, d=None):
        ni, nu = items.shape[0], users.shape[0]
        d = items.shape[1] if d is None else d
        P = self.L.ptr
        Y, U, lq, ii, up_, ls = (self.up(x) for x in (items, users, logq, iids, upos, np.asarray(lse, np.float32)))
        dI = self.nan(ni + GUARD, items.shape[1])
        rc = self.lib.rihip_inbatch_softmax_item_sweep(Y.data_ptr(), ni, ig, U.data_ptr(), nu, ug, d, inv_temp, P(lq), P(ii),
                                                       P(up_), ls.data_ptr(), n_global, dI.data_ptr(), self.st)
        self.t.cuda.synchronize()
        return rc, dI

    def item(self, items, users, ig, ug, inv_temp, n_global, lse, logq=None, iids=None, upos=None):
        rc, dI = self.item_raw(items, users, ig, ug, inv_temp, n_global, lse, logq, iids, upos)
        self.L.check(rc, "softmax_item_sweep")
        return self._cut(dI, items.shape[0], "dI")

    def last_error(self):
        return self.lib.rihip_last_error().decode()


@pytest.fixture(scope="module")
def gpu():
    return Dev()


def _ref(cs, inv_temp, n_global, lse_in=None):
    return R.reference(cs["users"], cs["items"], cs["user_goff"], cs["item_goff"], inv_temp, n_global, cs["logq"],
                       cs["user_pos_ids"], cs["item_ids"], lse_in=lse_in)


def check_user(gpu, cs, inv_temp, n_global, tag):
    d = cs["users"].shape[1]
    ref = _ref(cs, inv_temp, n_global)
    assert ref["user_ok"]
    bnd = R.bounds(ref, cs["users"], cs["items"], d, inv_temp)
    got = gpu.user(cs["users"], cs["items"], cs["user_goff"], cs["item_goff"], inv_temp, n_global, cs["logq"],
                   cs["user_pos_ids"], cs["item_ids"])
    ratios = {k: R.worst_ratio(got[k], ref[k], bnd[k]) for k in ("lse", "dU", "loss_part")}
    print(tag, "user", {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (tag, ratios)
    return got, ref, bnd


def check_item(gpu, cs, inv_temp, n_global, tag):
    """lse given to the sweep: the reference's own, rounded to f32 (0 for a user whose every pair is dropped)"""
    d = cs["users"].shape[1]
    lse = _ref(cs, inv_temp, n_global)["lse"]
    lse32 = np.where(np.isfinite(lse), lse, 0.0).astype(np.float32)
    ref = _ref(cs, inv_temp, n_global, lse_in=lse32)
    bnd = R.bounds(ref, cs["users"], cs["items"], d, inv_temp)
    got = gpu.item(cs["items"], cs["users"], cs["item_goff"], cs["user_goff"], inv_temp, n_global, lse32, cs["logq"],
                   cs["item_ids"], cs["user_pos_ids"])
    ratio = R.worst_ratio(got, ref["dI"], bnd["dI"])
    print(tag, "item dI", round(ratio, 3))
    assert ratio <= 1.0, (tag, ratio)
    return got, ref, bnd


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel against reference: every width, both temperatures, every shape; logq and ids given
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.USER_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("d", R.WIDTHS)
def test_user_sweep_against_reference(gpu, d, shape):
    nu, ni, ug, ig = shape
    for inv_temp in R.INV_TEMPS:
        cs = R.make_case(1000 + d + nu, nu, ni, ug, ig, d)
        check_user(gpu, cs, inv_temp, ig + ni + 5, (d, shape, inv_temp))


@pytest.mark.parametrize("shape", R.ITEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("d", R.WIDTHS)
def test_item_sweep_against_reference(gpu, d, shape):
    ni, nu, ig, ug = shape
    for inv_temp in R.INV_TEMPS:
        cs = R.make_case(2000 + d + nu, nu, ni, ug, ig, d)
        check_item(gpu, cs, inv_temp, max(ig + ni, ug + nu) + 5, (d, shape, inv_temp))


@pytest.mark.parametrize("with_logq,with_ids", [(False, False), (True, False), (False, True)])
def test_optional_arguments(gpu, with_logq, with_ids):
    for d, (nu, ni, ug, ig) in ((64, (129, 300, 77, 0)), (144, (33, 127, 94, 0))):
        cs = R.make_case(31, nu, ni, ug, ig, d, with_logq, with_ids)
        check_user(gpu, cs, 20.0, ni, (d, with_logq, with_ids))
        check_item(gpu, cs, 20.0, ni, (d, with_logq, with_ids))


@pytest.mark.parametrize("d", sorted(R.REALISTIC_CASES))
def test_realistic_cases(gpu, d):
    """the sizes at which one dropped pair would stand 100 x above the bound (tests/test_softmax_host.py)"""
    cs = R.make_realistic_case(d, R.REALISTIC_INV_TEMP)
    ni = cs["items"].shape[0]
    check_user(gpu, cs, R.REALISTIC_INV_TEMP, ni, ("realistic", d))
    check_item(gpu, cs, R.REALISTIC_INV_TEMP, ni, ("realistic", d))


# ---------------------------------------------------------------------------------------------------------------------
# 2. rescale paths: where the running maximum settles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ni", [300, 517])
@pytest.mark.parametrize("where", ["last", "first", "turn"])
def test_rescale_paths(gpu, ni, where):
    """last: logq falls by 10 per tile, so every tile raises every row's maximum and the last one holds it (a rescale by
    e^-10 per tile); first: it rises by 10 per tile, the first tile holds every maximum and later tiles only add small
    terms; turn: user i is a copy of an item of tile i mod T (cosine 1, logit 20 against |l| <~ 8 elsewhere)."""
    d, nu, inv_temp = 64, 130, 20.0
    T = R.cdiv(ni, R.SWT)
    cs = R.make_case(77, nu, ni, 0, 0, d, with_logq=True, with_ids=False)
    tile = np.arange(ni) // R.SWT
    if where == "turn":
        cs["logq"] = np.zeros(ni, np.float32)
        for i in range(nu):
            t = i % T
            j = min(t * R.SWT + (37 * i) % R.SWT, ni - 1)
            cs["users"][i] = cs["items"][j]
    else:
        cs["logq"] = ((-10.0 if where == "last" else 10.0) * tile).astype(np.float32)
    ref = _ref(cs, inv_temp, ni)
    arg_tile = np.argmax(ref["l"], axis=1) // R.SWT
    if where == "last":
        assert (arg_tile == T - 1).all()
    elif where == "first":
        assert (arg_tile == 0).all()
    else:
        assert (arg_tile == np.arange(nu) % T).all()
    check_user(gpu, cs, inv_temp, ni, ("rescale", where, ni))
    check_item(gpu, cs, inv_temp, ni, ("rescale", where, ni))


# ---------------------------------------------------------------------------------------------------------------------
# 3. overflow: logits up to +-256
# ---------------------------------------------------------------------------------------------------------------------
def _overflow_case():
    d, nu, ni = 64, 40, 150
    cs = R.make_case(5, nu, ni, 0, 0, d, with_logq=False, with_ids=False, norm=4.0)
    e = np.eye(d, dtype=np.float32)
    for j in range(8):          # users 0..7 lean on e_0 (cosine 0.9), their partners equal them: l_jj = 16 * 16 = 256
        cs["users"][j] = 4 * (np.float32(0.9) * e[0] + np.float32(np.sqrt(1 - 0.81)) * e[j + 1])
        cs["items"][j] = cs["users"][j]
        cs["items"][100 + j] = -cs["users"][j]                      # l = -256
    cs["items"][149] = -4 * e[0]      # item 149: l = -230.4 for users 0..7, whose lse is >= 256; its partner user 149 does not exist
    return cs


def test_overflow_scale_stays_finite_and_within_bound(gpu):
    cs = _overflow_case()
    inv_temp = 16.0
    ref = _ref(cs, inv_temp, 150)
    with np.errstate(over="ignore"):
        assert ref["l"].max() >= 255.9 and ref["l"].min() <= -255.9 and np.exp(np.float32(ref["l"].max())) == np.inf
    got, _, _ = check_user(gpu, cs, inv_temp, 150, "overflow")
    assert np.isfinite(got["dU"]).all() and np.isfinite(got["lse"]).all() and np.isfinite(got["loss_part"]).all()
    dI, _, _ = check_item(gpu, cs, inv_temp, 150, "overflow")
    assert np.isfinite(dI).all()


def test_underflowed_weights_are_exact_zeros(gpu):
    """item 149 is seen by users 0..7 only, each of which it loses to by e^-486: below 2^-150, nothing f32 can hold.  Its
    partner is not among them, so dI[149] must be exactly 0 in every component."""
    cs = _overflow_case()
    inv_temp = 16.0
    full = _ref(cs, inv_temp, 150)
    lse32 = full["lse"].astype(np.float32)[:8]
    part = R.reference(cs["users"][:8], cs["items"], 0, 0, inv_temp, 150, lse_in=lse32)
    assert 0 < part["p_item"][:, 149].max() < 2.0 ** -150
    dI = gpu.item(cs["items"], cs["users"][:8], 0, 0, inv_temp, 150, lse32)
    assert np.array_equal(dI[149], np.zeros(64, np.float32)), dI[149]
    bnd = R.bounds(part, cs["users"][:8], cs["items"], 64, inv_temp)
    assert R.worst_ratio(dI, part["dI"], bnd["dI"]) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. mask
# ---------------------------------------------------------------------------------------------------------------------
def test_masked_pair_contributes_exactly_zero(gpu):
    """one swept user whose positive's id also sits on item 7 (not its partner, partner user absent): with ids, dI[7] is
    exactly 0; without them it is not"""
    d, ni = 48, 40
    cs = R.make_case(9, 1, ni, 20, 0, d, with_logq=True, with_ids=True)
    cs["item_ids"] = np.arange(100, 100 + ni, dtype=np.int64)
    cs["item_ids"][7] = cs["item_ids"][20]
    cs["user_pos_ids"] = cs["item_ids"][[20]].copy()
    ref = _ref(cs, 20.0, ni)
    assert ref["dropped"].sum() == 1 and ref["dropped"][0, 7]
    lse32 = ref["lse"].astype(np.float32)
    args = (cs["items"], cs["users"], 0, 20, 20.0, ni, lse32, cs["logq"])
    with_ids = gpu.item(*args, cs["item_ids"], cs["user_pos_ids"])
    without = gpu.item(*args)
    assert np.array_equal(with_ids[7], np.zeros(d, np.float32))
    assert np.abs(without[7]).min() > 0
    keep = np.arange(ni) != 7
    assert np.array_equal(with_ids[keep], without[keep])     # the other items do not see the mask (lse is an input)


def test_null_ids_equal_ids_without_duplicates(gpu):
    d, nu, ni, ug = 144, 129, 300, 77
    cs = R.make_case(3, nu, ni, ug, 0, d, with_logq=True, with_ids=False)
    iids = np.arange(5000, 5000 + ni, dtype=np.int64)
    upos = iids[ug:ug + nu].copy()
    a = gpu.user(cs["users"], cs["items"], ug, 0, 20.0, ni, cs["logq"])
    b = gpu.user(cs["users"], cs["items"], ug, 0, 20.0, ni, cs["logq"], upos, iids)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    ia = gpu.item(cs["items"], cs["users"], 0, ug, 20.0, ni, a["lse"], cs["logq"])
    ib = gpu.item(cs["items"], cs["users"], 0, ug, 20.0, ni, a["lse"], cs["logq"], iids, upos)
    assert np.array_equal(ia, ib)


# ---------------------------------------------------------------------------------------------------------------------
# 5. slices of the users
# ---------------------------------------------------------------------------------------------------------------------
def test_item_sweep_is_additive_over_user_slices(gpu):
    """257 items, 161 users in three slices: items 0..160 meet their partner in exactly one slice, 161..256 in none"""
    d, nu, ni, inv_temp = 64, 161, 257, 20.0
    cs = R.make_case(21, nu, ni, 0, 0, d)
    lse = _ref(cs, inv_temp, ni)["lse"].astype(np.float32)
    full_ref = _ref(cs, inv_temp, ni, lse_in=lse)
    full = gpu.item(cs["items"], cs["users"], 0, 0, inv_temp, ni, lse, cs["logq"], cs["item_ids"], cs["user_pos_ids"])
    total = np.zeros((ni, d), np.float64)
    bound = R.bounds(full_ref, cs["users"], cs["items"], d, inv_temp)["dI"].copy()
    for lo, hi in ((0, 50), (50, 130), (130, 161)):
        us, up_ = cs["users"][lo:hi], cs["user_pos_ids"][lo:hi]
        part_ref = R.reference(us, cs["items"], lo, 0, inv_temp, ni, cs["logq"], up_, cs["item_ids"], lse_in=lse[lo:hi])
        got = gpu.item(cs["items"], us, 0, lo, inv_temp, ni, lse[lo:hi], cs["logq"], cs["item_ids"], up_)
        pb = R.bounds(part_ref, us, cs["items"], d, inv_temp)["dI"]
        assert R.worst_ratio(got, part_ref["dI"], pb) <= 1.0, (lo, hi)
        total += got
        bound += pb
    ratio = R.worst_ratio(total, full.astype(np.float64), bound)
    print("slices", round(ratio, 3))
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 6. contract
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors(gpu):
    cs = R.make_case(1, 33, 64, 10, 0, 32)
    U, Y, ids_u, ids_i = cs["users"], cs["items"], cs["user_pos_ids"], cs["item_ids"]
    lse = np.zeros(33, np.float32)

    def bad(rc, what):
        assert rc in (1, 3), (what, rc)            # RIHIP_ERR_ARG / RIHIP_ERR_SHAPE
        msg = gpu.last_error()
        assert "inbatch_softmax" in msg, (what, msg)
        return msg

    # a user-mode partner outside the item set: below, above, and a slice of the items
    for ug, ig in ((40, 0), (0, 5), (100, 50)):
        msg = bad(gpu.user_raw(U, Y, ug, ig, 1.0, 200)[0], "partner outside")
        assert "outside" in msg
    bad(gpu.user_raw(U, Y, 10, 0, 1.0, 64, upos=ids_u)[0], "one id array")
    bad(gpu.user_raw(U, Y, 10, 0, 1.0, 64, iids=ids_i)[0], "one id array")
    bad(gpu.item_raw(Y, U, 0, 10, 1.0, 64, lse, iids=ids_i)[0], "one id array")
    bad(gpu.item_raw(Y, U, 0, 10, 1.0, 64, lse, upos=ids_u)[0], "one id array")
    for it in (0.0, -1.0, float("nan"), float("inf")):
        bad(gpu.user_raw(U, Y, 10, 0, it, 64)[0], f"inv_temp {it}")
        bad(gpu.item_raw(Y, U, 0, 10, it, 64, lse)[0], f"inv_temp {it}")
    for d in (24, 272):
        assert gpu.user_raw(U, Y, 10, 0, 1.0, 64, d=d)[0] == 3
        assert gpu.item_raw(Y, U, 0, 10, 1.0, 64, lse, d=d)[0] == 3
        assert str(d) in gpu.last_error()
    # null outputs
    lib, t = gpu.lib, gpu.t
    Ud, Yd, o = gpu.up(U), gpu.up(Y), gpu.nan(64 * 32)
    assert lib.rihip_inbatch_softmax_user_sweep(Ud.data_ptr(), 33, 10, Yd.data_ptr(), 64, 0, 32, 1.0, None, None, None, 64,
                                                None, o.data_ptr(), o.data_ptr(), gpu.st) == 1
    assert lib.rihip_inbatch_softmax_item_sweep(Yd.data_ptr(), 64, 0, Ud.data_ptr(), 33, 10, 32, 1.0, None, None, None,
                                                o.data_ptr(), 64, None, gpu.st) == 1
    t.cuda.synchronize()
    assert np.isnan(o.cpu().numpy()).all()         # a rejected call launches nothing


def test_two_calls_are_bitwise_equal(gpu):
    cs = R.make_case(8, 130, 517, 200, 0, 144)
    a = [gpu.user(cs["users"], cs["items"], 200, 0, 20.0, 717, cs["logq"], cs["user_pos_ids"], cs["item_ids"])
         for _ in range(2)]
    for k in a[0]:
        assert np.array_equal(a[0][k], a[1][k]), k
    b = [gpu.item(cs["items"], cs["users"], 0, 200, 20.0, 717, a[0]["lse"], cs["logq"], cs["item_ids"], cs["user_pos_ids"])
         for _ in range(2)]
    assert np.array_equal(b[0], b[1])


# ---------------------------------------------------------------------------------------------------------------------
# 7. Python surface
# ---------------------------------------------------------------------------------------------------------------------
def _square_case(B=96, d=32, seed=4):
    cs = R.make_case(seed, B, B, 0, 0, d)
    cs["user_pos_ids"] = cs["item_ids"]          # square form: the user's positive is its own row's item
    return cs


def test_model_loss_forward_backward(gpu):
    import torch
    from recommendit_amd import TwoTowerModel
    B, d, temp = 96, 32, 0.05
    cs = _square_case(B, d)
    inv_temp = float(np.float32(1.0 / temp))
    ref = _ref(cs, inv_temp, B)
    assert ref["dropped"].any()
    bnd = R.bounds(ref, cs["users"], cs["items"], d, inv_temp)
    m = TwoTowerModel(10, 10, embed_dim=d, hidden_dim=64)
    U = torch.from_numpy(cs["users"]).cuda().requires_grad_(True)
    Y = torch.from_numpy(cs["items"]).cuda().requires_grad_(True)
    loss = m.in_batch_softmax_loss(U, Y, temperature=temp, logq=torch.from_numpy(cs["logq"]),
                                   item_ids=torch.from_numpy(cs["item_ids"]))
    loss.backward()
    lb = bnd["loss_part"].sum() / B + abs(ref["loss"]) * 2.0 ** -23
    assert abs(float(loss) - ref["loss"]) <= lb, (float(loss), ref["loss"], lb)
    assert R.worst_ratio(U.grad.cpu().numpy(), ref["dU"], bnd["dU"]) <= 1.0
    lse32 = ref["lse"].astype(np.float32)
    # dI is formed against the device's own f32 lse: the reference's, one f32 rounding of |lse| apart at most
    ref_i = _ref(cs, inv_temp, B, lse_in=lse32)
    bi = R.bounds(ref_i, cs["users"], cs["items"], d, inv_temp)["dI"] + (bnd["lse"].max() + 2.0 ** -23 * np.abs(lse32).max()) \
        * ref_i["M_dI"]
    assert R.worst_ratio(Y.grad.cpu().numpy(), ref_i["dI"], bi) <= 1.0
    with pytest.raises(ValueError):
        m.in_batch_softmax_loss(U, Y, temperature=0.0)


def test_model_loss_under_graph_capture(gpu):
    import torch
    from recommendit_amd.two_tower import softmax_loss_and_grads
    cs = _square_case(130, 48, seed=6)
    U, Y = gpu.up(cs["users"]), gpu.up(cs["items"])
    lq, ids = gpu.up(cs["logq"]), gpu.up(cs["item_ids"])
    eager = [x.clone() for x in softmax_loss_and_grads(U, Y, 20.0, lq, ids)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            outs = softmax_loss_and_grads(U, Y, 20.0, lq, ids)
    for o in outs:
        o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 8. trainer
# ---------------------------------------------------------------------------------------------------------------------
def _trainer(mode, B=96, d=32, H=64, nu=256, ni=300, **kw):
    import torch
    from oracle import fixtures as fx
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    sd = fx.make_state(nu, ni, d, H, 7)
    m = TwoTowerModel(nu, ni, embed_dim=d, hidden_dim=H, dropout=0.0)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m.train()
    return HipBPRTrainer(m, B, lr=1e-2, weight_decay=1e-5, loss_mode=mode, table_opt="dense", seed=3, **kw)


def _batch(B, nu=256, ni=300, seed=11):
    from oracle import fixtures as fx
    import torch
    u, p, gp, n, gn = fx.make_batch(nu, ni, B, seed=seed, boundary=False)
    c = lambda x: torch.from_numpy(np.asarray(x)).cuda()
    return c(u), c(p), c(gp), c(n), c(gn)


def test_trainer_step_equals_direct_calls(gpu):
    import torch
    B, d, ni = 96, 32, 300
    logq = torch.from_numpy(R.zipf_logq(np.random.RandomState(2), ni + 1))
    tr = _trainer("softmax", temperature=0.05, item_logq=logq, mask_duplicates=True)
    u, p, gp, _, _ = _batch(B)
    assert len(np.unique(p.cpu().numpy())) < B          # the batch has duplicate items: the mask is in play
    loss = tr.step(u, p, gp)
    torch.cuda.synchronize()
    lq = logq.cuda()[p]
    Un, Yn = tr.U.cpu().numpy(), tr.I.cpu().numpy()
    ids = p.cpu().numpy()
    inv_temp = float(np.float32(tr.inv_temp))
    got = gpu.user(Un, Yn, 0, 0, tr.inv_temp, B, lq.cpu().numpy(), ids, ids)
    dI = gpu.item(Yn, Un, 0, 0, tr.inv_temp, B, got["lse"], lq.cpu().numpy(), ids, ids)
    assert np.array_equal(tr.dU.cpu().numpy(), got["dU"]) and np.array_equal(tr.dI.cpu().numpy(), dI)
    out = gpu.nan(1)
    part = gpu.up(got["loss_part"])
    gpu.L.check(gpu.lib.rihip_sum_partials(part.data_ptr(), 1, 1.0 / B, out.data_ptr(), gpu.st))
    assert float(loss) == float(out[0])
    # ... and the direct call is the reference's
    cs = dict(users=Un, items=Yn, user_goff=0, item_goff=0, logq=lq.cpu().numpy(), user_pos_ids=ids, item_ids=ids)
    ref = _ref(cs, inv_temp, B)
    bnd = R.bounds(ref, Un, Yn, d, inv_temp)
    assert R.worst_ratio(got["dU"], ref["dU"], bnd["dU"]) <= 1.0


def test_trainer_other_modes_are_unchanged(gpu):
    """'inbatch' and 'sampled' of the same class against the existing public calls on the trainer's own tower outputs"""
    import torch
    from recommendit_amd.two_tower import inbatch_loss_and_grads
    B, d = 96, 32
    u, p, gp, n, gn = _batch(B)
    tr = _trainer("inbatch")
    loss = tr.step(u, p, gp)
    torch.cuda.synchronize()
    l2, dU, dI = inbatch_loss_and_grads(tr.U, tr.I, store_g=tr.inbatch_store_g)
    assert torch.equal(tr.dU, dU) and torch.equal(tr.dI, dI) and float(loss) == float(l2)
    tr = _trainer("sampled")
    loss = tr.step(u, torch.cat([p, n]), torch.cat([gp, gn]))
    torch.cuda.synchronize()
    l3 = gpu.nan(1)
    g = [gpu.nan(B, d) for _ in range(3)]
    ws = gpu.t.zeros(1024, dtype=torch.float64, device=gpu.dev)
    gpu.L.check(gpu.lib.rihip_bpr_pair_loss(tr.U.data_ptr(), tr.I.data_ptr(), tr.I[B:].data_ptr(), B, d, l3.data_ptr(),
                                            g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), ws.data_ptr(), gpu.st))
    torch.cuda.synchronize()
    assert torch.equal(tr.dU, g[0]) and torch.equal(tr.dI[:B], g[1]) and torch.equal(tr.dI[B:], g[2])
    assert float(loss) == float(l3[0])


def test_twenty_steps_lower_the_loss(gpu):
    import torch
    B, nu, ni = 96, 256, 300
    rng = np.random.RandomState(0)
    pos_of_user = rng.randint(1, ni + 1, size=nu + 1)            # one liked item per user: a learnable set of 256 pairs
    cnt = np.bincount(pos_of_user[1:], minlength=ni + 1).astype(np.float64)
    prob = np.where(cnt > 0, cnt, cnt[cnt > 0].min()) / cnt.sum()
    tr = _trainer("softmax", temperature=0.05, item_logq=torch.from_numpy(np.log(prob).astype(np.float32)))
    genres = torch.from_numpy((rng.rand(ni + 1, 18) < 0.2).astype(np.float32)).cuda()
    losses = []
    for step in range(20):
        u = rng.randint(1, nu + 1, size=B)
        p = torch.from_numpy(pos_of_user[u]).cuda()
        losses.append(tr.step(torch.from_numpy(u).cuda(), p, genres[p]).clone())    # step() returns its own loss buffer
    losses = [float(x) for x in losses]
    tr.check_errors()
    print("softmax loss, 20 steps:", [round(x, 3) for x in losses])
    assert np.isfinite(losses).all() and np.mean(losses[-3:]) < np.mean(losses[:3]) - 0.1, losses


def test_distributed_softmax_raises():
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    m = TwoTowerModel(20, 20, embed_dim=32, hidden_dim=64)
    with pytest.raises(ValueError, match="softmax"):
        HipBPRTrainer(m, 8, loss_mode="softmax", table_opt="sparse", distributed=True)
    with pytest.raises(ValueError, match="temperature"):
        HipBPRTrainer(m, 8, loss_mode="softmax", temperature=0.0)
