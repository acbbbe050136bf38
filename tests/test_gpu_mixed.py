"""The mixed in-batch objective (csrc/loss_mixed.hip) against tests/mixed_reference.py: the mining pass bit for bit on
weights the test writes, the apply pass given a selection (gmat bit for bit, the sums inside derived bounds), the whole
chain against the definition L_inbatch + hard_weight L_hard with the selection by f64 score, then the model method and
the trainer mode.  Nothing in the bounds comes from a device run.  Ratios are printed per case (run with -s)."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import inbatch_reference as IB  # noqa: E402
import mixed_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 3        # rows past the end of every output that must keep their prefill
IFILL = -77      # prefill of neg_idx


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
    def _cut(t, n, what, fill=None):
        a = t.cpu().numpy()
        rest = a[n:]
        assert (np.isnan(rest) if fill is None else rest == fill).all(), f"{what}: written outside [0, {n})"
        return a[:n]

    def mine_dev(self, gm, nu, ug, ni, m, skip, upos=None, iids=None, nsplit=0):
        """gm: device tensor.  Returns (rc, neg_idx, neg_w) as device tensors with guard rows."""
        P = self.L.ptr
        nb = self.lib.rihip_inbatch_gmat_mine_workspace_bytes(nu, ni, m, skip, nsplit)
        assert nb > 0, (nu, ni, m, skip, nsplit)
        ws = self.t.full((nb + 64,), 0xAB, dtype=self.t.uint8, device=self.dev)
        idx = self.t.full((nu + GUARD, m), IFILL, dtype=self.t.int32, device=self.dev)
        w = self.nan(nu + GUARD, m)
        rc = self.lib.rihip_inbatch_gmat_mine(gm.data_ptr(), nu, ug, ni, 0, m, skip, P(upos), P(iids), nsplit,
                                              idx.data_ptr(), w.data_ptr(), ws.data_ptr(), self.st)
        self.t.cuda.synchronize()
        assert (ws[nb:] == 0xAB).all(), "workspace written past its size"
        return rc, idx, w

    def mine(self, gmat, nu, ug, ni, m, skip, upos=None, iids=None, nsplit=0):
        rc, idx, w = self.mine_dev(self.up(gmat), nu, ug, ni, m, skip, self.up(upos), self.up(iids), nsplit)
        self.L.check(rc, "inbatch_gmat_mine")
        return dict(neg_idx=self._cut(idx, nu, "neg_idx", IFILL), neg_w=self._cut(w, nu, "neg_w"))

    def apply(self, gmat, users, items, ug, pos, m, neg_idx, neg_w, hw, n_global, dU_in, r_in):
        nu, ni, d = users.shape[0], items.shape[0], users.shape[1]
        gm, U, Y, ps = self.up(gmat), self.up(users), self.up(items), self.up(pos)
        ix, nw = self.up(np.asarray(neg_idx, np.int32)), self.up(np.asarray(neg_w, np.float32))
        dU, r = self.nan(nu + GUARD, d), self.nan(nu + GUARD)
        dU[:nu] = self.up(dU_in)
        r[:nu] = self.up(r_in)
        npart = self.lib.rihip_inbatch_mixed_loss_parts(nu)
        assert npart == R.cdiv(nu, R.OWN)
        part = self.nan(npart + GUARD, dtype=self.t.float64)
        self.L.check(self.lib.rihip_inbatch_mixed_apply(gm.data_ptr(), U.data_ptr(), nu, ug, Y.data_ptr(), ni, 0, d,
                                                        ps.data_ptr(), m, ix.data_ptr(), nw.data_ptr(), float(hw), n_global,
                                                        dU.data_ptr(), r.data_ptr(), part.data_ptr(), self.st),
                     "inbatch_mixed_apply")
        self.t.cuda.synchronize()
        return dict(gmat=gm.cpu().numpy(), dU=self._cut(dU, nu, "dU"), r=self._cut(r, nu, "r"),
                    loss_part=self._cut(part, npart, "loss_part"))

    def chain(self, users, items, ug, hw, m, skip, upos, iids, precision):
        """rowdot, user pass, mine, apply, item pass, the sum of both part arrays: the rectangular form of
        mixed_loss_and_grads, n_global = n_items"""
        t, lib, st, P = self.t, self.lib, self.st, self.L.ptr
        nu, ni, d = users.shape[0], items.shape[0], users.shape[1]
        U, Y, up_, ii = self.up(users), self.up(items), self.up(upos), self.up(iids)
        f32 = dict(dtype=t.float32, device=self.dev)
        pos, r = t.empty((nu,), **f32), t.empty((nu,), **f32)
        dU, dI = t.empty((nu, d), **f32), t.empty((ni, d), **f32)
        n_in, n_mx = lib.rihip_inbatch_loss_parts(nu, ni), lib.rihip_inbatch_mixed_loss_parts(nu)
        part = t.zeros((max(lib.rihip_inbatch_workspace_doubles(nu), n_in) + n_mx,), dtype=t.float64, device=self.dev)
        ws = t.empty((max(lib.rihip_inbatch_workspace_floats(nu, ni, d), lib.rihip_inbatch_workspace_floats(ni, nu, d)),), **f32)
        gm = self.nan(lib.rihip_inbatch_gmat_floats(nu, ni))
        idx, nw = t.empty((nu, m), dtype=t.int32, device=self.dev), t.empty((nu, m), **f32)
        mws = t.empty((lib.rihip_inbatch_gmat_mine_workspace_bytes(nu, ni, m, skip, 0),), dtype=t.uint8, device=self.dev)
        loss = t.empty((), **f32)
        ck = self.L.check
        ck(lib.rihip_rowdot(U.data_ptr(), Y.data_ptr(), nu, ug, d, pos.data_ptr(), st), "rowdot")
        ck(lib.rihip_inbatch_user_pass(U.data_ptr(), nu, ug, Y.data_ptr(), ni, 0, d, pos.data_ptr(), ni, dU.data_ptr(),
                                       r.data_ptr(), part.data_ptr(), ws.data_ptr(), gm.data_ptr(), precision, st), "user_pass")
        ck(lib.rihip_inbatch_gmat_mine(gm.data_ptr(), nu, ug, ni, 0, m, skip, P(up_), P(ii), 0, idx.data_ptr(),
                                       nw.data_ptr(), mws.data_ptr(), st), "mine")
        ck(lib.rihip_inbatch_mixed_apply(gm.data_ptr(), U.data_ptr(), nu, ug, Y.data_ptr(), ni, 0, d, pos.data_ptr(), m,
                                         idx.data_ptr(), nw.data_ptr(), float(hw), ni, dU.data_ptr(), r.data_ptr(),
                                         part[n_in:].data_ptr(), st), "apply")
        ck(lib.rihip_inbatch_item_pass(gm.data_ptr(), U.data_ptr(), nu, ug, ni, 0, d, r.data_ptr(), ni, dI.data_ptr(),
                                       ws.data_ptr(), precision, st), "item_pass")
        ck(lib.rihip_sum_partials(part.data_ptr(), n_in + n_mx, 1.0 / (ni * (ni - 1.0)), loss.data_ptr(), st), "sum")
        t.cuda.synchronize()
        return dict(loss=float(loss), dU=dU.cpu().numpy(), dI=dI.cpu().numpy(), neg_idx=idx.cpu().numpy(), U=U, Y=Y,
                    upos=up_, iids=ii)

    def hard_select(self, U, Y, nu, ug, ni, m, skip, upos, iids):
        t, P = self.t, self.L.ptr
        idx = t.empty((nu, m), dtype=t.int32, device=self.dev)
        sc, ps = t.empty((nu, m), dtype=t.float32, device=self.dev), t.empty((nu,), dtype=t.float32, device=self.dev)
        self.L.check(self.lib.rihip_inbatch_hard_select(U.data_ptr(), nu, ug, Y.data_ptr(), ni, 0, U.shape[1], m, skip,
                                                        P(upos), P(iids), idx.data_ptr(), sc.data_ptr(), ps.data_ptr(),
                                                        self.st), "hard_select")
        t.cuda.synchronize()
        return idx.cpu().numpy()

    def last_error(self):
        return self.lib.rihip_last_error().decode()


@pytest.fixture(scope="module")
def gpu():
    return Dev()


# ---------------------------------------------------------------------------------------------------------------------
# 1. mining alone, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms", R.M_SKIP, ids=lambda x: f"m{x[0]}s{x[1]}")
@pytest.mark.parametrize("shape", R.MINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mining_bit_for_bit(gpu, shape, ms):
    nu, ni, ug = shape
    (m, skip), mx = ms, R.max_nsplit(ni)
    assert gpu.lib.rihip_inbatch_gmat_mine_max_nsplit(ni) == mx
    ties = 0
    for kind in ("random", "ternary"):
        w = R.make_weights(kind, 50 + nu + m, nu, ni, ug)
        flat = gpu.up(R.blocked_gmat(w, nu, ni))                  # NaN wherever the pass may not read
        for mode in ("none", "dups", "below", "between"):
            upos, iids = R.make_mine_ids(mode, 60 + ni + skip, nu, ni, ug, m, skip)
            exp = R.mine(w, ug, 0, m, skip, upos, iids)
            up_, ii = gpu.up(upos), gpu.up(iids)
            first = None
            for nsplit in sorted({0, 1, min(3, mx), mx}):
                rc, idx, nw = gpu.mine_dev(flat, nu, ug, ni, m, skip, up_, ii, nsplit)
                gpu.L.check(rc, "inbatch_gmat_mine")
                got_i, got_w = gpu._cut(idx, nu, "neg_idx", IFILL), gpu._cut(nw, nu, "neg_w")
                tag = (shape, ms, kind, mode, nsplit)
                IB.check_equal(f"neg_idx {tag}", got_i, exp["neg_idx"])
                IB.check_equal(f"neg_w {tag}", got_w.view(np.uint32), exp["neg_w"].view(np.uint32))
                if first is None:                                  # two calls are bitwise equal
                    rc, idx2, nw2 = gpu.mine_dev(flat, nu, ug, ni, m, skip, up_, ii, nsplit)
                    assert gpu.t.equal(idx, idx2) and gpu.t.equal(nw.view(gpu.t.int32), nw2.view(gpu.t.int32))
                    first = True
            if kind == "ternary":
                ties += int((exp["neg_w"][:, 1:] == exp["neg_w"][:, :-1]).sum())
    if m > 1 and nu >= 31:
        assert ties > 0                                            # the index order decided ranks


def test_mining_leaves_gmat_alone_and_reads_only_used_blocks(gpu):
    nu, ni, ug = 130, 517, 200
    w = R.make_weights("random", 1, nu, ni, ug)
    host = R.blocked_gmat(w, nu, ni)
    flat = gpu.up(host)
    rc, idx, nw = gpu.mine_dev(flat, nu, ug, ni, 8, 0)
    assert rc == 0
    assert np.array_equal(flat.cpu().numpy().view(np.uint32), host.view(np.uint32))
    assert np.isnan(host).any() and not np.isnan(nw[:nu].cpu().numpy()).any()


def test_mining_argument_errors(gpu):
    nu, ni = 40, 70
    flat = gpu.up(R.blocked_gmat(R.make_weights("random", 1, nu, ni, 0), nu, ni))
    ids = gpu.up(np.arange(ni, dtype=np.int64))
    t = gpu.t
    idx, nw = t.empty((nu, 32), dtype=t.int32, device=gpu.dev), t.empty((nu, 32), dtype=t.float32, device=gpu.dev)
    ws = t.empty((1 << 20,), dtype=t.uint8, device=gpu.dev)

    def call(nu_=nu, ug=0, ni_=ni, m=8, skip=0, up_=None, ii=None, nsplit=0):
        P = gpu.L.ptr
        return gpu.lib.rihip_inbatch_gmat_mine(flat.data_ptr(), nu_, ug, ni_, 0, m, skip, P(up_), P(ii), nsplit,
                                               idx.data_ptr(), nw.data_ptr(), ws.data_ptr(), gpu.st)
    assert call() == 0
    for kw, word in ((dict(m=0), "m=0"), (dict(m=33), "m=33"), (dict(skip=-1), "skip=-1"), (dict(m=32, skip=33), "skip=33"),
                     (dict(ug=31), "partners outside"), (dict(nu_=0), "sizes"), (dict(up_=ids), "together"),
                     (dict(nsplit=-1), "nsplit"), (dict(nsplit=R.max_nsplit(ni) + 1), "nsplit")):
        assert call(**kw) != 0, kw
        assert word in gpu.last_error(), (kw, gpu.last_error())
    assert gpu.lib.rihip_inbatch_gmat_mine_workspace_bytes(nu, ni, 8, 0, R.max_nsplit(ni) + 1) == -1
    assert gpu.lib.rihip_inbatch_gmat_mine_workspace_bytes(nu, ni, 33, 0, 0) == -1
    t.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 2. apply alone, given selection and gmat
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.HARD_WEIGHTS)
@pytest.mark.parametrize("shape", R.APPLY_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("d", (32, 64, 128))
def test_apply_against_reference(gpu, d, shape, hw):
    nu, ni, ug = shape
    for m, skip in ((8, 0), (8, 3)):
        cs = R.make_apply_case(7, shape, d, m, skip)
        neg_idx, neg_w = cs["neg_idx"].copy(), cs["neg_w"].copy()
        neg_idx[1, :], neg_w[1, :] = -1, 0                                    # a row without negatives: c_i = 0
        neg_idx[2, m // 2:], neg_w[2, m // 2:] = -1, 0                        # a partly filled row
        host = R.blocked_gmat(cs["weights"], nu, ni)
        got = gpu.apply(host, cs["users"], cs["items"], ug, cs["pos"], m, neg_idx, neg_w, hw, cs["n_global"],
                        cs["dU_in"], cs["r_in"])
        ref = R.apply_reference(cs["weights"], cs["users"], cs["items"], cs["pos"], ug, 0, m, neg_idx, neg_w, hw,
                                cs["n_global"], cs["dU_in"], cs["r_in"])
        exp_flat = R.blocked_gmat(ref["weights"], nu, ni)
        IB.check_equal("gmat", got["gmat"].view(np.uint32), exp_flat.view(np.uint32))   # boosted entries and nothing else
        if hw == 0:
            IB.check_equal("r", got["r"].view(np.uint32), cs["r_in"].view(np.uint32))
            IB.check_equal("dU", got["dU"].view(np.uint32), cs["dU_in"].view(np.uint32))
            assert (got["loss_part"] == 0).all()
            continue
        assert (ref["weights"] != cs["weights"]).sum() == ref["ok"][ref["live"]].sum()
        bnd = R.apply_bounds(ref)
        ratios = {k: R.worst_ratio(got[k], ref[k], bnd[k]) for k in ("r", "dU", "loss_part")}
        print(f"apply d={d} shape={shape} m={m} skip={skip} hw={hw}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
        assert max(ratios.values()) <= 1.0, ratios
        # rows without negatives keep their inputs bit for bit
        assert got["r"][1] == cs["r_in"][1] and np.array_equal(got["dU"][1], cs["dU_in"][1])


def test_apply_argument_errors_and_out_of_range_slots(gpu):
    cs = R.make_apply_case(7, (33, 97, 30), 32, 8, 0)
    nu, ni, ug = 33, 97, 30
    host = R.blocked_gmat(cs["weights"], nu, ni)
    bad = cs["neg_idx"].copy()
    bad[0, 0], bad[0, 1] = ni, -5                                             # outside [0, n_items): empty slots
    got = gpu.apply(host, cs["users"], cs["items"], ug, cs["pos"], 8, bad, cs["neg_w"], 0.5, ni, cs["dU_in"], cs["r_in"])
    ref = R.apply_reference(cs["weights"], cs["users"], cs["items"], cs["pos"], ug, 0, 8, bad, cs["neg_w"], 0.5, ni,
                            cs["dU_in"], cs["r_in"])
    assert ref["c"][0] == 6
    IB.check_equal("gmat", got["gmat"].view(np.uint32), R.blocked_gmat(ref["weights"], nu, ni).view(np.uint32))
    assert R.worst_ratio(got["dU"], ref["dU"], R.apply_bounds(ref)["dU"]) <= 1.0
    for kw, word in ((dict(hw=-1.0), "hard_weight"), (dict(hw=float("nan")), "hard_weight"), (dict(n=1), "B=1")):
        with pytest.raises(RuntimeError, match=word):
            gpu.apply(host, cs["users"], cs["items"], ug, cs["pos"], 8, cs["neg_idx"], cs["neg_w"], kw.get("hw", 0.5),
                      kw.get("n", ni), cs["dU_in"], cs["r_in"])
    with pytest.raises(RuntimeError, match="embed_dim=48"):
        gpu.apply(host, np.zeros((nu, 48), np.float32), np.zeros((ni, 48), np.float32), ug, cs["pos"], 8, cs["neg_idx"],
                  cs["neg_w"], 0.5, ni, np.zeros((nu, 48), np.float32), cs["r_in"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the chain against the definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("d,precision", R.CHAIN_CASES)
def test_chain_against_definition(gpu, d, precision, shape):
    nu, ni, ug = shape
    m, skip = R.chain_m_skip(d, precision)
    hw = 0.5
    users, items, upos, iids = R.make_chain_case(R.CHAIN_SEED, shape, d)
    got = gpu.chain(users, items, ug, hw, m, skip, upos, iids, precision)
    cr = R.chain_reference(users, items, ug, hw, m, skip, upos, iids, precision, device_neg_idx=got["neg_idx"])
    ent = cr["entered"]
    assert 1.0 - ent.mean() <= 0.10, "more than a tenth of the rows left out of the selection comparison"
    IB.check_equal("neg_idx (rows that entered)", got["neg_idx"][ent], cr["ref_neg_idx"][ent])
    hs = gpu.hard_select(got["U"], got["Y"], nu, ug, ni, m, skip, got["upos"], got["iids"])
    IB.check_equal("neg_idx against rihip_inbatch_hard_select", got["neg_idx"][ent], hs[ent])
    bnd = R.chain_bounds(cr)
    ratios = dict(dU=R.worst_ratio(got["dU"], cr["dU"], bnd["dU"]), dI=R.worst_ratio(got["dI"], cr["dI"], bnd["dI"]),
                  loss=abs(got["loss"] - cr["loss"]) / bnd["loss"])
    print(f"chain d={d} p={precision} shape={shape} m={m} skip={skip}: left out {100 * (1 - ent.mean()):.1f} % "
          + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    if nu == ni:                                                   # the square form is mixed_loss_and_grads itself
        from recommendit_amd.two_tower import mixed_loss_and_grads
        loss, dU, dI, idx = mixed_loss_and_grads(got["U"], got["Y"], hw, m, skip, got["iids"], precision)
        assert float(loss) == got["loss"] and np.array_equal(idx.cpu().numpy(), got["neg_idx"])
        assert np.array_equal(dU.cpu().numpy(), got["dU"]) and np.array_equal(dI.cpu().numpy(), got["dI"])


@pytest.mark.parametrize("d", (32, 128))
def test_all_negatives_scale_the_in_batch_gradients(gpu, d):
    """m = B - 1, skip = 0, no ids: every other row is selected, so the mixed gradients are (1 + hard_weight) times the
    in-batch ones, within the chain's bounds"""
    B, hw = 33, 0.5
    users, items, _, _ = R.make_chain_case(3, (B, B, 0), d)
    got = gpu.chain(users, items, 0, hw, B - 1, 0, None, None, 0)
    assert (np.sort(got["neg_idx"], axis=1) == np.array([[j for j in range(B) if j != i] for i in range(B)])).all()
    cr = R.chain_reference(users, items, 0, hw, B - 1, 0, None, None, 0, device_neg_idx=got["neg_idx"])
    bnd = R.chain_bounds(cr)
    f = 1.0 + float(np.float32(hw))
    assert np.allclose(cr["dU"], f * cr["inb"]["dU"], rtol=0, atol=1e-14)       # the reference's own algebra
    assert R.worst_ratio(got["dU"], f * cr["inb"]["dU"], bnd["dU"]) <= 1.0
    assert R.worst_ratio(got["dI"], f * cr["inb"]["dI"], bnd["dI"]) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. model and trainer
# ---------------------------------------------------------------------------------------------------------------------
def test_model_loss_backward_gives_the_closed_form_gradients(gpu):
    import torch
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.two_tower import mixed_loss_and_grads
    B, d = 96, 64
    users, items, _, iids = R.make_chain_case(5, (B, B, 0), d)
    model = TwoTowerModel(10, 10, embed_dim=d, hidden_dim=64)
    U = torch.from_numpy(users).cuda().requires_grad_(True)
    Y = torch.from_numpy(items).cuda().requires_grad_(True)
    ids = torch.from_numpy(iids)
    loss = model.in_batch_mixed_loss(U, Y, hard_weight=0.5, n_hard=8, skip=1, item_ids=ids)
    loss.backward()
    l2, dU, dI, _ = mixed_loss_and_grads(U.detach(), Y.detach(), 0.5, 8, 1, ids)
    assert loss.item() == l2.item() and torch.equal(U.grad, dU) and torch.equal(Y.grad, dI)
    one = model.in_batch_mixed_loss(U[:1].detach().requires_grad_(True), Y[:1].detach())
    assert torch.isnan(one)                                         # B < 2: nan, as in_batch_bpr_loss
    fallback = "in_batch_bpr_loss \\+ hard_weight \\* in_batch_hard_bpr_loss"
    with pytest.raises(ValueError, match=fallback):
        model.in_batch_mixed_loss(torch.zeros((8, 48)).cuda(), torch.zeros((8, 48)).cuda())
    with pytest.raises(ValueError, match=fallback):
        mixed_loss_and_grads(U.detach(), Y.detach(), 0.5, 8, precision=1)
    big = torch.zeros((32769, 32), device="cuda")                  # 4.03 GiB of stored weights
    with pytest.raises(ValueError, match="4 GiB.*" + fallback):
        mixed_loss_and_grads(big, big, 0.5, 8)
    for kw in (dict(hard_weight=-1.0), dict(hard_weight=float("inf")), dict(n_hard=0), dict(n_hard=32, skip=33)):
        with pytest.raises(ValueError):
            model.in_batch_mixed_loss(U, Y, **kw)


def _trainer(mode, B=256, d=64, H=64, nu=512, ni=600, **kw):
    import torch
    from oracle import fixtures as fx
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    sd = fx.make_state(nu, ni, d, H, 7)
    m = TwoTowerModel(nu, ni, embed_dim=d, hidden_dim=H, dropout=0.0)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m.train()
    kw.setdefault("table_opt", "dense")
    return HipBPRTrainer(m, B, lr=1e-2, weight_decay=1e-5, loss_mode=mode, seed=3, **kw)


def _batch(B, nu=512, ni=600, seed=11):
    from oracle import fixtures as fx
    import torch
    u, p, gp, n, gn = fx.make_batch(nu, ni, B, seed=seed, boundary=False)
    c = lambda x: torch.from_numpy(np.asarray(x)).cuda()
    return c(u), c(p), c(gp)


@pytest.mark.parametrize("table_opt", ["dense", "sparse"])
def test_trainer_weight_zero_is_the_inbatch_mode_bit_for_bit(gpu, table_opt):
    import torch
    B = 256
    runs = []
    for mode, kw in (("inbatch", {}), ("mixed", dict(hard_weight=0.0, n_hard=8))):
        tr = _trainer(mode, table_opt=table_opt, **kw)
        losses = []
        for step in range(3):
            u, p, gp = _batch(B, seed=step * 13)
            losses.append(tr.step(u, p, gp).item())
        tr.check_errors()
        runs.append((losses, {k: v.detach().clone() for k, v in tr.model.named_parameters()}))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


@pytest.mark.parametrize("mask", [True, False])
def test_trainer_step_equals_mixed_loss_and_grads(gpu, mask):
    import torch
    from recommendit_amd.two_tower import mixed_loss_and_grads
    B = 256
    tr = _trainer("mixed", hard_weight=0.5, n_hard=8, hard_skip=1, mask_duplicates=mask)
    u, p, gp = _batch(B)
    assert len(np.unique(p.cpu().numpy())) < B          # the batch has duplicate items: the mask is in play
    loss = tr.step(u, p, gp).clone()
    torch.cuda.synchronize()
    l2, dU, dI, idx = mixed_loss_and_grads(tr.U, tr.I, 0.5, 8, 1, p if mask else None)
    assert torch.equal(tr.dU, dU) and torch.equal(tr.dI, dI) and torch.equal(tr.neg_idx, idx)
    assert float(loss) == float(l2)
    tr.check_errors()


def test_trainer_graph_replay_equals_eager(gpu):
    import torch
    B = 256
    outs = []
    for use_graph in (False, True):
        tr = _trainer("mixed", hard_weight=0.5, n_hard=8, table_opt="sparse", use_graph=use_graph)
        losses = []
        for step in range(4):
            u, p, gp = _batch(B, seed=step * 13)
            losses.append(tr.step(u, p, gp).item())
        assert (tr._graph is not None) == use_graph
        tr.check_errors()
        outs.append((losses, {k: v.detach().clone() for k, v in tr.model.named_parameters()}))
    assert outs[0][0] == outs[1][0]
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


def test_twenty_steps_are_finite_and_differ_from_weight_zero(gpu):
    import torch
    B, nu, ni = 256, 512, 600
    final = []
    for hw in (0.0, 0.5):
        rng = np.random.RandomState(0)
        pos_of_user = rng.randint(1, ni + 1, size=nu + 1)
        genres = torch.from_numpy((rng.rand(ni + 1, 18) < 0.2).astype(np.float32)).cuda()
        tr = _trainer("mixed", hard_weight=hw, n_hard=8)
        losses = []
        for step in range(20):
            u = rng.randint(1, nu + 1, size=B)
            p = torch.from_numpy(pos_of_user[u]).cuda()
            losses.append(tr.step(torch.from_numpy(u).cuda(), p, genres[p]).clone())
        losses = [float(x) for x in losses]
        tr.check_errors()
        print(f"mixed loss at hard_weight={hw}, 20 steps:", [round(x, 3) for x in losses])
        assert np.isfinite(losses).all(), losses
        final.append((losses, tr.model.user_tower.embedding.weight.detach().clone()))
    assert final[0][0] != final[1][0] and not torch.equal(final[0][1], final[1][1])


def test_trainer_argument_errors():
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    m = TwoTowerModel(20, 20, embed_dim=32, hidden_dim=64)
    for kw, word in ((dict(hard_weight=-0.5), "hard_weight"), (dict(hard_weight=float("nan")), "hard_weight"),
                     (dict(distributed=True, table_opt="sparse"), "single-GPU"), (dict(inbatch_precision=1), "stored-G"),
                     (dict(inbatch_store_g=False), "stored-G"), (dict(n_hard=0), "n_hard")):
        with pytest.raises(ValueError, match=word):
            HipBPRTrainer(m, 8, loss_mode="mixed", **kw)
    with pytest.raises(ValueError, match="stored-G"):
        HipBPRTrainer(TwoTowerModel(20, 20, embed_dim=48, hidden_dim=64), 8, loss_mode="mixed")


@pytest.mark.parametrize("store_g", [None, True])
def test_trainer_raises_when_the_stored_weights_do_not_fit(monkeypatch, store_g):
    """batch 1 024: 4 MiB of stored weights.  None takes the stored-G form only inside half of the free memory, True
    inside all of it; with 3 MiB reported free both must raise before anything is allocated for the weights."""
    import torch
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    m = TwoTowerModel(20, 20, embed_dim=32, hidden_dim=64)
    real = torch.cuda.mem_get_info
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (3 << 20, real(*a, **k)[1]))
    with pytest.raises(ValueError, match="stored weights.*free"):
        HipBPRTrainer(m, 1024, loss_mode="mixed", table_opt="sparse", inbatch_store_g=store_g)
    monkeypatch.setattr(torch.cuda, "mem_get_info", real)
    assert HipBPRTrainer(m, 1024, loss_mode="mixed", table_opt="sparse", inbatch_store_g=store_g).gmat is not None
