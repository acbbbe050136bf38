"""The in-batch hard-negative entries (csrc/loss_hard.hip) against the f64 reference of tests/hard_reference.py.  The
selection is compared bit for bit on inputs whose scores are exact in f32; the gradient entry is fed the reference's own
selection and must stay inside the bounds derived there (BOUNDS_DOC; nothing in them comes from a device run).  Every
output buffer is prefilled and carries guard rows that must keep the prefill.  Ratios are printed per case (run with -s)."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import hard_reference as R  # noqa: E402

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

    def select_raw(self, users, items, ug, ig, m, skip, upos=None, iids=None, d=None):
        nu, ni = users.shape[0], items.shape[0]
        d = users.shape[1] if d is None else d
        P = self.L.ptr
        U, Y, up_, ii = (self.up(x) for x in (users, items, upos, iids))
        mm = max(m, 1)
        out = dict(neg_idx=self.t.full((nu + GUARD, mm), IFILL, dtype=self.t.int32, device=self.dev),
                   neg_score=self.nan(nu + GUARD, mm), pos_score=self.nan(nu + GUARD))
        rc = self.lib.rihip_inbatch_hard_select(U.data_ptr(), nu, ug, Y.data_ptr(), ni, ig, d, m, skip, P(up_), P(ii),
                                                out["neg_idx"].data_ptr(), out["neg_score"].data_ptr(),
                                                out["pos_score"].data_ptr(), self.st)
        self.t.cuda.synchronize()
        return rc, out

    def select(self, users, items, ug, ig, m, skip, upos=None, iids=None):
        rc, out = self.select_raw(users, items, ug, ig, m, skip, upos, iids)
        self.L.check(rc, "inbatch_hard_select")
        nu = users.shape[0]
        return dict(neg_idx=self._cut(out["neg_idx"], nu, "neg_idx", IFILL), neg_score=self._cut(out["neg_score"], nu, "neg_score"),
                    pos_score=self._cut(out["pos_score"], nu, "pos_score"))

    def grads_raw(self, users, items, ug, ig, m, neg_idx, neg_score, pos_score, n_global, d=None):
        nu, ni = users.shape[0], items.shape[0]
        d = users.shape[1] if d is None else d
        U, Y = self.up(users), self.up(items)
        ni_, ns_, ps_ = (self.up(np.asarray(neg_idx, np.int32)), self.up(np.asarray(neg_score, np.float32)),
                         self.up(np.asarray(pos_score, np.float32)))
        npart = self.lib.rihip_inbatch_hard_loss_parts(nu)
        assert npart == R.cdiv(nu, R.OWN)
        nb = self.lib.rihip_inbatch_hard_workspace_bytes(nu, ni, max(1, min(m, 32)))
        assert nb > 0
        ws = self.t.empty((nb,), dtype=self.t.uint8, device=self.dev)
        out = dict(dU=self.nan(nu + GUARD, users.shape[1]), dI=self.nan(ni + GUARD, users.shape[1]),
                   loss_part=self.nan(npart + GUARD, dtype=self.t.float64))
        rc = self.lib.rihip_inbatch_hard_grads(U.data_ptr(), nu, ug, Y.data_ptr(), ni, ig, d, m, ni_.data_ptr(), ns_.data_ptr(),
                                               ps_.data_ptr(), n_global, out["dU"].data_ptr(), out["dI"].data_ptr(),
                                               out["loss_part"].data_ptr(), ws.data_ptr(), self.st)
        self.t.cuda.synchronize()
        return rc, out

    def grads(self, users, items, ug, ig, m, neg_idx, neg_score, pos_score, n_global):
        rc, out = self.grads_raw(users, items, ug, ig, m, neg_idx, neg_score, pos_score, n_global)
        self.L.check(rc, "inbatch_hard_grads")
        nu, ni = users.shape[0], items.shape[0]
        return dict(dU=self._cut(out["dU"], nu, "dU"), dI=self._cut(out["dI"], ni, "dI"),
                    loss_part=self._cut(out["loss_part"], R.cdiv(nu, R.OWN), "loss_part"))

    def last_error(self):
        return self.lib.rihip_last_error().decode()


@pytest.fixture(scope="module")
def gpu():
    return Dev()


def check_select(gpu, cs, m, skip, tag):
    exp = R.select(cs["users"], cs["items"], cs["user_goff"], cs["item_goff"], m, skip, cs["user_pos_ids"], cs["item_ids"])
    got = gpu.select(cs["users"], cs["items"], cs["user_goff"], cs["item_goff"], m, skip, cs["user_pos_ids"], cs["item_ids"])
    assert np.array_equal(exp["neg_score"].astype(np.float32).astype(np.float64), exp["neg_score"]), "scores not exact in f32"
    assert np.array_equal(got["neg_idx"], exp["neg_idx"]), (tag, "neg_idx")
    assert np.array_equal(got["neg_score"], exp["neg_score"].astype(np.float32)), (tag, "neg_score")
    assert np.array_equal(got["pos_score"], exp["pos_score"].astype(np.float32)), (tag, "pos_score")
    return got, exp


# ---------------------------------------------------------------------------------------------------------------------
# 1. selection, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("d", R.WIDTHS)
def test_selection_bit_for_bit(gpu, d, shape):
    nu, ni, ug, ig = shape
    ties = 0
    for with_ids in (False, True):
        cs = R.make_grid_case(100 + d + nu, nu, ni, ug, ig, d, with_ids)
        for m, skip in R.M_SKIP:
            _, exp = check_select(gpu, cs, m, skip, (d, shape, m, skip, with_ids))
        S = exp["S"]
        ties += sum(len(np.unique(S[i])) < ni for i in range(nu))
    if ni >= 127 and d <= 64:
        assert ties > 0          # equal scores are in play: the index half of the order decides


# ---------------------------------------------------------------------------------------------------------------------
# 2. ties and edges
# ---------------------------------------------------------------------------------------------------------------------
def test_identical_rows_take_the_lowest_eligible_indices(gpu):
    d, nu, ni, ug = 48, 40, 200, 150
    row = R.grid_rows(np.random.RandomState(3), 1, d)
    cs = dict(users=np.repeat(row, nu, 0), items=np.repeat(row, ni, 0), user_goff=ug, item_goff=0)
    iids = np.arange(1000, 1000 + ni, dtype=np.int64)
    iids[[0, 2, 5]] = iids[ug + 7]                 # user 7's positive also sits on items 0, 2 and 5
    cs["item_ids"], cs["user_pos_ids"] = iids, iids[ug:ug + nu].copy()
    got, _ = check_select(gpu, cs, 8, 0, "identical")
    assert got["neg_idx"][0].tolist() == list(range(8))
    assert got["neg_idx"][7].tolist() == [1, 3, 4, 6, 7, 8, 9, 10]           # the masked rows are skipped
    cs2 = dict(cs, user_goff=3, user_pos_ids=iids[3:3 + nu].copy())
    got, _ = check_select(gpu, cs2, 8, 0, "identical, partner low")
    assert got["neg_idx"][1].tolist() == [0, 1, 2, 3, 5, 6, 7, 8]            # user 1's partner is item 4
    got, _ = check_select(gpu, cs2, 8, 3, "identical, skip")
    assert got["neg_idx"][1].tolist() == [3, 5, 6, 7, 8, 9, 10, 11]


@pytest.mark.parametrize("ni,m,skip", [(5, 8, 0), (9, 8, 3), (12, 8, 3), (40, 32, 32), (64, 32, 32), (65, 32, 32)])
def test_fewer_items_than_slots(gpu, ni, m, skip):
    nu = min(ni, 33)
    cs = R.make_grid_case(ni, nu, ni, 0, 0, 64, with_ids=False)
    got, exp = check_select(gpu, cs, m, skip, ("few", ni, m, skip))
    c = np.clip(ni - 1 - skip, 0, m)
    assert ((got["neg_idx"] >= 0).sum(axis=1) == c).all() and (exp["c"] == c).all()
    assert (got["neg_idx"][:, c:] == -1).all() and (got["neg_score"][:, c:] == 0).all()     # empties come last


def test_rows_without_negatives_give_exact_zeros(gpu):
    d = 32
    # one item: nothing is eligible
    cs = R.make_unit_case(1, 1, 1, 0, 0, d, with_ids=False)
    sel = gpu.select(cs["users"], cs["items"], 0, 0, 8, 0)
    assert (sel["neg_idx"] == -1).all() and (sel["neg_score"] == 0).all()
    g = gpu.grads(cs["users"], cs["items"], 0, 0, 8, sel["neg_idx"], sel["neg_score"], sel["pos_score"], 1)
    assert g["loss_part"].tolist() == [0.0] and not g["dU"].any() and not g["dI"].any()
    # user 1's positive id sits on every other item: c_1 = 0, the other rows are ordinary
    nu = ni = 6
    cs = R.make_unit_case(2, nu, ni, 0, 0, d, with_ids=False)
    iids = np.full(ni, 7, np.int64)
    upos = np.array([100, 7, 102, 103, 104, 105], np.int64)
    sel = gpu.select(cs["users"], cs["items"], 0, 0, 4, 0, upos, iids)
    assert (sel["neg_idx"][1] == -1).all() and ((sel["neg_idx"] >= 0).sum(axis=1) == [4, 0, 4, 4, 4, 4]).all()
    ref = R.reference(cs["users"], cs["items"], 0, 0, 4, ni, sel["neg_idx"], sel["neg_score"], sel["pos_score"])
    g = gpu.grads(cs["users"], cs["items"], 0, 0, 4, sel["neg_idx"], sel["neg_score"], sel["pos_score"], ni)
    assert not g["dU"][1].any() and ref["loss_rows"][1] == 0
    for k in g:
        assert np.isfinite(g[k]).all(), k
    bnd = R.bounds(ref, cs["users"], cs["items"])
    assert max(R.worst_ratio(g[k], ref[k], bnd[k]) for k in g) <= 1.0


def test_masked_item_with_the_highest_score_is_never_selected(gpu):
    d, nu, ni, ug = 64, 33, 140, 20
    cs = R.make_grid_case(11, nu, ni, ug, 0, d, with_ids=False)
    cs["items"][130] = cs["users"][4]                    # item 130 is user 4's own row: the highest score of that row
    iids = np.arange(500, 500 + ni, dtype=np.int64)
    iids[130] = iids[ug + 4]
    cs["item_ids"], cs["user_pos_ids"] = iids, iids[ug:ug + nu].copy()
    S = cs["users"][4].astype(np.float64) @ cs["items"].astype(np.float64).T
    assert S.argmax() == 130
    got, _ = check_select(gpu, cs, 8, 0, "masked")
    assert 130 not in got["neg_idx"][4]
    plain = gpu.select(cs["users"], cs["items"], ug, 0, 8, 0)
    assert plain["neg_idx"][4][0] == 130


# ---------------------------------------------------------------------------------------------------------------------
# 3. list maintenance: where the best M sit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ni", [300, 517])
@pytest.mark.parametrize("where", ["first", "last", "ascending"])
def test_list_maintenance_paths(gpu, ni, where):
    """score of item j = v_j / 4096 for every user (u_0 = 1, u_1 = 2^-6; y_0 = (v // 64) / 64, y_1 = (v % 64) / 64), all
    v distinct.  first: v falls with j, the first tile holds every list and later tiles never pass the threshold;
    last: v falls with j except in the last tile, which lies above everything; ascending: v rises with j, every full
    tile replaces every list entirely."""
    d, nu = 64, 130
    T = R.cdiv(ni, 128)
    j = np.arange(ni)
    if where == "ascending":
        v = j.copy()
    else:
        v = ni - 1 - j
        if where == "last":
            v[(T - 1) * 128:] += 2 * ni
    v = v - 1024                                                   # both signs
    rng = np.random.RandomState(ni)
    users = R.grid_rows(rng, nu, d)
    users[:, 0], users[:, 1] = 1.0, 2.0 ** -6
    items = np.zeros((ni, d), np.float32)
    items[:, 0], items[:, 1] = (v // 64) / 64.0, (v % 64) / 64.0
    assert np.abs(items).max() <= 1.0
    cs = dict(users=users, items=items, user_goff=0, item_goff=0, user_pos_ids=None, item_ids=None)
    for m, skip in ((8, 3), (32, 32)):
        got, exp = check_select(gpu, cs, m, skip, (where, ni, m, skip))
        assert np.array_equal(exp["S"][0], v / 4096.0)
        M = skip + m
        if where == "first":
            assert got["neg_idx"].max() < 128
        elif where == "last" and ni - (T - 1) * 128 > M:
            assert got["neg_idx"].min() >= (T - 1) * 128
        elif where == "ascending":
            prev = None
            for t in range(1, ni // 128 + 1):                      # the running lists after every full tile are disjoint
                top = set(np.argsort(-v[:128 * t])[:M + 1].tolist())
                assert prev is None or not (top & prev)
                prev = top


# ---------------------------------------------------------------------------------------------------------------------
# 4. gradients: fed the reference's selection, independent of the select kernel
# ---------------------------------------------------------------------------------------------------------------------
def check_grads(gpu, cs, m, n_global, tag):
    ug, ig = cs["user_goff"], cs["item_goff"]
    ref = R.reference(cs["users"], cs["items"], ug, ig, m, n_global, cs["neg_idx"], cs["neg_score"], cs["pos_score"])
    bnd = R.bounds(ref, cs["users"], cs["items"])
    got = gpu.grads(cs["users"], cs["items"], ug, ig, m, cs["neg_idx"], cs["neg_score"], cs["pos_score"], n_global)
    ratios = {k: R.worst_ratio(got[k], ref[k], bnd[k]) for k in ("loss_part", "dU", "dI")}
    print(tag, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (tag, ratios)
    untouched = ref["run"] == 0
    assert not got["dI"][untouched].any(), (tag, "dI rows that nothing selects must be exact zeros")
    return got, ref, bnd


@pytest.mark.parametrize("case", R.grad_cases(), ids=lambda c: f"{c[0]}-" + "x".join(map(str, c[1])) + f"-m{c[2]}s{c[3]}")
def test_gradients_against_reference(gpu, case):
    d, shape, m, skip, with_ids = case
    cs = R.make_grad_case(d, shape, m, skip, with_ids)
    check_grads(gpu, cs, m, shape[3] + shape[1] + 5, case)


def test_item_gradient_is_additive_over_user_slices(gpu):
    d, shape, m = 64, (130, 517, 200, 0), 8
    cs = R.make_grad_case(d, shape, m, 0, True)
    full, full_ref, full_b = check_grads(gpu, cs, m, 517, "whole")
    total, bound = np.zeros((517, d)), full_b["dI"].copy()
    for lo, hi in ((0, 50), (50, 130)):
        part = dict(cs, users=cs["users"][lo:hi], user_goff=200 + lo, neg_idx=cs["neg_idx"][lo:hi],
                    neg_score=cs["neg_score"][lo:hi], pos_score=cs["pos_score"][lo:hi])
        got, _, pb = check_grads(gpu, part, m, 517, ("slice", lo, hi))
        total += got["dI"]
        bound += pb["dI"]
    ratio = R.worst_ratio(total, full["dI"].astype(np.float64), bound)
    print("slices", round(ratio, 3))
    assert ratio <= 1.0


@pytest.mark.parametrize("d", [48, 64])
def test_all_negatives_equal_the_in_batch_bpr_sweep(gpu, d):
    """m = 32 with B = 33: every other row is a negative, the loss is the in-batch BPR.  Both entries get the same
    partner scores (rihip_rowdot); the hard entry gets the f64 scores rounded once to f32 (k_neg = 1).  The two
    references are then the same numbers, and the outputs agree within the sum of the two derived bounds."""
    import inbatch_reference as IR
    B, m = 33, 32
    t, lib, st = gpu.t, gpu.lib, gpu.st
    cs = R.make_unit_case(40 + d, B, B, 0, 0, d, with_ids=False)
    U, Y = gpu.up(cs["users"]), gpu.up(cs["items"])
    pos, r = gpu.nan(B), gpu.nan(B)
    gpu.L.check(lib.rihip_rowdot(U.data_ptr(), Y.data_ptr(), B, 0, d, pos.data_ptr(), st))
    dU, dI = gpu.nan(B, d), gpu.nan(B, d)
    part = t.zeros((lib.rihip_inbatch_workspace_doubles(B),), dtype=t.float64, device=gpu.dev)
    ws = t.empty((lib.rihip_inbatch_workspace_floats(B, B, d),), dtype=t.float32, device=gpu.dev)
    gpu.L.check(lib.rihip_inbatch_sweep(1, U.data_ptr(), B, 0, Y.data_ptr(), B, 0, d, pos.data_ptr(), None, B, dU.data_ptr(),
                                        r.data_ptr(), part.data_ptr(), ws.data_ptr(), 0, st))
    gpu.L.check(lib.rihip_inbatch_sweep(0, Y.data_ptr(), B, 0, U.data_ptr(), B, 0, d, pos.data_ptr(), r.data_ptr(), B,
                                        dI.data_ptr(), None, None, ws.data_ptr(), 0, st))
    t.cuda.synchronize()
    posn = pos.cpu().numpy()
    nparts = lib.rihip_inbatch_loss_parts(B, B)
    sweep_loss = part.cpu().numpy()[:nparts].sum() / (B * (B - 1.0))
    iref = IR.realistic_reference(cs["users"], cs["items"], posn, 0, 0, B)
    ib = IR.bound_sums(iref, posn, d, 0)
    sel = R.select(cs["users"], cs["items"], 0, 0, m, 0)
    assert (sel["c"] == m).all()
    ref = R.reference(cs["users"], cs["items"], 0, 0, m, B, sel["neg_idx"], None, posn)
    hb = R.bounds(ref, cs["users"], cs["items"], k_neg=1, k_pos=0)
    assert np.allclose(ref["dU"], iref["dU"], rtol=1e-11, atol=1e-18) and np.allclose(ref["dI"], iref["dI"], rtol=1e-11, atol=1e-18)
    got = gpu.grads(cs["users"], cs["items"], 0, 0, m, sel["neg_idx"], sel["neg_score"].astype(np.float32), posn, B)
    ratios = dict(dU=R.worst_ratio(got["dU"], dU.cpu().numpy().astype(np.float64), hb["dU"] + ib["dU"]),
                  dI=R.worst_ratio(got["dI"], dI.cpu().numpy().astype(np.float64), hb["dI"] + ib["dI"]),
                  loss=abs(got["loss_part"].sum() / B - sweep_loss)
                  / (hb["loss_part"].sum() / B + ib["loss_part"].sum() / (B * (B - 1.0))))
    print("hard m = B - 1 against the in-batch sweep", d, {k: round(float(v), 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    assert abs(got["loss_part"].sum() / B - ref["loss"]) <= hb["loss_part"].sum() / B


# ---------------------------------------------------------------------------------------------------------------------
# 5. contract
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors(gpu):
    cs = R.make_unit_case(1, 33, 64, 10, 0, 32, with_ids=True)
    U, Y, ids_u, ids_i = cs["users"], cs["items"], cs["user_pos_ids"], cs["item_ids"]
    neg, sc, ps = np.zeros((33, 8), np.int32), np.zeros((33, 8), np.float32), np.zeros(33, np.float32)

    def bad(res, what, code=1, untouched=("neg_idx", "neg_score", "pos_score")):
        rc, out = res
        assert rc == code, (what, rc)
        msg = gpu.last_error()
        assert "inbatch_hard" in msg, (what, msg)
        for k in untouched:                                  # a rejected call launches nothing
            a = out[k].cpu().numpy()
            assert (a == IFILL).all() if k == "neg_idx" else np.isnan(a).all(), (what, k)
        return msg

    g_out = ("dU", "dI", "loss_part")
    for m, skip in ((0, 0), (33, 0), (-1, 0), (8, -1), (32, 33), (1, 64)):
        assert "m=" in bad(gpu.select_raw(U, Y, 10, 0, m, skip), f"m={m} skip={skip}")
    for m in (0, 33, -1):
        bad(gpu.grads_raw(U, Y, 10, 0, m, neg, sc, ps, 64), f"grads m={m}", untouched=g_out)
    for d in (24, 272, 0):
        assert str(d) in bad(gpu.select_raw(U, Y, 10, 0, 8, 0, d=d), f"d={d}", code=3)
        assert str(d) in bad(gpu.grads_raw(U, Y, 10, 0, 8, neg, sc, ps, 64, d=d), f"grads d={d}", code=3, untouched=g_out)
    for ug, ig in ((40, 0), (0, 5), (100, 50)):              # a partner below, above, and outside a slice of the items
        assert "outside" in bad(gpu.select_raw(U, Y, ug, ig, 8, 0), "partner outside")
        assert "outside" in bad(gpu.grads_raw(U, Y, ug, ig, 8, neg, sc, ps, 200), "partner outside", untouched=g_out)
    bad(gpu.select_raw(U, Y, 10, 0, 8, 0, upos=ids_u), "one id array")
    bad(gpu.select_raw(U, Y, 10, 0, 8, 0, iids=ids_i), "one id array")
    bad(gpu.grads_raw(U, Y, 10, 0, 8, neg, sc, ps, 0), "n_global = 0", untouched=g_out)
    # null outputs
    lib, t = gpu.lib, gpu.t
    Ud, Yd, o = gpu.up(U), gpu.up(Y), gpu.nan(64 * 32)
    oi = t.full((33 * 8,), IFILL, dtype=t.int32, device=gpu.dev)
    assert lib.rihip_inbatch_hard_select(Ud.data_ptr(), 33, 10, Yd.data_ptr(), 64, 0, 32, 8, 0, None, None, None, o.data_ptr(),
                                         o.data_ptr(), gpu.st) == 1
    assert lib.rihip_inbatch_hard_select(Ud.data_ptr(), 33, 10, Yd.data_ptr(), 64, 0, 32, 8, 0, None, None, oi.data_ptr(),
                                         o.data_ptr(), None, gpu.st) == 1
    assert lib.rihip_inbatch_hard_grads(Ud.data_ptr(), 33, 10, Yd.data_ptr(), 64, 0, 32, 8, oi.data_ptr(), o.data_ptr(),
                                        o.data_ptr(), 64, o.data_ptr(), None, o.data_ptr(), o.data_ptr(), gpu.st) == 1
    assert lib.rihip_inbatch_hard_grads(Ud.data_ptr(), 33, 10, Yd.data_ptr(), 64, 0, 32, 8, oi.data_ptr(), o.data_ptr(),
                                        o.data_ptr(), 64, o.data_ptr(), o.data_ptr(), o.data_ptr(), None, gpu.st) == 1
    t.cuda.synchronize()
    assert np.isnan(o.cpu().numpy()).all() and (oi.cpu().numpy() == IFILL).all()
    assert lib.rihip_inbatch_hard_workspace_bytes(33, 64, 0) == -1 and lib.rihip_inbatch_hard_workspace_bytes(0, 64, 8) == -1


def test_out_of_range_slots_count_as_empty(gpu):
    """the gradient entry reads indices another launch wrote: one outside [0, n_items) is an empty slot, never an address"""
    cs = R.make_grad_case(32, (33, 127, 94, 0), 8, 0, False)
    cs["neg_idx"] = cs["neg_idx"].copy()
    cs["neg_idx"][3, 2], cs["neg_idx"][5, 0], cs["neg_idx"][9, :] = 127, -5, 2 ** 31 - 1
    check_grads(gpu, cs, 8, 127, "out of range")


def test_two_calls_are_bitwise_equal(gpu):
    cs = R.make_unit_case(8, 130, 517, 200, 0, 144, with_ids=True)
    a = [gpu.select(cs["users"], cs["items"], 200, 0, 8, 3, cs["user_pos_ids"], cs["item_ids"]) for _ in range(2)]
    for k in a[0]:
        assert np.array_equal(a[0][k], a[1][k]), k
    b = [gpu.grads(cs["users"], cs["items"], 200, 0, 8, a[0]["neg_idx"], a[0]["neg_score"], a[0]["pos_score"], 717)
         for _ in range(2)]
    for k in b[0]:
        assert np.array_equal(b[0][k], b[1][k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 6. Python surface
# ---------------------------------------------------------------------------------------------------------------------
def _square_case(B=96, d=32, seed=4):
    cs = R.make_unit_case(seed, B, B, 0, 0, d, with_ids=True)
    cs["user_pos_ids"] = cs["item_ids"]          # square form: the user's positive is its own row's item
    return cs


def _square_reference(cs, m, skip):
    """selection and gradients from the f64 scores; the device's scores are chains of d fused multiply-adds, so the
    case must keep every gap between consecutive ranks above twice that error for the two selections to agree"""
    B, d = cs["users"].shape
    sel = R.select(cs["users"], cs["items"], 0, 0, m, skip, cs["user_pos_ids"], cs["item_ids"])
    el = R.eligible(B, B, 0, 0, cs["user_pos_ids"], cs["item_ids"])
    assert R.selection_margin(sel, el, m, skip) > 4 * d * R.U32, "choose another seed: a near-tie at a rank edge"
    ref = R.reference(cs["users"], cs["items"], 0, 0, m, B, sel["neg_idx"])
    return sel, ref, R.bounds(ref, cs["users"], cs["items"], k_neg=d, k_pos=d)


def test_model_loss_forward_backward(gpu):
    import torch
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.two_tower import hard_negatives
    B, d, m, skip = 96, 32, 8, 2
    cs = _square_case(B, d)
    sel, ref, bnd = _square_reference(cs, m, skip)
    assert not R.eligible(B, B, 0, 0, cs["user_pos_ids"], cs["item_ids"])[~np.eye(B, dtype=bool)].all()   # the mask is in play
    model = TwoTowerModel(10, 10, embed_dim=d, hidden_dim=64)
    U = torch.from_numpy(cs["users"]).cuda().requires_grad_(True)
    Y = torch.from_numpy(cs["items"]).cuda().requires_grad_(True)
    ids = torch.from_numpy(cs["item_ids"])
    neg_idx, neg_score, pos_score = hard_negatives(U.detach(), Y.detach(), m, skip, ids)
    assert np.array_equal(neg_idx.cpu().numpy(), sel["neg_idx"])
    assert np.abs(neg_score.cpu().numpy() - sel["neg_score"]).max() <= d * R.U32 * ref["a_neg"].max()
    loss = model.in_batch_hard_bpr_loss(U, Y, n_hard=m, skip=skip, item_ids=ids)
    loss.backward()
    lb = bnd["loss_part"].sum() / B + abs(ref["loss"]) * 2.0 ** -23
    assert abs(loss.item() - ref["loss"]) <= lb, (loss.item(), ref["loss"], lb)
    assert R.worst_ratio(U.grad.cpu().numpy(), ref["dU"], bnd["dU"]) <= 1.0
    assert R.worst_ratio(Y.grad.cpu().numpy(), ref["dI"], bnd["dI"]) <= 1.0
    for kw in (dict(n_hard=0), dict(n_hard=33), dict(skip=-1), dict(n_hard=32, skip=33)):
        with pytest.raises(ValueError):
            model.in_batch_hard_bpr_loss(U, Y, **kw)


def test_model_loss_under_graph_capture(gpu):
    import torch
    from recommendit_amd.two_tower import hard_loss_and_grads
    cs = _square_case(130, 48, seed=6)
    U, Y, ids = gpu.up(cs["users"]), gpu.up(cs["items"]), gpu.up(cs["item_ids"])
    eager = [x.clone() for x in hard_loss_and_grads(U, Y, 8, 1, ids)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            outs = hard_loss_and_grads(U, Y, 8, 1, ids)
    for o in outs[:3]:
        o.fill_(float("nan"))
    outs[3].fill_(IFILL)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 7. trainer
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
    kw.setdefault("table_opt", "dense")
    return HipBPRTrainer(m, B, lr=1e-2, weight_decay=1e-5, loss_mode=mode, seed=3, **kw)


def _batch(B, nu=256, ni=300, seed=11):
    from oracle import fixtures as fx
    import torch
    u, p, gp, n, gn = fx.make_batch(nu, ni, B, seed=seed, boundary=False)
    c = lambda x: torch.from_numpy(np.asarray(x)).cuda()
    return c(u), c(p), c(gp)


@pytest.mark.parametrize("mask", [True, False])
def test_trainer_step_equals_direct_calls(gpu, mask):
    import torch
    B, d, m, skip = 96, 32, 8, 1
    tr = _trainer("hard", n_hard=m, hard_skip=skip, mask_duplicates=mask)
    u, p, gp = _batch(B)
    assert len(np.unique(p.cpu().numpy())) < B          # the batch has duplicate items: the mask is in play
    loss = tr.step(u, p, gp)
    torch.cuda.synchronize()
    Un, Yn, ids = tr.U.cpu().numpy(), tr.I.cpu().numpy(), p.cpu().numpy()
    sel = gpu.select(Un, Yn, 0, 0, m, skip, *((ids, ids) if mask else (None, None)))
    for k in sel:
        assert np.array_equal(getattr(tr, k).cpu().numpy(), sel[k]), k
    got = gpu.grads(Un, Yn, 0, 0, m, sel["neg_idx"], sel["neg_score"], sel["pos_score"], B)
    assert np.array_equal(tr.dU.cpu().numpy(), got["dU"]) and np.array_equal(tr.dI.cpu().numpy(), got["dI"])
    out = gpu.nan(1)
    part = gpu.up(got["loss_part"])
    gpu.L.check(gpu.lib.rihip_sum_partials(part.data_ptr(), 1, 1.0 / B, out.data_ptr(), gpu.st))
    assert float(loss) == float(out[0])
    # ... and the direct call is the reference's for the selection it made
    ref = R.reference(Un, Yn, 0, 0, m, B, sel["neg_idx"], sel["neg_score"], sel["pos_score"])
    bnd = R.bounds(ref, Un, Yn)
    assert R.worst_ratio(got["dU"], ref["dU"], bnd["dU"]) <= 1.0 and R.worst_ratio(got["dI"], ref["dI"], bnd["dI"]) <= 1.0
    if mask:                                            # no row trains against another row's copy of its own positive
        idx = sel["neg_idx"]
        assert not (np.where(idx >= 0, ids[np.maximum(idx, 0)], -1) == ids[:, None]).any()


def test_trainer_graph_replay_equals_eager(gpu):
    """the select sweep and the rocPRIM sort of the gradient entry inside the captured step: graph == eager, bitwise"""
    import torch
    B = 96
    outs = []
    for use_graph in (False, True):
        tr = _trainer("hard", n_hard=8, table_opt="sparse", use_graph=use_graph)
        losses = []
        for step in range(5):
            u, p, gp = _batch(B, seed=step * 13)
            losses.append(tr.step(u, p, gp).item())
        assert (tr._graph is not None) == use_graph
        tr.check_errors()
        outs.append((losses, {k: v.detach().clone() for k, v in tr.model.named_parameters()}))
    assert outs[0][0] == outs[1][0]
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


def test_twenty_steps_lower_the_loss(gpu):
    import torch
    B, nu, ni = 96, 256, 300
    rng = np.random.RandomState(0)
    pos_of_user = rng.randint(1, ni + 1, size=nu + 1)            # one liked item per user: a learnable set of 256 pairs
    tr = _trainer("hard", n_hard=8)
    genres = torch.from_numpy((rng.rand(ni + 1, 18) < 0.2).astype(np.float32)).cuda()
    losses = []
    for step in range(20):
        u = rng.randint(1, nu + 1, size=B)
        p = torch.from_numpy(pos_of_user[u]).cuda()
        losses.append(tr.step(torch.from_numpy(u).cuda(), p, genres[p]).clone())    # step() returns its own loss buffer
    losses = [float(x) for x in losses]
    tr.check_errors()
    print("hard-negative loss, 20 steps:", [round(x, 3) for x in losses])
    assert np.isfinite(losses).all() and np.mean(losses[-3:]) < np.mean(losses[:3]), losses


def test_distributed_hard_raises():
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    m = TwoTowerModel(20, 20, embed_dim=32, hidden_dim=64)
    with pytest.raises(ValueError, match="hard"):
        HipBPRTrainer(m, 8, loss_mode="hard", table_opt="sparse", distributed=True)
    with pytest.raises(ValueError, match="n_hard"):
        HipBPRTrainer(m, 8, loss_mode="hard", n_hard=0)
