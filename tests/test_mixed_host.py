"""CPU: the host reference of the mixed in-batch objective tests (tests/mixed_reference.py): its selection on hand-made
weights, the mixed gradients against the two existing references, the sensitivity of every apply case used on the GPU,
the share of rows the chain cases leave out of the selection comparison, and the argument errors that need no device."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import hard_reference as H  # noqa: E402
import inbatch_reference as IB  # noqa: E402
import mixed_reference as R  # noqa: E402


def test_mine_on_hand_made_weights():
    # one user (global 2) against six items; weights .5 .25 [partner] .25 1 0 -> item 4, then 0, then 1 and 3 tie
    w = np.array([[0.5], [0.25], [0.0], [0.25], [1.0], [0.0]], np.float32)
    sel = R.mine(w, 2, 0, 3, 0)
    assert sel["neg_idx"].tolist() == [[4, 0, 1]] and sel["neg_w"].tolist() == [[1.0, 0.5, 0.25]]
    assert R.mine(w, 2, 0, 3, 2)["neg_idx"].tolist() == [[1, 3, 5]]          # an eligible 0 is a candidate
    sel = R.mine(w, 2, 0, 4, 3)
    assert sel["neg_idx"].tolist() == [[3, 5, -1, -1]] and sel["c"].tolist() == [2]
    # the partner's slot is never a candidate whatever it holds; -0 and +0 are one weight
    w2 = np.array([[-0.0], [0.0], [9.0], [-0.0]], np.float32)
    assert R.mine(w2, 2, 0, 3, 0)["neg_idx"].tolist() == [[0, 1, 3]]
    iids = np.array([10, 11, 12, 13, 12, 15], np.int64)
    assert R.mine(w, 2, 0, 2, 0, np.array([12], np.int64), iids)["neg_idx"].tolist() == [[0, 1]]
    assert R.mine(w[:1], 0, 0, 8, 0)["c"].tolist() == [0]


def test_blocked_gmat_layout():
    nu, ni = 33, 70
    w = R.make_weights("random", 1, nu, ni, 5)
    flat = R.blocked_gmat(w, nu, ni)
    ub = IB.g_ub(nu)
    for j, i in ((0, 0), (31, 32), (69, 32), (33, 7)):
        assert flat[((j // 32) * ub + i // 32) * 1024 + (j % 32) * 32 + i % 32] == w[j, i]
    full = IB.decode_gmat(flat, nu, ni)
    assert (full[:96, 33:64] == 0).all() and (full[70:96, :64] == 0).all()
    assert np.isnan(full[96:]).all() and np.isnan(full[:, 64:]).all()


def test_special_rows_exist():
    """the id modes give a row below skip, a row between skip and skip + m, and the weights an all-zero row"""
    nu, ni, ug = 130, 517, 200
    w = R.make_weights("ternary", 3, nu, ni, ug)
    assert (w[:, 0] == 0).all()
    for m, skip in R.M_SKIP:
        upos, iids = R.make_mine_ids("below", 4, nu, ni, ug, m, skip)
        sel = R.mine(w, ug, 0, m, skip, upos, iids)
        assert sel["c"][0] == 0 and sel["c"][-1] == 0 and sel["eligible_count"][0] <= skip
        upos, iids = R.make_mine_ids("between", 4, nu, ni, ug, m, skip)
        sel = R.mine(w, ug, 0, m, skip, upos, iids)
        assert skip <= sel["eligible_count"][0] <= skip + m and (m == 1 or 0 < sel["c"][0] < m)
        assert (sel["c"][1:-1] == m).all()


@pytest.mark.parametrize("d", (32, 64, 128))
def test_apply_reference_is_inbatch_plus_weighted_hard(d):
    """r and dU of apply_reference on top of the in-batch values equal in-batch + hard_weight * hard (hard_reference, fed
    the same selection and f32 scores): the algebra of the boost, to the f32 roundings of sigma, f_i and D"""
    cs = R.make_apply_case(7, (33, 97, 30), d, 8, 0)
    hw, n = 0.5, cs["n_global"]
    ref = R.apply_reference(cs["weights"], cs["users"], cs["items"], cs["pos"], cs["user_goff"], 0, 8, cs["neg_idx"],
                            cs["neg_w"], hw, n, cs["dU_in"], cs["r_in"])
    hard = H.reference(cs["users"], cs["items"], cs["user_goff"], 0, 8, n, cs["neg_idx"], pos_score=cs["pos"])
    exp_dU = cs["dU_in"].astype(np.float64) + hw * hard["dU"]
    mag = np.abs(cs["dU_in"]) + hw * (hard["M_dU"] + hard["C_dU"])
    assert (np.abs(ref["dU"] - exp_dU) <= 8 * R.U32 * mag).all()
    exp_part = hw * n * (n - 1.0) * hard["loss"]
    assert abs(ref["loss_part"].sum() - exp_part) <= 1e-12 * exp_part
    # hard_weight = 0: nothing moves
    ref0 = R.apply_reference(cs["weights"], cs["users"], cs["items"], cs["pos"], cs["user_goff"], 0, 8, cs["neg_idx"],
                             cs["neg_w"], 0.0, n, cs["dU_in"], cs["r_in"])
    assert np.array_equal(ref0["weights"], cs["weights"]) and np.array_equal(ref0["r"], cs["r_in"].astype(np.float64))
    assert np.array_equal(ref0["dU"], cs["dU_in"].astype(np.float64)) and (ref0["loss_part"] == 0).all()


@pytest.mark.parametrize("shape", R.APPLY_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("d", (32, 64, 128))
def test_one_pair_stands_above_the_apply_bounds(d, shape):
    """every apply case of tests/test_gpu_mixed.py: one selected pair's contribution is >= 100 x the bound of the output
    it lands in, so the bounds cannot hide a missing pair"""
    for m, skip in ((8, 0), (8, 3)):
        cs = R.make_apply_case(7, shape, d, m, skip)
        for hw in R.HARD_WEIGHTS[1:]:
            ref = R.apply_reference(cs["weights"], cs["users"], cs["items"], cs["pos"], cs["user_goff"], 0, m,
                                    cs["neg_idx"], cs["neg_w"], hw, cs["n_global"], cs["dU_in"], cs["r_in"])
            ratios = R.one_pair_ratios(ref, R.apply_bounds(ref), cs["items"])
            print(f"d={d} shape={shape} m={m} skip={skip} hw={hw}: " + " ".join(f"{k}={v:.0f}" for k, v in ratios.items()))
            assert min(ratios.values()) >= 100, ratios


@pytest.mark.parametrize("shape", R.CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("d,precision", R.CHAIN_CASES)
def test_chain_cases_leave_out_at_most_a_tenth(d, precision, shape):
    """the reference alone: the rows whose f64 weights at ranks 0 .. skip + m stand closer than the stored weights' bounds"""
    m, skip = R.chain_m_skip(d, precision)
    users, items, upos, iids = R.make_chain_case(R.CHAIN_SEED, shape, d)
    cr = R.chain_reference(users, items, shape[2], 0.5, m, skip, upos, iids, precision)
    out = 1.0 - cr["entered"].mean()
    print(f"d={d} precision={precision} shape={shape}: {100 * out:.1f} % of the rows left out")
    assert out <= 0.10


def test_python_argument_errors_without_a_device():
    from recommendit_amd.two_tower import _check_hard_weight, mixed_loss_and_grads
    import torch
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="hard_weight"):
            _check_hard_weight(bad, "x")
    assert _check_hard_weight(0, "x") == 0.0
    U = torch.zeros((4, 48))
    with pytest.raises(ValueError, match="in_batch_bpr_loss \\+ hard_weight \\* in_batch_hard_bpr_loss"):
        mixed_loss_and_grads(U, U, 0.1, 2)
    U = torch.zeros((4, 64))
    with pytest.raises(ValueError, match="precision 0 or 2.*in_batch_bpr_loss \\+ hard_weight"):
        mixed_loss_and_grads(U, U, 0.1, 2, precision=1)
