"""CPU: the host reference of the in-batch hard-negative tests (tests/hard_reference.py) against the in-batch BPR oracle,
its selection on hand-made rows, the sensitivity of every gradient case used on the GPU, and the argument errors of the
Python surface that need no device."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import hard_reference as R  # noqa: E402


@pytest.mark.parametrize("B,d", [(2, 16), (7, 48), (33, 64)])
def test_all_negatives_equal_in_batch_bpr(B, d):
    """m = B - 1, skip = 0, no ids: every other row is selected, c_i = B - 1 and the loss is the in-batch BPR of
    oracle/two_tower_np.py.  The oracle returns its f64 results rounded to f32: agreement to that one rounding."""
    from oracle import two_tower_np as O
    cs = R.make_unit_case(5, B, B, 0, 0, d, with_ids=False)
    sel = R.select(cs["users"], cs["items"], 0, 0, B - 1, 0)
    assert (sel["c"] == B - 1).all()
    assert all(sorted(sel["neg_idx"][i]) == [j for j in range(B) if j != i] for i in range(B))
    ref = R.reference(cs["users"], cs["items"], 0, 0, B - 1, B, sel["neg_idx"])
    loss, dU, dI = O.in_batch_bpr_loss(cs["users"], cs["items"])
    assert abs(ref["loss"] - float(loss)) <= 2.0 ** -24 * abs(ref["loss"])
    for got, exp, mag in ((ref["dU"], dU, ref["M_dU"] + ref["C_dU"]), (ref["dI"], dI, ref["M_dI"] + ref["C_dI"])):
        # the oracle's matrix products add in another order: f64 rounding of the un-cancelled sum, then the f32 cast
        assert (np.abs(got - exp) <= 2.0 ** -24 * np.abs(got) + 2.0 ** -45 * mag + 2.0 ** -149).all()


def test_selection_on_hand_made_rows():
    # one user (global 2) against six items; scores 5 3 [partner] 3 9 1 -> item 4 (9), then 1 and 3 tie at 3: lower first
    S = np.array([[5.0, 3.0, 7.0, 3.0, 9.0, 1.0]])
    U, Y = np.zeros((1, 16), np.float32), np.zeros((6, 16), np.float32)
    sel = R.select(U, Y, 2, 0, 3, 0, scores=S)
    assert sel["neg_idx"].tolist() == [[4, 0, 1]] and sel["neg_score"].tolist() == [[9.0, 5.0, 3.0]]
    assert sel["pos_score"].tolist() == [7.0] and sel["c"].tolist() == [3]
    sel = R.select(U, Y, 2, 0, 3, 2, scores=S)                      # skip the two hardest
    assert sel["neg_idx"].tolist() == [[1, 3, 5]]
    sel = R.select(U, Y, 2, 0, 4, 3, scores=S)                      # the order runs out: empties last
    assert sel["neg_idx"].tolist() == [[3, 5, -1, -1]] and sel["neg_score"].tolist() == [[3.0, 1.0, 0.0, 0.0]]
    assert sel["c"].tolist() == [2]
    # the highest-scoring item carries the id of the user's positive: never selected; the partner's own id is no mask
    iids = np.array([10, 11, 12, 13, 12, 15], np.int64)
    sel = R.select(U, Y, 2, 0, 2, 0, np.array([12], np.int64), iids, scores=S)
    assert sel["neg_idx"].tolist() == [[0, 1]]
    # the tie order is by GLOBAL index whatever the offset of the slice
    sel = R.select(U, Y, 102, 100, 6, 0, scores=np.ones((1, 6)))
    assert sel["neg_idx"].tolist() == [[0, 1, 3, 4, 5, -1]]
    # -0 and +0 are one score
    sel = R.select(U, Y, 2, 0, 2, 0, scores=np.array([[0.0, -0.0, 9.0, -0.0, 0.0, -1.0]]))
    assert sel["neg_idx"].tolist() == [[0, 1]]
    # one item only: nothing is eligible
    sel = R.select(U[:, :], Y[:1], 0, 0, 8, 0, scores=np.array([[3.0]]))
    assert sel["c"].tolist() == [0] and (sel["neg_idx"] == -1).all()


def test_empty_rows_have_zero_loss_and_gradient():
    cs = R.make_unit_case(1, 3, 3, 0, 0, 16, with_ids=False)
    neg = np.array([[1, -1], [-1, -1], [0, 1]], np.int32)
    ref = R.reference(cs["users"], cs["items"], 0, 0, 2, 3, neg)
    assert ref["c"].tolist() == [1, 0, 2] and ref["loss_rows"][1] == 0 and not ref["dU"][1].any()
    assert np.isfinite(ref["loss"]) and np.isfinite(ref["dU"]).all() and np.isfinite(ref["dI"]).all()
    # row 1 selects nothing, so its partner item 1 receives only what rows 0 and 2 send it
    exp = ref["w"][0, 0] * cs["users"][0].astype(np.float64) + ref["w"][2, 1] * cs["users"][2].astype(np.float64)
    assert np.allclose(ref["dI"][1], exp, rtol=1e-15, atol=0)


def test_reference_bookkeeping():
    """W is the row sum of the weights, and every selected pair plus one partner term per non-empty row lands in dI"""
    cs = R.make_grad_case(64, (33, 127, 94, 0), 8, 3, True)
    ref = R.reference(cs["users"], cs["items"], 94, 0, 8, 127, cs["neg_idx"], cs["neg_score"], cs["pos_score"])
    assert np.allclose(ref["W"], ref["w"].sum(axis=1))
    assert ref["run"].sum() == ref["ok"].sum() + (ref["c"] > 0).sum()


def test_one_pair_stands_above_every_bound():
    """for every gradient case of tests/test_gpu_hard_negatives.py one selected pair's contribution is >= 100 x the bound
    of the output it lands in: a dropped or misplaced pair cannot hide inside a bound"""
    worst = {}
    for d, shape, m, skip, with_ids in R.grad_cases():
        cs = R.make_grad_case(d, shape, m, skip, with_ids)
        nu, ni, ug, ig = shape
        ref = R.reference(cs["users"], cs["items"], ug, ig, m, ig + ni + 5, cs["neg_idx"], cs["neg_score"], cs["pos_score"])
        bnd = R.bounds(ref, cs["users"], cs["items"])
        for k, v in R.one_pair_ratios(ref, bnd, cs["users"], cs["items"]).items():
            if v < worst.get(k, (np.inf,))[0]:
                worst[k] = (v, d, shape, m, skip)
    print("smallest one-pair ratios:", worst)
    assert min(v[0] for v in worst.values()) >= 100, worst


def test_bounds_cover_an_f32_emulation():
    """the reference's own arithmetic redone in f32 (NumPy, another summation order) stays inside the derived bounds: a
    bound that a faithful f32 evaluation breaks would be wrong"""
    cs = R.make_grad_case(64, (129, 300, 77, 0), 8, 0, True)
    ref = R.reference(cs["users"], cs["items"], 77, 0, 8, 300, cs["neg_idx"], cs["neg_score"], cs["pos_score"])
    bnd = R.bounds(ref, cs["users"], cs["items"])
    f = np.float32
    z = (cs["neg_score"] - cs["pos_score"][:, None]).astype(f)
    sg = (f(1) / (f(1) + np.exp(-z, dtype=f))) * ref["ok"]
    w = (sg * (f(1) / (f(300) * np.maximum(ref["c"], 1).astype(f)))[:, None]).astype(f)
    dU = np.zeros_like(cs["users"])
    for s in range(8):
        dU += w[:, s, None] * cs["items"][ref["jj"][:, s]]
    dU -= w.sum(axis=1, dtype=f)[:, None] * cs["items"][ref["drow"]]
    assert R.worst_ratio(dU, ref["dU"], bnd["dU"]) <= 1.0


def test_trainer_argument_errors_need_no_device():
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.train_embeddings import EmbeddingTrainer
    from recommendit_amd.trainer import HipBPRTrainer
    m = TwoTowerModel(20, 20, embed_dim=32, hidden_dim=64)
    for kw in (dict(n_hard=0), dict(n_hard=33), dict(n_hard=8, hard_skip=-1), dict(n_hard=32, hard_skip=33),
               dict(n_hard=2.5)):
        with pytest.raises(ValueError, match="n_hard"):
            HipBPRTrainer(m, 8, loss_mode="hard", **kw)
        with pytest.raises(ValueError, match="n_hard"):
            EmbeddingTrainer(loss_mode="hard", **kw)
    with pytest.raises(ValueError, match="hard"):
        HipBPRTrainer(m, 8, loss_mode="hard", table_opt="sparse", distributed=True)
    with pytest.raises(ValueError, match="multiple of 16"):
        HipBPRTrainer(TwoTowerModel(20, 20, embed_dim=24, hidden_dim=64), 8, loss_mode="hard")
    import torch
    U = torch.zeros(4, 32)
    for kw in (dict(n_hard=0), dict(n_hard=40), dict(skip=-1), dict(n_hard=32, skip=40)):
        with pytest.raises(ValueError):
            m.in_batch_hard_bpr_loss(U, U, **kw)
    with pytest.raises(ValueError):
        m.in_batch_hard_bpr_loss(U, torch.zeros(5, 32))
    with pytest.raises(ValueError):
        m.in_batch_hard_bpr_loss(U, U, item_ids=torch.zeros(3, dtype=torch.int64))
