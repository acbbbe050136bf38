"""The host reference of the in-batch sampled softmax (tests/softmax_reference.py) against torch CPU f64 autograd, the
sizing rule of its realistic cases, and the properties the GPU tests rely on.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import softmax_reference as R  # noqa: E402


def torch_loss_and_grads(cs, inv_temp, n_global):
    """cross_entropy on the masked logits, reduction='sum' scaled by 1 / n_global, f64 autograd"""
    U = torch.tensor(cs["users"].astype(np.float64), requires_grad=True)
    Y = torch.tensor(cs["items"].astype(np.float64), requires_grad=True)
    nu, ni = U.shape[0], Y.shape[0]
    logits = inv_temp * (U @ Y.T)
    if cs["logq"] is not None:
        logits = logits - torch.tensor(cs["logq"].astype(np.float64))[None, :]
    target = torch.arange(nu) + cs["user_goff"] - cs["item_goff"]
    if cs["item_ids"] is not None:
        same = torch.tensor(cs["item_ids"])[None, :] == torch.tensor(cs["user_pos_ids"])[:, None]
        same[torch.arange(nu), target] = False
        logits = logits.masked_fill(same, float("-inf"))
    loss = torch.nn.functional.cross_entropy(logits, target, reduction="sum") / n_global
    loss.backward()
    return float(loss.detach()), U.grad.numpy(), Y.grad.numpy()


# (seed, n_users, n_items, user_goff, item_goff, d, inv_temp, n_global, logq, ids)
TORCH_CASES = [
    (11, 40, 40, 0, 0, 16, 20.0, 40, True, True),
    (12, 33, 70, 50, 30, 48, 1.0, 200, False, True),
    (13, 57, 90, 7, 0, 64, 5.0, 90, True, False),
    (14, 25, 61, 12, 5, 32, 20.0, 61, False, False),
]


@pytest.mark.parametrize("case", TORCH_CASES, ids=lambda c: f"seed{c[0]}")
def test_reference_equals_torch_autograd(case):
    seed, nu, ni, ug, ig, d, inv_temp, ng, with_logq, with_ids = case
    cs = R.make_case(seed, nu, ni, ug, ig, d, with_logq, with_ids)
    ref = R.reference(cs["users"], cs["items"], ug, ig, inv_temp, ng, cs["logq"], cs["user_pos_ids"], cs["item_ids"])
    assert ref["user_ok"]
    # the item-mode expectation uses the f32-rounded lse (what a caller passes on); autograd corresponds to the exact one
    p = ref["p"]
    dI_exact = ref["c"] * (p.T @ cs["users"].astype(np.float64))
    irow, iok = R.partner_of_items(ni, ig, nu, ug)
    dI_exact -= ref["c"] * np.where(iok[:, None], cs["users"].astype(np.float64)[irow], 0.0)
    loss, gU, gY = torch_loss_and_grads(cs, inv_temp, ng)
    assert abs(ref["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    np.testing.assert_allclose(ref["dU"], gU, rtol=0, atol=1e-13)
    np.testing.assert_allclose(dI_exact, gY, rtol=0, atol=1e-13)
    # ... and the f32 rounding of lse moves dI by no more than 2^-24 |lse| relative to its un-cancelled size
    slack = 2.0 ** -24 * (np.abs(ref["lse"]).max() + 1) * ref["M_dI"] + 1e-15
    assert np.all(np.abs(ref["dI"] - gY) <= slack)
    if with_ids:
        assert ref["dropped"].any()


@pytest.mark.parametrize("d", sorted(R.REALISTIC_CASES))
def test_realistic_sizes_follow_the_ladder_rule(d):
    """the table holds the LARGEST rung at which one pair stands >= 100 x above the bound of lse, dU and dI"""
    shape = R.REALISTIC_CASES[d]
    ratios = R.rung_ratios(d, R.REALISTIC_INV_TEMP, shape)
    print(d, shape, {k: round(v, 1) for k, v in ratios.items()})
    assert min(ratios.values()) >= 100, ratios
    assert R.choose_rung(d, R.REALISTIC_INV_TEMP) == shape


def test_no_rung_qualifies_at_inv_temp_20():
    """documented in softmax_reference.py: a sharp softmax's least likely pair is below every rounding bound"""
    assert R.choose_rung(64, 20.0) is None


def test_item_mode_is_additive_over_user_slices():
    nu, ni, ug, ig, d, inv_temp, ng = 161, 257, 0, 0, 32, 20.0, 257
    cs = R.make_case(21, nu, ni, ug, ig, d)
    full = R.reference(cs["users"], cs["items"], ug, ig, inv_temp, ng, cs["logq"], cs["user_pos_ids"], cs["item_ids"])
    lse32 = full["lse_used"].astype(np.float32)
    total = np.zeros_like(full["dI"])
    for lo, hi in ((0, 50), (50, 130), (130, 161)):
        part = R.reference(cs["users"][lo:hi], cs["items"], ug + lo, ig, inv_temp, ng, cs["logq"],
                           cs["user_pos_ids"][lo:hi], cs["item_ids"], lse_in=lse32[lo:hi])
        total += part["dI"]
    np.testing.assert_allclose(total, full["dI"], rtol=0, atol=1e-15)


def test_duplicate_ids_really_mask_pairs():
    cs = R.make_case(5, 129, 300, 77, 0, 16)
    ref = R.reference(cs["users"], cs["items"], 77, 0, 20.0, 300, cs["logq"], cs["user_pos_ids"], cs["item_ids"])
    assert ref["dropped"].sum() >= 5 and not (ref["dropped"] & ref["diag"]).any()
    assert np.all(ref["p"][ref["dropped"]] == 0) and np.all(ref["p_item"][ref["dropped"]] == 0)
    free = R.reference(cs["users"], cs["items"], 77, 0, 20.0, 300, cs["logq"])
    rows = ref["dropped"].any(axis=1)
    assert np.all(ref["lse"][rows] < free["lse"][rows]) and np.array_equal(ref["lse"][~rows], free["lse"][~rows])


def test_item_log_q():
    from recommendit_amd.train_embeddings import item_log_q
    lq = item_log_q(np.array([3, 3, 3, 1, 4, 4]), 6)
    assert lq.dtype == np.float32 and lq.shape == (6,)
    np.testing.assert_allclose(lq[[1, 3, 4]], np.log([1 / 6, 3 / 6, 2 / 6]), rtol=1e-6)
    np.testing.assert_allclose(lq[[0, 2, 5]], np.log(1 / 6), rtol=1e-6)      # never seen: the smallest positive probability
