"""The sampled-negative training step with the dense optimiser, phase by phase against tests/step_reference.py.

Both forms of the step are checked: the one-launch step (csrc/step_persistent.hip: forward, loss gradient, data and weight
gradients, scatter, norm, clip and Adam between three grid barriers) and the seven-launch step.  Every case runs three
consecutive steps on different batches with the learning rate changed before the second; after each step every buffer
the trainer exposes is compared with the float64 evaluation of its stage on the float32 inputs the previous stage
stored (bounds and cap: the docstring of step_reference.py; the cap condition is proven in tests/test_step_host.py).
Steps 2 and 3 run with whatever step 1 left in the caches, the recycled barrier counters and the table gradients the
previous step must have left zero.  Run with -s for the worst error / tolerance per tensor."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu


def _report(name, value):
    print(f"[worst] {name}: {value:.3f}")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _trainer(c, persistent, guard_rows=0):
    """a trainer on the case's initial state.  guard_rows: the tables (and the tables' moments) are the leading rows of
    larger buffers whose remaining rows hold a sentinel"""
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    m = TwoTowerModel(S.NU, S.NI, embed_dim=c.d, hidden_dim=c.H, dropout=c.p)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c.sd.items()})
    m = m.cuda()
    guards = []
    if guard_rows:
        for emb in (m.user_tower.embedding, m.item_tower.embedding):
            n = emb.weight.shape[0]
            big = torch.full((n + guard_rows, c.d), SENTINEL, dtype=torch.float32, device="cuda")
            big[:n].copy_(emb.weight.data)
            emb.weight.data = big[:n]
            guards.append(big[n:])
    m.train(c.train)
    tr = HipBPRTrainer(m, c.B, lr=c.lrs[0], weight_decay=c.wd, betas=(S.B1, S.B2), eps=S.EPS, max_norm=c.max_norm,
                       loss_mode="sampled", table_opt="dense", seed=c.seed, persistent=persistent)
    assert tr.persistent == persistent
    if guard_rows:      # (before the first step: the one-launch step reads the moments' addresses when it first runs)
        for opt in (tr.uopt, tr.iopt):
            n = opt.m.shape[0]
            for name in ("m", "v"):
                big = torch.full((n + guard_rows, c.d), SENTINEL, dtype=torch.float32, device="cuda")
                big[:n].zero_()
                setattr(opt, name, big[:n])
                guards.append(big[n:])
    return m, tr, guards


SENTINEL = 7.0


def _np(x):
    return x.detach().cpu().numpy().copy()


def _snapshot(m, tr):
    got = {n: _np(getattr(tr, n)) for n in ("U", "I", "hidU", "hidI", "denU", "denI", "dU", "dI", "dXu", "dXi")}
    got.update(loss=_np(tr.loss), gnorm=_np(tr.gnorm).reshape(()), coef=_np(tr.coef).reshape(()), hyper=_np(tr.hyper_dev))
    got["g"] = {k: _np(tr.gv[k]) for k in S.MLP_KEYS}
    got["p"] = {k: _np(v) for k, v in m.named_parameters()}
    got["m"], got["v"] = {}, {}
    for k in S.MLP_KEYS:       # the moments of a tensor sit where its gradient view sits in the flat buffers
        o = (tr.gv[k].data_ptr() - tr.flat_g.data_ptr()) // 4
        n = tr.gv[k].numel()
        got["m"][k] = _np(tr.flat_m[o:o + n].view_as(tr.gv[k]))
        got["v"][k] = _np(tr.flat_v[o:o + n].view_as(tr.gv[k]))
    for k, opt in zip(S.TAB_KEYS, (tr.uopt, tr.iopt)):
        got["m"][k], got["v"][k] = _np(opt.m), _np(opt.v)
    return got


def _state(got):
    return S.next_state(got)


def _run(c, persistent, steps=3):
    m, tr, _ = _trainer(c, persistent)
    out = []
    for k in range(steps):
        u, it, g = c.batches[k]
        tr.step(_dev(u), _dev(it), _dev(g), lr=c.lrs[k])
        torch.cuda.synchronize()
        assert int(tr.step_dev.item()) == k + 2
        out.append(_snapshot(m, tr))
    tr.check_errors()
    return out


@pytest.mark.parametrize("persistent", [True, False], ids=["one_launch", "seven_launches"])
@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_every_phase_of_three_steps(name, persistent):
    """
    case           d, H, B          reaches
    one_row        32, 64, 1        one row; pos and neg in item tile 0; 1 / B = 1; dropout on; clip active; wd > 0; the
                                    padding id as the user of step 2 and the negative of step 3
    tile_boundary  48, 96, 33       2 user and 3 item tiles, the pos / neg boundary inside item tile 1, last tiles of 1 and 2
                                    rows; dropout on; wd = 0; padding id at user, pos and neg positions
    min_width      16, 16, 40       minimum widths, the dynamic-LDS floor, item K1 = 34 padded to 40; eval mode with p = 0.5
    odd_widths     240, 208, 70     multiples of 16 that are not multiples of 32: partial weight-gradient tiles and
                                    partial lanes; dropout on; clip active; wd > 0
    second_wgrad   256, 256, 96     288 weight-gradient tiles on 256 workgroups: 32 run the loop twice; largest LDS
                                    request; eval mode with p = 0.5; wd = 0
    max_batch      32, 32, 2048     64 user and 128 item tiles; item ids in {1, 2, 3}; user rows 1 and 257 (one owner)
                                    interleaved; wd > 0
    full_list      32, 32, 2048     all 4096 item ids = 5: one list of exactly 4096 positions; clip active; wd = 0
    (the counts are asserted in tests/test_step_host.py::test_cases_reach_the_loops_they_are_named_for)
    """
    c = S.make_case(name)
    prev = S.initial_state(c)
    worst = {}
    for k, got in enumerate(_run(c, persistent)):
        for n, v in S.check_step(c, k, prev, got).items():
            n = n.split(".")[0] + ("." + n.split(".")[-2] + "." + n.split(".")[-1] if "mlp" in n else
                                   ".table" if "embedding" in n else "")
            worst[n] = max(worst.get(n, 0.0), v)
        coef = float(got["coef"])
        assert (coef < 1.0) if c.max_norm < 1.0 else (coef == 1.0), (k, coef)
        prev = _state(got)
    for n in sorted(worst):
        _report(f"{name} {'one launch' if persistent else 'seven launches'} {n} error/tolerance", worst[n])
    if c.wd == 0.0:       # a row that no batch touched: nothing may have moved, bit for bit
        for key, rows, n_rows in zip(S.TAB_KEYS, S.touched_rows(c), (c.nu1, c.ni1)):
            idle = np.setdiff1d(np.arange(n_rows), rows)
            assert idle.size > 1
            assert np.array_equal(got["p"][key][idle].view(np.uint32), c.sd[key][idle].view(np.uint32)), key
            assert not got["m"][key][idle].any() and not got["v"][key][idle].any(), key
    else:                 # the padding row decays like every other row (its values are checked above, against a
        for key in S.TAB_KEYS:      # reference that gives row 0 no gradient): every element of it has moved
            assert (got["p"][key][0] != c.sd[key][0]).all(), key


@pytest.mark.parametrize("name", ["tile_boundary", "second_wgrad", "max_batch"])
def test_one_launch_step_is_deterministic(name):
    """two trainers from the same state on the same batches: every combine has a fixed order, so everything is bitwise
    equal"""
    c = S.make_case(name)
    a, b = _run(c, True)[-1], _run(c, True)[-1]
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
    for n in ("loss", "gnorm", "coef"):
        assert np.array_equal(bits(a[n]), bits(b[n])), n
    for grp in ("p", "m", "v"):
        for key in S.ALL_KEYS:
            assert np.array_equal(bits(a[grp][key]), bits(b[grp][key])), (grp, key)


def test_an_id_outside_the_table_is_reported_and_harmless():
    """one item id beyond the table in the second step.  The forward reads row 0 for it and raises the error word, the
    data backward never reads ids, the weight gradients read row 0, the scatter drops it (tower_generic_body.h and the
    scatter of step_persistent.hip: each guards the id before it forms an address).  The step's values are those of the
    reference, which treats the id the same way, and the words behind the tables and their moments keep their sentinel."""
    import copy
    c = copy.copy(S.make_case("tile_boundary"))
    c.batches = [tuple(a.copy() for a in b) for b in c.batches]
    c.batches[1][1][c.B + 7] = c.ni1 + 3          # three rows into the guard region
    m, tr, guards = _trainer(c, True, guard_rows=8)
    prev = S.initial_state(c)
    for k in range(2):
        u, it, g = c.batches[k]
        tr.step(_dev(u), _dev(it), _dev(g), lr=c.lrs[k])
        torch.cuda.synchronize()
        got = _snapshot(m, tr)
        S.check_step(c, k, prev, got)
        prev = _state(got)
        if k == 0:
            tr.check_errors()
    with pytest.raises(RuntimeError, match="outside its embedding table"):
        tr.check_errors()
    for gd in guards:
        assert bool((gd == SENTINEL).all())
