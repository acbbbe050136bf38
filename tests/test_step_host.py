"""CPU proof of tests/step_reference.py: the staged float64 reference of the training step agrees with stock torch
(autograd, clip_grad_norm_, torch.optim.Adam) in float64, every tolerance of every GPU case leaves a factor four over a
plain sequential float32 evaluation (the cap condition), the cases reach the loops they are named for, and the checks
turn red for a wrong value in every stage."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_reference as S  # noqa: E402

F64 = np.float64


def _torch_steps(c):
    """three steps of a plain restatement of the model; yields what step_reference.f64_step returns"""
    dd = torch.float64
    prm = {k: torch.tensor(c.sd[k].astype(F64), requires_grad=True) for k in S.ALL_KEYS}
    opt = torch.optim.Adam([prm[k] for k in S.ALL_KEYS], lr=c.lrs[0], betas=(S.B1, S.B2), eps=S.EPS, weight_decay=c.wd)
    for k, (u, it, g) in enumerate(c.batches):
        for grp in opt.param_groups:
            grp["lr"] = c.lrs[k]
        keep = S.keep_masks(c, k + 1)
        got, leaf = dict(g={}, p={}, m={}, v={}), {}
        for ti, (tower, ids, gen, sfx) in enumerate((("user_tower", u, None, "U"), ("item_tower", it, g, "I"))):
            x = Fn.embedding(torch.from_numpy(ids), prm[f"{tower}.embedding.weight"], padding_idx=0)
            x.retain_grad()
            xin = x if gen is None else torch.cat([x, torch.from_numpy(gen).to(dd)], dim=1)
            h = torch.relu(Fn.linear(xin, prm[f"{tower}.mlp.0.weight"], prm[f"{tower}.mlp.0.bias"]))
            if keep[ti] is not None:
                h = h * torch.from_numpy(keep[ti]).to(dd) * c.scale
            y = Fn.linear(h, prm[f"{tower}.mlp.3.weight"], prm[f"{tower}.mlp.3.bias"])
            out = Fn.normalize(y, dim=-1, eps=1e-12)
            out.retain_grad()
            leaf[sfx] = (x, out)
            got["hid" + sfx], got[sfx] = h.detach().numpy(), out.detach().numpy()
            got["den" + sfx] = y.norm(dim=-1).clamp_min(1e-12).detach().numpy()
        Uo, Io = leaf["U"][1], leaf["I"][1]
        loss = Fn.softplus(-((Uo * Io[:c.B]).sum(-1) - (Uo * Io[c.B:]).sum(-1))).mean()
        opt.zero_grad()
        loss.backward()
        got.update(loss=loss.item(), dU=Uo.grad.numpy().copy(), dI=Io.grad.numpy().copy(),
                   dXu=leaf["U"][0].grad.numpy().copy(), dXi=leaf["I"][0].grad.numpy().copy())
        got["g"] = {key: prm[key].grad.numpy().copy() for key in S.MLP_KEYS}
        got["gtab"] = [prm[key].grad.numpy().copy() for key in S.TAB_KEYS]
        tn = float(torch.nn.utils.clip_grad_norm_([prm[key] for key in S.ALL_KEYS], c.max_norm))
        got.update(gnorm=tn, coef=float(np.linalg.norm(np.concatenate([prm[key].grad.numpy().ravel() for key in S.ALL_KEYS]))
                                        / tn))
        opt.step()
        for key in S.ALL_KEYS:
            got["p"][key] = prm[key].detach().numpy().copy()
            got["m"][key] = opt.state[prm[key]]["exp_avg"].numpy().copy()
            got["v"][key] = opt.state[prm[key]]["exp_avg_sq"].numpy().copy()
        yield got


def _close(name, a, b, rel=1e-11):
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = max(float(np.abs(b).max()), 1e-300)
    assert float(np.abs(a - b).max()) <= rel * scale, (name, float(np.abs(a - b).max()) / scale)


@pytest.mark.parametrize("name", [c[0] for c in S.HOST_CASES])
def test_every_stage_agrees_with_torch_in_float64(name):
    """three steps; duplicate ids, the padding id at user / positive / negative positions, an active clip with wd = 0
    (host_a, dropout masks given) and an inactive one with wd > 0 (host_b)"""
    c = S.make_case(name)
    ids = np.concatenate([np.concatenate(b[:2]) for b in c.batches])
    assert (ids == 0).any() and len(np.unique(c.batches[0][0])) < c.B
    prev = S.initial_state(c)
    for k, want in enumerate(_torch_steps(c)):
        got = S.f64_step(c, k, prev)
        assert (got["coef"] < 1.0) == (c.max_norm < 1.0), (k, got["coef"])
        for n in ("hidU", "hidI", "denU", "denI", "U", "I", "dU", "dI", "loss", "dXu", "dXi", "gnorm", "coef"):
            _close(f"step {k + 1} {n}", got[n], want[n])
        for i in (0, 1):
            _close(f"step {k + 1} table gradient {i}", got["gtab"][i], want["gtab"][i])
            assert not got["gtab"][i][0].any()
        for key in S.MLP_KEYS:
            _close(f"step {k + 1} g {key}", got["g"][key], want["g"][key])
        for key in S.ALL_KEYS:
            for w in "mvp":
                _close(f"step {k + 1} {w} {key}", got[w][key], want[w][key], rel=1e-9 if w == "p" else 1e-11)
            # the float32-constant form the GPU check uses (adam_f64) differs only by the rounding of coef and the betas:
            # 1 - float32(0.999) is 1.3e-5 away from 1e-3, relatively
            gk = got["gtab"][S.TAB_KEYS.index(key)] if key in S.TAB_KEYS else got["g"][key]
            mv = S.stage_adam_mv(prev.p[key], gk, prev.m[key], prev.v[key], got["hyper"], c.wd, np.float32(got["coef"]))
            _close(f"step {k + 1} adam_f64 m {key}", mv.m, want["m"][key], rel=1e-4)
            _close(f"step {k + 1} adam_f64 v {key}", mv.v, want["v"][key], rel=1e-4)
        prev = S.next_state(got)


_F32_RUNS = {}


def _f32_run(name):
    """the sequential float32 trajectory of a case: [(state before, stored values)] per step"""
    if name not in _F32_RUNS:
        c = S.make_case(name)
        prev, steps = S.initial_state(c), []
        for k in range(3):
            got = S.f32_step(c, k, prev)
            steps.append((prev, got))
            prev = S.next_state(got)
        _F32_RUNS[name] = steps
    return _F32_RUNS[name]


@pytest.mark.parametrize("name", S.CASE_NAMES + tuple(c[0] for c in S.HOST_CASES))
def test_cap_condition_sequential_float32_within_a_quarter(name):
    """every tensor of every step: |sequential float32 - float64| <= 1/4 of the tolerance the GPU test uses"""
    c = S.make_case(name)
    worst = {}
    for k, (prev, got) in enumerate(_f32_run(name)):
        for n, v in S.check_step(c, k, prev, got, slack=0.25).items():
            worst[n] = max(worst.get(n, 0.0), v)
        assert (float(got["coef"]) < 1.0) == (c.max_norm < 1.0), (k, got["coef"])
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print(f"[worst] {name} float32 / tolerance: " + ", ".join(f"{n} {v:.3f}" for n, v in top))


def test_cases_reach_the_loops_they_are_named_for():
    sch = {n: S.schedule(S.make_case(n)) for n in S.CASE_NAMES}
    assert (sch["one_row"]["user_tiles"], sch["one_row"]["item_tiles"]) == (1, 1)
    assert (sch["tile_boundary"]["user_tiles"], sch["tile_boundary"]["item_tiles"]) == (2, 3)       # 33 = 32 + 1, 66 = 64 + 2
    assert sch["min_width"]["wgrad_tiles"] == 1 + 1 + 2 + 1 and S.make_case("min_width").d + S.N_GENRES == 34
    assert sch["odd_widths"]["wgrad_tiles"] == (7 * 8 + 8 * 7) + (7 * 9 + 8 * 7) and 240 % 32 and 208 % 32
    assert sch["odd_widths"]["wgrad_tiles"] <= S.NWG
    # (256, 256) is the only supported shape whose weight-gradient tiles outnumber the workgroups
    assert sch["second_wgrad"]["wgrad_tiles"] == 288 and sch["second_wgrad"]["wgrad_second"] == 32
    assert all(sch[n]["wgrad_second"] == 0 for n in S.CASE_NAMES if n != "second_wgrad")
    assert (sch["max_batch"]["user_tiles"], sch["max_batch"]["item_tiles"]) == (64, 128)
    assert sch["full_list"]["longest_list"] == S.SCAT_LIST and sch["max_batch"]["longest_list"] < S.SCAT_LIST
    for k, (u, it, _) in enumerate(S.make_case("max_batch").batches):
        assert set(np.unique(it)) == {1, 2, 3}
        mine = u[u % S.NWG == 1]                   # the list of workgroup 1, in batch order
        assert {1, 257} <= set(mine) and (np.diff(mine) != 0).sum() > 500      # two rows of one owner interleaved
        pos = np.flatnonzero(u % S.NWG == 1)
        same = pos[:, None] % 256 == pos[None, :] % 256
        assert (same & (u[pos][:, None] != u[pos][None, :])).any()             # equal positions mod 256, different rows


def test_check_turns_red_for_a_wrong_value_in_every_stage():
    """one element of one stored tensor moved by 2^-9 of the tensor's largest value (eight caps)"""
    c = S.make_case("host_b")
    prev, got = _f32_run("host_b")[1]
    S.check_step(c, 1, prev, got)
    for n in ("hidU", "denI", "I", "dU", "dI", "loss", "dXu", "dXi", "gnorm", "coef"):
        bad = dict(got)
        a = np.array(got[n], dtype=np.float32, copy=True).reshape(np.shape(got[n]))
        flat = a.reshape(-1)
        i = int(np.argmax(np.abs(flat)))
        flat[i] += np.float32(2.0 ** -9) * np.abs(flat[i])
        bad[n] = a
        with pytest.raises(AssertionError, match="error / tolerance"):
            S.check_step(c, 1, prev, bad)
    for grp in ("g", "m", "v", "p"):
        for key in (S.MLP_KEYS[0], S.TAB_KEYS[1]) if grp != "g" else (S.MLP_KEYS[1], S.MLP_KEYS[6]):
            bad = dict(got)
            bad[grp] = dict(got[grp])
            a = got[grp][key].copy()
            i = np.unravel_index(int(np.argmax(np.abs(a))), a.shape)
            a[i] += np.float32(2.0 ** -9) * np.abs(a[i])
            bad[grp][key] = a
            with pytest.raises(AssertionError, match="error / tolerance"):
                S.check_step(c, 1, prev, bad)


def test_persistent_step_supported_shapes():
    """B in [1, 2048], widths multiples of 16 from 16 to 256 (a host function of the library: no GPU needed)"""
    from recommendit_amd import _lib as L
    ok = L.lib().rihip_bpr_step_persistent_supported
    assert [ok(B, 32, 32) for B in (1, 2048)] == [1, 1] and [ok(B, 32, 32) for B in (0, 2049)] == [0, 0]
    for w in (16, 256):
        assert ok(64, w, 32) == 1 and ok(64, 32, w) == 1
    for w in (8, 24, 272):
        assert ok(64, w, 32) == 0 and ok(64, 32, w) == 0
