"""Sampled BPR with K negatives per positive on the GPU: rihip_bpr_multi_loss against the float64 reference and its
invariants, rihip_sample_negatives_multi against its integer restatement, the K-negative training step stage by stage, and
the dataset / EmbeddingTrainer wiring.  References and tolerances: tests/multineg_reference.py (a tolerance is a
function of the inputs and the header's operation order; a check fails when error / tolerance exceeds 1).  Run with -s
for the worst error / tolerance per tensor."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multineg_reference as M  # noqa: E402
import step_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu
F32, I64 = np.float32, np.int64
GRID_CAP = 1024          # workgroups of the loss launch; each holds 4 waves of 64 / (d / 4) rows in the 16-byte form


def _L():
    from recommendit_amd import _lib as L
    return L, L.lib(), torch.device("cuda"), torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(x):
    return x.detach().cpu().numpy().copy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _report(name, value):
    print(f"[worst] {name}: {value:.3f}")


# ------------------------------------------------------------------------------------------------------------------- #
# Loss kernel                                                                                                          #
# ------------------------------------------------------------------------------------------------------------------- #
def _rows(rng, shape, unit=True):
    x = rng.standard_normal(shape)
    if unit:
        x /= np.linalg.norm(x, axis=-1, keepdims=True)
    return x.astype(F32)


def _inputs(B, K, d, seed, unit=True):
    """every N_k block holds data of its own, so a k-major indexing slip is an O(1) error"""
    rng = np.random.default_rng(seed)
    return _rows(rng, (B, d), unit), _rows(rng, (B, d), unit), _rows(rng, (K, B, d), unit)


def _multi(U, P, N, with_loss=True, offset=0, entry="multi"):
    """run the entry; offset: every device array is a view `offset` floats into a larger buffer.  Returns loss (or None),
    dU, dP, dN and the double partials."""
    L, lib, dev, st = _L()
    K, B, d = N.shape

    def put(a):
        buf = torch.full((a.size + offset + 4,), 9.0, dtype=torch.float32, device=dev)
        v = buf[offset:offset + a.size]
        v.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
        return buf, v
    bufs = [put(a) for a in (U, P, N, np.zeros_like(U), np.zeros_like(P), np.zeros_like(N))]
    for _, v in bufs[3:]:
        v.fill_(float("nan"))
    (u, p, n, du, dp, dn) = (v for _, v in bufs)
    ws = torch.full((1024,), -1.0, dtype=torch.float64, device=dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    lp = loss.data_ptr() if with_loss else None
    if entry == "multi":
        L.check(lib.rihip_bpr_multi_loss(u.data_ptr(), p.data_ptr(), n.data_ptr(), B, K, d, lp, du.data_ptr(), dp.data_ptr(),
                                         dn.data_ptr(), ws.data_ptr(), st), "bpr_multi_loss")
        nparts = lib.rihip_bpr_multi_nparts(B, K)
    else:
        assert K == 1
        L.check(lib.rihip_bpr_pair_loss(u.data_ptr(), p.data_ptr(), n.data_ptr(), B, d, lp, du.data_ptr(), dp.data_ptr(),
                                        dn.data_ptr(), ws.data_ptr(), st), "bpr_pair_loss")
        nparts = lib.rihip_bpr_pair_nparts(B)
    torch.cuda.synchronize()
    for buf, v in bufs:          # nothing outside the views was written
        assert bool((buf[:offset] == 9.0).all()) and bool((buf[offset + v.numel():] == 9.0).all())
    return (float(loss.item()) if with_loss else None, _np(du).reshape(B, d), _np(dp).reshape(B, d),
            _np(dn).reshape(K, B, d), _np(ws)[:nparts])


def _check_against_f64(tag, U, P, N, **kw):
    loss, dU, dP, dN, _ = _multi(U, P, N, **kw)
    ref = M.loss_and_grads_f64(U, P, N)
    r = dict(loss=S._ratio(loss, ref.loss, ref.e_loss), dU=S._ratio(dU, ref.dU, ref.e_dU),
             dP=S._ratio(dP, ref.dP, ref.e_dP), dN=S._ratio(dN, ref.dN, ref.e_dN))
    for n, v in r.items():
        _report(f"{tag} {n} error/tolerance", v)
    assert all(v <= 1.0 for v in r.values()), r
    return ref


@pytest.mark.parametrize("B,K,d", [(1, 1, 32), (5, 2, 64), (67, 3, 128), (300, 8, 128), (33, 17, 64), (64, 4, 16),
                                   (70, 5, 48), (9, 2, 144), (40, 3, 256), (6, 2, 7)])
def test_loss_and_gradients_against_f64(B, K, d):
    """unit-norm rows.  d = 32 / 64 / 128: the tuned 16-byte kernels; 16, 48, 144, 256: the 16-byte kernel with a runtime
    width (partial lane groups); 7: the scalar kernel.  K = 17 and 5: a last chunk of the k loop that is not full."""
    _check_against_f64(f"B={B} K={K} d={d}", *_inputs(B, K, d, seed=B * 1000 + K * 10 + d))


def test_misaligned_pointers_take_the_scalar_path():
    """every array starts one float into its buffer: d = 64 runs the scalar kernel, and nothing outside is written"""
    _check_against_f64("misaligned d=64", *_inputs(37, 3, 64, seed=2), offset=1)


def test_more_than_one_trip_of_the_grid_stride_loop():
    """d = 32 holds 8 rows per wave, 32 per workgroup: beyond GRID_CAP * 32 rows the first workgroups take a second trip,
    and the last one of those is a partial wave"""
    B = GRID_CAP * 32 + 40
    assert _L()[1].rihip_bpr_multi_nparts(B, 2) == GRID_CAP
    _check_against_f64(f"grid-stride B={B}", *_inputs(B, 2, 32, seed=4))


def test_large_scores_of_both_signs():
    """unnormalised rows scaled so that |z| reaches 40 with both signs: both sigma branches and the softplus limits"""
    B, K, d = 64, 3, 64
    U, P, N = _inputs(B, K, d, seed=6, unit=True)
    scale = np.linspace(0.5, 6.5, B).astype(F32)[:, None]
    U, P = U * scale, P * scale
    N = N * scale[None]
    P[::2] = U[::2]                   # z = +|u|^2 - u.n: up to +42
    N[0, 1::2] = U[1::2]              # z = u.p - |u|^2: down to -42
    ref = _check_against_f64("large |z|", U, P, N)
    assert ref.z.max() > 38 and ref.z.min() < -38 and (np.abs(ref.z) < 1).any()


@pytest.mark.parametrize("d", [32, 64, 128, 48])
@pytest.mark.parametrize("B", [1, 300])
def test_k1_is_the_pair_loss_bit_for_bit(B, d):
    U, P, N = _inputs(B, 1, d, seed=B + d)
    for with_loss in (True, False):
        a = _multi(U, P, N, with_loss=with_loss)
        b = _multi(U, P, N, with_loss=with_loss, entry="pair")
        assert _L()[1].rihip_bpr_multi_nparts(B, 1) == _L()[1].rihip_bpr_pair_nparts(B)
        if with_loss:
            assert np.array_equal(_bits(F32(a[0])), _bits(F32(b[0])))
        for x, y, name in zip(a[1:], b[1:], ("dU", "dP", "dN", "partials")):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), name


@pytest.mark.parametrize("B,K,d", [(300, 4, 64), (77, 3, 20), (GRID_CAP * 8 + 3, 2, 128)])
def test_partials_and_determinism(B, K, d):
    """loss = NULL leaves the double partials; their host sum times 1 / (B K) is the returned loss to the last float32
    rounding; two calls are bitwise equal"""
    U, P, N = _inputs(B, K, d, seed=9)
    a = _multi(U, P, N, with_loss=True)
    b = _multi(U, P, N, with_loss=False)
    c = _multi(U, P, N, with_loss=True)
    host = F32(b[4].sum() / (B * K))
    assert abs(float(host) - a[0]) <= float(np.spacing(F32(a[0])))
    assert np.array_equal(_bits(F32(a[0])), _bits(F32(c[0])))
    for x, y, z in zip(a[1:], b[1:], c[1:]):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(z).view(np.uint8))


def test_loss_entry_refuses_bad_arguments():
    L, lib, dev, st = _L()
    x = [torch.zeros(64, dtype=torch.float32, device=dev) for _ in range(6)]      # B = 2, K = 2, d = 8
    ws = torch.zeros(1024, dtype=torch.float64, device=dev)
    p = [t.data_ptr() for t in x]
    good = [p[0], p[1], p[2], 2, 2, 8, None, p[3], p[4], p[5], ws.data_ptr(), st]

    def refused(i, v, what):
        a = list(good)
        a[i] = v
        assert lib.rihip_bpr_multi_loss(*a) == 1, what          # RIHIP_ERR_ARG
        msg = lib.rihip_last_error().decode()
        assert "bpr_multi_loss" in msg and len(msg) > 20, (what, msg)
    for i, name in ((0, "U"), (1, "P"), (2, "N"), (7, "dU"), (8, "dP"), (9, "dN"), (10, "workspace")):
        refused(i, None, name + " = NULL")
    refused(3, 0, "B = 0")
    refused(3, -1, "B < 0")
    refused(4, 0, "K = 0")
    refused(5, 0, "d = 0")
    refused(3, (2 ** 31 - 1) // 3 + 1, "(1 + K) B = 2^31")
    refused(4, 2 ** 31 - 1, "(1 + K) overflows int")
    assert lib.rihip_bpr_multi_loss(*good) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- #
# Sampler                                                                                                              #
# ------------------------------------------------------------------------------------------------------------------- #
def _sample(users, K, cat, prob, alias, rated, stride, seed, max_attempts, entry="multi"):
    L, lib, dev, st = _L()
    ud, cd = _dev(users), _dev(cat)
    rd = _dev(rated if rated.shape[0] else np.zeros(1, I64))
    n = users.shape[0]
    neg = torch.full((K * n + 3,), -99, dtype=torch.int64, device=dev)
    gu = torch.zeros(1, dtype=torch.int32, device=dev)
    if entry == "multi":
        pd_ = None if prob is None else _dev(np.asarray(prob, np.uint32).view(np.int32))
        ad = None if alias is None else _dev(np.asarray(alias, np.int32))
        L.check(lib.rihip_sample_negatives_multi(ud.data_ptr(), n, K, cd.data_ptr(), cat.shape[0],
                                                 None if pd_ is None else pd_.data_ptr(),
                                                 None if ad is None else ad.data_ptr(), rd.data_ptr(), rated.shape[0],
                                                 stride, seed, max_attempts, neg.data_ptr(), gu.data_ptr(), st), "sample")
    else:
        L.check(lib.rihip_sample_negatives(ud.data_ptr(), n, cd.data_ptr(), cat.shape[0], rd.data_ptr(), rated.shape[0],
                                           stride, seed, max_attempts, neg.data_ptr(), gu.data_ptr(), st), "sample")
    out = _np(neg)
    assert (out[K * n:] == -99).all()
    return out[:K * n], int(gu.item())


def _world(n, nc, rng):
    """users 1 .. 40 over a catalogue of nc non-contiguous ids: user 1 rated all but two items, user 2 everything, the
    others a tenth; (users, catalog, rated keys, key stride)"""
    stride = 3 * nc + 7
    cat = np.sort(rng.permutation(3 * nc)[:nc] + 1).astype(I64)
    users = rng.integers(1, 41, size=n).astype(I64)
    users[:min(n, 3)] = [1, 2, 3][:min(n, 3)]
    keys = [1 * stride + cat[2:], 2 * stride + cat]
    for u in range(3, 41):
        keys.append(u * stride + cat[rng.random(nc) < 0.1])
    return users, cat, np.unique(np.concatenate(keys)).astype(I64), stride


def _table(nc, rng, kind):
    from recommendit_amd.negative_sampling import alias_table
    if kind == "uniform":
        return None, None
    w = rng.random(nc) ** 3
    w[::3] = 0.0
    if not w.any():
        w[0] = 1.0
    prob, alias = alias_table(w)
    if kind == "out_of_range":          # entries outside [0, nc) are read as "the column itself"
        alias = alias.copy()
        alias[::2] = nc + 5
        alias[1::4] = -1
    return prob, alias


@pytest.mark.parametrize("nc", [1, 7, 3706])
@pytest.mark.parametrize("n", [1, 1000, 3001])
@pytest.mark.parametrize("kind", ["uniform", "weighted", "out_of_range"])
def test_sampler_equals_the_restatement(n, nc, kind):
    """neg_out and gave_up, for K in {1, 3, 8} and max_attempts in {1, 2, 1000}, with an empty rated set and with users who
    rated all but two items (many attempts) and everything (they give up and keep the last pick)"""
    rng = np.random.default_rng(n * 10 + nc)
    users, cat, rated, stride = _world(n, nc, rng)
    prob, alias = _table(nc, rng, kind)
    seed = 0x1234_5678_9ABC_DEF1 + n + nc
    for K, max_attempts, rk in ((1, 1000, rated), (3, 2, rated), (8, 1000, rated), (3, 1, rated), (3, 1000, np.zeros(0, I64))):
        got, gu = _sample(users, K, cat, prob, alias, rk, stride, seed, max_attempts)
        ref, ref_gu = M.sample_negatives_multi_np(users, K, cat, prob, alias, rk, stride, seed, max_attempts)
        np.testing.assert_array_equal(got, ref)
        assert gu == ref_gu, (K, max_attempts)
        hit = np.isin(np.tile(users, K) * stride + got, rk)
        assert gu == int(hit.sum())
        if rk.shape[0] == 0:
            assert gu == 0
        elif n >= 2:                     # user 2 rated everything: each of its K slots gives up
            assert gu >= K * int((users == 2).sum())
    if kind == "weighted":               # a weight of zero is never drawn, rated set or not
        w0 = cat[::3]
        got, _ = _sample(users, 8, cat, prob, alias, np.zeros(0, I64), stride, seed, 1000)
        assert nc == 1 or not np.isin(got, w0).any()


@pytest.mark.parametrize("max_attempts", [1, 1000])
def test_sampler_k1_without_a_table_is_the_existing_entry(max_attempts):
    rng = np.random.default_rng(77)
    users, cat, rated, stride = _world(3001, 3706, rng)
    a = _sample(users, 1, cat, None, None, rated, stride, 42, max_attempts)
    b = _sample(users, 1, cat, None, None, rated, stride, 42, max_attempts, entry="single")
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1] == b[1]


def test_sampler_entry_refuses_bad_arguments():
    L, lib, dev, st = _L()
    x = torch.ones(8, dtype=torch.int64, device=dev)
    t = torch.zeros(8, dtype=torch.int32, device=dev)
    p = x.data_ptr()
    good = [p, 4, 2, p, 8, None, None, p, 8, 100, 1, 10, p, None, st]
    for i, v, what in ((0, None, "users"), (3, None, "catalog"), (7, None, "rated"), (12, None, "neg_out"), (1, -1, "n < 0"),
                       (2, 0, "K = 0"), (2, -2, "K < 0"), (4, 0, "n_catalog = 0"), (4, 2 ** 32, "n_catalog = 2^32"),
                       (8, -1, "n_rated < 0"), (9, 0, "key_stride = 0"), (11, 0, "max_attempts = 0"),
                       (5, t.data_ptr(), "alias_prob alone"), (6, t.data_ptr(), "alias_idx alone")):
        a = list(good)
        a[i] = v
        assert lib.rihip_sample_negatives_multi(*a) == 1, what
        msg = lib.rihip_last_error().decode()
        assert "sample_negatives_multi" in msg, (what, msg)
    assert lib.rihip_sample_negatives_multi(*good) == 0
    a = list(good)
    a[1] = 0                                                        # an empty batch is fine and writes nothing
    assert lib.rihip_sample_negatives_multi(*a) == 0
    torch.cuda.synchronize()
    assert bool((x == 1).all())


# ------------------------------------------------------------------------------------------------------------------- #
# Trainer                                                                                                              #
# ------------------------------------------------------------------------------------------------------------------- #
def _trainer(c, **kw):
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    m = TwoTowerModel(S.NU, S.NI, embed_dim=c.d, hidden_dim=c.H, dropout=kw.pop("dropout", c.p))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c.sd.items()})
    m = m.cuda()
    m.train(True)
    kw.setdefault("n_negatives", c.K)
    tr = HipBPRTrainer(m, c.B, lr=c.lrs[0], weight_decay=c.wd, betas=(S.B1, S.B2), eps=S.EPS, max_norm=c.max_norm,
                       loss_mode="sampled", table_opt="sparse" if c.sparse else "dense", seed=c.seed, **kw)
    return m, tr


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


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_every_stage_of_three_k_negative_steps(name):
    """
    k3_dense    K = 3, B = 96,  (d, H) = (32, 64),   dense;  wd > 0, clip active
    k2_dense    K = 2, B = 70,  (48, 96),            dense;  the runtime-width loss kernel; wd = 0
    k4_sparse   K = 4, B = 128, (64, 128),           row-sparse tables: only the rows of the batches move, row 0 never
    dropout 0; the learning rate changes before step 2; each stage is evaluated in float64 on what the previous stage
    stored (tests/multineg_reference.check_step)
    """
    c = M.make_case(name)
    m, tr = _trainer(c)
    assert tr.nI == (1 + c.K) * c.B and not tr.persistent
    prev = S.initial_state(c)
    worst = {}
    for k, (u, it, g) in enumerate(c.batches):
        tr.step(_dev(u), _dev(it), _dev(g), lr=c.lrs[k])
        torch.cuda.synchronize()
        assert int(tr.step_dev.item()) == k + 2
        got = _snapshot(m, tr)
        for n, v in M.check_step(c, k, prev, got).items():
            n = n.split(".")[0] + (".table" if "embedding" in n else ".mlp" if "mlp" in n else "")
            worst[n] = max(worst.get(n, 0.0), v)
        coef = float(got["coef"])
        assert (coef < 1.0) if c.max_norm < 1.0 else (coef == 1.0), (k, coef)
        prev = S.next_state(got)
    tr.check_errors()
    for n in sorted(worst):
        _report(f"{name} {n} error/tolerance", worst[n])
    if c.sparse:
        for key, ids in zip(S.TAB_KEYS, (np.concatenate([b[0] for b in c.batches]), np.concatenate([b[1] for b in c.batches]))):
            idle = np.setdiff1d(np.arange(c.sd[key].shape[0]), np.unique(ids))
            assert idle.size > 50 and idle[0] == 0
            assert np.array_equal(_bits(got["p"][key][idle]), _bits(c.sd[key][idle])), key
            assert not got["m"][key][idle].any() and not got["v"][key][idle].any(), key
            moved = np.unique(ids)
            assert (got["p"][key][moved] != c.sd[key][moved]).any(axis=1).all(), key


def _three_steps(c, batches, **kw):
    m, tr = _trainer(c, **kw)
    losses = []
    for k, (u, it, g) in enumerate(batches):
        losses.append(tr.step(_dev(u), _dev(it), _dev(g), lr=c.lrs[k % 3]).clone())
    torch.cuda.synchronize()
    tr.check_errors()
    got = _snapshot(m, tr)
    return [_np(x) for x in losses], got


def _assert_same_state(a, b):
    for la, lb in zip(a[0], b[0]):
        assert np.array_equal(_bits(la), _bits(lb))
    for grp in ("p", "m", "v"):
        for key in S.ALL_KEYS:
            assert np.array_equal(_bits(a[1][grp][key]), _bits(b[1][grp][key])), (grp, key)


@pytest.mark.parametrize("name", ["tile_boundary", "k4_sparse"], ids=["dense", "sparse"])
def test_one_negative_is_the_step_it_was(name):
    """HipBPRTrainer(n_negatives=1) against the default-constructed trainer over three steps, dropout on: parameters,
    moments and losses bit for bit"""
    from recommendit_amd.trainer import HipBPRTrainer
    if name == "tile_boundary":
        c = S.make_case(name)
        c = type(c)(**{**vars(c), "sparse": False, "K": 1})
        batches = c.batches
    else:
        c = M.make_case(name)
        batches = [(u, it[:2 * c.B], g[:2 * c.B]) for u, it, g in c.batches]
    a = _three_steps(c, batches, dropout=0.5, n_negatives=1)
    import inspect
    assert inspect.signature(HipBPRTrainer.__init__).parameters["n_negatives"].default == 1
    # the default-constructed trainer: the keyword is not passed at all
    from recommendit_amd import TwoTowerModel
    m2 = TwoTowerModel(S.NU, S.NI, embed_dim=c.d, hidden_dim=c.H, dropout=0.5)
    m2.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c.sd.items()})
    m2 = m2.cuda()
    m2.train(True)
    tr2 = HipBPRTrainer(m2, c.B, lr=c.lrs[0], weight_decay=c.wd, betas=(S.B1, S.B2), eps=S.EPS, max_norm=c.max_norm,
                        loss_mode="sampled", table_opt="sparse" if c.sparse else "dense", seed=c.seed)
    assert tr2.nI == 2 * c.B and tr2.n_negatives == 1
    losses = [tr2.step(_dev(u), _dev(it), _dev(g), lr=c.lrs[k]).clone() for k, (u, it, g) in enumerate(batches)]
    torch.cuda.synchronize()
    _assert_same_state(a, ([_np(x) for x in losses], _snapshot(m2, tr2)))


def test_graph_replay_equals_eager():
    """K = 2, four steps, dropout on: the captured step replays the K-negative loss launch bit for bit"""
    c = M.make_case("k2_dense")
    batches = list(c.batches) + [c.batches[0]]
    a = _three_steps(c, batches, dropout=0.5, use_graph=False)
    b = _three_steps(c, batches, dropout=0.5, use_graph=True)
    _assert_same_state(a, b)


def test_trainer_refusals_on_the_device():
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    c = M.make_case("k3_dense")
    m, tr = _trainer(c)
    u, it, g = c.batches[0]
    with pytest.raises(ValueError, match=str((1 + c.K) * c.B)):
        tr.step(_dev(u), _dev(it[:2 * c.B]), _dev(g[:2 * c.B]))
    mk = lambda: TwoTowerModel(S.NU, S.NI, embed_dim=32, hidden_dim=64).cuda()
    with pytest.raises(ValueError, match="persistent"):
        HipBPRTrainer(mk(), 64, n_negatives=2, persistent=True)
    with pytest.raises(ValueError, match="single-GPU for now"):
        HipBPRTrainer(mk(), 64, n_negatives=2, table_opt="sparse", distributed=True)
    with pytest.raises(ValueError, match="loss_mode='sampled'"):
        HipBPRTrainer(mk(), 64, n_negatives=2, loss_mode="inbatch")


# ------------------------------------------------------------------------------------------------------------------- #
# Dataset and EmbeddingTrainer                                                                                         #
# ------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def small_world():
    from recommendit_amd.synthetic import ml1m_like
    from recommendit_amd.train_embeddings import build_item_genre_dict
    ratings, movies, gm = ml1m_like(n_users=300, n_item_ids=260, n_catalog=240, n_ratings=20000, seed=2)
    return ratings, movies, gm, build_item_genre_dict(movies)


def _ds(world):
    from recommendit_amd.train_embeddings import UserItemDataset
    ratings, movies, gm, gd = world
    return UserItemDataset(ratings, gd, sorted(movies["item_id"].tolist()))


def test_epoch_batches_with_three_negatives(small_world):
    ratings, movies, gm, _ = small_world
    ds = _ds(small_world)
    gen = torch.Generator(device="cuda"); gen.manual_seed(0)
    rated = set((ratings["user_id"] * 10000 + ratings["item_id"]).tolist())
    catalog = set(movies["item_id"].tolist())
    B, K, seen = 512, 3, 0
    for u, items, genres in ds.epoch_batches(B, gen, n_negatives=K):
        assert u.shape == (B,) and items.shape == ((1 + K) * B,) and genres.shape == ((1 + K) * B, 18)
        un, it = _np(u), _np(items)
        assert set(it[B:].tolist()) <= catalog
        for k in range(K):               # negative k of sample i sits at (1 + k) B + i and is not in user i's rated set
            assert all(int(a) * 10000 + int(b) not in rated for a, b in zip(un, it[(1 + k) * B:(2 + k) * B]))
        assert all(int(a) * 10000 + int(b) in rated for a, b in zip(un, it[:B]))
        np.testing.assert_array_equal(_np(genres), gm[it])
        seen += 1
    assert seen == len(ds) // B and ds.negatives_given_up() == 0


def test_default_sampling_is_the_existing_entry_at_the_derived_seed(small_world):
    """sample_negatives at its defaults against a direct rihip_sample_negatives call at the seed the dataset derives:
    the default epoch draws what it drew before the K-negative path existed"""
    L, lib, dev, st = _L()
    ds = _ds(small_world)
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    u = torch.from_numpy(ds.user_ids[:777].copy()).cuda()
    for call in (1, 2):
        got = ds.sample_negatives(u, gen)
        assert got.shape == u.shape
        seed = (gen.initial_seed() * 0x9E3779B97F4A7C15 + call) & ((1 << 63) - 1)
        ref = torch.empty_like(u)
        L.check(lib.rihip_sample_negatives(u.data_ptr(), u.numel(), ds.d_catalog.data_ptr(), ds.d_catalog.numel(),
                                           ds.d_rated.data_ptr(), ds.d_rated.numel(), ds.M, seed, 1000, ref.data_ptr(), None,
                                           st), "sample")
        assert torch.equal(got, ref)
    # ... and the default epoch_batches is positives || those negatives
    ds2, ds3 = _ds(small_world), _ds(small_world)
    g2 = torch.Generator(device="cuda"); g2.manual_seed(5)
    g3 = torch.Generator(device="cuda"); g3.manual_seed(5)
    a = [tuple(_np(x) for x in b) for b in ds2.epoch_batches(1024, g2)]
    b = [tuple(_np(x) for x in b) for b in ds3.epoch_batches(1024, g3, n_negatives=1)]
    assert len(a) == len(b) > 2 and all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))
    users0 = a[0][0]
    seed = (g2.initial_seed() * 0x9E3779B97F4A7C15 + 1) & ((1 << 63) - 1)
    ref, _ = M.sample_negatives_multi_np(users0, 1, ds2.all_items_array, None, None, _np(ds2.d_rated), ds2.M, seed, 1000)
    assert np.array_equal(a[0][1][1024:], ref)


def test_weighted_dataset_sampling_equals_the_restatement(small_world):
    ds = _ds(small_world)
    ds.set_negative_sampling(alpha=0.75)
    prob, alias = ds._alias_host
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    u = torch.from_numpy(ds.user_ids[:1500].copy()).cuda()
    for call, K in ((1, 1), (2, 4)):
        got = _np(ds.sample_negatives(u, gen, n_negatives=K))
        seed = (gen.initial_seed() * 0x9E3779B97F4A7C15 + call) & ((1 << 63) - 1)
        ref, gu = M.sample_negatives_multi_np(_np(u), K, ds.all_items_array, prob, alias, _np(ds.d_rated), ds.M, seed, 1000)
        assert gu == 0 and np.array_equal(got, ref)
    ds.set_negative_sampling()           # back to uniform: the existing entry again
    got = _np(ds.sample_negatives(u, gen))
    seed = (gen.initial_seed() * 0x9E3779B97F4A7C15 + 3) & ((1 << 63) - 1)
    ref, _ = M.sample_negatives_multi_np(_np(u), 1, ds.all_items_array, None, None, _np(ds.d_rated), ds.M, seed, 1000)
    assert np.array_equal(got, ref)


def test_embedding_trainer_with_weighted_multi_negatives(small_world, tmp_path):
    """it runs, records a finite loss, leaves the device error word clean and saves; no quality assertion"""
    from recommendit_amd.train_embeddings import EmbeddingTrainer
    ratings, movies, _, _ = small_world
    out = tmp_path / "tt.pt"
    tr = EmbeddingTrainer(model_output_path=str(out), embed_dim=32, epochs=1, batch_size=512, learning_rate=5e-3,
                          dropout=0.1, seed=0, n_negatives=2, negative_alpha=0.75)
    tr.train(ratings, movies)
    assert len(tr.history) == 1 and np.isfinite(tr.history[0]["loss"]) and 0.0 < tr.history[0]["loss"] < 1.0
    assert tr.trainer.n_negatives == 2 and tr.trainer.nI == 3 * 512
    tr.trainer.check_errors()
    assert out.exists() and out.stat().st_size > 0
