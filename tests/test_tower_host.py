"""CPU-only checks of the tower-loop tests' own infrastructure (tests/tower_reference.py):

  * the exact reference equals oracle/two_tower_np.py on the same inputs, and torch autograd of the model's definition
    in f64 on a small case;
  * every case the GPU tests build satisfies the 2^24 exactness condition;
  * the schedule restatement reproduces the "first B with a second iteration" of every kernel and shows, for every case,
    the loop region it reaches;
  * every comparison helper goes red for each defect a multi-tile loop can have, injected into an otherwise correct
    result.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tower_reference as R  # noqa: E402

from oracle import two_tower_np as O  # noqa: E402

F32, F64 = np.float32, np.float64


# --------------------------------------------------------------------------------------------------------------------
# the reference against the oracle and against autograd
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("d,H,item", [(128, 128, True), (64, 128, False), (48, 96, True)])
def test_forward_reference_equals_the_oracle(d, H, item, train):
    B = 777
    c = R.forward_case(d, H, item, B)
    ref = R.forward_rows(c, np.arange(B), train)
    p = O.TowerParams(*(v.astype(F32) for v in (c.table, c.W1, c.b1, c.W2, c.b2)))
    keep = O.dropout_keep_mask(R.seed_eff(c), c.row0, B, H, c.p) if train else None
    out, cache = O.tower_forward(p, c.ids, None if c.genres is None else c.genres.astype(F32), keep, c.p if train else 0.0)
    assert np.array_equal(cache["h"], ref.hid)
    assert np.array_equal(cache["y"].astype(F64), ref.y)
    R.check_rows_exact("hid", cache["h"], ref.hid)
    R.check_out_denom(out, cache["denom"][:, 0], ref)               # numpy f32: correctly rounded sqrt and division
    assert ref.exact.any() and np.array_equal(out[ref.exact].astype(F64), ref.out[ref.exact])


def test_keep_rows_is_the_oracle_mask_with_the_step_clock_folded_in():
    c = R.forward_case(32, 64, False, 500)
    rows = np.r_[np.arange(64, 96), np.arange(10, 20), np.arange(300, 364)]
    full = O.dropout_keep_mask(R.seed_eff(c), c.row0, 500, 64, c.p)
    assert np.array_equal(R.keep_rows(c, rows), full[rows])
    sm = int(O.splitmix64(np.array([c.seed], dtype=np.uint64))[0])
    # the kernel: seed_mul = splitmix64(splitmix64(seed) + step); the oracle hashes its seed argument once
    assert int(O.splitmix64(np.array([R.seed_eff(c)], dtype=np.uint64))[0]) == \
        int(O.splitmix64(np.array([(sm + c.step) % (1 << 64)], dtype=np.uint64))[0])
    assert not np.array_equal(full, O.dropout_keep_mask(c.seed, c.row0, 500, 64, c.p))
    assert 0.45 < full.mean() < 0.55


@pytest.mark.parametrize("d,H,item", [(128, 128, True), (32, 64, False), (144, 80, True)])
def test_backward_reference_equals_the_oracle(d, H, item):
    B = 1500
    c = R.backward_case(d, H, item, B)
    p = O.TowerParams(c.table.astype(F32), c.W1.astype(F32), np.zeros(H, F32), c.W2.astype(F32), np.zeros(d, F32))
    cache = dict(out=c.out.astype(F32), denom=c.denom.astype(F32)[:, None], h=c.hid.astype(F32), x=c.x.astype(F32),
                 keep=np.ones((B, H), dtype=bool), dropout_p=0.5)
    got = O.tower_backward(p, cache, c.gout.astype(F32))
    assert c.clamp.sum() > 10
    R.check_rows_exact("dX", got[0], c.ref.dX)
    R.check_grads(got[1:], R.weight_grads(c.ref, c.hid, c.x))
    dX = np.rint(c.ref.dX)
    assert np.array_equal(O.embedding_scatter_add(c.n_rows, c.ids, dX.astype(F32)).astype(F64),
                          R.scatter_reference(0.0, c.n_rows, c.ids, dX))


def test_references_equal_torch_autograd_in_f64():
    """the model's definition (embedding -> cat genres -> Linear -> ReLU -> Dropout -> Linear -> F.normalize) in torch
    f64 with the mask fixed, loss = <out, G>"""
    d, H, B = 32, 64, 70
    c = R.forward_case(d, H, True, B)
    fr = R.forward_rows(c, np.arange(B), True)
    rng = np.random.default_rng(3)
    G = rng.standard_normal((B, d))
    tt = lambda a: torch.tensor(np.asarray(a, dtype=F64), requires_grad=True)
    table, W1, b1, W2, b2 = (tt(v) for v in (c.table, c.W1, c.b1, c.W2, c.b2))
    x = torch.cat([torch.nn.functional.embedding(torch.from_numpy(c.ids), table, padding_idx=0), torch.from_numpy(c.genres)], 1)
    h = torch.relu(x @ W1.T + b1) * torch.from_numpy(R.keep_rows(c, np.arange(B)).astype(F64)) * 2.0
    out = torch.nn.functional.normalize(h @ W2.T + b2, dim=-1, eps=1e-12)
    (out * torch.from_numpy(G)).sum().backward()
    np.testing.assert_allclose(out.detach().numpy(), fr.out, rtol=1e-13, atol=0)
    br = R.backward_rows(fr.x, c.W1, c.W2, G, fr.out, fr.denom, fr.hid, 2.0, d)
    for got, want in zip((W1.grad, b1.grad, W2.grad, b2.grad), R.weight_grads(br, fr.hid, fr.x)):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(table.grad.numpy(), R.scatter_reference(0.0, c.n_rows, c.ids, br.dX), rtol=1e-11, atol=1e-12)


# --------------------------------------------------------------------------------------------------------------------
# exactness of every case; schedules
# --------------------------------------------------------------------------------------------------------------------
def test_every_forward_case_satisfies_the_exactness_condition():
    seen = set()
    for kind, d, H, item, B in R.forward_cases() + [("pair", d, H, False, 5000) for d, H in ((64, 128), (32, 64), (128, 128))]:
        if (d, H, item, B) in seen:
            continue
        seen.add((d, H, item, B))
        c = R.forward_case(d, H, item, B)              # raises when a sum of |terms| reaches 2^24
        assert max(c.abs_sums.values()) < R.LIMIT
        assert {0, 1, c.n_rows - 1} <= set(c.ids.tolist()) and len(set(c.ids.tolist())) < B


def test_the_builders_refuse_a_case_that_would_lose_exactness(monkeypatch):
    monkeypatch.setattr(R, "LIMIT", 1000.0)
    with pytest.raises(AssertionError, match="2\\^24"):
        R.forward_case.__wrapped__(32, 64, True, 300)
    with pytest.raises(AssertionError, match="2\\^24"):
        R.backward_case.__wrapped__(32, 64, True, 3000)


@pytest.mark.parametrize("kind,d,H,item,B", R.backward_cases() + [("bwd64", d, H, False, 5000) for d, H in ((64, 128), (32, 64), (128, 128))])
def test_every_backward_case_satisfies_the_exactness_condition(kind, d, H, item, B):
    c = R.backward_case(d, H, item, B)
    assert max(c.abs_sums.values()) / R.GRID < R.LIMIT and c.abs_sums["dh"] <= 8.0
    assert {0, c.n_rows - 1} <= set(c.ids.tolist()) and c.clamp.any()


def test_first_batch_size_with_a_second_iteration():
    """the table of the launch code: rows per pass of the whole grid"""
    want = dict(fwd2=65536, bwd_data=65536, wgrad=8192, bwd3=8192, fwd64=32768, bwd64=16384, gen_fwd=32768,
                gen_bwd_data=32768)
    for kind, rows in want.items():
        assert R.Schedule(kind, rows).pass_rows == rows
        assert R.Schedule(kind, rows).coverage()["max_iterations"] == 1, kind
        assert R.Schedule(kind, rows + 1).coverage()["max_iterations"] == 2, kind
    # generic weight gradient: contiguous batch splits, want = ceil(2 NCU / ceil(output tiles / 4)) <= min(ntiles, NCU)
    assert R.gen_wgrad_split(32 * 128, 48, 96, False) == (1, 128)          # 14 output tiles -> 4 groups -> 128 splits
    assert R.gen_wgrad_split(32 * 128 + 1, 48, 96, False)[0] == 2
    s = R.Schedule("gen_wgrad", 32869, 256, 256, True)
    assert sorted(t for w in range(s.nwalkers) for t in s.tiles_of(w)) == list(range(s.ntiles))


def test_every_case_reaches_its_loop_region():
    for kind, d, H, item, B in R.forward_cases():
        s = R.Schedule(kind, B)
        cov = s.coverage()
        assert cov["second"] and cov["ragged_later"] and cov["idle_last_pass"], (kind, B)
        assert cov["third"] == (B > 2 * s.pass_rows)
        assert sorted(t for w in range(s.nwalkers) for t in s.tiles_of(w)) == list(range(s.ntiles))
    thirds = {kind: False for kind in ("fwd64", "fwd2", "bwd64", "bwd2", "bwd3")}
    for kind, d, H, item, B in R.forward_cases() + R.backward_cases():
        if kind in thirds and R.Schedule({"bwd2": "wgrad"}.get(kind, kind), B).coverage()["third"]:
            thirds[kind] = True
    assert all(thirds.values()), thirds
    for kind, d, H, item, B in R.backward_cases():
        rows, slabs = R.backward_schedules(kind, B, d, H, item)
        cov = slabs.coverage()
        assert cov["second"], (kind, B)
        assert cov["both_buffers"] == (True if kind == "bwd2" else None), (kind, B)
        if kind != "gen":
            assert cov["nslab_gt16"] and cov["ragged_later"] and cov["idle_last_pass"], (kind, B)
        else:
            assert rows.coverage()["second"] and rows.coverage()["ragged_later"]
    # the data kernel of the two-kernel backward iterates only at the two largest sizes
    assert [R.Schedule("bwd_data", B).coverage()["max_iterations"] for k, d, H, it, B in R.backward_cases()
            if k == "bwd2" and not it] == [1, 1, 2, 3]
    # pair launches: the user tower stays below one pass, the item tower goes past it
    assert R.Schedule("fwd64", 5000).nwalkers == 79 and R.Schedule("fwd64", R.case_B("fwd64", 0)).nwalkers == 512
    assert R.Schedule("bwd64", 5000).nslab == 79 and R.Schedule("bwd64", R.case_B("bwd64", 0)).nslab == 256
    assert R.slab_groups(256)[3][:3] == [3, 19, 35] and len(R.slab_groups(256)) == 16 and R.slab_groups(5) == [[0], [1], [2], [3], [4]]


# --------------------------------------------------------------------------------------------------------------------
# every helper red for every defect
# --------------------------------------------------------------------------------------------------------------------
def _red(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


@pytest.fixture(scope="module")
def fwd():
    """a correct forward result of the prefetched kernel's smallest case, as f32 arrays"""
    d, H, item, B = 32, 64, True, R.case_B("fwd2", 0)
    c = R.forward_case(d, H, item, B)
    ref = R.forward_rows(c, np.arange(B), True)
    s = R.Schedule("fwd2", B)
    good = dict(hid=ref.hid.copy(), out=ref.out.astype(F32), den=ref.denom.astype(F32))
    return c, ref, s, good


def _fwd_checks_red(ref, s, res):
    _red(R.check_rows_exact, "hid", res["hid"], ref.hid, s)
    _red(R.check_out_denom, res["out"], res["den"], ref, s)


def test_forward_helpers_pass_a_correct_result(fwd):
    c, ref, s, good = fwd
    R.check_rows_exact("hid", good["hid"], ref.hid, s)
    eo, ed = R.check_out_denom(good["out"], good["den"], ref, s)
    assert eo <= 1.0 and ed <= 1.0                       # the f32 rounding of the reference itself: half an ulp = 1 u
    # one more ulp than the bound allows is red: the bound is not slack
    worse = dict(good, out=good["out"] * F32(1 + 8 * R.U))
    _red(R.check_out_denom, worse["out"], worse["den"], ref, s)
    # a power-of-two-norm row that is one ulp off is red although it is within the bound
    i = int(np.flatnonzero(ref.exact)[0])
    off = dict(good, den=good["den"].copy())
    off["den"][i] = np.nextafter(off["den"][i], F32(np.inf))
    _red(R.check_out_denom, off["out"], off["den"], ref, s)


@pytest.mark.parametrize("defect", ["dropped", "swapped", "stale_prefetch", "first_iteration_mask"])
def test_forward_helpers_are_red_for(defect, fwd):
    c, ref, s, good = fwd
    res = {k: v.copy() for k, v in good.items()}
    t1 = 1
    t2 = s.tiles_of(t1)[1]                               # the same walker's second tile
    r1, r2 = s.rows_of_tile(t1), s.rows_of_tile(t2)
    assert len(r1) == len(r2) == 32 and s.where(t2) == (t1, 1)
    if defect == "dropped":
        for v in res.values():
            v[r2] = R.SENTINEL
    elif defect == "swapped":
        for v in res.values():
            v[r1], v[r2] = v[r2].copy(), v[r1].copy()
    else:
        if defect == "stale_prefetch":                   # tile t1 computed from tile t1 + stride's ids and genres
            w = R.forward_rows(c, r2, True, mask_rows=r1)
            dst = r1
        else:                                            # the later tile masked with the counters of the row within the pass
            w = R.forward_rows(c, r2, True, mask_rows=r1)
            w2 = R.forward_rows(c, r2, True)
            assert not np.array_equal(w.hid, w2.hid)
            dst = r2
        res["hid"][dst], res["out"][dst], res["den"][dst] = w.hid, w.out.astype(F32), w.denom.astype(F32)
    _fwd_checks_red(ref, s, res)
    with pytest.raises(AssertionError, match=f"tile {t2 if defect in ('dropped', 'first_iteration_mask') else t1} "):
        R.check_rows_exact("hid", res["hid"], ref.hid, s)


def test_only_the_genres_stale_is_red_too(fwd):
    """the prefetched gather reading the current tile's genres with the next tile's ids"""
    c, ref, s, good = fwd
    t2 = s.tiles_of(1)[1]
    r1, r2 = s.rows_of_tile(1), s.rows_of_tile(t2)
    mixed_genres = c.genres.copy()
    mixed_genres[r2] = c.genres[r1]
    c2 = type(c)(**{**vars(c), "genres": mixed_genres})
    w = R.forward_rows(c2, r2, True)
    res = {k: v.copy() for k, v in good.items()}
    res["hid"][r2], res["out"][r2], res["den"][r2] = w.hid, w.out.astype(F32), w.denom.astype(F32)
    _fwd_checks_red(ref, s, res)


@pytest.fixture(scope="module")
def bwd():
    d, H, item, B = 32, 64, True, R.case_B("bwd64", 0)
    c = R.backward_case(d, H, item, B)
    s = R.Schedule("bwd64", B)
    return c, s, R.reference_slabs(c, s)


def _grads_of(c, slabs, skip=None):
    return R.split_slab(R.reduce_slabs(slabs, skip), c.d, c.H, c.K1)


def test_backward_helpers_pass_a_correct_result(bwd):
    c, s, slabs = bwd
    R.check_rows_exact("dX", c.ref.dX.astype(F32), c.ref.dX, s)
    R.check_slabs(slabs.astype(F32), slabs, c.d, c.H, c.K1)
    R.check_grads([g.astype(F32) for g in _grads_of(c, slabs)], R.weight_grads(c.ref, c.hid, c.x))
    # f32 summation of the slabs in another order gives the same bits: the point of the exact inputs
    rev = slabs.astype(F32)[::-1].sum(0, dtype=F32)
    assert np.array_equal(rev.astype(F64), R.reduce_slabs(slabs))


@pytest.mark.parametrize("defect", ["dropped", "twice", "swapped", "stale_prefetch", "ragged_leak", "slab_left_out"])
def test_backward_helpers_are_red_for(defect, bwd):
    c, s, slabs = bwd
    good_g = R.weight_grads(c.ref, c.hid, c.x)
    w = 1
    t1, t2 = s.tiles_of(w)[:2]
    r1, r2 = s.rows_of_tile(t1), s.rows_of_tile(t2)
    dX = c.ref.dX.astype(F32)
    bad = slabs.copy()
    if defect == "dropped":
        bad = R.reference_slabs(c, s, lambda k: [t for t in s.tiles_of(k) if t != t2])
        dX[r2] = R.SENTINEL
    elif defect == "twice":
        bad = R.reference_slabs(c, s, lambda k: s.tiles_of(k) + ([t2] if k == w else []))
    elif defect == "swapped":
        dX[r1], dX[r2] = dX[r2].copy(), dX[r1].copy()
    elif defect == "stale_prefetch":                      # tile t1's dPre multiplied with tile t2's gathered rows
        bad[w, : c.H * c.K1] += (c.ref.dpre[r1].T @ (c.x[r2] - c.x[r1])).ravel()
    elif defect == "ragged_leak":                         # the clamped rows past B (copies of row B - 1) are summed
        last = s.ntiles - 1
        pad = s.tile - len(s.rows_of_tile(last))
        assert pad > 0 and s.where(last)[1] >= 1
        rows = np.full(pad, c.B - 1)
        bad[s.where(last)[0]] += R.pack_slab(R.weight_grads(c.ref, c.hid, c.x, rows))
    elif defect == "slab_left_out":
        R.check_slabs(slabs, slabs, c.d, c.H, c.K1)
        _red(R.check_grads, _grads_of(c, slabs, skip=w + 16), good_g)
        return
    if defect in ("dropped", "swapped"):
        with pytest.raises(AssertionError, match=f"tile {t2 if defect == 'dropped' else t1} "):
            R.check_rows_exact("dX", dX, c.ref.dX, s)
    if defect == "swapped":
        # two tiles of one workgroup land in the same slab: the sums cannot see their order, the per-row output does
        R.check_slabs(bad, slabs, c.d, c.H, c.K1)
        return
    with pytest.raises(AssertionError, match=f"slab {w if defect != 'ragged_leak' else s.where(s.ntiles - 1)[0]} "):
        R.check_slabs(bad, slabs, c.d, c.H, c.K1)
    _red(R.check_grads, _grads_of(c, bad), good_g)


def test_scatter_reference_skips_row_zero_and_bad_ids():
    ids = np.array([0, 3, 3, 9, -1, 1])
    dX = np.arange(12, dtype=F64).reshape(6, 2)
    g = R.scatter_reference(4.0, 5, ids, dX)
    assert np.array_equal(g, np.array([[4, 4], [14, 15], [4, 4], [10, 12], [4, 4]], dtype=F64))


# --------------------------------------------------------------------------------------------------------------------
# realistic values: how far a dropped tile stands above the derived bounds
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H,tile", [(128, 128, 32), (64, 128, 64)])
def test_a_dropped_tile_is_above_the_realistic_bounds(d, H, tile):
    """For the inputs of test_default_path_realistic_values: the contribution of one 32-row tile against the bound
    (depth + c) u sum|terms| of every weight gradient, smallest over every 16th tile.  A result that lacks a tile is red
    as soon as one element's contribution exceeds twice its bound (the kernel's own error is at most one bound), so 2 is
    the factor asserted: for every tile in dW1, dW2 and db2, and in db1 for the item tower.  The factor of 100 one would
    like cannot hold at this B with sound constants: a tile is 1 / 2 052 of the batch while (depth + c) u is about 3.5e-5,
    which caps an average element near 14; measured minima: user dW1 2.5-2.9, db1 1.0-1.1, dW2 35-44, db2 3.8-4.5;
    item dW1 9.8-16.7, db1 2.4-3.6, dW2 31-42, db2 14-16."""
    sd, calls = R.realistic_tower_inputs(d, H)
    dU, dP, dN = O.bpr_loss(*(c.fwd.out.astype(F32) for c in calls))[1:]
    B = R.REALISTIC["B"]
    depth = R.summation_depth(B, tile)
    assert depth == (9 * 33 if tile == 32 else 5 * 65) + 33
    for c, g in zip(calls[:2], (dU, dP)):
        bw = R.backward_with_bounds(c.fwd.x, c.prm[1], c.prm[3], g, c.fwd.out.astype(F32), c.fwd.denom.astype(F32),
                                    c.fwd.hid.astype(F32), c.scale, d, depth)
        worst = R.dropped_tile_ratios(bw, range(0, B // 32, 16))
        print(f"({d}, {H}) {c.tower}: smallest dropped-tile / bound ratio " + ", ".join(f"{k} {v:.1f}" for k, v in worst.items()))
        for k in ("dW1", "dW2", "db2") + (("db1",) if c.tower == "item_tower" else ()):
            assert worst[k] > 2.0, (c.tower, k, worst[k])
        assert worst["db1"] > 1.0
    # the helper itself: inside the bound green, outside red
    ref, bound = np.array([1.0, -2.0]), np.array([1e-6, 1e-6])
    assert R.check_within("x", ref + 0.5e-6, ref, bound) == pytest.approx(0.5)
    _red(R.check_within, "x", ref + np.array([0.0, 1.5e-6]), ref, bound)
