"""GPU: the optimiser (csrc/optim.hip) and negative-sampler (csrc/sampler.hip) kernels at the C ABI, each against the
independent float64 / integer references of oracle/optim_np.py (pinned to stock torch and NumPy in
tests/test_optim_host.py).

Every tolerance below is a rounding count of the float32 chain the header documents (u = 2^-24), or exact equality;
none is taken from what the kernels return.  Worst cases observed are recorded in profiles/r07_optim_kernel_tests.md.
"""
import ctypes
import itertools
import logging
import math

import numpy as np
import pytest
import torch

from oracle import optim_np as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
F = np.float32


def _L():
    from recommendit_amd import _lib as L
    return L, L.lib(), L.device(), L.stream_ptr()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ulps32(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def _report(name, value):
    print(f"[worst] {name}: {value:.3f}")


# ------------------------------------------------------------------------------------------ norm and clip
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 4099, (1 << 22) + 3])
def test_sumsq_partials_against_float64(n):
    """The 64 partials of rihip_sumsq add up to the float64 sum of squares within 4u: each pair of squares is formed
    in float32 (<= 3 roundings on non-negative terms), the float64 accumulation is negligible beside that.
    n covers an empty body, a tail only, body + tail, and more than one grid-stride trip (2^22 > 64 * 256 * 4)."""
    L, lib, dev, st = _L()
    rng = np.random.default_rng(100 + n % 97)
    x = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 15, n)).astype(F)   # |x| <= 1e15: squares stay finite
    xd = _dev(np.concatenate([x, np.full(4, 3e18, F)]), dev)           # the words after x[n) must not be read
    npart = lib.rihip_sumsq_nparts()
    assert npart == 64
    part = torch.full((npart,), float("nan"), dtype=torch.float64, device=dev)
    L.check(lib.rihip_sumsq(xd.data_ptr(), n, part.data_ptr(), st), "sumsq")
    got = math.fsum(_np(part).tolist())
    ref = R.sumsq_f64(x)
    if n == 0:
        assert got == 0.0
    else:
        _report(f"sumsq n={n} rel/u", abs(got - ref) / ref / U)
        assert abs(got - ref) <= 4 * U * ref


def _partials(rng, n_part, norm):
    w = rng.random(n_part) + 0.05
    return w * (norm * norm / w.sum())


@pytest.mark.parametrize("n_part", [1, 64, 65, 3000])
@pytest.mark.parametrize("norm", [0.0, 0.02, 0.9999999, 1.0000001, 37.5])
def test_clip_coef_and_clip_coef_step_against_float32_reference(n_part, norm):
    """coef and total_norm of both entry points within 2 float32 ulps of clip_coef_f32 on the same partials (a norm
    below, just below, just above and far above max_norm = 1; an all-zero gradient gives exactly 1); the two entry
    points agree bitwise."""
    L, lib, dev, st = _L()
    rng = np.random.default_rng(n_part)
    part = _partials(rng, n_part, norm)
    pd_ = _dev(part, dev)
    ref_c, ref_n = R.clip_coef_f32(math.fsum(part.tolist()), 1.0)
    out = torch.full((4,), float("nan"), dtype=torch.float32, device=dev)     # coef, norm, coef_step, norm_step
    step = torch.tensor([3], dtype=torch.int64, device=dev)
    lr = torch.tensor([LR], dtype=torch.float32, device=dev)
    hyper = torch.zeros(2, dtype=torch.float32, device=dev)
    p0 = out.data_ptr()
    L.check(lib.rihip_clip_coef(pd_.data_ptr(), n_part, 1.0, p0, p0 + 4, st), "clip_coef")
    L.check(lib.rihip_clip_coef_step(pd_.data_ptr(), n_part, 1.0, p0 + 8, p0 + 12, step.data_ptr(), lr.data_ptr(), B1, B2,
                                     hyper.data_ptr(), None, 0, 0.0, None, st), "clip_coef_step")
    c, nrm, cs, ns = _np(out)
    assert _same_bits(np.array([c, nrm]), np.array([cs, ns]))
    if norm == 0.0:
        assert c == 1.0 and nrm == 0.0
    else:
        _report(f"clip n_part={n_part} norm={norm} coef ulps", float(_ulps32(c, ref_c)))
        assert _ulps32(c, ref_c) <= 2 and _ulps32(nrm, ref_n) <= 2
    if norm >= 1.001:
        assert c < 1.0
    if norm <= 0.999:
        assert c == 1.0
    # the norm output is optional
    L.check(lib.rihip_clip_coef(pd_.data_ptr(), n_part, 1.0, p0 + 8, None, st), "clip_coef")
    assert _same_bits(_np(out)[2:3], np.array([c]))


# ------------------------------------------------------------------------------------------ clock
@pytest.mark.parametrize("t", [1, 2, 7, 1000, 10 ** 5, 10 ** 6])
def test_adam_clock_entry_points(t):
    """rihip_adam_hyper_step: '*step_dev += 1, then hyper for that t'.  rihip_clip_coef_step: 'hyper for t = *step_dev
    (the step that is running), then *step_dev = t + 1'.  step_dev exactly, hyper_dev within 2 float32 ulps of the
    float64 reference on the float32 lr / betas; *lr_dev changes between the two calls of each sequence."""
    L, lib, dev, st = _L()
    lr1, lr2 = F(LR), F(3.7e-4)
    lr = torch.tensor([lr1], dtype=torch.float32, device=dev)
    hyper = torch.full((2,), float("nan"), dtype=torch.float32, device=dev)
    part = _dev(np.array([0.25, 0.5]), dev)
    cn = torch.zeros(2, dtype=torch.float32, device=dev)

    def check(t_ref, lr_ref, step_expected, step):
        assert int(step.item()) == step_expected
        ref = R.adam_hyper(lr_ref, F(B1), F(B2), t_ref)
        ul = _ulps32(_np(hyper), np.array(ref))
        _report(f"clock t={t_ref} hyper ulps", float(ul.max()))
        assert (ul <= 2).all(), (t_ref, _np(hyper), ref)

    step = torch.tensor([t - 1], dtype=torch.int64, device=dev)          # pre-increment form
    L.check(lib.rihip_adam_hyper_step(step.data_ptr(), lr.data_ptr(), B1, B2, hyper.data_ptr(), st), "hyper_step")
    check(t, lr1, t, step)
    lr.fill_(float(lr2))
    L.check(lib.rihip_adam_hyper_step(step.data_ptr(), lr.data_ptr(), B1, B2, hyper.data_ptr(), st), "hyper_step")
    check(t + 1, lr2, t + 1, step)

    step = torch.tensor([t], dtype=torch.int64, device=dev)              # running-step form
    lr.fill_(float(lr1))
    args = (part.data_ptr(), 2, 1.0, cn.data_ptr(), cn.data_ptr() + 4, step.data_ptr(), lr.data_ptr(), B1, B2,
            hyper.data_ptr(), None, 0, 0.0, None, st)
    L.check(lib.rihip_clip_coef_step(*args), "clip_coef_step")
    check(t, lr1, t + 1, step)
    lr.fill_(float(lr2))
    L.check(lib.rihip_clip_coef_step(*args), "clip_coef_step")
    check(t + 1, lr2, t + 2, step)


def test_clip_coef_step_sums_the_loss_partials():
    L, lib, dev, st = _L()
    rng = np.random.default_rng(1)
    lp = rng.random(777)
    out = torch.zeros(3, dtype=torch.float32, device=dev)
    step = torch.tensor([1], dtype=torch.int64, device=dev)
    lr = torch.tensor([LR], dtype=torch.float32, device=dev)
    hyper = torch.zeros(2, dtype=torch.float32, device=dev)
    part, lpd = _dev(np.array([4.0]), dev), _dev(lp, dev)
    L.check(lib.rihip_clip_coef_step(part.data_ptr(), 1, 1.0, out.data_ptr(), out.data_ptr() + 4, step.data_ptr(),
                                     lr.data_ptr(), B1, B2, hyper.data_ptr(), lpd.data_ptr(), 777, 1.0 / 777,
                                     out.data_ptr() + 8, st), "clip_coef_step")
    assert _ulps32(_np(out)[2], math.fsum(lp.tolist()) / 777) <= 1


# ------------------------------------------------------------------------------------------ dense Adam
def _adam_inputs(rng, shape):
    """p ~ N(0,1), g = +-10^U(-4,0), m ~ 1e-2 N(0,1), v = 10^U(-8,-2): sqrt(v) >> eps everywhere, so no element sits in
    Adam's eps region and none has to be excluded from the bounds."""
    p = rng.standard_normal(shape).astype(F)
    g = (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-4, 0, shape)).astype(F)
    m = (1e-2 * rng.standard_normal(shape)).astype(F)
    v = (10.0 ** rng.uniform(-8, -2, shape)).astype(F)
    return p, g, m, v


def _hyper32(lr, t):
    """the float32 pair the kernels work with: the float64 reference rounded once"""
    h = R.adam_hyper(F(lr), F(B1), F(B2), t)
    return float(F(h[0])), float(F(h[1]))


def _check_adam(tag, got_p, got_m, got_v, p, g, m, v, t, wd, coef, lr=LR):
    """|dm| <= 6u S_m, |dv| <= 8u v, |dp| <= u |p| + 16u (|upd| + lr' S_m / denom): roundings counted along each chain
    of adam_elem (g' <= 3, m 3 more; g'^2 .. v <= 7; sqrt / div / +eps / div / mul <= 9 and m's error carried through
    lr'/denom; the final subtraction u |p|).  FMA contraction only lowers the counts.  A wrong bias correction, a
    missing wd p, or g^2 taken before the clip scaling is off by >= 1e3 u."""
    ref = R.adam_f64(p, g, m, v, _hyper32(lr, t), F(B1), F(B2), F(EPS), F(wd), coef)
    lr1 = _hyper32(lr, t)[0]
    em = np.abs(got_m.astype(np.float64) - ref.m) / (U * ref.s_m)
    ev = np.abs(got_v.astype(np.float64) - ref.v) / (U * ref.v)
    bound_p = U * np.abs(ref.p) + 16 * U * (np.abs(ref.upd) + lr1 * ref.s_m / ref.denom)
    ep = np.abs(got_p.astype(np.float64) - ref.p) / bound_p
    _report(f"{tag} dm/(u S_m)", float(em.max()))
    _report(f"{tag} dv/(u v)", float(ev.max()))
    _report(f"{tag} dp/bound", float(ep.max()))
    assert em.max() <= 6, (tag, "m", float(em.max()))
    assert ev.max() <= 8, (tag, "v", float(ev.max()))
    assert ep.max() <= 1, (tag, "p", float(ep.max()))
    assert np.abs(ref.upd).max() > 1e-5          # the step moved something: the bounds are not vacuous


_DENSE = {}


def _dense_case(n, dev):
    if n not in _DENSE:
        _DENSE.clear()
        host = _adam_inputs(np.random.default_rng(n % 1000), n)
        _DENSE[n] = (host, tuple(_dev(a, dev) for a in host))
    return _DENSE[n]


@pytest.mark.parametrize("t", [1, 7, 1000, 10 ** 5])
@pytest.mark.parametrize("n", [(1 << 20) + 3, 3 << 21])
def test_adam_dense_against_float64(n, t):
    """n = 2^20 + 3 has a tail; n = 3 * 2^21 exceeds the 2048 x 256 x 4-element grid, so the stride loop iterates.
    wd in {0, 1e-5} x coef in {NULL, 0.37}; with hyper_dev (made by rihip_adam_hyper_step, host lr / step arguments
    then deliberately wrong) and without: the two agree bitwise."""
    L, lib, dev, st = _L()
    (p, g, m, v), (pd_, gd, md, vd) = _dense_case(n, dev)
    stepd = torch.tensor([t - 1], dtype=torch.int64, device=dev)
    lrd = torch.tensor([LR], dtype=torch.float32, device=dev)
    hyper = torch.zeros(2, dtype=torch.float32, device=dev)
    L.check(lib.rihip_adam_hyper_step(stepd.data_ptr(), lrd.data_ptr(), B1, B2, hyper.data_ptr(), st), "hyper_step")
    coefd = torch.tensor([0.37], dtype=torch.float32, device=dev)
    for wd, coef in itertools.product([0.0, 1e-5], [None, 0.37]):
        outs = []
        for use_dev in (False, True):
            P, M, V = pd_.clone(), md.clone(), vd.clone()
            L.check(lib.rihip_adam_dense(P.data_ptr(), gd.data_ptr(), M.data_ptr(), V.data_ptr(), n,
                                         77.0 if use_dev else LR, B1, B2, EPS, wd, 0 if use_dev else t,
                                         coefd.data_ptr() if coef is not None else None,
                                         hyper.data_ptr() if use_dev else None, st), "adam_dense")
            outs.append((_np(P), _np(M), _np(V)))
        for a, b in zip(*outs):
            assert _same_bits(a, b)
        _check_adam(f"dense n={n} t={t} wd={wd} coef={coef}", *outs[0], p, g, m, v, t, wd, coef)
    assert _same_bits(_np(gd), g)


def test_adam_dense_all_zero_state_leaves_everything_bitwise_unchanged():
    L, lib, dev, st = _L()
    n = 4099
    p = np.random.default_rng(0).standard_normal(n).astype(F)
    P = _dev(p, dev)
    Z = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(3)]
    L.check(lib.rihip_adam_dense(P.data_ptr(), Z[0].data_ptr(), Z[1].data_ptr(), Z[2].data_ptr(), n, LR, B1, B2, EPS, 0.0,
                                 1, None, None, st), "adam_dense")
    assert _same_bits(_np(P), p)
    for z in Z:
        assert _same_bits(_np(z), np.zeros(n, F))


def test_adam_dense_multi_with_zero_grad_mask_against_float64():
    L, lib, dev, st = _L()
    sizes = [(1 << 20) + 3, 640, 40001]
    rng = np.random.default_rng(77)
    host = [_adam_inputs(rng, n) for n in sizes]
    devs = [[_dev(a, dev) for a in h] for h in host]
    coefd = torch.tensor([0.37], dtype=torch.float32, device=dev)
    PA, NA = ctypes.c_void_p * 3, ctypes.c_int64 * 3
    col = lambda k: PA(*[d[k].data_ptr() for d in devs])
    L.check(lib.rihip_adam_dense_multi(3, col(0), col(1), col(2), col(3), NA(*sizes), 0b101, LR, B1, B2, EPS, 1e-5, 7,
                                       coefd.data_ptr(), None, st), "adam_dense_multi")
    for k, (h, d) in enumerate(zip(host, devs)):
        _check_adam(f"multi tensor {k}", _np(d[0]), _np(d[2]), _np(d[3]), *h, 7, 1e-5, 0.37)
        if k == 1:
            assert _same_bits(_np(d[1]), h[1])
        else:
            assert _same_bits(_np(d[1]), np.zeros(sizes[k], F))


# ------------------------------------------------------------------------------------------ row-sparse path
def _offset_f32(shape, dev, off, fill=None):
    """float32 [shape] whose data pointer is `off` floats past a 16-byte boundary"""
    n = int(np.prod(shape))
    flat = torch.empty(n + 4, dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    t = flat[off:off + n].view(*shape)
    if fill is not None:
        t.copy_(fill)
    return t


def _n_unique(L, lib, ws, B, d):
    out = ctypes.c_void_p()
    L.check(lib.rihip_rows_n_unique_ptr(ws.data_ptr(), B, d, ctypes.byref(out)), "n_unique_ptr")
    off = out.value - ws.data_ptr()
    assert 0 <= off <= ws.numel() - 4
    return int(ws[off:off + 4].view(torch.int32).item())


def _run_rows(ids, dX, d, hint, table, m, v, adam, dx_off=0, gc_off=0, in_place=False):
    """rihip_rows_group -> rihip_rows_reduce -> rihip_adam_rows (skipped when adam is None) on copies of table / m / v
    (on the tensors themselves when in_place).  adam = (t, wd, coef, use_hyper_dev).  Returns host copies of
    everything a caller can observe."""
    L, lib, dev, st = _L()
    B = ids.shape[0]
    nbytes = lib.rihip_rows_workspace_bytes(B, d)
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    idd = _dev(ids, dev)
    dXd = _offset_f32((B, d), dev, dx_off, _dev(dX, dev))
    uniq = torch.full((B,), -7, dtype=torch.int64, device=dev)
    Gc = _offset_f32((B, d), dev, gc_off)
    Gc.fill_(float("nan"))
    part = torch.full((lib.rihip_rows_nparts(),), float("nan"), dtype=torch.float64, device=dev)
    L.check(lib.rihip_rows_group(idd.data_ptr(), B, d, hint, uniq.data_ptr(), ws.data_ptr(), ws.numel(), st), "group")
    L.check(lib.rihip_rows_reduce(dXd.data_ptr(), B, d, uniq.data_ptr(), ws.data_ptr(), Gc.data_ptr(), part.data_ptr(),
                                  st), "reduce")
    nu = _n_unique(L, lib, ws, B, d)
    assert 1 <= nu <= B
    out = {"nu": nu, "uniq": _np(uniq), "Gc": _np(Gc)[:nu].copy(), "part": _np(part)}
    if adam is not None:
        t, wd, coef, use_dev = adam
        T, M, V = (table, m, v) if in_place else (table.clone(), m.clone(), v.clone())
        hyper = torch.zeros(2, dtype=torch.float32, device=dev)
        if use_dev:
            stepd = torch.tensor([t - 1], dtype=torch.int64, device=dev)
            lrd = torch.tensor([LR], dtype=torch.float32, device=dev)
            L.check(lib.rihip_adam_hyper_step(stepd.data_ptr(), lrd.data_ptr(), B1, B2, hyper.data_ptr(), st), "hyper")
        coefd = torch.tensor([coef if coef is not None else 1.0], dtype=torch.float32, device=dev)
        L.check(lib.rihip_adam_rows(T.data_ptr(), M.data_ptr(), V.data_ptr(), uniq.data_ptr(), Gc.data_ptr(), B, d,
                                    ws.data_ptr(), 77.0 if use_dev else LR, B1, B2, EPS, wd, 0 if use_dev else t,
                                    coefd.data_ptr() if coef is not None else None,
                                    hyper.data_ptr() if use_dev else None, st), "adam_rows")
        out["T"], out["M"], out["V"] = T, M, V
    torch.cuda.synchronize()
    return out


def _check_group_reduce(tag, out, ids, dX, n_rows_ref):
    """uniq / n_unique exactly; |Gc - float64 sum| <= (c - 1) u sum|x| per element (the summation bound of any order);
    Gc of the padding row exactly 0; sum(part) = sum Gc^2 of the returned Gc to N 2^-53 (float64 accumulation)."""
    uniq, pos = R.group_rows(ids, n_rows_ref)
    nu = out["nu"]
    assert nu == uniq.shape[0], (tag, nu, uniq.shape[0])
    np.testing.assert_array_equal(out["uniq"][:nu], uniq)
    G, A, cnt = R.reduce_rows_f64(dX, uniq, pos)
    Gc = out["Gc"].astype(np.float64)
    bound = (cnt - 1)[:, None] * U * A
    err = np.abs(Gc - G)
    assert (err <= bound).all(), (tag, float((err - bound).max()))
    multi = cnt > 1
    if multi.any() and (bound[multi] > 0).any():
        sel = bound > 0
        _report(f"{tag} Gc err/bound", float((err[sel] / bound[sel]).max()))
    assert (out["Gc"][uniq == 0] == 0).all()
    ref_ss = float(np.sum(Gc * Gc))
    got_ss = math.fsum(out["part"].tolist())
    assert abs(got_ss - ref_ss) <= Gc.size * 2.0 ** -53 * ref_ss, (tag, got_ss, ref_ss)
    return uniq, cnt


def _check_rows_adam(tag, out, table, m, v, uniq, adam):
    """touched rows meet the dense-Adam bounds with g = the Gc the kernel was given; every other row of table / m / v
    is bitwise unchanged; row 0 starts as zeros and stays zeros whether or not id 0 is in the batch"""
    t, wd, coef, _ = adam
    dev = table.device
    ud = _dev(uniq, dev)
    for name, new, old in (("table", out["T"], table), ("m", out["M"], m), ("v", out["V"], v)):
        changed = (new.view(torch.int32) != old.view(torch.int32)).any(dim=1)
        touched = torch.zeros_like(changed)
        touched[ud] = True
        assert not bool((changed & ~touched).any()), (tag, name, "an untouched row changed")
    nz = uniq != 0
    if nz.any():
        un = _dev(uniq[nz], dev)
        _check_adam(tag, _np(out["T"][un]), _np(out["M"][un]), _np(out["V"][un]), _np(table[un]), out["Gc"][nz],
                    _np(m[un]), _np(v[un]), t, wd, coef)
    for new in (out["T"], out["M"], out["V"]):
        assert _same_bits(_np(new[0]), np.zeros(new.shape[1], F))


def _rows_state(rng, n_rows, d, dev):
    p, _, m, v = _adam_inputs(rng, (n_rows, d))
    p[0] = 0; m[0] = 0; v[0] = 0
    return _dev(p, dev), _dev(m, dev), _dev(v, dev)


def _grad_rows(rng, B, d):
    return (rng.choice([-1.0, 1.0], (B, d)) * 10.0 ** rng.uniform(-4, 0, (B, d))).astype(F)


def _hot_ids(B, n_rows, with0):
    """17 distinct rows below the hot row, the hot row on a third of the batch, distinct rows above it: in sorted order
    the hot segment starts at position 17 (mod 32 when B >= 64) and, at B = 65 536, spans 683 blocks of 32"""
    low = min(17, B - 1)
    hot = max(1, min(B // 3, B - low))
    rest = B - low - hot
    h = 100
    ids = np.concatenate([np.arange(low) + (0 if with0 else 1), np.full(hot, h), h + 1 + np.arange(rest)]).astype(np.int64)
    assert ids.max() < n_rows and (B < 64 or int((ids < h).sum()) % 32 == 17)
    return ids


def _pattern_ids(pattern, rng, B, n_rows, with0):
    if pattern == "distinct":
        ids = rng.permutation(n_rows - 1)[:B].astype(np.int64) + 1
        if with0:
            ids[B // 2] = 0
        return ids
    if pattern == "equal":
        return np.full(B, 0 if with0 else n_rows - 1, dtype=np.int64)
    if pattern == "hot":
        return rng.permutation(_hot_ids(B, n_rows, with0))
    if pattern == "zipf":
        ids = np.minimum(rng.zipf(1.05, size=B), n_rows - 1).astype(np.int64)
        if with0:
            ids[rng.integers(0, B, 5)] = 0
        return ids
    raise ValueError(pattern)


# (d, dX offset, Gc offset): the scalar kernels incl. d > 64 lanes; the alignment fall-back of the float4 forms at d = 64
# (a 4-byte offset of dX moves the reduce, one of Gc moves the reduce and the row Adam); the float4 forms
_LAYOUTS = [(16, 0, 0), (20, 0, 0), (48, 0, 0), (256, 0, 0), (64, 1, 0), (64, 0, 1), (32, 0, 0), (64, 0, 0), (128, 0, 0)]
# (t, weight_decay, coef, hyper_dev): large step counts, wd = 0 and the hyper_dev override among them
_ADAM_CFG = [(1, 1e-5, None, False), (1000, 0.0, 0.37, True), (10 ** 5, 1e-5, 0.37, True), (7, 0.0, None, False)]


def _rows_case(tag, ids, d, dx_off, gc_off, n_rows, adam, rng, state=None):
    L, lib, dev, st = _L()
    B = ids.shape[0]
    dX = _grad_rows(rng, B, d)
    table, m, v = state if state is not None else _rows_state(rng, n_rows, d, dev)
    runs = [_run_rows(ids, dX, d, n_rows, table, m, v, adam, dx_off, gc_off) for _ in range(2)]
    a, b = runs
    assert a["nu"] == b["nu"] and _same_bits(a["uniq"][:a["nu"]], b["uniq"][:b["nu"]]), (tag, "uniq not repeatable")
    assert _same_bits(a["Gc"], b["Gc"]) and _same_bits(a["part"], b["part"]), (tag, "Gc / part not repeatable")
    for k in ("T", "M", "V"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (tag, k, "not repeatable")
    uniq, cnt = _check_group_reduce(tag, a, ids, dX, n_rows)
    _check_rows_adam(tag, a, table, m, v, uniq, adam)
    return cnt


@pytest.mark.parametrize("d,dx_off,gc_off", _LAYOUTS)
@pytest.mark.parametrize("B", [1, 31, 32, 33, 777])
def test_rows_path_small_batches(B, d, dx_off, gc_off):
    """B = 1, B around the RB = 32 block of sorted positions, and an odd B, on every kernel form; all-distinct,
    all-equal, one-hot-row and skewed ids, each with and without the padding id 0."""
    n_rows = 1000
    rng = np.random.default_rng(B * 1000 + d + dx_off + 2 * gc_off)
    _, _, dev, _ = _L()
    state = _rows_state(rng, n_rows, d, dev)
    k = 0
    for pattern, with0 in itertools.product(["distinct", "equal", "hot", "zipf"], [False, True]):
        ids = _pattern_ids(pattern, rng, B, n_rows, with0)
        adam = _ADAM_CFG[k % 4]
        k += 1
        _rows_case(f"rows B={B} d={d} off=({dx_off},{gc_off}) {pattern} id0={with0}", ids, d, dx_off, gc_off, n_rows, adam,
                   rng, state)


@pytest.mark.parametrize("d,dx_off,gc_off,pattern,with0", [
    (128, 0, 0, "hot", False), (64, 0, 0, "hot", True), (32, 0, 0, "distinct", True), (64, 1, 0, "hot", False),
    (64, 0, 1, "zipf", True), (20, 0, 0, "hot", True), (48, 0, 0, "equal", False), (256, 0, 0, "hot", False),
    (16, 0, 0, "distinct", False)])
def test_rows_path_batch_65536(d, dx_off, gc_off, pattern, with0):
    """B = 65 536: the hot row owns 21 845 samples from sorted position 17 on (683 blocks of 32, the first and last
    partial); all-equal is one segment of 2048 blocks."""
    n_rows = 70_000
    rng = np.random.default_rng(d * 7 + dx_off + 2 * gc_off)
    ids = _pattern_ids(pattern, rng, 65536, n_rows, with0)
    cnt = _rows_case(f"rows B=65536 d={d} off=({dx_off},{gc_off}) {pattern} id0={with0}", ids, d, dx_off, gc_off, n_rows,
                     _ADAM_CFG[(d // 16) % 4], rng)
    if pattern == "hot":
        assert cnt.max() == 65536 // 3


def test_rows_path_zipf_over_a_million_rows():
    """Zipf ids over a 1 M x 128 table at B = 65 536 (the headline configuration's shape).  The table, m and v are
    filled with one constant each so that 'untouched rows unchanged' needs no second copy of 1.5 GB."""
    L, lib, dev, st = _L()
    n_rows, d, B = 1_000_000, 128, 65536
    rng = np.random.default_rng(42)
    ids = np.minimum(rng.zipf(1.05, size=B), n_rows - 1).astype(np.int64)
    ids[:4] = [0, n_rows - 1, 1, 0]
    dX = _grad_rows(rng, B, d)
    consts = (0.5, 0.01, 1e-4)
    adam = (1000, 1e-5, 0.37, True)
    prev = None
    for rep in range(2):
        state = [torch.full((n_rows, d), c, dtype=torch.float32, device=dev) for c in consts]
        for s in state:
            s[0] = 0
        out = _run_rows(ids, dX, d, n_rows, *state, adam, in_place=True)
        uniq, cnt = _check_group_reduce("rows zipf 1M", out, ids, dX, n_rows)
        ud = _dev(uniq, dev)
        for s, c in zip(state, consts):
            changed = (s != c).any(dim=1)
            touched = torch.zeros_like(changed)
            touched[ud] = True
            touched[0] = True
            assert not bool((changed & ~touched).any())
            assert _same_bits(_np(s[0]), np.zeros(d, F))
        nz = uniq != 0
        rows = [_np(s[ud[torch.from_numpy(nz).to(dev)]]) for s in state]
        k = int(nz.sum())
        _check_adam("rows zipf 1M", *rows, np.full((k, d), consts[0], F), out["Gc"][nz], np.full((k, d), consts[1], F),
                    np.full((k, d), consts[2], F), adam[0], adam[1], adam[2])
        cur = (out["nu"], out["uniq"][:out["nu"]], out["Gc"], out["part"], *rows)
        if prev is not None:
            assert all(_same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(prev, cur))
        prev = cur
        del state, out
        torch.cuda.empty_cache()
    assert cnt.max() > 1000


# ------------------------------------------------------------------------------------------ sampler
def _sample(users, cat, rated, M, seed, max_attempts, with_counter=True, n=None):
    L, lib, dev, st = _L()
    ud, cd, rd = _dev(users, dev), _dev(cat, dev), _dev(rated, dev)
    n = users.shape[0] if n is None else n
    neg = torch.full((max(users.shape[0], 1),), -99, dtype=torch.int64, device=dev)
    gu = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(lib.rihip_sample_negatives(ud.data_ptr(), n, cd.data_ptr(), cat.shape[0], rd.data_ptr(), rated.shape[0], M, seed,
                                       max_attempts, neg.data_ptr(), gu.data_ptr() if with_counter else None, st), "sample")
    return _np(neg), int(gu.item())


def _ml1m_shaped(rng):
    cat = np.sort(rng.choice(np.arange(1, 700), size=480, replace=False)).astype(np.int64)   # non-contiguous ids
    M = 700
    rated = np.unique(rng.integers(1, 601, size=60000) * M + rng.choice(cat, size=60000))
    users = rng.integers(1, 601, size=70000).astype(np.int64)
    return users, cat, rated, M


def test_sampler_equals_integer_restatement_ml1m_shape():
    users, cat, rated, M = _ml1m_shaped(np.random.default_rng(8))
    seed = 0x1234_5678_9ABC_DEF1
    neg, gu = _sample(users, cat, rated, M, seed, 1000)
    ref, ref_gu = R.sample_negatives_np(users, cat, rated, M, seed, 1000)
    np.testing.assert_array_equal(neg, ref)
    assert gu == ref_gu == 0 and not np.isin(users * M + neg, rated).any()
    neg2, _ = _sample(users, cat, rated, M, seed, 1000)
    np.testing.assert_array_equal(neg2, neg)                                   # same seed: bitwise equal
    neg3, _ = _sample(users, cat, rated, M, seed + 1, 1000)
    assert (neg3 != neg).mean() > 0.9                                          # another seed: another batch
    neg4, gu4 = _sample(users, cat, rated, M, seed, 1000, with_counter=False)   # gave_up = NULL
    np.testing.assert_array_equal(neg4, neg)
    # few attempts: some samples give up, and the count and the kept (rated) items are the restatement's
    neg5, gu5 = _sample(users, cat, rated, M, seed, 2)
    ref5, ref_gu5 = R.sample_negatives_np(users, cat, rated, M, seed, 2)
    np.testing.assert_array_equal(neg5, ref5)
    assert gu5 == ref_gu5 == int(np.isin(users * M + neg5, rated).sum()) > 0


def test_sampler_single_item_catalogue_and_unknown_users():
    cat = np.array([42], dtype=np.int64)
    M = 64
    rated = np.array([3 * M + 42, 9 * M + 41], dtype=np.int64)
    users = np.array([3, 9, 1000, 3, 5, 123456] * 40, dtype=np.int64)        # 1000, 5, 123456: no ratings at all
    neg, gu = _sample(users, cat, rated, M, 5, 7)
    ref, ref_gu = R.sample_negatives_np(users, cat, rated, M, 5, 7)
    np.testing.assert_array_equal(neg, ref)
    assert (neg == 42).all() and gu == ref_gu == int((users == 3).sum())


@pytest.mark.parametrize("max_attempts", [1, 50])
def test_sampler_user_who_rated_the_whole_catalogue(max_attempts):
    rng = np.random.default_rng(4)
    cat = np.array([3, 8, 9, 20, 31], dtype=np.int64)
    M = 32
    rated = np.sort(np.concatenate([7 * M + cat, [5 * M + 8, 6 * M + 3]])).astype(np.int64)
    users = rng.choice([5, 6, 7, 11], size=4099).astype(np.int64)
    neg, gu = _sample(users, cat, rated, M, 99, max_attempts)
    ref, ref_gu = R.sample_negatives_np(users, cat, rated, M, 99, max_attempts)
    np.testing.assert_array_equal(neg, ref)
    assert gu == ref_gu
    hit = np.isin(users * M + neg, rated)
    assert gu == int(hit.sum()) >= int((users == 7).sum())
    if max_attempts == 50:
        assert gu == int((users == 7).sum())


def test_sampler_empty_batch_writes_nothing():
    users, cat, rated, M = _ml1m_shaped(np.random.default_rng(8))
    neg, gu = _sample(users[:16], cat, rated, M, 1, 10, n=0)
    assert (neg == -99).all() and gu == 0


def test_dataset_counts_exhausted_negatives_and_warns_once_per_epoch(caplog):
    """UserItemDataset.sample_negatives hands the kernel a device counter; epoch_batches reads it once, at the end of the
    epoch, and warns when a sample kept a rated item."""
    import pandas as pd
    from recommendit_amd.train_embeddings import UserItemDataset
    items = list(range(1, 9))
    rows = [(1, i, 5.0) for i in items] + [(2, 1, 5.0), (2, 2, 4.0), (3, 3, 5.0), (3, 4, 2.0)]   # user 1 rated everything
    df = pd.DataFrame(rows, columns=["user_id", "item_id", "rating"])
    ds = UserItemDataset(df, {i: np.zeros(18, np.float32) for i in items}, items)
    gen = torch.Generator(device="cuda"); gen.manual_seed(0)
    assert ds.negatives_given_up() == 0
    u = torch.tensor([1, 2, 1, 3, 1], dtype=torch.int64, device="cuda")
    neg = ds.sample_negatives(u, gen, max_attempts=20)
    assert ds.negatives_given_up() == 3 and int(neg[1]) not in (1, 2) and int(neg[3]) not in (3, 4)
    assert ds.negatives_given_up(reset=True) == 3 and ds.negatives_given_up() == 0
    with caplog.at_level(logging.WARNING, logger="recommendit_amd.train_embeddings"):
        n_batches = sum(1 for _ in ds.epoch_batches(4, gen))
    assert n_batches == len(ds) // 4
    warned = [r for r in caplog.records if "exhausted their attempts" in r.getMessage()]
    assert len(warned) == 1 and ds.negatives_given_up() == 0
    caplog.clear()
    clean = UserItemDataset(df[df["user_id"] != 1], {i: np.zeros(18, np.float32) for i in items}, items)
    with caplog.at_level(logging.WARNING, logger="recommendit_amd.train_embeddings"):
        assert sum(1 for _ in clean.epoch_batches(2, gen)) == 1
    assert not [r for r in caplog.records if "exhausted" in r.getMessage()]


# ------------------------------------------------------------------------------------------ ids outside the table
@pytest.mark.parametrize("d", [32, 20])
def test_rows_path_ids_outside_the_table(d):
    """The documented contract: an id outside [0, n_rows) becomes the padding row 0 and its gradient is dropped.  With
    the n_rows hint only the low 10 bits are sorted, and 1029 and 2^40 + 5 share them with row 5: they must not split
    row 5's run.  uniq strictly ascending, Gc = the float64 sums over the in-range samples, one Adam step moves row 5
    exactly once.  No address outside the table can be formed: seg_starts_kernel clamps every id it stores when
    n_rows > 0, and Gc / the block partials are indexed by batch position.

    Without the hint (n_rows = 0) the library cannot know the table's size: only negative ids become row 0, the others
    are rows in their own right -- so group and reduce are checked, and the row Adam (which would address row
    2^40 + 5) is not run."""
    n_rows, B = 1000, 200
    rng = np.random.default_rng(d)
    ids = rng.integers(1, n_rows, size=B).astype(np.int64)
    ids[:7] = [5, n_rows + 29, 5, -2, n_rows + 7, (1 << 40) + 5, 0]
    ids[50], ids[60], ids[61] = 5, n_rows - 1, 1
    assert (n_rows + 29) % 1024 == 5 and ((1 << 40) + 5) % 1024 == 5
    dX = _grad_rows(rng, B, d)
    _, _, dev, _ = _L()
    table, m, v = _rows_state(rng, n_rows, d, dev)
    adam = (7, 1e-5, 0.37, False)
    a = _run_rows(ids, dX, d, n_rows, table, m, v, adam)
    nu = a["nu"]
    assert (np.diff(a["uniq"][:nu]) > 0).all(), a["uniq"][:min(nu, 12)]
    uniq, cnt = _check_group_reduce(f"stray ids d={d} hint", a, ids, dX, n_rows)
    assert cnt[uniq == 0][0] == 5 and cnt[uniq == 5][0] == int((ids == 5).sum()) >= 3
    _check_rows_adam(f"stray ids d={d} hint", a, table, m, v, uniq, adam)
    # row 5 moved once, by the sum of all its samples: its m against one float64 step from that sum, within the m bound
    # plus the summation bound of Gc carried through (1 - b1) coef
    x5 = dX[ids == 5].astype(np.float64)
    ref5 = R.adam_f64(_np(table[5]), x5.sum(axis=0), _np(m[5]), _np(v[5]), _hyper32(LR, 7), F(B1), F(B2), F(EPS), F(1e-5),
                      0.37)
    slack = 6 * U * ref5.s_m + (1.0 - float(F(B1))) * 0.37 * (x5.shape[0] - 1) * U * np.abs(x5).sum(axis=0)
    assert (np.abs(_np(a["M"][5]).astype(np.float64) - ref5.m) <= slack).all()
    b = _run_rows(ids, dX, d, n_rows, table, m, v, adam)
    assert _same_bits(a["Gc"], b["Gc"]) and torch.equal(a["T"].view(torch.int32), b["T"].view(torch.int32))

    c = _run_rows(ids, dX, d, 0, table, m, v, None)                # no hint: group + reduce only
    assert (np.diff(c["uniq"][:c["nu"]]) > 0).all(), c["uniq"][:min(c["nu"], 12)]
    uniq0, cnt0 = _check_group_reduce(f"stray ids d={d} no hint", c, ids, dX, 0)
    assert cnt0[uniq0 == 0][0] == 2 and uniq0[-1] == (1 << 40) + 5
