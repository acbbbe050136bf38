"""GPU parity of the stored-G in-batch passes at a shape whose tiles run in the steady-state loops (d = 128, 8-wave
workgroups: at least 4 096 owners and 16 384 swept rows in both passes), with everything the one-tile code still has to
catch around them: ragged owner and swept counts, a diagonal band that is not tile-aligned and falls at a different
place in every workgroup, and four swept-range splits.  Oracle: the rectangular closed form, evaluated in fp64 over
blocks of users.  Tolerances are those of test_inbatch_stored_g_rectangular_rank_form (same kernels, same oracle).
"""
import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import two_tower_np as O

pytestmark = pytest.mark.gpu


def test_inbatch_stored_g_steady_loops_ragged():
    from recommendit_amd import _lib as L
    lib, dev, st = L.lib(), L.device(), L.stream_ptr()
    Bl, G, off, d = 16420, 16650, 77, 128
    rng = np.random.RandomState(16420)
    U, I = fx.unit_rows(rng, Bl, d), fx.unit_rows(rng, G, d)
    Ud, Id = torch.from_numpy(U).to(dev).contiguous(), torch.from_numpy(I).to(dev).contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    pos = torch.empty(Bl, **f32); r = torch.empty(Bl, **f32)
    dU = torch.empty(Bl, d, **f32); dI = torch.full((G, d), float("nan"), **f32)
    lp = torch.zeros(max(1024, lib.rihip_inbatch_workspace_doubles(Bl)), dtype=torch.float64, device=dev)
    ws = torch.empty(max(lib.rihip_inbatch_workspace_floats(Bl, G, d), lib.rihip_inbatch_workspace_floats(G, Bl, d)), **f32)
    gm = torch.full((lib.rihip_inbatch_gmat_floats(Bl, G),), float("nan"), **f32)   # unwritten blocks must not leak
    loss = torch.empty((), **f32)
    L.check(lib.rihip_rowdot(Ud.data_ptr(), Id.data_ptr(), Bl, off, d, pos.data_ptr(), st), "rowdot")
    L.check(lib.rihip_inbatch_user_pass(Ud.data_ptr(), Bl, off, Id.data_ptr(), G, 0, d, pos.data_ptr(), G,
                                        dU.data_ptr(), r.data_ptr(), lp.data_ptr(), ws.data_ptr(), gm.data_ptr(), 0, st), "up")
    L.check(lib.rihip_inbatch_item_pass(gm.data_ptr(), Ud.data_ptr(), Bl, off, G, 0, d, r.data_ptr(), G, dI.data_ptr(),
                                        ws.data_ptr(), 0, st), "ip")
    L.check(lib.rihip_sum_partials(lp.data_ptr(), lib.rihip_inbatch_loss_parts(Bl, G), 1.0 / (G * (G - 1.0)),
                                   loss.data_ptr(), st), "sum")
    torch.cuda.synchronize()
    lo, dUo, dIo = 0.0, np.empty((Bl, d), np.float32), np.zeros((G, d), np.float64)
    for b0 in range(0, Bl, 2048):   # the oracle over blocks of users: loss and dI are sums over users
        b1 = min(b0 + 2048, Bl)
        l, du, di = O.in_batch_bpr_loss(U[b0:b1], I, owner_offset=off + b0, n_global=G)
        lo += float(l)
        dUo[b0:b1] = du
        dIo += di
    assert abs(loss.item() - lo) < 3e-6
    np.testing.assert_allclose(dU.cpu().numpy(), dUo, atol=3e-9, rtol=3e-4)
    np.testing.assert_allclose(dI.cpu().numpy(), dIo, atol=3e-9, rtol=3e-4)
