"""CPU: the NumPy model of a PQ index update under frozen codebooks (tests/pq_update_reference.py) applied step by step
equals the model built from the final corpus -- the property the GPU tests then ask of the handle.  Also: the header
declares the two exports and the loader binds them, and the opt-in flag defaults to today's behaviour."""
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_reference as P  # noqa: E402
import pq_residual_reference as PR  # noqa: E402
import pq_update_reference as PU  # noqa: E402
import sq8_reference as S  # noqa: E402
import sq8_update_reference as U  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


def _case(residual, seed, d=24, dsub=8, N0=500, nlist=5):
    X0, C, lists0 = PR.clustered(seed, N0, d, nlist, spread=0.25)
    pool, _, _ = PR.clustered(seed + 1, 900, d, nlist, spread=0.4)
    assign = lambda X: np.argmax(X.astype(np.float64) @ C.astype(np.float64).T, axis=1)    # noqa: E731
    lists0 = assign(X0)
    m, s = S.train_quantizer(X0)
    dpad = U.dpad_of(d)
    c0 = U.padded_codes(X0, m, s, dpad)
    if residual:
        book = PR.train(c0, PR.list_codes(C, m, s, dpad), lists0, dsub, 2)[0]
    else:
        book = P.train(c0, dsub, 2)[0]
    return X0, pool, C, lists0, assign, m, s, book


@pytest.mark.parametrize("residual", [False, True])
def test_twelve_random_updates_equal_the_from_scratch_model(residual):
    rng = np.random.RandomState(17 + residual)
    nlist = 5
    X0, pool, C, lists0, assign, m, s, book = _case(residual, 40 + residual)
    ids0 = rng.permutation(10 * len(X0))[:len(X0)].astype(np.int64)
    tags0 = rng.randint(0, 64, len(X0)).astype(np.uint32)
    Cres = C if residual else None
    A = PU.PqModel.from_corpus(X0, ids0, lists0, nlist, m, s, book, Cres, tags0)
    # the from-scratch build under injected codebooks is the plain reference's assignment of the (residual) codes
    c0 = U.padded_codes(X0, m, s, A.layout.dpad)
    if residual:
        want, dist, rcl = PR.assign_with(c0, A.K, lists0, book)
        assert (A.build_residual_clamped, A.build_distortion) == (rcl, dist)
    else:
        want, dist = P.assign(c0, book)
        assert A.build_distortion == dist
    np.testing.assert_array_equal(A.pq_codes(), want)
    next_pool, next_id, totals = 0, 10 ** 7, [0, 0, 0]
    for step in range(12):
        op = step % 3
        take = int(rng.randint(1, 70))
        rows = np.arange(next_pool, next_pool + take)
        next_pool += take
        scale = 3.0 if step >= 9 else 1.0                                    # the last rounds: rows far outside both grids
        Xn = (scale * pool[rows]).astype(np.float32)
        words = rng.randint(0, 64, take).astype(np.uint32)
        if op == 0:
            gone = rng.choice(A.ids, int(rng.randint(1, 60)), replace=False)
            out = A.update(np.concatenate([gone, [-1 - step]]), pool[:0], [])
            assert out == dict(dropped=len(gone), clamped=0, residual_clamped=0, distortion=0)
        elif op == 1:
            out = A.update([], Xn, np.arange(next_id, next_id + take), assign(Xn), words)
        else:
            stored = rng.choice(A.ids, take // 2, replace=False)
            ids = rng.permutation(np.concatenate([stored, np.arange(next_id, next_id + take - len(stored))]))
            out = A.update(ids, Xn, ids, assign(Xn), words)
            assert out["dropped"] == len(stored)
        next_id += take
        totals = [totals[0] + out["clamped"], totals[1] + out["residual_clamped"], totals[2] + out["distortion"]]
        B = PU.PqModel.from_corpus(A.X, A.ids, A.lists(), nlist, m, s, book, Cres, A.tags_by_row())
        PU.same_state(A, B)
        assert (A.pq_physical()[A.layout.row_ids < 0] == 0).all()
    assert A.stats[0] == 12 and A.stats[3:] == totals and totals[0] > 0 and totals[2] > 0
    assert (totals[1] > 0) == residual                                        # the scaled rows leave the residual grid too
    assert A.decoded().dtype == (np.int16 if residual else np.int8)


def test_a_flat_model_and_refusals():
    rng = np.random.RandomState(5)
    X0, pool, C, lists0, assign, m, s, book = _case(False, 60, N0=300)
    ids0 = np.arange(100, 400, dtype=np.int64)
    A = PU.PqModel.from_corpus(X0, ids0, None, 1, m, s, book)
    B = PU.PqModel.from_corpus(X0, ids0, None, 1, m, s, book)
    for kind, drop, X, add in [(1, [], pool[:3], [7, 8, 7]), (1, [101, 102, 101], pool[:0], []),
                               (2, [101], pool[:2], [9, 105]), (3, ids0, pool[:0], [])]:
        with pytest.raises(PU.Refused) as e:
            A.update(drop, X, add)
        assert e.value.kind == kind
        PU.same_state(A, B)
    assert A.update([5, 6], pool[:0], [])["dropped"] == 0 and A.stats == [0] * 6
    out = A.update(ids0[:40], pool[:70], np.arange(1000, 1070))
    assert out["dropped"] == 40 and out["residual_clamped"] == 0 and out["distortion"] == A.stats[5] > 0
    keep = ~np.isin(ids0, ids0[:40])
    PU.same_state(A, PU.PqModel.from_corpus(np.concatenate([X0[keep], pool[:70]]), np.concatenate([ids0[keep], np.arange(1000, 1070)]),
                                            None, 1, m, s, book))


def test_the_header_declares_the_update_abi_and_the_loader_binds_it():
    from recommendit_amd import _lib
    hdr = (ROOT / "include" / "recommendit_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("rihip_pq_update_apply", "rihip_pq_update_stats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["rihip_pq_update_apply"] == _lib.SIGNATURES["rihip_sq8_update_apply"]     # the same parameter list
    mk = (ROOT / "recommendit_amd" / "csrc" / "Makefile").read_text()
    assert "pq_update.hip" in mk
    src = (ROOT / "recommendit_amd" / "csrc" / "pq_update.hip").read_text()
    assert "#pragma clang fp contract(off)" in src
    for name in ("pq_update_encode_kernel", "pq_update_repack_kernel", "sq8_update_run"):
        assert name in src, name


def test_updates_stay_opt_in():
    from recommendit_amd import PQIndex, SQ8Index
    idx = PQIndex(embed_dim=32)
    assert idx.frozen_updates is False
    x = np.zeros((1, 32), np.float32)
    for call in (lambda: idx.add_items(x, [1]), lambda: idx.remove_items([1]), lambda: idx.update_items(x, [1]),
                 lambda: idx.add_items_device(None, [1])):
        with pytest.raises(NotImplementedError, match="rebuild"):
            call()
    assert idx._update_entry() == SQ8Index._UPDATE == "rihip_sq8_update_apply"       # the C refusal stays where it was
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="frozen_updates"):
            idx.frozen_updates = bad
    assert idx.frozen_updates is False
    idx.frozen_updates = True
    assert idx.frozen_updates is True and idx._update_entry() == "rihip_pq_update_apply"
    for call in (lambda: idx.add_items(x, [1]), lambda: idx.remove_items([1]), lambda: idx.update_items(x, [1])):
        with pytest.raises(RuntimeError, match="Index not built."):                  # SQ8Index's calls from here on
            call()
    assert PQIndex(embed_dim=32).frozen_updates is False                             # per index, not per class
    assert SQ8Index(embed_dim=8)._update_entry() == "rihip_sq8_update_apply"
