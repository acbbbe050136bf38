"""GPU: filtered retrieval -- per-query tag predicates tested inside the index scan (csrc/scan_f32.hip and csrc/ivf_search.hip, FILT instantiations; driver: csrc/topk.hip).

Every comparison is EQUALITY of scores and ids on every query, ties included.  Vectors, queries and injected centroids are
small integers (-3..3) searched with normalized=True, so every inner product is exact in f32 and f64 alike.  The oracle
is made of oracle/retrieval_np.py: per query, the passing rows `a` in ascending order, the plain oracle search over X[a]
(ascending `a` keeps "ties -> lowest row"; probing depends on the centroids alone), rows mapped back through `a`, padded.
"""
import pickle

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import gbdt_np as G
from oracle import ranking_features_np as RF
from oracle import retrieval_np as R

pytestmark = pytest.mark.gpu

ERR_STATE = 5          # RIHIP_ERR_STATE (csrc/common.h)


# ---- oracle ----------------------------------------------------------------------------------------------------------
def _passes(tags, pred):
    any_of, all_of, none_of = (int(v) for v in pred)
    t = tags.astype(np.int64)
    ok = (t & all_of) == all_of
    ok &= (t & none_of) == 0
    if any_of:
        ok &= (t & any_of) != 0
    return ok


def _oracle(Q, X, tags, preds, k, ivf=None, allowed=None):
    """preds uint32 [nq,3]; ivf = (centroids, assign, nprobe) or None (flat); allowed: optional bool [nq,N] AND-ed in.
    Queries that share a predicate (and have no `allowed`) share one oracle call; every query gets its own rows."""
    nq = Q.shape[0]
    out_s = np.full((nq, k), -np.inf, np.float32)
    out_r = np.full((nq, k), -1, np.int64)
    groups = {}
    for q in range(nq):
        key = tuple(int(v) for v in preds[q]) + ((q,) if allowed is not None else ())
        groups.setdefault(key, []).append(q)
    for key, qs in groups.items():
        ok = _passes(tags, key[:3])
        if allowed is not None:
            ok = ok & allowed[key[3]]
        a = np.nonzero(ok)[0]
        if a.size == 0:
            continue
        if ivf is None:
            s, r = R.topk_ip_exact_f32(Q[qs], X[a], k)
        else:
            C, assign, nprobe = ivf
            s, r = R.ivf_search(Q[qs], X[a], C, assign[a], nprobe, k)
        w = r.shape[1]
        out_s[qs, :w] = s
        out_r[qs, :w] = np.where(r >= 0, a[np.maximum(r, 0)], -1)
    return out_s, out_r


def _ints(rng, n, d):
    return rng.randint(-3, 4, size=(n, d)).astype(np.float32)


def _check(got, exp, what=""):
    s, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    np.testing.assert_array_equal(i, exp[1], err_msg=what)
    np.testing.assert_array_equal(s.view(np.uint32), exp[0].view(np.uint32), err_msg=what)


def _mixed_preds(rng, nq, bits=6):
    """per-query predicates over `bits` tag bits mixing any_of / all_of / none_of"""
    p = np.zeros((nq, 3), np.uint32)
    for q in range(nq):
        kind = q % 5
        b = rng.permutation(bits)
        if kind == 0:
            p[q] = (1 << b[0] | 1 << b[1], 0, 0)
        elif kind == 1:
            p[q] = (0, 1 << b[0] | 1 << b[1], 0)
        elif kind == 2:
            p[q] = (0, 0, 1 << b[0] | 1 << b[1] | 1 << b[2])
        elif kind == 3:
            p[q] = (1 << b[0], 1 << b[1], 1 << b[2])
        else:
            p[q] = (1 << b[0] | 1 << b[1] | 1 << b[2], 1 << b[3], 1 << b[4] | 1 << b[5])
    return p


# ---- 1. flat dense path (N <= 65 536) ------------------------------------------------------------------------------
def _flat_small():
    from recommendit_amd import FAISSIndex
    rng = np.random.RandomState(101)
    N, d, nq, k = 1000, 20, 130, 50          # d padded to the 32-wide kernel; nq crosses the 128-query workgroup
    X, Q = _ints(rng, N, d), _ints(rng, nq, d)
    tags = rng.randint(0, 64, N).astype(np.uint32)
    tags[:30] |= 1 << 20                     # 30 rows carry a caller bit: fewer than k pass
    idx = FAISSIndex(embed_dim=d, exact=True)
    idx.build_from_device(torch.from_numpy(X).cuda(), np.arange(N) + 7)      # item id = row + 7
    preds = _mixed_preds(rng, nq)
    preds[0] = (0, 0, 0)                     # pass-all
    preds[1] = (0, 1 << 25, 0)               # none pass
    preds[2] = (1 << 20, 0, 0)               # fewer than k pass
    preds[129] = (0, 1 << 20, 1)             # (beyond the first workgroup) fewer than k
    return idx, X, Q, tags, preds, N, d, nq, k


def test_flat_dense_path_equals_oracle():
    idx, X, Q, tags, preds, N, d, nq, k = _flat_small()
    qd = torch.from_numpy(Q).cuda()
    with pytest.raises(ValueError, match="tags"):
        idx.batch_search_device(qd, k=k, normalized=True, item_filter=(0, 0, 0))
    idx.set_item_tags(tags)
    assert idx.has_item_tags
    np.testing.assert_array_equal(idx.item_tags(), tags)
    exp_s, exp_r = _oracle(Q, X, tags, preds, k)
    assert (exp_r[1] == -1).all() and 0 < (exp_r[2] >= 0).sum() < k and 0 < (exp_r[129] >= 0).sum() < k
    exp_i = np.where(exp_r >= 0, exp_r + 7, -1)
    for f in (preds, torch.from_numpy(preds.view(np.int32)).cuda()):
        _check(idx.batch_search_device(qd, k=k, normalized=True, item_filter=f), (exp_s, exp_i))
    hs, hi = idx.batch_search(Q, k=k, item_filter=preds)           # (integer rows: the wrapper's normalisation changes
    assert ((hi >= 0) == (exp_i >= 0)).all()                       # scores, not which rows pass)
    # pass-all == the plain search, bit for bit (shared tuple and per-query rows)
    plain = idx.batch_search_device(qd, k=k, normalized=True)
    for f in ((0, 0, 0), np.zeros((nq, 3), np.uint32)):
        got = idx.batch_search_device(qd, k=k, normalized=True, item_filter=f)
        assert torch.equal(got[1], plain[1]) and torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))
    assert torch.equal(idx.batch_search_device(qd, k=k, normalized=True, item_filter=preds)[1][0], plain[1][0])
    n, redone = idx.filtered_stats()
    assert n >= 4 * nq and redone == 0                             # the dense path has no fallback
    # single-query host entry
    ds, di = idx.search(Q[2], k=k, item_filter=tuple(int(v) for v in preds[2]))
    assert sorted(di.tolist()) == sorted(exp_i[2][exp_i[2] >= 0].tolist())     # (30 rows pass: all of them)


# ---- 2. flat thresholded path (N > 65 536) ---------------------------------------------------------------------------
GROUPS = [("100%", (0, 0, 0)), ("50%", (1, 0, 0)), ("2%", (0, 1 << 8, 0)), ("0.2%", (0, 1 << 9, 0)),
          ("0.05%", (1 << 10, 0, 0)), ("0%", (0, 1 << 11, 0))]


@pytest.fixture(scope="module")
def flat_large():
    from recommendit_amd import FAISSIndex
    rng = np.random.RandomState(202)
    N, d, nq, k = 70001, 32, 130, 100        # > 65 536 and no multiple of 32; default two_precision
    X, Q = _ints(rng, N, d), _ints(rng, nq, d)
    tags = rng.randint(0, 64, N).astype(np.uint32)
    for bit, n in ((8, 1400), (9, 140), (10, 35)):     # 2 %, 0.2 % (>= k rows, fewer sampled than the rank), 0.05 % (< k)
        tags[rng.choice(N, n, replace=False)] |= 1 << bit
    idx = FAISSIndex(embed_dim=d, exact=True)
    idx.build_from_device(torch.from_numpy(X).cuda(), np.arange(N))
    idx.set_item_tags(tags)
    exp = {name: _oracle(Q, X, tags, np.tile(np.array(p, np.uint32), (nq, 1)), k) for name, p in GROUPS}
    return idx, torch.from_numpy(Q).cuda(), exp, nq, k


def test_flat_thresholded_path_shared_predicate(flat_large):
    idx, qd, exp, nq, k = flat_large
    assert (exp["0.2%"][1] >= 0).all() and ((exp["0.05%"][1] >= 0).sum(1) == 35).all() and (exp["0%"][1] == -1).all()
    for name, p in GROUPS:
        n0, r0 = idx.filtered_stats()
        _check(idx.batch_search_device(qd, k=k, normalized=True, item_filter=p), exp[name], name)
        n1, r1 = idx.filtered_stats()
        assert n1 - n0 == nq
        print(f"shared predicate {name}: {r1 - r0} of {nq} queries re-done by the exact fallback")
        if name in ("0.2%", "0.05%", "0%"):
            # few passing rows are an ordinary answer: every passing row is a candidate, nothing is re-done
            assert r1 - r0 == 0, name
    plain = idx.batch_search_device(qd, k=k, normalized=True)
    _check(plain, exp["100%"], "plain")


def test_flat_thresholded_path_per_query_predicates(flat_large):
    idx, qd, exp, nq, k = flat_large
    grp = np.arange(nq) % len(GROUPS)
    preds = np.array([GROUPS[g][1] for g in grp], np.uint32)
    exp_s = np.stack([exp[GROUPS[g][0]][0][q] for q, g in enumerate(grp)])
    exp_r = np.stack([exp[GROUPS[g][0]][1][q] for q, g in enumerate(grp)])
    n0, r0 = idx.filtered_stats()
    _check(idx.batch_search_device(qd, k=k, normalized=True, item_filter=preds), (exp_s, exp_r))
    n1, r1 = idx.filtered_stats()
    print(f"per-query predicates, all groups: {r1 - r0} of {n1 - n0} queries re-done by the exact fallback")
    sel = np.nonzero(grp >= 3)[0]                                  # the 0.2 %, 0.05 % and 0 % groups on their own
    got = idx.batch_search_device(qd[torch.from_numpy(sel).cuda()].contiguous(), k=k, normalized=True,
                                  item_filter=torch.from_numpy(preds[sel].view(np.int32)).cuda())
    _check(got, (exp_s[sel], exp_r[sel]))
    n2, r2 = idx.filtered_stats()
    assert n2 - n1 == sel.size and r2 - r1 == 0


# ---- 3. IVF dense path -------------------------------------------------------------------------------------------------
def _ivf_small():
    from recommendit_amd import FAISSIndex
    rng = np.random.RandomState(303)
    N, d, nq, k, nlist, nprobe = 6000, 64, 40, 50, 16, 4
    X, Q, C = _ints(rng, N, d), _ints(rng, nq, d), _ints(rng, nlist, d)
    sizes = np.array([1500, 1203, 900, 700, 500, 400, 300, 200, 100, 77, 50, 40, 20, 7, 3, 0])   # uneven; 1203 % 64 != 0; one empty
    assert sizes.sum() == N and sizes.size == nlist
    assign = rng.permutation(np.repeat(np.arange(nlist), sizes)).astype(np.int32)
    tags = rng.randint(0, 64, N).astype(np.uint32)
    idx = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=nprobe)
    idx.build_from_device(torch.from_numpy(X).cuda(), np.arange(N), centroids=C, assign=assign)
    return idx, X, Q, C, assign, tags, N, d, nq, k, nlist, nprobe


def test_ivf_dense_path_equals_oracle():
    idx, X, Q, C, assign, tags, N, d, nq, k, nlist, nprobe = _ivf_small()
    idx.set_item_tags(tags)
    rng = np.random.RandomState(304)
    preds = _mixed_preds(rng, nq)
    preds[0] = (0, 0, 0)
    preds[1] = (0, 63, 0)                    # 1 row in 64 passes: some probed sets hold fewer than k
    preds[2] = (0, 1 << 30, 0)               # none
    qd = torch.from_numpy(Q).cuda()
    exp = _oracle(Q, X, tags, preds, k, ivf=(C, assign, nprobe))
    short = ((exp[1] >= 0).sum(1) < k) & ((exp[1] >= 0).sum(1) > 0)
    assert short.any() and (exp[1][2] == -1).all()
    _check(idx.batch_search_device(qd, k=k, normalized=True, item_filter=preds), exp)
    plain = idx.batch_search_device(qd, k=k, normalized=True)
    got = idx.batch_search_device(qd, k=k, normalized=True, item_filter=(0, 0, 0))
    assert torch.equal(got[1], plain[1]) and torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))
    _check(plain, _oracle(Q, X, tags, np.zeros((nq, 3), np.uint32), k, ivf=(C, assign, nprobe)))
    # one query (the single-request shape of the prepare kernel) with a shared predicate
    _check(idx.batch_search_device(qd[1:2].contiguous(), k=k, normalized=True, item_filter=(0, 63, 0)),
           (exp[0][1:2], exp[1][1:2]))


# ---- 4. IVF thresholded path -------------------------------------------------------------------------------------------
IVF_GROUPS = [("100%", (0, 0, 0)), ("30%", (0, 0, 1 << 8)), ("1%", (1 << 9, 0, 0)), ("0%", (0, 1 << 11, 0))]


@pytest.fixture(scope="module")
def ivf_large():
    """cap_full = 8 lists of ~12 500 > 16 384; 4k = 256 <= cap_full / 16; nq * cap_df = 96 * ~100 000 > 2^23: the
    sampled-threshold pass A and the thresholded pass B run"""
    from recommendit_amd import FAISSIndex
    rng = np.random.RandomState(404)
    N, d, nq, k, nlist, nprobe = 200_000, 32, 96, 64, 16, 8
    X, Q, C = _ints(rng, N, d), _ints(rng, nq, d), _ints(rng, nlist, d)
    assign = rng.randint(0, nlist, N).astype(np.int32)
    assert np.bincount(assign).max() * nprobe * nq > (1 << 23)
    tags = rng.randint(0, 64, N).astype(np.uint32)
    tags[rng.rand(N) < 0.7] |= 1 << 8        # none_of bit 8: 30 % pass
    tags[rng.rand(N) < 0.01] |= 1 << 9       # 1 %
    idx = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=nprobe)
    idx.build_from_device(torch.from_numpy(X).cuda(), np.arange(N), centroids=C, assign=assign)
    idx.set_item_tags(tags)
    exp = {name: _oracle(Q, X, tags, np.tile(np.array(p, np.uint32), (nq, 1)), k, ivf=(C, assign, nprobe))
           for name, p in IVF_GROUPS}           # (computed once: shared by the tests below, never changed)
    return idx, torch.from_numpy(Q).cuda(), exp, nq, k


def test_ivf_thresholded_path_equals_oracle(ivf_large):
    idx, qd, exp, nq, k = ivf_large
    assert (exp["0%"][1] == -1).all() and (exp["1%"][1] >= 0).all()
    for name, p in IVF_GROUPS:
        b = idx.filtered_stats()[1]
        _check(idx.batch_search_device(qd, k=k, normalized=True, item_filter=p), exp[name], name)
        print(f"IVF thresholded, shared {name}: {idx.filtered_stats()[1] - b} of {nq} re-done by the exact fallback")
    _check(idx.batch_search_device(qd, k=k, normalized=True), exp["100%"], "plain")
    # per-query predicates: the four pass rates interleaved in one batch
    grp = np.arange(nq) % len(IVF_GROUPS)
    preds = np.array([IVF_GROUPS[g][1] for g in grp], np.uint32)
    exp_s = np.stack([exp[IVF_GROUPS[g][0]][0][q] for q, g in enumerate(grp)])
    exp_r = np.stack([exp[IVF_GROUPS[g][0]][1][q] for q, g in enumerate(grp)])
    n0, r0 = idx.filtered_stats()
    _check(idx.batch_search_device(qd, k=k, normalized=True, item_filter=preds), (exp_s, exp_r))
    n1, r1 = idx.filtered_stats()
    print(f"IVF thresholded, mixed pass rates: {r1 - r0} of {n1 - n0} queries re-done by the exact fallback")


def test_filtered_search_refused_while_a_deferred_search_is_pending(ivf_large):
    from recommendit_amd import _lib as L
    idx, qd, exp, nq, k = ivf_large
    ref = idx.batch_search_device(qd, k=k, normalized=True, item_filter=(1 << 9, 0, 0))
    idx.set_deferred_check(True)
    try:
        plain = idx.batch_search_device(qd, k=k, normalized=True)
        assert idx.search_pending()
        with pytest.raises(RuntimeError, match="pending"):
            idx.batch_search_device(qd, k=k, normalized=True, item_filter=(1 << 9, 0, 0))
        pred = torch.tensor([1 << 9, 0, 0], dtype=torch.int32, device="cuda")
        s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        r = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        rc = L.lib().rihip_ip_index_search_filtered(idx.index._h, qd.data_ptr(), nq, k, pred.data_ptr(), 0, s.data_ptr(),
                                                    r.data_ptr(), L.stream_ptr())
        assert rc == ERR_STATE
        idx.finish_search()
        assert not idx.search_pending()
        # with the deferred check still switched on, the filtered search checks synchronously and leaves nothing pending
        got = idx.batch_search_device(qd, k=k, normalized=True, item_filter=(1 << 9, 0, 0))
        assert not idx.search_pending()
        assert torch.equal(got[1], ref[1]) and torch.equal(got[0], ref[0])
    finally:
        idx.set_deferred_check(False)


# ---- 4b. the exact re-do applies the predicate too --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_fallback_redo_applies_the_predicate(kind):
    """nine rows in ten are copies of one vector: for the queries that like it, far more passing rows tie at the threshold
    than the candidate list holds, so they are re-done by the exact fallback -- with their own predicates"""
    from recommendit_amd import FAISSIndex
    rng = np.random.RandomState(505)
    if kind == "flat":
        N, d, nq, k = 70001, 32, 130, 100
    else:
        N, d, nq, k, nlist, nprobe = 200_000, 32, 96, 64, 16, 8
    X, Q = _ints(rng, N, d), _ints(rng, nq, d)
    X[rng.rand(N) < 0.9] = 3.0
    tags = rng.randint(0, 64, N).astype(np.uint32)
    tags[rng.rand(N) < 0.01] |= 1 << 9
    preds = np.array([((1, 0, 0), (0, 1 << 9, 0), (0, 2, 4))[q % 3] for q in range(nq)], np.uint32)   # 50 %, 1 %, 25 %
    if kind == "flat":
        idx = FAISSIndex(embed_dim=d, exact=True)
        idx.build_from_device(torch.from_numpy(X).cuda(), np.arange(N))
        ivf = None
    else:
        C = _ints(rng, nlist, d)
        assign = rng.randint(0, nlist, N).astype(np.int32)
        idx = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=nprobe)
        idx.build_from_device(torch.from_numpy(X).cuda(), np.arange(N), centroids=C, assign=assign)
        ivf = (C, assign, nprobe)
    idx.set_item_tags(tags)
    exp = _oracle(Q, X, tags, preds, k, ivf=ivf)
    qd = torch.from_numpy(Q).cuda()
    _check(idx.batch_search_device(qd, k=k, normalized=True, item_filter=preds), exp)
    n, redone = idx.filtered_stats()
    print(f"{kind}, tied corpus: {redone} of {n} queries re-done by the exact fallback")
    assert n == nq and 1 <= redone <= nq - nq // 3          # the 1 % queries keep every passing row: never re-done
    sel = torch.arange(1, nq, 3, device="cuda")
    _check(idx.batch_search_device(qd[sel].contiguous(), k=k, normalized=True, item_filter=(0, 1 << 9, 0)),
           (exp[0][1::3], exp[1][1::3]))
    assert idx.filtered_stats() == (n + sel.numel(), redone)


# ---- 5. handle and API edges -------------------------------------------------------------------------------------------
def test_handle_and_api_edges():
    from recommendit_amd import _lib as L
    idx, X, Q, tags, preds, N, d, nq, k = _flat_small()
    qd = torch.from_numpy(Q).cuda()
    lib = L.lib()
    pred = torch.from_numpy(preds.view(np.int32)).cuda()
    s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    r = torch.empty((nq, k), dtype=torch.int64, device="cuda")

    def c_search(stride=3, kk=k):
        return lib.rihip_ip_index_search_filtered(idx.index._h, qd.data_ptr(), nq, kk, pred.data_ptr(), stride, s.data_ptr(),
                                                  r.data_ptr(), L.stream_ptr())
    assert lib.rihip_ip_index_has_tags(idx.index._h) == 0
    assert c_search() == ERR_STATE                                          # no tags
    idx.set_item_tags(tags)
    assert lib.rihip_ip_index_has_tags(idx.index._h) == 1
    assert c_search(stride=2) != 0 and c_search(kk=0) != 0
    exp_s, exp_r = _oracle(Q, X, tags, preds, k)
    # id map off: row numbers; on: item ids (row + 7)
    L.check(lib.rihip_ip_index_set_id_map(idx.index._h, None), "set_id_map")
    assert c_search() == 0
    _check((s, r), (exp_s, exp_r))
    got = idx.batch_search_device(qd, k=k, normalized=True, item_filter=preds)
    _check(got, (exp_s, np.where(exp_r >= 0, exp_r + 7, -1)))
    # bad predicate shapes
    for bad in ((1, 2), np.zeros((nq, 2), np.uint32), np.zeros((nq + 1, 3), np.uint32), np.zeros((nq, 3), np.float32),
                torch.zeros((nq, 3), dtype=torch.int64, device="cuda"), (1 << 33, 0, 0)):
        with pytest.raises(ValueError):
            idx.batch_search_device(qd, k=k, normalized=True, item_filter=bad)
    # k = 1 and k = ntotal
    for kk in (1, N):
        e = _oracle(Q, X, tags, preds, kk)
        _check(idx.batch_search_device(qd, k=kk, normalized=True, item_filter=preds),
               (e[0], np.where(e[1] >= 0, e[1] + 7, -1)), f"k={kk}")
    # tags keyed by id; unnamed ids keep theirs; clearing
    idx.set_item_tags(np.array([1 << 25, 1 << 25], np.uint32), item_ids=[7 + 5, 7 + 900])
    t2 = tags.copy(); t2[[5, 900]] = 1 << 25
    np.testing.assert_array_equal(idx.item_tags(), t2)
    got = idx.batch_search_device(qd[:3].contiguous(), k=k, normalized=True, item_filter=(0, 1 << 25, 0))
    assert sorted(got[1][0][:2].tolist()) == [12, 907] and (got[1][:, 2:] == -1).all()
    with pytest.raises(ValueError):
        idx.set_item_tags(np.array([1], np.uint32), item_ids=[5])          # id 5 is not stored (ids start at 7)
    with pytest.raises(ValueError):
        idx.set_item_tags(tags[:10])
    idx.clear_item_tags()
    assert not idx.has_item_tags and idx.item_tags() is None
    with pytest.raises(ValueError, match="tags"):
        idx.batch_search_device(qd, k=k, normalized=True, item_filter=preds)


# ---- 6. composition and lifecycle ----------------------------------------------------------------------------------------
def test_filter_composes_with_exclusion():
    from recommendit_amd import SeenItems
    idx, X, Q, tags, preds, N, d, nq, k = _flat_small()
    idx.set_item_tags(tags)
    rng = np.random.RandomState(61)
    full_s, full_r = _oracle(Q, X, tags, preds, N)
    lists, allowed = [], np.ones((nq, N), bool)
    for q in range(nq):
        head = full_r[q, :(0, 1, 20, 60)[q % 4]]
        lst = np.unique(np.concatenate([head[head >= 0], rng.choice(N, 100, replace=False)]))
        lists.append(lst + 7)                                               # item ids
        allowed[q, lst] = False
    store = SeenItems.from_pairs(np.repeat(np.arange(nq), [len(l) for l in lists]), np.concatenate(lists), n_users=nq)
    exp_s, exp_r = _oracle(Q, X, tags, preds, k, allowed=allowed)
    exp_i = np.where(exp_r >= 0, exp_r + 7, -1)
    qd = torch.from_numpy(Q).cuda()
    for uids in (list(range(nq)), torch.arange(nq, device="cuda")):
        _check(idx.batch_search_device(qd, k=k, normalized=True, exclude=store, user_ids=uids, item_filter=preds),
               (exp_s, exp_i))
    assert idx.exclusion_deficit() == 0


def test_tags_follow_the_live_catalogue_and_persistence(tmp_path):
    from recommendit_amd import FAISSIndex
    idx, X, Q, C, assign, tags, N, d, nq, k, nlist, nprobe = _ivf_small()
    rng = np.random.RandomState(62)
    qd = torch.from_numpy(Q).cuda()
    preds = _mixed_preds(rng, nq)
    # an untagged index: updates and saved files as they always were
    p0 = tmp_path / "plain.idx"
    idx.save(str(p0))
    plain_idx, plain_meta = p0.read_bytes(), p0.with_suffix(".meta.pkl").read_bytes()
    assert sorted(pickle.loads(plain_meta)) == ["embed_dim", "item_id_to_faiss_idx", "item_ids", "n_lists", "n_probe"]
    idx.set_item_tags(tags)
    p1 = tmp_path / "tagged.idx"
    idx.save(str(p1))
    assert p1.read_bytes() == plain_idx                                      # the handle file does not carry tags
    meta = pickle.loads(p1.with_suffix(".meta.pkl").read_bytes())
    assert sorted(meta) == ["embed_dim", "item_id_to_faiss_idx", "item_ids", "item_tags", "n_lists", "n_probe"]
    np.testing.assert_array_equal(meta["item_tags"], tags)
    back = FAISSIndex.load(str(p1))
    assert back.has_item_tags
    np.testing.assert_array_equal(back.item_tags(), tags)
    ref = idx.batch_search_device(qd, k=k, normalized=True, item_filter=preds)
    got = back.batch_search_device(qd, k=k, normalized=True, item_filter=preds)
    assert torch.equal(got[1], ref[1]) and torch.equal(got[0], ref[0])
    idx.clear_item_tags()
    p2 = tmp_path / "cleared.idx"
    idx.save(str(p2))
    assert p2.read_bytes() == plain_idx and p2.with_suffix(".meta.pkl").read_bytes() == plain_meta
    assert not FAISSIndex.load(str(p2)).has_item_tags
    # tagged index: remove + add(tags=) + update
    idx.set_item_tags(tags)
    ids = np.arange(N)
    cur_x, cur_t, cur_ids = X.copy(), tags.copy(), ids.copy()
    drop = rng.choice(N, 400, replace=False)
    assert idx.remove_items(drop) == 400
    keep = ~np.isin(cur_ids, drop)
    cur_x, cur_t, cur_ids = cur_x[keep], cur_t[keep], cur_ids[keep]
    assert idx.has_item_tags
    np.testing.assert_array_equal(idx.item_tags(), cur_t)
    add_x, add_t = _ints(rng, 300, d), rng.randint(0, 64, 300).astype(np.uint32)
    add_ids = np.arange(N, N + 300)
    idx.add_items_device(torch.from_numpy(add_x).cuda(), add_ids, tags=add_t)
    cur_x, cur_t, cur_ids = np.concatenate([cur_x, add_x]), np.concatenate([cur_t, add_t]), np.concatenate([cur_ids, add_ids])
    idx.add_items_device(torch.from_numpy(add_x[:5].copy()).cuda(), np.arange(N + 300, N + 305))      # no tags: 0
    cur_x, cur_t = np.concatenate([cur_x, add_x[:5]]), np.concatenate([cur_t, np.zeros(5, np.uint32)])
    cur_ids = np.concatenate([cur_ids, np.arange(N + 300, N + 305)])
    # update_items normalises on the host: use unit-length integer rows (one +-1 entry) so they stay exact
    up_ids = np.concatenate([cur_ids[rng.choice(cur_ids.size, 50, replace=False)], [N + 1000, N + 1001]])
    up_x = np.zeros((up_ids.size, d), np.float32)
    up_x[np.arange(up_ids.size), rng.randint(0, d, up_ids.size)] = rng.choice([-1.0, 1.0], up_ids.size)
    up_t = rng.randint(0, 64, up_ids.size).astype(np.uint32)
    idx.update_items(up_x, up_ids, tags=up_t)
    keep = ~np.isin(cur_ids, up_ids)
    cur_x, cur_t = np.concatenate([cur_x[keep], up_x]), np.concatenate([cur_t[keep], up_t])
    cur_ids = np.concatenate([cur_ids[keep], up_ids])
    # update_items without tags: a replaced id keeps its word, a new id gets 0
    up2 = np.array([cur_ids[3], N + 2000])
    up2_x = np.zeros((2, d), np.float32); up2_x[0, 1] = 1.0; up2_x[1, 2] = -1.0
    idx.update_items(up2_x, up2)
    t3 = cur_t[3]
    keep = ~np.isin(cur_ids, up2)
    cur_x, cur_t = np.concatenate([cur_x[keep], up2_x]), np.concatenate([cur_t[keep], [t3, 0]]).astype(np.uint32)
    cur_ids = np.concatenate([cur_ids[keep], up2])
    np.testing.assert_array_equal(idx.item_ids, cur_ids)
    np.testing.assert_array_equal(idx.item_tags(), cur_t)
    # == a from-scratch build of the final corpus with the final tags
    fresh = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=nprobe)
    fresh.build_from_device(torch.from_numpy(cur_x).cuda(), cur_ids, centroids=C, assign=idx.list_assignment())
    fresh.set_item_tags(cur_t)
    a = idx.batch_search_device(qd, k=k, normalized=True, item_filter=preds)
    b = fresh.batch_search_device(qd, k=k, normalized=True, item_filter=preds)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    e = _oracle(Q, cur_x, cur_t, preds, k, ivf=(C, idx.list_assignment(), nprobe))
    _check(a, (e[0], np.where(e[1] >= 0, cur_ids[np.maximum(e[1], 0)], -1)))
    with pytest.raises(ValueError, match="tags"):
        FAISSIndex.load(str(p2)).add_items_device(torch.from_numpy(add_x[:1].copy()).cuda(), [N + 5000], tags=[1])


# ---- 7. the serving pipeline ---------------------------------------------------------------------------------------------
def _pipeline(tmp_path, nu=120, ni=3000, d=64, H=128, kc=200):
    """the small pipeline of tests/test_gpu_exclude.py; genre 17 is rare (fewer than 20 items)"""
    from recommendit_amd import FAISSIndex, LightGBMRanker, TwoTowerModel
    from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns
    sd = fx.make_state(nu, ni, d, H, seed=21)
    model = TwoTowerModel(nu, ni, d, H)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    rng = np.random.RandomState(2)
    item_ids = list(range(1, ni + 1))
    genres = (rng.rand(ni, 18) < 0.15).astype(np.float32)
    genres[:, 17] = 0
    genres[rng.choice(ni, 12, replace=False), 17] = 1
    E = model.get_item_embeddings(item_ids, genres)
    index = FAISSIndex(embed_dim=d, exact=True)
    index.build_ivf_index(E, item_ids)
    forest = G.random_forest_model(60, 31, 50, seed=5, names=feature_columns())
    p = tmp_path / "r.lgbm"
    p.write_text(G.write_text_model(forest))
    ranker = LightGBMRanker.load(str(p))
    store = GpuFeatureStore(nu, ni)
    ut = store.user.copy(); it = store.item.copy()
    ut[1:, :6] = rng.rand(nu, 6) * [5, 8, 1, 1, 1, 1]; ut[1:, 6:] = rng.rand(nu, 18)
    it[1:, :5] = rng.rand(ni, 5) * [5, 9, 1, 1.5, 1]; it[1:, 5:] = genres
    store.load_arrays(ut, it)
    pipe = GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=kc, top_k_results=20)
    return pipe, model, index, forest, E, item_ids, ut, it, genres


def test_pipeline_serves_a_genre_filter(tmp_path):
    from recommendit_amd import SeenItems
    from recommendit_amd.recommender import feature_columns
    pipe, model, index, forest, E, item_ids, ut, it, genres = _pipeline(tmp_path)
    users = list(range(1, 41))
    base = [t.clone() for t in pipe.recommend_batch(users)]
    with pytest.raises(ValueError, match="tags"):
        pipe.recommend_batch(users, item_filter=(1, 0, 0))
    tags = pipe.store.item_genre_tags(item_ids)
    np.testing.assert_array_equal(tags, (genres > 0).astype(np.int64) @ (1 << np.arange(18)))
    index.set_item_tags(tags)
    # item_filter=None: bitwise what it was without tags
    again = pipe.recommend_batch(users)
    assert all(torch.equal(a, b) for a, b in zip(again, base))
    with pytest.raises(ValueError, match="graph"):
        pipe.recommend_batch(users[:4], graph=True, item_filter=(1, 0, 0))
    U = np.stack([model.get_user_embedding(u) for u in users])
    Un, En = R.normalize_rows(U), R.normalize_rows(E)
    _, rows = R.topk_ip_exact(Un, En, len(item_ids))
    for g in (3, 17):
        ids, sc, rs = [t.cpu().numpy() for t in pipe.recommend_batch(users, item_filter=(1 << g, 0, 0))]
        has = genres[:, g] > 0
        n_has = int(has.sum())
        for qi, u in enumerate(users):
            got = ids[qi][ids[qi] >= 0]
            assert it[got, 5 + g].all(), (g, u)                              # only items of the genre (store's vector)
            full = np.array([item_ids[r] for r in rows[qi]])
            cand = full[has[full - 1]][:200].tolist()
            n = min(20, len(cand))
            assert got.size == n and (ids[qi][n:] == -1).all()
            user_feat = dict(zip([nm for nm, _ in RF.USER_SCALARS], ut[u, :6]), genre_pref=list(ut[u, 6:]))
            items = {c: dict(zip([nm for nm, _ in RF.ITEM_SCALARS], it[c, :5]), genre_vector=list(it[c, 5:])) for c in cand}
            X = RF.feature_matrix(RF.build_ranking_features(user_feat, items, cand), feature_columns())
            s = G.predict_raw(forest, X)
            order = np.argsort(-s, kind="stable")[:n]
            np.testing.assert_allclose(sc[qi][:n], s[order], rtol=0, atol=1e-12)
            assert len(set(got.tolist()) - set(cand)) <= 1                    # (retrieval near-ties at the 200th candidate)
        if g == 17:
            assert n_has == 12 and (ids[:, 12:] == -1).all() and (ids[:, :12] >= 0).all()
    # batch == single request
    one = pipe.get_recommendations(users[5], item_filter=(1 << 3, 0, 0))
    ids3 = pipe.recommend_batch(users, item_filter=(1 << 3, 0, 0))[0].cpu().numpy()
    assert [r["item_id"] for r in one] == ids3[5].tolist()
    with pytest.raises(ValueError, match="graph"):
        pipe.get_recommendations(users[5], graph=True, item_filter=(1 << 3, 0, 0))
    # with a seen store: filter AND not-seen
    seen = {u: ids3[qi][:5].tolist() for qi, u in enumerate(users)}
    pipe.set_seen(SeenItems.from_dict(seen, n_users=121))
    ids4 = pipe.recommend_batch(users, item_filter=(1 << 3, 0, 0))[0].cpu().numpy()
    for qi, u in enumerate(users):
        got = ids4[qi][ids4[qi] >= 0]
        assert got.size == 20 and it[got, 5 + 3].all() and not np.isin(got, seen[u]).any()
    assert pipe.exclusion_deficit() == 0
    pipe.set_seen(None)
    assert all(torch.equal(a, b) for a, b in zip(pipe.recommend_batch(users), base))
