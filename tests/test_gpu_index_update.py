"""GPU: add_items / remove_items / update_items of a built FAISSIndex (csrc/index_update.hip).

An update is one repack of the corpus under the existing centroids, and it must leave the handle bit for bit in the
state a from-scratch build of the final corpus with the same centroids and the same list of every row gives.  So the
core check is EQUALITY (saved files byte-identical, arrays equal, search results equal), not a tolerance; the oracle
(oracle/retrieval_np.py) is compared with the tolerance of tests/test_gpu_ivf_oracle.py, whose helpers are restated here."""
import pickle

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import gbdt_np as G
from oracle import retrieval_np as R

pytestmark = pytest.mark.gpu
TOL = 2e-6


# ---- helpers restated from tests/test_gpu_ivf_oracle.py ------------------------------------------------------------------
def _clustered(rng, N, d, n_centers, spread=0.35):
    """unit rows around n_centers directions: what item-tower outputs look like (lists of uneven size)"""
    centers = fx.unit_rows(rng, n_centers, d)
    w = rng.dirichlet(np.full(n_centers, 0.7))
    which = rng.choice(n_centers, N, p=w)
    X = centers[which] + spread * rng.randn(N, d).astype(np.float32) / np.sqrt(d)
    return R.normalize_rows(X)


def _compare_search(idx, Q, X, nprobe, k, min_checked=0.9):
    C, a = idx.centroids(), idx.list_assignment()
    sc, rows = idx.batch_search(Q, k=k)
    kk = min(k, X.shape[0])
    o_s, o_r, probe, coarse = R.ivf_search(Q, X, C, a, nprobe, kk, return_probe=True)
    srt = -np.sort(-coarse, axis=1)
    checked = 0
    for q in range(Q.shape[0]):
        if nprobe < C.shape[0] and srt[q, nprobe - 1] - srt[q, nprobe] < 4 * TOL:
            continue                                   # coarse boundary is a float near-tie: either list set is right
        checked += 1
        n_ok = int((o_r[q] >= 0).sum())
        assert int((rows[q] >= 0).sum()) == n_ok, (q, n_ok)                 # same number of results, same -1 padding
        assert (rows[q, n_ok:] == -1).all() and np.isneginf(sc[q, n_ok:]).all()
        np.testing.assert_allclose(sc[q, :n_ok], o_s[q, :n_ok], atol=TOL, rtol=0)
        if (rows[q, :n_ok] == o_r[q, :n_ok]).all():
            continue
        # order/membership may differ only among float near-ties
        diff = np.nonzero(rows[q, :n_ok] != o_r[q, :n_ok])[0]
        for i in diff:                                   # position i ties with a neighbour (f32 vs f64 rounding)
            gaps = [abs(float(o_s[q, i]) - float(o_s[q, j])) for j in (i - 1, i + 1) if 0 <= j < n_ok]
            assert min(gaps) < 4 * TOL or i == n_ok - 1, (q, i, gaps)
        extra = set(rows[q, :n_ok].tolist()) ^ set(o_r[q, :n_ok].tolist())
        if extra:                                       # a swap across the k-th boundary: scores equal within TOL
            true = X[sorted(extra)].astype(np.float64) @ Q[q].astype(np.float64)
            assert np.abs(true - o_s[q, n_ok - 1]).max() < 4 * TOL, (q, extra)
    assert checked >= min_checked * Q.shape[0], checked
    return sc, rows, o_s, o_r


class _RowView:
    """an index whose batch_search answers in ROW numbers (what _compare_search compares with the oracle's rows)"""

    def __init__(self, idx):
        self.idx = idx

    def centroids(self):
        return self.idx.centroids()

    def list_assignment(self):
        return self.idx.list_assignment()

    def batch_search(self, Q, k):
        sc, ids = self.idx.batch_search(Q, k=k)
        order = np.argsort(self.idx.item_ids, kind="stable")
        pos = np.searchsorted(self.idx.item_ids[order], np.where(ids < 0, self.idx.item_ids[order[0]], ids))
        return sc, np.where(ids < 0, -1, order[pos])


# ---- the NumPy model of an index: (ids, vectors, list of every row) ------------------------------------------------------
class _Model:
    def __init__(self, X, ids, lists=None):
        self.X, self.ids = X.copy(), np.asarray(ids, dtype=np.int64).copy()
        self.lists = None if lists is None else np.asarray(lists, dtype=np.int32).copy()

    def remove(self, ids):
        gone = np.isin(self.ids, np.asarray(ids, dtype=np.int64))
        self.X, self.ids = self.X[~gone], self.ids[~gone]
        if self.lists is not None:
            self.lists = self.lists[~gone]
        return int(gone.sum())

    def add(self, X, ids, lists=None):
        self.X = np.concatenate([self.X, X])
        self.ids = np.concatenate([self.ids, np.asarray(ids, dtype=np.int64)])
        if self.lists is not None:
            self.lists = np.concatenate([self.lists, np.asarray(lists, dtype=np.int32)])


def _ivf(X, ids, C, a, nprobe):
    from recommendit_amd import FAISSIndex
    idx = FAISSIndex(embed_dim=X.shape[1], n_lists=C.shape[0], n_probe=nprobe)
    idx.build_from_device(torch.from_numpy(np.ascontiguousarray(X)).cuda(), np.asarray(ids, dtype=np.int64), centroids=C,
                          assign=np.asarray(a, dtype=np.int32))
    return idx


def _flat(X, ids):
    from recommendit_amd import FAISSIndex
    idx = FAISSIndex(embed_dim=X.shape[1], exact=True)
    idx.build_from_device(torch.from_numpy(np.ascontiguousarray(X)).cuda(), np.asarray(ids, dtype=np.int64))
    return idx


def _assigned(idx, X):
    """the index's own list of rows that are not stored (the device quantizer)"""
    return idx.assign_lists(torch.from_numpy(np.ascontiguousarray(X)).cuda()).cpu().numpy()


def _assert_same_state(A, B, tmp_path, Q, k, tag):
    """A (updated) against B (built from scratch): files, arrays and search results are EQUAL"""
    p1, p2 = tmp_path / f"{tag}_a.idx", tmp_path / f"{tag}_b.idx"
    A.save(str(p1))
    B.save(str(p2))
    assert p1.read_bytes() == p2.read_bytes(), tag
    assert A.index.ntotal == B.index.ntotal
    np.testing.assert_array_equal(A.item_ids, B.item_ids)
    np.testing.assert_array_equal(A._item_ids_dev.cpu().numpy(), B.item_ids)
    np.testing.assert_array_equal(A.reconstruct(), B.reconstruct())
    if A.index.is_ivf:
        np.testing.assert_array_equal(A.centroids(), B.centroids())
        np.testing.assert_array_equal(A.list_assignment(), B.list_assignment())
        assert A.list_stats() == B.list_stats()
    sa, ia = A.batch_search(Q, k=k)
    sb, ib = B.batch_search(Q, k=k)
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(sa, sb)
    return sa, ia


def _sizes(idx):
    return np.bincount(idx.list_assignment(), minlength=idx.centroids().shape[0])


# ---- 1. state equality ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N0,nlist", [(64, 30000, 40), (96, 30000, 40), (32, 30000, 257)])
def test_update_leaves_the_state_of_a_from_scratch_build(tmp_path, d, N0, nlist):
    """d = 96 runs at the kernel width 128 (du < d).  Steps: (a) a list emptied completely + unknown drop ids, nothing
    added; (b) rows added, nothing dropped, so that a list ends exactly on a 64-row granule; (c) that list grows across
    the boundary; (d) an upsert of stored and new ids."""
    rng = np.random.RandomState(71 + d)
    nprobe, k = 6, 100
    Xall = _clustered(rng, N0 + 20000, d, 20)
    X0, pool = Xall[:N0], Xall[N0:]
    C = R.kmeans_ip(X0, nlist, n_iter=2, seed=7)
    a0 = R.ivf_assign(X0, C).astype(np.int32)
    ids0 = np.arange(1000, 1000 + N0, dtype=np.int64)
    pool_ids = np.arange(500000, 500000 + len(pool), dtype=np.int64)
    Q = np.concatenate([fx.unit_rows(rng, 60, d), pool[:20], X0[:20]])
    A = _ivf(X0, ids0, C, a0, nprobe)
    m = _Model(X0, ids0, a0)
    pool_list = _assigned(A, pool)
    assert A.list_stats()["n_lists"] == nlist

    def check(tag):
        B = _ivf(m.X, m.ids, C, m.lists, nprobe)
        _assert_same_state(A, B, tmp_path, Q, k, tag)
        np.testing.assert_array_equal(_sizes(A), np.bincount(m.lists, minlength=nlist))

    # (a) empty the smallest non-empty list; ids that are not stored are ignored and not counted; n_add = 0
    sizes = np.bincount(a0, minlength=nlist)
    victim = int(np.where(sizes > 0, sizes, N0 + 1).argmin())
    gone = ids0[a0 == victim]
    n = A.remove_items(np.concatenate([[7, 999, 10**12], gone[::-1], [-5]]))
    assert n == len(gone) == m.remove(gone)
    assert _sizes(A)[victim] == 0 and A.list_stats()["empty"] == int((np.bincount(m.lists, minlength=nlist) == 0).sum())
    check("a")
    # (b) n_drop = 0: the list with most pool rows is filled up to a granule boundary exactly
    T = int(np.bincount(pool_list, minlength=nlist).argmax())
    of_T = np.nonzero(pool_list == T)[0]
    fill = int(-_sizes(A)[T] % 64) or 64
    assert len(of_T) >= fill + 3, (len(of_T), fill)
    others = np.nonzero(pool_list != T)[0][:500]
    pick = np.sort(np.concatenate([of_T[:fill], others]))
    assert A.add_items_device(torch.from_numpy(pool[pick]).cuda(), pool_ids[pick]) == len(pick)
    m.add(pool[pick], pool_ids[pick], pool_list[pick])
    assert _sizes(A)[T] % 64 == 0
    check("b")
    # (c) three more rows of that list: it grows across the granule boundary
    pick = of_T[fill:fill + 3]
    assert A.add_items_device(torch.from_numpy(pool[pick]).cuda(), pool_ids[pick]) == 3
    m.add(pool[pick], pool_ids[pick], pool_list[pick])
    assert _sizes(A)[T] % 64 == 3
    check("c")
    # (d) upsert through the host entry (rows are normalised as build_ivf_index does): 300 stored ids get a new vector,
    # 200 ids are new
    stored = rng.choice(m.ids, 300, replace=False)
    fresh = np.arange(900000, 900200, dtype=np.int64)
    E = (3.0 * _clustered(rng, 500, d, 20)).astype(np.float32)
    En = np.ascontiguousarray(E / np.maximum(np.linalg.norm(E, axis=1, keepdims=True), 1e-8), dtype=np.float32)
    up_ids = np.concatenate([stored[:150], fresh, stored[150:]])
    assert A.update_items(E, up_ids) == (300, 200)
    assert m.remove(stored) == 300
    m.add(En, up_ids, _assigned(A, En))
    check("d")


# ---- 2. against the oracle ------------------------------------------------------------------------------------------------------
def test_updated_index_against_the_oracle():
    rng = np.random.RandomState(81)
    Xall = _clustered(rng, 34000, 64, 20)
    X0, Xa = Xall[:30000], Xall[30000:]
    C = R.kmeans_ip(X0, 40, n_iter=3, seed=7)
    a0 = R.ivf_assign(X0, C)
    rm = rng.choice(30000, 3000, replace=False)
    Q = np.concatenate([fx.unit_rows(rng, 100, 64), Xa[:28]])
    nprobe, k = 6, 100
    A = _ivf(X0, np.arange(30000), C, a0, nprobe)
    assert A.remove_items(rm) == 3000
    assert A.add_items_device(torch.from_numpy(Xa).cuda(), np.arange(30000, 34000)) == 4000
    keep = np.ones(30000, dtype=bool)
    keep[rm] = False
    Xf = np.concatenate([X0[keep], Xa])
    np.testing.assert_array_equal(A.item_ids, np.concatenate([np.arange(30000)[keep], np.arange(30000, 34000)]))
    np.testing.assert_array_equal(A.reconstruct(), Xf)
    # the list of every added row is the oracle's arg-max wherever the margin is clear
    got = A.list_assignment()
    np.testing.assert_array_equal(got[:27000], a0[keep])
    S = Xa.astype(np.float64) @ C.astype(np.float64).T
    srt = -np.sort(-S, axis=1)
    clear = srt[:, 0] - srt[:, 1] > 4 * TOL
    print("clear arg-max margin:", clear.mean())
    assert clear.mean() > 0.99
    np.testing.assert_array_equal(got[27000:][clear], R.ivf_assign(Xa, C)[clear])
    sc, rows, o_s, o_r = _compare_search(_RowView(A), Q, Xf, nprobe, k)
    share = float((rows >= 27000).mean())
    print("share of hits that are added rows:", share, "| empty lists:", A.list_stats()["empty"])
    assert share > 0.02                                  # the added rows are really served
    assert A.list_stats()["empty"] == int((np.bincount(got, minlength=40) == 0).sum())


# ---- 3. flat index ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N0,n_rm,n_add", [(20000, 1500, 700), (70000, 2000, 3000), (66000, 1500, 0), (65000, 0, 2500)])
def test_flat_index_update_equals_a_from_scratch_build(tmp_path, N0, n_rm, n_add):
    """the bf16 filter copy exists above 65 536 rows: a corpus below, one above, one update that crosses the size
    downwards and one upwards; above it the two-precision result equals the all-f32 search"""
    from recommendit_amd import _lib
    rng = np.random.RandomState(83)
    d, k = 64, 200
    Xall = fx.unit_rows(rng, N0 + n_add, d)
    X0, Xa = Xall[:N0], Xall[N0:]
    ids0 = np.arange(10, 10 + N0, dtype=np.int64)
    add_ids = np.arange(10**6, 10**6 + n_add, dtype=np.int64)
    Q = np.concatenate([fx.unit_rows(rng, 100, d), X0[:14], Xa[:14]])
    A = _flat(X0, ids0)
    m = _Model(X0, ids0)
    rm = rng.choice(ids0, n_rm, replace=False)
    if n_rm and n_add:
        assert A.remove_items(rm) == n_rm
        assert A.add_items_device(torch.from_numpy(Xa).cuda(), add_ids) == n_add
    elif n_rm:
        assert A.remove_items(np.concatenate([rm, [3, 4]])) == n_rm
    else:
        assert A.add_items(Xa, add_ids) == n_add            # unit rows: the host normalisation divides by ~1
        Xa = np.ascontiguousarray(Xa / np.maximum(np.linalg.norm(Xa, axis=1, keepdims=True), 1e-8), dtype=np.float32)
    m.remove(rm)
    m.add(Xa, add_ids)
    assert A.list_stats() == {"n_lists": 0}
    B = _flat(m.X, m.ids)
    s2, r2 = _assert_same_state(A, B, tmp_path, Q, k, "flat")
    o_s, o_r = R.topk_ip_exact(Q, m.X, k)
    np.testing.assert_allclose(s2, o_s, atol=TOL, rtol=0)
    assert (r2 == m.ids[o_r]).mean() > 0.995                                  # near-tie swaps only
    # test_two_precision_search_equals_all_f32, after an update
    _lib.check(_lib.lib().rihip_ip_index_set_two_precision(A.index._h, 0))
    s1, r1 = A.batch_search(Q, k=k)
    np.testing.assert_allclose(s2, s1, atol=1e-6, rtol=0)
    assert (r1 == r2).mean() > 0.999


# ---- 4. a sequence of updates ------------------------------------------------------------------------------------------------
def test_twenty_random_updates_follow_the_model(tmp_path):
    rng = np.random.RandomState(85)
    d, N0, nlist, nprobe = 64, 6000, 16, 4
    Xall = _clustered(rng, N0 + 8000, d, 12)
    X0, pool = Xall[:N0], Xall[N0:]
    C = R.kmeans_ip(X0, nlist, n_iter=2, seed=3)
    a0 = R.ivf_assign(X0, C).astype(np.int32)
    ids0 = rng.permutation(10 * N0)[:N0].astype(np.int64)            # ids in no order
    A = _ivf(X0, ids0, C, a0, nprobe)
    m = _Model(X0, ids0, a0)
    pool_list = _assigned(A, pool)
    next_pool, next_id, graveyard = 0, 10**7, []
    Q = np.concatenate([fx.unit_rows(rng, 40, d), pool[:12]])
    for step in range(20):
        op = step % 4
        take = int(rng.randint(1, 400))
        rows = np.arange(next_pool, next_pool + take)
        next_pool += take
        if op == 0:                                       # remove stored ids (+ some that are not stored)
            ids = rng.choice(m.ids, int(rng.randint(1, 500)), replace=False)
            graveyard.extend(ids[:50].tolist())
            assert A.remove_items(np.concatenate([ids, [-1 - step]])) == m.remove(ids) == len(ids)
        elif op == 1:                                     # add: new ids and ids that were removed earlier (re-add)
            back = np.array(graveyard[:min(len(graveyard), take // 2)], dtype=np.int64)
            graveyard = graveyard[len(back):]
            ids = np.concatenate([back, np.arange(next_id, next_id + take - len(back))])
            next_id += take
            assert A.add_items_device(torch.from_numpy(pool[rows]).cuda(), ids) == take
            m.add(pool[rows], ids, pool_list[rows])
        elif op == 2:                                     # upsert
            stored = rng.choice(m.ids, take // 2, replace=False)
            ids = rng.permutation(np.concatenate([stored, np.arange(next_id, next_id + take - len(stored))]))
            next_id += take
            assert A.update_items(pool[rows], ids) == (len(stored), take - len(stored))
            m.remove(stored)
            Xn = np.ascontiguousarray(pool[rows] / np.maximum(np.linalg.norm(pool[rows], axis=1, keepdims=True), 1e-8),
                                      dtype=np.float32)
            m.add(Xn, ids, _assigned(A, Xn))
        else:                                             # remove and re-add the same ids with the same vectors
            sel = rng.choice(len(m.ids), min(take, 200), replace=False)
            ids, X, lists = m.ids[sel], m.X[sel], m.lists[sel]
            assert A.remove_items(ids) == m.remove(ids)
            assert A.add_items_device(torch.from_numpy(np.ascontiguousarray(X)).cuda(), ids) == len(ids)
            m.add(X, ids, lists)
        np.testing.assert_array_equal(A.item_ids, m.ids)
        np.testing.assert_array_equal(A.reconstruct(), m.X)
        np.testing.assert_array_equal(A.list_assignment(), m.lists)
        assert A.index.ntotal == len(m.ids) == A.stats()["n_vectors"] == A.stats()["n_item_ids"]
        assert A._item_id_to_faiss_idx == {int(i): r for r, i in enumerate(m.ids)}
        st = A.list_stats()
        sz = np.bincount(m.lists, minlength=nlist)
        assert (st["min"], st["max"], st["empty"]) == (sz.min(), sz.max(), int((sz == 0).sum()))
    _compare_search(_RowView(A), Q, m.X, nprobe, 100)
    _assert_same_state(A, _ivf(m.X, m.ids, C, m.lists, nprobe), tmp_path, Q, 100, "seq")


# ---- 5. update_items ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_update_items_equals_remove_then_add(tmp_path, exact):
    rng = np.random.RandomState(87)
    d, N0 = 32, 9000
    X0 = _clustered(rng, N0, d, 10)
    ids0 = np.arange(N0, dtype=np.int64) * 3
    C = R.kmeans_ip(X0, 12, n_iter=2, seed=3)
    a0 = R.ivf_assign(X0, C)
    mk = (lambda: _flat(X0, ids0)) if exact else (lambda: _ivf(X0, ids0, C, a0, 4))
    A, B = mk(), mk()
    E = 2.0 * _clustered(rng, 700, d, 10)
    ids = np.concatenate([rng.choice(ids0, 450, replace=False), np.arange(1, 750, 3)])    # 450 stored, 250 unknown
    ids = rng.permutation(ids)
    assert A.update_items(E, ids) == (450, 250)
    assert B.remove_items(ids) == 450
    assert B.add_items(E, ids) == 700
    Q = np.concatenate([fx.unit_rows(rng, 50, d), R.normalize_rows(E[:14])])
    _assert_same_state(A, B, tmp_path, Q, 50, "upsert")
    assert A.update_items(np.empty((0, d), np.float32), []) == (0, 0)


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_rejected_updates_leave_the_index_as_it_was(exact):
    from recommendit_amd import FAISSIndex, _lib
    rng = np.random.RandomState(89)
    d, N0 = 64, 5000
    X0 = _clustered(rng, N0, d, 10)
    ids0 = np.arange(100, 100 + N0, dtype=np.int64)
    C = R.kmeans_ip(X0, 10, n_iter=2, seed=3)
    A = _flat(X0, ids0) if exact else _ivf(X0, ids0, C, R.ivf_assign(X0, C), 4)
    Q = fx.unit_rows(rng, 30, d)
    s0, i0 = A.batch_search(Q, k=40)
    gen0 = int(_lib.lib().rihip_scratch_generation())
    new = fx.unit_rows(rng, 4, d)
    with pytest.raises(ValueError, match="103"):                      # stored and not dropped in the same call
        A.add_items(new, [9001, 9002, 103, 9003])
    with pytest.raises(ValueError, match="9002"):                     # repeated inside one call
        A.add_items(new, [9001, 9002, 9003, 9002])
    with pytest.raises(ValueError, match="9002"):
        A.update_items(new, [9001, 9002, 9003, 9002])
    with pytest.raises(ValueError, match="177"):
        A.remove_items([150, 177, 160, 177])
    with pytest.raises(ValueError):                                   # wrong width
        A.add_items(fx.unit_rows(rng, 4, d // 2), [9001, 9002, 9003, 9004])
    with pytest.raises(ValueError):
        A.add_items_device(torch.from_numpy(fx.unit_rows(rng, 4, d + 4)).cuda(), [9001, 9002, 9003, 9004])
    with pytest.raises(ValueError):                                   # ids and rows do not pair up
        A.add_items(new, [9001, 9002])
    with pytest.raises(ValueError, match="empty"):                    # would leave the index empty
        A.remove_items(ids0)
    # nothing to do: nothing changes, nothing is re-captured
    assert A.remove_items([]) == 0 and A.remove_items([1, 2, 10**9]) == 0
    assert A.add_items(np.empty((0, d), np.float32), []) == 0
    assert int(_lib.lib().rihip_scratch_generation()) == gen0
    assert A.index.ntotal == N0 and A._item_id_to_faiss_idx == {} and not A._id_map_stale
    np.testing.assert_array_equal(A.item_ids, ids0)
    s1, i1 = A.batch_search(Q, k=40)
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_array_equal(s1, s0)
    # an accepted update is seen by graph holders: the generation advances
    assert A.remove_items([150]) == 1
    assert int(_lib.lib().rihip_scratch_generation()) > gen0
    for call in (lambda e: e.add_items(new, [1, 2, 3, 4]), lambda e: e.remove_items([1]),
                 lambda e: e.update_items(new, [1, 2, 3, 4]), lambda e: e.list_stats(),
                 lambda e: e.add_items_device(torch.from_numpy(new).cuda(), [1, 2, 3, 4])):
        with pytest.raises(RuntimeError, match="Index not built."):
            call(FAISSIndex(embed_dim=d, exact=exact))


def test_update_refused_while_a_deferred_check_is_pending():
    """shape of test_deferred_exactness_check_equals_the_synchronous_search: the thresholded IVF pass defers its check"""
    from recommendit_amd import FAISSIndex
    rng = np.random.RandomState(5)
    N, d, nq, k = 300_000, 128, 600, 500
    X = fx.unit_rows(rng, N, d)
    X[:6000] = X[0]                                         # (one long list, as there: the scan takes its thresholded path)
    idx = FAISSIndex(embed_dim=d, n_lists=100, n_probe=10)
    idx.build_from_device(torch.from_numpy(X).cuda(), np.arange(N))
    q = torch.from_numpy(fx.unit_rows(rng, nq, d)).cuda()
    s0, r0 = idx.batch_search_device(q, k=k, normalized=True)
    idx.set_deferred_check(True)
    s1, r1 = idx.batch_search_device(q, k=k, normalized=True)
    assert idx.search_pending()
    with pytest.raises(RuntimeError, match="pending"):
        idx.remove_items([7000])
    with pytest.raises(RuntimeError, match="pending"):
        idx.add_items(X[:2], [N + 1, N + 2])
    idx.finish_search()
    idx.set_deferred_check(False)
    assert idx.index.ntotal == N
    torch.testing.assert_close(r1, r0, rtol=0, atol=0)
    assert idx.remove_items([7000]) == 1 and idx.index.ntotal == N - 1
    s2, r2 = idx.batch_search_device(q, k=k, normalized=True)
    assert not (r2 == 7000).any()


# ---- 7. persistence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_updated_index_saves_and_loads_in_both_formats(tmp_path, exact):
    from recommendit_amd import FAISSIndex
    rng = np.random.RandomState(91)
    d, N0 = 64, 8000
    Xall = _clustered(rng, N0 + 900, d, 10)
    X0, Xa = Xall[:N0], Xall[N0:]
    ids0 = list(range(500, 500 + N0))
    A = FAISSIndex(embed_dim=d, n_lists=20, n_probe=5, exact=exact)
    A.build_ivf_index(X0, ids0)
    assert A._item_id_to_faiss_idx == {i: r for r, i in enumerate(ids0)} and not A._id_map_stale
    assert A.remove_items(ids0[100:700]) == 600
    assert A.add_items(Xa, list(range(90000, 90900))) == 900
    assert A._id_map_stale                                          # no million-entry dict inside the update
    want_ids = np.array(ids0[:100] + ids0[700:] + list(range(90000, 90900)))
    Q = np.concatenate([fx.unit_rows(rng, 40, d), Xa[:10]])
    s0, i0 = A.batch_search(Q, k=60)
    assert np.isin(i0[i0 >= 0], want_ids).all() and (i0 >= 90000).any()
    for fmt in ("rihip", "faiss"):
        p = tmp_path / f"{fmt}.index"
        A.save(str(p), format=fmt)
        with open(p.with_suffix(".meta.pkl"), "rb") as f:
            meta = pickle.load(f)
        assert meta["item_id_to_faiss_idx"] == {int(i): r for r, i in enumerate(want_ids)}
        np.testing.assert_array_equal(meta["item_ids"], want_ids)
        back = FAISSIndex.load(str(p))
        assert back.exact == exact and back.index.ntotal == len(want_ids)
        s1, i1 = back.batch_search(Q, k=60)
        np.testing.assert_array_equal(i1, i0)
        np.testing.assert_array_equal(s1, s0)
        # a loaded index can be updated in turn
        assert back.remove_items([90000]) == 1 and not (back.batch_search(Q, k=60)[1] == 90000).any()
    assert not A._id_map_stale and A._item_id_to_faiss_idx[90899] == len(want_ids) - 1


# ---- 8. serving ------------------------------------------------------------------------------------------------------------------
def _pipeline(tmp_path, index, model, nu, ni, genres, seen=None):
    from recommendit_amd import LightGBMRanker
    from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns
    forest = G.random_forest_model(60, 31, 50, seed=5, names=feature_columns())
    p = tmp_path / "r.lgbm"
    p.write_text(G.write_text_model(forest))
    ranker = LightGBMRanker.load(str(p))
    rng = np.random.RandomState(2)
    store = GpuFeatureStore(nu, ni)
    ut = store.user.copy(); it = store.item.copy()
    ut[1:, :6] = rng.rand(nu, 6) * [5, 8, 1, 1, 1, 1]; ut[1:, 6:] = rng.rand(nu, 18)
    it[1:, :5] = rng.rand(ni, 5) * [5, 9, 1, 1.5, 1]; it[1:, 5:] = genres
    store.load_arrays(ut, it)
    return GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=200, top_k_results=20, seen=seen)


@pytest.mark.parametrize("with_seen", [False, True])
def test_serving_follows_the_catalogue(tmp_path, with_seen):
    from recommendit_amd import FAISSIndex, SeenItems, TwoTowerModel
    nu, ni, d, H = 300, 6000, 64, 128
    sd = fx.make_state(nu, ni, d, H, seed=21)
    model = TwoTowerModel(nu, ni, d, H)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    rng = np.random.RandomState(2)
    item_ids = list(range(1, ni + 1))
    genres = (rng.rand(ni, 18) < 0.15).astype(np.float32)
    E = model.get_item_embeddings(item_ids, genres)
    index = FAISSIndex(embed_dim=d, n_lists=8, n_probe=4)
    index.build_ivf_index(E, item_ids)
    users = list(range(1, 65))
    uid = torch.tensor(users, device="cuda")
    q = model.get_user_embeddings(uid, as_tensor=True)
    seen = None
    if with_seen:
        _, unf = index.batch_search_device(q, k=400, normalized=True)
        unf = unf.cpu().numpy()
        seen = SeenItems.from_dict({u: unf[qi][unf[qi] >= 0][5:45].tolist() for qi, u in enumerate(users)}, n_users=nu + 1)
    pipe = _pipeline(tmp_path, index, model, nu, ni, genres, seen)
    ids0 = pipe.recommend_batch(users)[0].cpu().numpy()
    g0 = pipe.recommend_batch(users[:8], graph=True)[0].cpu().numpy()
    np.testing.assert_array_equal(g0, ids0[:8])
    removed = int(ids0[0, 0])                               # an item that was recommended (also served through the graph)
    chosen, new_id = 4, ni + 1                              # query row 4 = user 5; the new id is outside the feature
    a0 = index.list_assignment()                            # store's item table: it is served with the default row
    C = index.centroids()
    new_vec = q[chosen:chosen + 1].cpu().numpy()
    assert index.remove_items([removed]) == 1
    assert index.add_items(new_vec, [new_id]) == 1
    ids1, sc1, rs1 = [t.cpu().numpy() for t in pipe.recommend_batch(users)]
    g1 = [t.cpu().numpy() for t in pipe.recommend_batch(users[:8], graph=True)]
    assert not (ids1 == removed).any() and not (g1[0] == removed).any()
    cs, cand = index.batch_search_device(q, k=200, normalized=True)
    assert int(cand[chosen, 0]) == new_id and abs(float(cs[chosen, 0]) - 1.0) < 1e-5
    assert not (cand == removed).any()
    # a fresh pipeline over a from-scratch index of the final catalogue
    En = np.ascontiguousarray(E / np.maximum(np.linalg.norm(E, axis=1, keepdims=True), 1e-8), dtype=np.float32)
    keep = np.array(item_ids) != removed
    nn = np.ascontiguousarray(new_vec / np.maximum(np.linalg.norm(new_vec, axis=1, keepdims=True), 1e-8), dtype=np.float32)
    Xf = np.concatenate([En[keep], nn])
    af = np.concatenate([a0[keep], _assigned(index, nn)])
    fresh = _ivf(Xf, np.concatenate([np.array(item_ids)[keep], [new_id]]), C, af, 4)
    (tmp_path / "b").mkdir()
    pipe_b = _pipeline(tmp_path / "b", fresh, model, nu, ni, genres, seen)
    want = [t.cpu().numpy() for t in pipe_b.recommend_batch(users)]
    for got, exp in zip((ids1, sc1, rs1), want):
        np.testing.assert_array_equal(got, exp)
    gb = [t.cpu().numpy() for t in pipe_b.recommend_batch(users[:8], graph=True)]
    for got, exp, eager in zip(g1, gb, want):
        np.testing.assert_array_equal(got, exp)
        np.testing.assert_array_equal(got, eager[:8])
    if with_seen:
        for qi, u in enumerate(users):
            assert not np.isin(ids1[qi], unf[qi][5:45]).any()
        assert pipe.exclusion_deficit() == 0


# ---- 9. full size ----------------------------------------------------------------------------------------------------------------
def test_full_size_one_percent_churn_equals_a_from_scratch_build():
    """BASELINE cfg5: 1M x 128, 100 lists, nprobe 10, k 500; 10 000 rows out, 10 000 rows in"""
    from recommendit_amd import FAISSIndex
    rng = np.random.RandomState(93)
    N, d, nlist, nprobe, k, r = 1_000_000, 128, 100, 10, 500, 10_000
    Xall = fx.unit_rows(rng, N + r, d)
    A = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=nprobe)
    A.build_from_device(torch.from_numpy(Xall[:N]).cuda(), np.arange(N), kmeans_iters=4)
    C, a0 = A.centroids(), A.list_assignment()
    rm = rng.choice(N, r, replace=False)
    xa = torch.from_numpy(Xall[N:]).cuda()
    a_new = A.assign_lists(xa).cpu().numpy()
    assert A.remove_items(rm) == r
    assert A.add_items_device(xa, np.arange(N, N + r)) == r
    keep = np.ones(N, dtype=bool)
    keep[rm] = False
    Xf = np.concatenate([Xall[:N][keep], Xall[N:]])
    ids_f = np.concatenate([np.arange(N)[keep], np.arange(N, N + r)])
    B = _ivf(Xf, ids_f, C, np.concatenate([a0[keep], a_new]), nprobe)
    Q = np.concatenate([fx.unit_rows(rng, 90, d), Xall[N:N + 38]])
    sa, ia = A.batch_search(Q, k=k)
    sb, ib = B.batch_search(Q, k=k)
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(sa, sb)
    assert (ia >= 0).all() and (ia >= N).any() and not np.isin(ia, rm).any()
    np.testing.assert_array_equal(A.item_ids, ids_f)
    np.testing.assert_array_equal(A.list_assignment(), B.list_assignment())
    np.testing.assert_array_equal(A.reconstruct(), Xf)
