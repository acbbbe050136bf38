"""GPU: add_items / remove_items / update_items of an SQ8Index (csrc/sq8_update.hip, rihip_sq8_update_*).

An update is one repack of the code matrix under the index's own centroids and quantiser, and it must leave the handle
bit for bit in the state from_index(f32 index of the final corpus with the same centroids and lists,
ranges=quantizer()) + set_item_tags + attach_vectors gives.  Every comparison is an EQUALITY over all queries of its
batch: integer scores with the lower-row tie rule make that possible.  tests/sq8_update_reference.py is the NumPy model;
tests/test_sq8_update_host.py shows that it has the same property."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import gbdt_np as G
from oracle import retrieval_np as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_reference as S  # noqa: E402
import sq8_refine_reference as RF  # noqa: E402
import sq8_update_reference as U  # noqa: E402

pytestmark = pytest.mark.gpu
NPROBE, K = 6, 100
FILT = (0b000110, 0b000001, 0b100000)          # any of bits 1-2, bit 0 set, bit 5 clear: about 3 tag words in 16 pass


def _clustered(rng, N, d, n_centers, spread=0.35):
    """unit rows around n_centers directions (tests/test_gpu_index_update.py): lists of uneven size"""
    centers = fx.unit_rows(rng, n_centers, d)
    w = rng.dirichlet(np.full(n_centers, 0.7))
    which = rng.choice(n_centers, N, p=w)
    X = centers[which] + spread * rng.randn(N, d).astype(np.float32) / np.sqrt(d)
    return R.normalize_rows(X)


def _unit(X):
    return np.ascontiguousarray(X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-8), dtype=np.float32)


def _dev(X):
    return torch.from_numpy(np.ascontiguousarray(X)).cuda()


def _f32(X, ids, C=None, lists=None, nprobe=NPROBE):
    """the f32 index of a corpus: IVF with these centroids and this list of every row, or exact (C None)"""
    from recommendit_amd import FAISSIndex
    if C is None:
        idx = FAISSIndex(embed_dim=X.shape[1], exact=True)
        idx.build_from_device(_dev(X), np.asarray(ids, dtype=np.int64))
        return idx
    idx = FAISSIndex(embed_dim=X.shape[1], n_lists=C.shape[0], n_probe=nprobe)
    idx.build_from_device(_dev(X), np.asarray(ids, dtype=np.int64), centroids=C, assign=np.asarray(lists, dtype=np.int32))
    return idx


class _Corpus:
    """the model corpus in insertion order: rows, ids, list of every row (None: flat), tag words (None: untagged)"""

    def __init__(self, X, ids, lists=None, tags=None):
        self.X, self.ids = X.copy(), np.asarray(ids, dtype=np.int64).copy()
        self.lists = None if lists is None else np.asarray(lists, dtype=np.int32).copy()
        self.tags = None if tags is None else np.asarray(tags, dtype=np.uint32).copy()

    def remove(self, ids):
        gone = np.isin(self.ids, np.asarray(ids, dtype=np.int64))
        self.X, self.ids = self.X[~gone], self.ids[~gone]
        if self.lists is not None:
            self.lists = self.lists[~gone]
        if self.tags is not None:
            self.tags = self.tags[~gone]
        return int(gone.sum())

    def add(self, X, ids, lists=None, tags=None):
        self.X = np.concatenate([self.X, X])
        self.ids = np.concatenate([self.ids, np.asarray(ids, dtype=np.int64)])
        if self.lists is not None:
            self.lists = np.concatenate([self.lists, np.asarray(lists, dtype=np.int32)])
        if self.tags is not None:
            self.tags = np.concatenate([self.tags, np.zeros(len(ids), np.uint32) if tags is None else np.asarray(tags, np.uint32)])

    def old_tags(self, ids):
        """the word every id carries now, 0 for an id that is not stored (what an upsert without tags= keeps)"""
        pos = {int(i): r for r, i in enumerate(self.ids)}
        return np.array([self.tags[pos[int(i)]] if int(i) in pos else 0 for i in ids], dtype=np.uint32)


def _scratch(m, C, quant, vectors, nprobe=NPROBE):
    """B: from_index of the model corpus with the same centroids, lists and quantiser, the model's tags, the vectors"""
    from recommendit_amd import SQ8Index
    src = _f32(m.X, m.ids, C, m.lists, nprobe)
    B = SQ8Index.from_index(src, ranges=quant, keep_vectors=vectors)
    if m.tags is not None:
        B.set_item_tags(m.tags)
    del src
    return B


def _search(idx, qd, k=K, **kw):
    out = idx.batch_search_device(qd, k=k, normalized=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _same_lists(x, y, what):
    assert len(x) == len(y), what
    for i, (a, b) in enumerate(zip(x, y)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what} [{i}]")


def _assert_same_state(A, B, tmp_path, qd, tag, k=K):
    """A (updated) against B (from scratch): files, arrays and every kind of search result are EQUAL, all queries"""
    p1, p2 = tmp_path / f"{tag}_a.sq8", tmp_path / f"{tag}_b.sq8"
    A.save(str(p1))
    B.save(str(p2))
    assert p1.read_bytes() == p2.read_bytes(), tag
    assert A.index.ntotal == B.index.ntotal == len(A.item_ids)
    np.testing.assert_array_equal(A.codes(), B.codes())
    np.testing.assert_array_equal(A.reconstruct(), B.reconstruct())
    _same_lists(A.quantizer(), B.quantizer(), "quantizer")
    np.testing.assert_array_equal(A.item_ids, B.item_ids)
    np.testing.assert_array_equal(A._item_ids_dev.cpu().numpy(), B.item_ids)
    assert A._item_id_to_faiss_idx == {int(i): r for r, i in enumerate(B.item_ids)}
    assert A.has_item_tags == B.has_item_tags and A.has_vectors == B.has_vectors
    sa, sb = A.stats(), B.stats()
    assert sa.keys() == sb.keys() and all(sa[key] == sb[key] for key in ("n_vectors", "n_lists", "device_bytes", "n_item_ids"))
    for mode in ("dense", "thresholded", "auto"):
        _same_lists(_search(A, qd, k, mode=mode, return_int=True), _search(B, qd, k, mode=mode, return_int=True), f"{tag} {mode}")
    if A.has_item_tags:
        np.testing.assert_array_equal(A.item_tags(), B.item_tags())
        nq = qd.shape[0]
        per_q = np.tile(np.array(FILT, dtype=np.uint32), (nq, 1))
        per_q[::3] = (0, 0, 0)
        per_q[1::3] = (0b11, 0, 0b1000)
        for flt in (FILT, per_q):
            for mode in ("dense", "thresholded"):
                _same_lists(_search(A, qd, k, mode=mode, return_int=True, item_filter=flt),
                            _search(B, qd, k, mode=mode, return_int=True, item_filter=flt), f"{tag} filtered {mode}")
    if A.has_vectors:
        _same_lists(A.refine_ranges(), B.refine_ranges(), "refine_ranges")
        for factor in (1, 2):
            _same_lists(_search(A, qd, k, refine=factor, return_cert=True), _search(B, qd, k, refine=factor, return_cert=True),
                        f"{tag} refine {factor}")


# ---- 1. + 2. state equality, and against NumPy directly ---------------------------------------------------------------------
@pytest.mark.parametrize("d,nlist", [(32, 24), (64, 24), (96, 257)])
def test_update_leaves_the_state_of_a_from_scratch_build(tmp_path, d, nlist):
    """d = 32: 64-byte rows over 32 f32 columns; d = 96: du < dk = 128.  Steps: (a) a list emptied completely + unknown
    drop ids; (b) a list filled exactly to a 64-row granule; (c) three more rows of it; (d) an upsert of 300 stored and 200
    fresh ids through the host entry.  The f32 index is gone before the first update."""
    from recommendit_amd import SQ8Index
    rng = np.random.RandomState(71 + d)
    N0 = 6000
    Xall = _clustered(rng, N0 + 8000, d, 20)
    X0, pool = Xall[:N0], Xall[N0:]
    C = R.kmeans_ip(X0, nlist, n_iter=2, seed=7)
    a0 = R.ivf_assign(X0, C).astype(np.int32)
    ids0 = np.arange(1000, 1000 + N0, dtype=np.int64)
    pool_ids = np.arange(500000, 500000 + len(pool), dtype=np.int64)
    tags0 = rng.randint(0, 64, N0).astype(np.uint32)
    qd = _dev(np.concatenate([fx.unit_rows(rng, 60, d), pool[:20], X0[:20]]))
    src = _f32(X0, ids0, C, a0)
    A = SQ8Index.from_index(src, keep_vectors=True)
    A.set_item_tags(tags0)
    del src
    quant = A.quantizer()
    m = _Corpus(X0, ids0, a0, tags0)
    pool_list = A.assign_lists(_dev(pool)).cpu().numpy()
    # the index's own quantizer of new rows is the arg-max list wherever the margin is clear
    cs = pool.astype(np.float64) @ C.astype(np.float64).T
    srt = -np.sort(-cs, axis=1)
    clear = srt[:, 0] - srt[:, 1] > 1e-5
    assert clear.mean() > 0.99
    np.testing.assert_array_equal(pool_list[clear], cs.argmax(axis=1)[clear])
    gen = [int(_gen())]

    def check(tag):
        assert int(_gen()) > gen[0]                    # captured serve graphs are stale after a real change
        gen[0] = int(_gen())
        _assert_same_state(A, _scratch(m, C, quant, True), tmp_path, qd, tag)

    sizes = np.bincount(a0, minlength=nlist)
    victim = int(np.where(sizes > 0, sizes, N0 + 1).argmin())
    gone = ids0[a0 == victim]
    assert A.remove_items(np.concatenate([[7, 999, 10**12], gone[::-1], [-5]])) == len(gone) == m.remove(gone)
    check("a")
    T = int(np.bincount(pool_list, minlength=nlist).argmax())
    of_T = np.nonzero(pool_list == T)[0]
    fill = int(-np.bincount(m.lists, minlength=nlist)[T] % 64) or 64
    assert len(of_T) >= fill + 3, (len(of_T), fill)
    others = np.nonzero(pool_list != T)[0][:500]
    pick = np.sort(np.concatenate([of_T[:fill], others]))
    t_new = rng.randint(0, 64, len(pick)).astype(np.uint32)
    assert A.add_items_device(_dev(pool[pick]), pool_ids[pick], tags=t_new) == len(pick)
    m.add(pool[pick], pool_ids[pick], pool_list[pick], t_new)
    assert np.bincount(m.lists, minlength=nlist)[T] % 64 == 0
    check("b")
    pick = of_T[fill:fill + 3]
    assert A.add_items_device(_dev(pool[pick]), pool_ids[pick]) == 3           # no tags=: the new rows' words are 0
    m.add(pool[pick], pool_ids[pick], pool_list[pick])
    check("c")
    stored = rng.choice(m.ids, 300, replace=False)
    fresh = np.arange(900000, 900200, dtype=np.int64)
    E = (3.0 * _clustered(rng, 500, d, 20)).astype(np.float32)
    En = _unit(E)
    up_ids = np.concatenate([stored[:150], fresh, stored[150:]])
    kept_words = m.old_tags(up_ids)                                            # a replaced id keeps its word, a new id gets 0
    assert A.update_items(E, up_ids) == (300, 200)
    assert m.remove(stored) == 300
    m.add(En, up_ids, A.assign_lists(_dev(En)).cpu().numpy(), kept_words)
    check("d")
    assert A.update_stats()["updates"] == 4 and A.update_stats()["added"] == len(others) + fill + 3 + 500

    # 2. against NumPy directly: the codes, and the dense search over the probed lists of the reference
    mq, sq = quant
    codes = S.encode(m.X, mq, sq)
    np.testing.assert_array_equal(A.codes(), codes)
    ref = U.Sq8Model.from_corpus(m.X, m.ids, m.lists, nlist, mq, sq, m.tags)
    np.testing.assert_array_equal(A.item_tags(), ref.tags_by_row())
    Q = qd.cpu().numpy()
    n, t, b = S.encode_queries(Q, mq, sq)
    allowed = RF.probe_mask(Q, C, m.lists, NPROBE)
    want_rows, want_S = S.topk(S.int_scores(n, codes), K, allowed)
    sc, rows, ints = [x.cpu().numpy() for x in A.search_rows_device(qd, K, mode="dense", return_int=True)]
    np.testing.assert_array_equal(rows, want_rows)
    np.testing.assert_array_equal(ints[want_rows >= 0], want_S[want_rows >= 0])
    assert (rows >= len(m.ids) - 500).any()                                   # the upserted rows are served


def _gen():
    from recommendit_amd import _lib
    return _lib.lib().rihip_scratch_generation()


# ---- 3. drift: rows outside the frozen quantiser's range --------------------------------------------------------------------
def test_rows_outside_the_quantisers_range_are_clamped_and_counted():
    from recommendit_amd import SQ8Index
    rng = np.random.RandomState(97)
    d, N0, nlist = 64, 6000, 24
    X0 = _clustered(rng, N0, d, 20)
    C = R.kmeans_ip(X0, nlist, n_iter=2, seed=7)
    a0 = R.ivf_assign(X0, C).astype(np.int32)
    src = _f32(X0, np.arange(N0), C, a0)
    A = SQ8Index.from_index(src, keep_vectors=True)                             # a trained quantiser
    del src
    mq, sq = A.quantizer()
    np.testing.assert_array_equal(mq, S.train_quantizer(X0)[0])
    e0, _ = A.refine_ranges()
    Xs = np.ascontiguousarray(3.0 * _clustered(rng, 50, d, 20), dtype=np.float32)      # not normalised
    lists = A.assign_lists(_dev(Xs)).cpu().numpy()
    assert A.add_items_device(_dev(Xs), np.arange(N0, N0 + 50)) == 50
    want = U.clamp_count(Xs, mq, sq)
    st = A.update_stats()
    assert st["last_clamped"] == st["clamped"] == want > 0 and st == dict(updates=1, dropped=0, added=50, clamped=want, last_clamped=want)
    v = np.rint((Xs - mq[None, :]) / sq[None, :])
    got = A.codes()[N0:]
    np.testing.assert_array_equal(got, S.encode(Xs, mq, sq))
    assert (got[v > 127] == 127).all() and (got[v < -127] == -127).all()
    m = _Corpus(X0, np.arange(N0), a0)
    m.add(Xs, np.arange(N0, N0 + 50), lists)
    B = _scratch(m, C, (mq, sq), True)
    e1, a1 = A.refine_ranges()
    _same_lists((e1, a1), B.refine_ranges(), "ranges")
    _same_lists((e1, a1), RF.ranges(m.X, A.codes(), mq, sq), "ranges against NumPy")
    assert (e1 >= e0).all() and (e1 > e0).any()
    # a certificate on the drifted index still tells the truth: every certified query equals the brute force over its
    # probed lists under f.  The clamped rows make e_j large, so at factor 4 few queries (or none) are certified by the
    # bound; at k_scan = 8 000 > N stage 1 holds every probed row, so every query is certified by the first clause and
    # the re-score reads the attached f32 rows of kept and of added rows alike.
    Q = np.concatenate([fx.unit_rows(rng, 40, d), _unit(Xs[:10])])
    bf_r, bf_s = RF.brute_force(Q, m.X, 10, RF.probe_mask(Q, C, m.lists, NPROBE))
    for factor in (4, 800):
        sc, rows, cert, _ = [x.cpu().numpy() for x in A.search_rows_device(_dev(Q), 10, refine=factor, return_cert=True)]
        ok = cert == 1
        print(f"certified queries on the drifted index at factor {factor}:", int(ok.sum()), "of", len(Q))
        np.testing.assert_array_equal(rows[ok], bf_r[ok])
        np.testing.assert_array_equal(sc[ok], bf_s[ok])
    assert ok.all() and (bf_r[40:, 0] >= N0).all()         # the scaled rows' own directions find them first


# ---- 4. flat ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N0,n_rm,n_add", [(4000, 300, 150), (4032, 0, 96), (4100, 200, 0)])
def test_flat_handle_update_equals_a_from_scratch_build(tmp_path, N0, n_rm, n_add):
    """(4 032, 0, 96) goes from a granule-exact N to a granule-exact N"""
    from recommendit_amd import SQ8Index
    rng = np.random.RandomState(83)
    d = 64
    Xall = fx.unit_rows(rng, N0 + n_add, d)
    X0, Xa = Xall[:N0], Xall[N0:]
    ids0 = np.arange(10, 10 + N0, dtype=np.int64)
    add_ids = np.arange(10**6, 10**6 + n_add, dtype=np.int64)
    tags0 = rng.randint(0, 64, N0).astype(np.uint32)
    qd = _dev(np.concatenate([fx.unit_rows(rng, 60, d), X0[:20], Xall[-20:]]))
    src = _f32(X0, ids0)
    A = SQ8Index.from_index(src, keep_vectors=True)
    A.set_item_tags(tags0)
    del src
    quant = A.quantizer()
    m = _Corpus(X0, ids0, None, tags0)
    assert (A.assign_lists(_dev(Xall[:70])).cpu().numpy() == 0).all()
    rm = rng.choice(ids0, n_rm, replace=False)
    if n_rm:
        assert A.remove_items(np.concatenate([rm, [3, 4]])) == n_rm == m.remove(rm)
    if n_add:
        t_new = rng.randint(0, 64, n_add).astype(np.uint32)
        assert A.add_items_device(_dev(Xa), add_ids, tags=t_new) == n_add
        m.add(Xa, add_ids, None, t_new)
    assert A.index.nlist == 1 and A.index.ntotal == N0 - n_rm + n_add
    _assert_same_state(A, _scratch(m, None, quant, True), tmp_path, qd, "flat")
    np.testing.assert_array_equal(A.codes(), S.encode(m.X, *quant))


# ---- 5. without vectors and without tags ------------------------------------------------------------------------------------
def test_bare_handle_update_equals_the_bare_from_scratch_handle(tmp_path):
    from recommendit_amd import SQ8Index
    rng = np.random.RandomState(85)
    d, N0, nlist = 96, 6000, 24
    Xall = _clustered(rng, N0 + 700, d, 20)
    X0, Xa = Xall[:N0], Xall[N0:]
    C = R.kmeans_ip(X0, nlist, n_iter=2, seed=7)
    a0 = R.ivf_assign(X0, C).astype(np.int32)
    ids0 = rng.permutation(10 * N0)[:N0].astype(np.int64)
    src = _f32(X0, ids0, C, a0)
    A = SQ8Index.from_index(src)
    del src
    quant = A.quantizer()
    m = _Corpus(X0, ids0, a0)
    rm = rng.choice(ids0, 400, replace=False)
    add_ids = np.arange(10**6, 10**6 + 700, dtype=np.int64)
    lists = A.assign_lists(_dev(Xa)).cpu().numpy()
    assert A.remove_items(rm) == 400 == m.remove(rm)
    assert A.add_items(Xa, add_ids) == 700
    m.add(_unit(Xa), add_ids, lists)
    assert not A.has_vectors and not A.has_item_tags
    assert A.stats()["has_vectors"] is False and A.stats()["has_item_tags"] is False
    qd = _dev(np.concatenate([fx.unit_rows(rng, 60, d), Xa[:20], X0[:20]]))
    _assert_same_state(A, _scratch(m, C, quant, False), tmp_path, qd, "bare")
    with pytest.raises(ValueError, match="without tags"):
        A.add_items(Xa[:2], [5 * 10**6, 5 * 10**6 + 1], tags=[1, 2])
    with pytest.raises(ValueError, match="without tags"):
        A.update_items(Xa[:2], [5 * 10**6, 5 * 10**6 + 1], tags=[1, 2])
    assert A.index.ntotal == len(m.ids)


# ---- 6. lockstep with the f32 index ---------------------------------------------------------------------------------------------
def test_lockstep_with_the_f32_index_then_attach():
    from recommendit_amd import SQ8Index
    rng = np.random.RandomState(87)
    d, N0, nlist = 64, 6000, 24
    Xall = _clustered(rng, N0 + 900, d, 20)
    X0, pool = Xall[:N0], Xall[N0:]
    ids0 = np.arange(N0, dtype=np.int64) * 3
    C = R.kmeans_ip(X0, nlist, n_iter=2, seed=7)
    F = _f32(X0, ids0, C, R.ivf_assign(X0, C))
    Q8 = SQ8Index.from_index(F)
    quant = Q8.quantizer()
    rm = rng.choice(ids0, 500, replace=False)
    stay = ids0[~np.isin(ids0, rm)]
    ups = [("remove", rm, None),
           ("add", np.arange(10**6, 10**6 + 600), pool[:600]),
           ("update", np.concatenate([stay[1000:1200], np.arange(2 * 10**6, 2 * 10**6 + 100)]), 2.0 * pool[600:])]
    for op, ids, X in ups:
        for idx in (F, Q8):
            if op == "remove":
                assert idx.remove_items(ids) == 500
            elif op == "add":
                assert idx.add_items(X, ids) == 600
            else:
                assert idx.update_items(X, ids) == (200, 100)
    np.testing.assert_array_equal(Q8.item_ids, F.item_ids)
    Q8.attach_vectors(F)                               # same rows, same order, same lists: accepted
    fresh = SQ8Index.from_index(F, ranges=quant, keep_vectors=True)
    _same_lists(Q8.refine_ranges(), fresh.refine_ranges(), "ranges")
    np.testing.assert_array_equal(Q8.codes(), fresh.codes())
    np.testing.assert_array_equal(Q8.codes(), S.encode(F.reconstruct(), *quant))


# ---- 7. equivalence, a model run, refusals --------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_update_items_equals_remove_then_add(tmp_path, exact):
    from recommendit_amd import SQ8Index
    rng = np.random.RandomState(89)
    d, N0 = 32, 6000
    X0 = _clustered(rng, N0, d, 10)
    ids0 = np.arange(N0, dtype=np.int64) * 3
    C = R.kmeans_ip(X0, 12, n_iter=2, seed=3)
    tags0 = rng.randint(0, 64, N0).astype(np.uint32)

    def mk():
        src = _f32(X0, ids0) if exact else _f32(X0, ids0, C, R.ivf_assign(X0, C), 4)
        idx = SQ8Index.from_index(src, keep_vectors=True)
        idx.set_item_tags(tags0)
        return idx
    A, B = mk(), mk()
    E = 2.0 * _clustered(rng, 700, d, 10)
    ids = rng.permutation(np.concatenate([rng.choice(ids0, 450, replace=False), np.arange(1, 750, 3)]))    # 450 stored, 250 not
    assert A.update_items(E, ids) == (450, 250)
    words = np.where(np.isin(ids, ids0), tags0[np.minimum(ids // 3, N0 - 1)], 0).astype(np.uint32)
    assert B.remove_items(ids) == 450
    assert B.add_items(E, ids, tags=words) == 700         # (remove forgets the words; an upsert without tags= keeps them)
    qd = _dev(np.concatenate([fx.unit_rows(rng, 50, d), _unit(E[:14])]))
    _assert_same_state(A, B, tmp_path, qd, "upsert", k=50)
    assert A.update_items(np.empty((0, d), np.float32), []) == (0, 0)


def test_twelve_random_updates_follow_the_model(tmp_path):
    from recommendit_amd import SQ8Index
    rng = np.random.RandomState(91)
    d, N0, nlist, nprobe = 64, 6000, 16, 4
    Xall = _clustered(rng, N0 + 4000, d, 12)
    X0, pool = Xall[:N0], Xall[N0:]
    C = R.kmeans_ip(X0, nlist, n_iter=2, seed=3)
    a0 = R.ivf_assign(X0, C).astype(np.int32)
    ids0 = rng.permutation(10 * N0)[:N0].astype(np.int64)            # ids in no order
    tags0 = rng.randint(0, 64, N0).astype(np.uint32)
    src = _f32(X0, ids0, C, a0, nprobe)
    A = SQ8Index.from_index(src, keep_vectors=True)
    A.set_item_tags(tags0)
    del src
    mq, sq = A.quantizer()
    pool_list = A.assign_lists(_dev(pool)).cpu().numpy()
    M = U.Sq8Model.from_corpus(X0, ids0, a0, nlist, mq, sq, tags0)
    next_pool, next_id = 0, 10**7
    for step in range(12):
        op = step % 3
        take = int(rng.randint(1, 300))
        rows = np.arange(next_pool, next_pool + take)
        next_pool += take
        if op == 0:
            ids = rng.choice(M.ids, int(rng.randint(1, 400)), replace=False)
            assert A.remove_items(np.concatenate([ids, [-1 - step]])) == M.update(ids, pool[:0], [])[0] == len(ids)
        elif op == 1:
            ids = np.arange(next_id, next_id + take)
            words = rng.randint(0, 64, take).astype(np.uint32)
            assert A.add_items_device(_dev(pool[rows]), ids, tags=words) == take
            M.update([], pool[rows], ids, pool_list[rows], words)
        else:
            stored = rng.choice(M.ids, take // 2, replace=False)
            ids = rng.permutation(np.concatenate([stored, np.arange(next_id, next_id + take - len(stored))]))
            words = rng.randint(0, 64, take).astype(np.uint32)
            assert A.update_items(pool[rows], ids, tags=words) == (len(stored), take - len(stored))
            Xn = _unit(pool[rows])
            M.update(ids, Xn, ids, A.assign_lists(_dev(Xn)).cpu().numpy(), words)
        next_id += take
        np.testing.assert_array_equal(A.item_ids, M.ids)
        np.testing.assert_array_equal(A.codes(), M.codes_by_row())
        np.testing.assert_array_equal(A.item_tags(), M.tags_by_row())
        assert A.index.ntotal == len(M.ids) == A.stats()["n_vectors"] == A.stats()["n_item_ids"]
    st = A.update_stats()
    assert [st["updates"], st["dropped"], st["added"], st["clamped"]] == M.stats
    m = _Corpus(M.X, M.ids, M.lists(), M.tags_by_row())
    qd = _dev(np.concatenate([fx.unit_rows(rng, 40, d), pool[:12]]))
    _assert_same_state(A, _scratch(m, C, (mq, sq), True, nprobe), tmp_path, qd, "seq")


@pytest.mark.parametrize("exact", [False, True])
def test_rejected_updates_leave_the_index_as_it_was(tmp_path, exact):
    from recommendit_amd import SQ8Index
    rng = np.random.RandomState(93)
    d, N0 = 64, 5000
    X0 = _clustered(rng, N0, d, 10)
    ids0 = np.arange(100, 100 + N0, dtype=np.int64)
    C = R.kmeans_ip(X0, 10, n_iter=2, seed=3)
    src = _f32(X0, ids0) if exact else _f32(X0, ids0, C, R.ivf_assign(X0, C), 4)
    A = SQ8Index.from_index(src, keep_vectors=True)
    A.set_item_tags(rng.randint(0, 64, N0).astype(np.uint32))
    del src
    qd = _dev(fx.unit_rows(rng, 30, d))
    before = _search(A, qd, 40, return_int=True) + _search(A, qd, 40, refine=2, return_cert=True) + [A.codes(), A.item_tags()]
    A.save(str(tmp_path / "before.sq8"))
    gen0 = int(_gen())
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
        A.add_items_device(_dev(fx.unit_rows(rng, 4, d + 4)), [9001, 9002, 9003, 9004])
    with pytest.raises(ValueError):                                   # ids and rows do not pair up
        A.add_items(new, [9001, 9002])
    with pytest.raises(ValueError, match="empty"):                    # would leave the index empty
        A.remove_items(ids0)
    assert A.remove_items([]) == 0 and A.remove_items([1, 2, 10**9]) == 0     # nothing to do: nothing changes
    assert A.add_items(np.empty((0, d), np.float32), []) == 0
    assert int(_gen()) == gen0
    assert A.index.ntotal == N0 and A.update_stats()["updates"] == 0
    np.testing.assert_array_equal(A.item_ids, ids0)
    after = _search(A, qd, 40, return_int=True) + _search(A, qd, 40, refine=2, return_cert=True) + [A.codes(), A.item_tags()]
    _same_lists(after, before, "after the refusals")
    A.save(str(tmp_path / "after.sq8"))
    assert (tmp_path / "after.sq8").read_bytes() == (tmp_path / "before.sq8").read_bytes()
    assert A.remove_items([150]) == 1 and int(_gen()) > gen0          # an accepted update is seen by graph holders


# ---- 8. serving ------------------------------------------------------------------------------------------------------------------
def _pipeline(tmp_path, index, model, nu, ni, genres):
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
    return GpuRecommendationPipeline(model, index, ranker, store, top_k_candidates=200, top_k_results=20)


def test_serving_follows_the_catalogue(tmp_path):
    """test_serving_follows_the_catalogue of tests/test_gpu_index_update.py over an SQ8Index pipeline.  A pipeline over
    an SQ8Index refuses graph=True by design (tests/test_gpu_sq8_index.py pins the ValueError), so the eager chain is
    what is compared, and the refusal is checked to be what it was."""
    from recommendit_amd import FAISSIndex, SQ8Index, TwoTowerModel
    nu, ni, d, H = 300, 6000, 64, 128
    sd = fx.make_state(nu, ni, d, H, seed=21)
    model = TwoTowerModel(nu, ni, d, H)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    rng = np.random.RandomState(2)
    item_ids = list(range(1, ni + 1))
    genres = (rng.rand(ni, 18) < 0.15).astype(np.float32)
    E = model.get_item_embeddings(item_ids, genres)
    src = FAISSIndex(embed_dim=d, n_lists=8, n_probe=4)
    src.build_ivf_index(E, item_ids)
    a0, C = src.list_assignment(), src.centroids()
    index = SQ8Index.from_index(src)
    del src
    quant = index.quantizer()
    users = list(range(1, 65))
    uid = torch.tensor(users, device="cuda")
    q = model.get_user_embeddings(uid, as_tensor=True)
    pipe = _pipeline(tmp_path, index, model, nu, ni, genres)
    ids0 = pipe.recommend_batch(users)[0].cpu().numpy()
    removed = int(ids0[0, 0])                               # an item that was recommended
    chosen, new_id = 4, ni + 1                              # query row 4 = user 5
    new_vec = q[chosen:chosen + 1].cpu().numpy()
    assert index.remove_items([removed]) == 1
    assert index.add_items(new_vec, [new_id]) == 1
    ids1, sc1, rs1 = [t.cpu().numpy() for t in pipe.recommend_batch(users)]
    assert not (ids1 == removed).any()
    cs, cand = index.batch_search_device(q, k=200, normalized=True)
    assert int(cand[chosen, 0]) == new_id and not (cand == removed).any()
    # a fresh pipeline over the from-scratch SQ8 index of the final catalogue with the same quantiser
    keep = np.array(item_ids) != removed
    nn = _unit(new_vec)
    m = _Corpus(np.concatenate([_unit(E)[keep], nn]), np.concatenate([np.array(item_ids)[keep], [new_id]]),
                np.concatenate([a0[keep], index.assign_lists(_dev(nn)).cpu().numpy()]))
    fresh = _scratch(m, C, quant, False, 4)
    (tmp_path / "b").mkdir()
    pipe_b = _pipeline(tmp_path / "b", fresh, model, nu, ni, genres)
    want = [t.cpu().numpy() for t in pipe_b.recommend_batch(users)]
    _same_lists([ids1, sc1, rs1], want, "served")
    for p in (pipe, pipe_b):
        with pytest.raises(ValueError, match="SQ8"):
            p.recommend_batch(users[:8], graph=True)


# ---- 9. full size ----------------------------------------------------------------------------------------------------------------
def test_full_size_one_percent_churn_equals_a_from_scratch_build():
    """1M x 128, 100 lists, nprobe 10, k 500; 10 000 rows out, 10 000 rows in; tags, no vectors"""
    from recommendit_amd import FAISSIndex, SQ8Index
    rng = np.random.RandomState(95)
    N, d, nlist, nprobe, k, r = 1_000_000, 128, 100, 10, 500, 10_000
    Xall = fx.unit_rows(rng, N + r, d)
    tags0 = rng.randint(0, 64, N).astype(np.uint32)
    t_new = rng.randint(0, 64, r).astype(np.uint32)
    F = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=nprobe)
    F.build_from_device(torch.from_numpy(Xall[:N]).cuda(), np.arange(N), kmeans_iters=2)
    C, a0 = F.centroids(), F.list_assignment()
    A = SQ8Index.from_index(F)
    A.set_item_tags(tags0)
    del F
    quant = A.quantizer()
    rm = rng.choice(N, r, replace=False)
    xa = torch.from_numpy(Xall[N:]).cuda()
    a_new = A.assign_lists(xa).cpu().numpy()
    assert A.remove_items(rm) == r
    assert A.add_items_device(xa, np.arange(N, N + r), tags=t_new) == r
    keep = np.ones(N, dtype=bool)
    keep[rm] = False
    m = _Corpus(np.concatenate([Xall[:N][keep], Xall[N:]]), np.concatenate([np.arange(N)[keep], np.arange(N, N + r)]),
                np.concatenate([a0[keep], a_new]), np.concatenate([tags0[keep], t_new]))
    B = _scratch(m, C, quant, False, nprobe)
    qd = _dev(np.concatenate([fx.unit_rows(rng, 90, d), Xall[N:N + 38]]))
    ra, rb = _search(A, qd, k, return_int=True), _search(B, qd, k, return_int=True)
    _same_lists(ra, rb, "full size")
    _same_lists(_search(A, qd, k, return_int=True, item_filter=FILT), _search(B, qd, k, return_int=True, item_filter=FILT), "filtered")
    assert (ra[1] >= 0).all() and (ra[1] >= N).any() and not np.isin(ra[1], rm).any()
    np.testing.assert_array_equal(A.item_ids, m.ids)
    np.testing.assert_array_equal(A.codes(), B.codes())
