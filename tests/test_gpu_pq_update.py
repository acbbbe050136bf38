"""GPU: add_items / remove_items / update_items of a PQIndex under frozen codebooks (csrc/pq_update.hip,
rihip_pq_update_*; opt-in through PQIndex.frozen_updates).

An update is one repack of the entry-number matrix under the index's own centroids, SQ8 quantiser, list codes and
codebooks, and it must leave the handle bit for bit in the state
    PQIndex.from_index(f32 index of the final corpus with the same centroids and lists, dsub=, ranges=quantizer(),
                       codebooks=codebooks(), by_residual=) + set_item_tags + attach_vectors
gives.  Injected codebooks skip the training and a row's bytes are a function of the row, its list and the frozen state,
so nothing here is a tolerance: every comparison is an EQUALITY over all queries of its batch.
tests/pq_update_reference.py is the NumPy model; tests/test_pq_update_host.py shows that it has the same property.
The corpus helpers are those of tests/test_gpu_sq8_update.py, whose shapes these tests follow."""
import ctypes as C_
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import retrieval_np as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_reference as P  # noqa: E402
import pq_residual_reference as PR  # noqa: E402
import pq_update_reference as PU  # noqa: E402
import sq8_reference as S  # noqa: E402
import sq8_refine_reference as RF  # noqa: E402
import test_gpu_sq8_update as T  # noqa: E402   (helpers only: _clustered, _unit, _dev, _f32, _Corpus, _search, _same_lists, _gen, _pipeline)

pytestmark = pytest.mark.gpu
NPROBE, K, FILT = T.NPROBE, T.K, T.FILT
_clustered, _unit, _dev, _f32, _Corpus, _search, _same_lists, _gen = (T._clustered, T._unit, T._dev, T._f32, T._Corpus, T._search,
                                                                      T._same_lists, T._gen)


def _scratch(m, C, A, vectors, nprobe=NPROBE):
    """B: from_index of the model corpus with A's centroids and lists, A's quantiser and A's codebooks injected, the
    model's tags, the vectors"""
    from recommendit_amd import PQIndex
    src = _f32(m.X, m.ids, C, m.lists, nprobe)
    B = PQIndex.from_index(src, dsub=A.dsub, ranges=A.quantizer(), codebooks=A.codebooks(), by_residual=A.by_residual,
                           keep_vectors=vectors)
    if m.tags is not None:
        B.set_item_tags(m.tags)
    del src
    return B


def _same_files(A, B, tmp_path, tag):
    p1, p2 = tmp_path / f"{tag}_a.pq", tmp_path / f"{tag}_b.pq"
    A.save(str(p1))
    B.save(str(p2))
    data = p1.read_bytes()
    assert data == p2.read_bytes(), tag
    assert data[:8] == (b"RIHIPPR1" if A.by_residual else b"RIHIPPQ1")
    return data


def _assert_same_state(A, B, tmp_path, qd, tag, k=K):
    """A (updated) against B (from scratch): files, every accessor and every kind of search result are EQUAL, all queries"""
    _same_files(A, B, tmp_path, tag)
    assert A.index.ntotal == B.index.ntotal == len(A.item_ids)
    assert A.dsub == B.dsub and A.by_residual == B.by_residual
    np.testing.assert_array_equal(A.pq_codes(), B.pq_codes())
    np.testing.assert_array_equal(A.codebooks(), B.codebooks())
    ca, cb = A.codes(), B.codes()
    assert ca.dtype == cb.dtype == (np.int16 if A.by_residual else np.int8)
    np.testing.assert_array_equal(ca, cb)
    if A.by_residual:
        np.testing.assert_array_equal(A.list_codes(), B.list_codes())
    np.testing.assert_array_equal(A.reconstruct(), B.reconstruct())
    _same_lists(A.quantizer(), B.quantizer(), "quantizer")
    np.testing.assert_array_equal(A.item_ids, B.item_ids)
    np.testing.assert_array_equal(A._item_ids_dev.cpu().numpy(), B.item_ids)
    assert A._item_id_to_faiss_idx == {int(i): r for r, i in enumerate(B.item_ids)}
    assert A.has_item_tags == B.has_item_tags and A.has_vectors == B.has_vectors
    sa, sb = A.stats(), B.stats()
    assert sa.keys() == sb.keys() and all(sa[key] == sb[key] for key in ("n_vectors", "n_lists", "device_bytes", "n_item_ids",
                                                                        "bytes_per_vector", "by_residual"))
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


# ---- 1. state equality, and against NumPy directly --------------------------------------------------------------------------
@pytest.mark.parametrize("d,nlist,dsub,by_residual", [(32, 24, 8, False), (64, 24, 16, True), (96, 257, 8, True), (128, 24, 16, False)])
def test_update_leaves_the_state_of_a_from_scratch_build(tmp_path, d, nlist, dsub, by_residual):
    """d = 32: dk 32 < dpad 64 (sub-spaces that lie in the padding columns); d = 96: du < dk = dpad = 128 and more lists
    than rows per granule.  Steps: (a) a list emptied completely + unknown, negative and huge drop ids; (b) a list filled
    exactly to a 64-row granule + 500 rows elsewhere, with tags=; (c) three more rows of it, without tags=; (d) an upsert
    of 300 stored and 200 fresh ids through the host entry.  The f32 index is gone before the first update."""
    from recommendit_amd import PQIndex
    rng = np.random.RandomState(171 + d)
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
    A = PQIndex.from_index(src, dsub=dsub, n_iter=2, keep_vectors=True, by_residual=by_residual, frozen_updates=True)
    A.set_item_tags(tags0)
    del src
    quant, book = A.quantizer(), A.codebooks()
    n_build = A.train_stats()["distortion"]
    m = _Corpus(X0, ids0, a0, tags0)
    pool_list = A.assign_lists(_dev(pool)).cpu().numpy()
    gen = [int(_gen())]

    def check(tag):
        assert int(_gen()) > gen[0]                    # captured serve graphs are stale after a real change
        gen[0] = int(_gen())
        _assert_same_state(A, _scratch(m, C, A, True), tmp_path, qd, tag)
        np.testing.assert_array_equal(A.codebooks(), book)            # frozen
        _same_lists(A.quantizer(), quant, "frozen quantiser")

    sizes = np.bincount(a0, minlength=nlist)
    victim = int(np.where(sizes > 0, sizes, N0 + 1).argmin())
    gone = ids0[a0 == victim]
    assert A.remove_items(np.concatenate([[7, 999, 10**12], gone[::-1], [-5]])) == len(gone) == m.remove(gone)
    check("a")
    T_ = int(np.bincount(pool_list, minlength=nlist).argmax())
    of_T = np.nonzero(pool_list == T_)[0]
    fill = int(-np.bincount(m.lists, minlength=nlist)[T_] % 64) or 64
    assert len(of_T) >= fill + 3, (len(of_T), fill)
    others = np.nonzero(pool_list != T_)[0][:500]
    pick = np.sort(np.concatenate([of_T[:fill], others]))
    t_new = rng.randint(0, 64, len(pick)).astype(np.uint32)
    assert A.add_items_device(_dev(pool[pick]), pool_ids[pick], tags=t_new) == len(pick)
    m.add(pool[pick], pool_ids[pick], pool_list[pick], t_new)
    assert np.bincount(m.lists, minlength=nlist)[T_] % 64 == 0
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
    st = A.update_stats()
    assert st["updates"] == 4 and st["added"] == len(others) + fill + 3 + 500 and st["dropped"] == len(gone) + 300
    assert st["distortion_added"] > 0 and len(n_build) == 3       # both halves of the drift signal exist on a built index

    # against NumPy directly: the entry numbers, and the dense search over the probed lists of the reference
    mq, sq = quant
    ref = PU.PqModel.from_corpus(m.X, m.ids, m.lists, nlist, mq, sq, book, C if by_residual else None, m.tags, assign=P.assign_blas)
    np.testing.assert_array_equal(A.pq_codes(), ref.pq_codes())
    np.testing.assert_array_equal(A.item_tags(), ref.tags_by_row())
    dec = ref.decoded()
    np.testing.assert_array_equal(A.codes(), dec[:, :d])
    Q = qd.cpu().numpy()
    n, t, b = S.encode_queries(Q, mq, sq)
    allowed = RF.probe_mask(Q, C, m.lists, NPROBE)
    scores = PR.int_scores(n, dec) if by_residual else S.int_scores(n, dec[:, :d])
    want_rows, want_S = S.topk(scores, K, allowed)
    sc, rows, ints = [x.cpu().numpy() for x in A.search_rows_device(qd, K, mode="dense", return_int=True)]
    np.testing.assert_array_equal(rows, want_rows)
    np.testing.assert_array_equal(ints[want_rows >= 0], want_S[want_rows >= 0])
    assert (rows >= len(m.ids) - 500).any()                                   # the upserted rows are served


# ---- 2. ties and block edges ------------------------------------------------------------------------------------------------
def _grid_quant(d):
    return np.zeros(d, np.float32), np.full(d, 1.0 / 128.0, np.float32)      # code = 128 x exactly


@pytest.mark.parametrize("dsub", [8, 16])
def test_a_tie_between_equal_entries_keeps_the_lowest(tmp_path, dsub):
    """entries 3 and 200 of every sub-space are equal; added rows that decode exactly onto codebook entries get the lowest
    entry that holds their sub-vector (3, never 200) at distance 0"""
    from recommendit_amd import PQIndex
    rng = np.random.RandomState(31 + dsub)
    d, N0, n_add = 64, 300, 130
    M = 64 // dsub
    book = rng.randint(-127, 128, (M, 256, dsub)).astype(np.int8)
    book[:, 200] = book[:, 3]
    for mm in range(M):                                                     # no other coincidence among the entries
        assert len(np.unique(book[mm], axis=0)) == 255
    quant = _grid_quant(d)
    X0 = fx.unit_rows(rng, N0, d)
    pick = rng.randint(0, 256, (n_add, M))
    pick[:40] = 200
    pick[40:80] = 3
    pick[80:, ::2] = 200
    Xa = (np.concatenate([book[mm][pick[:, mm]] for mm in range(M)], axis=1).astype(np.float32) / np.float32(128.0))
    np.testing.assert_array_equal(S.encode(Xa, *quant), (Xa * 128).astype(np.int8))
    ids0, add_ids = np.arange(N0, dtype=np.int64), np.arange(5000, 5000 + n_add, dtype=np.int64)
    A = PQIndex.from_index(_f32(X0, ids0), dsub=dsub, ranges=quant, codebooks=book, keep_vectors=True, frozen_updates=True)
    assert A.add_items_device(_dev(Xa), add_ids) == n_add                   # (as they are: not normalised)
    want = np.where(pick == 200, 3, pick).astype(np.uint8)
    assert (want[:80] == 3).all()
    np.testing.assert_array_equal(A.pq_codes()[N0:], want)
    st = A.update_stats()
    assert st["last_distortion"] == 0 == st["distortion_added"] and st["clamped"] == 0 and st["added"] == n_add
    np.testing.assert_array_equal(A.codes()[N0:], (Xa * 128).astype(np.int8))       # decoded exactly onto the rows
    m = _Corpus(X0, ids0)
    m.add(Xa, add_ids)
    qd = _dev(np.concatenate([fx.unit_rows(rng, 30, d), _unit(Xa[:10])]))
    _assert_same_state(A, _scratch(m, None, A, True), tmp_path, qd, "tie", k=50)


@pytest.mark.parametrize("N0", [70, 6000])
@pytest.mark.parametrize("n_add", [1, 255, 257, 2049])
def test_flat_handle_block_edges_equal_a_from_scratch_build(tmp_path, N0, n_add):
    """a flat handle (nlist == 1); n_add crosses the workgroup (256) and the rows-per-block (2 048) boundaries of the
    encode kernel; N0 = 70 trains codebooks with repeated entries, i.e. ties in every sub-space"""
    from recommendit_amd import PQIndex
    rng = np.random.RandomState(37 + N0 + n_add)
    d = 64
    Xall = fx.unit_rows(rng, N0 + n_add, d)
    X0, Xa = Xall[:N0], Xall[N0:]
    ids0, add_ids = np.arange(10, 10 + N0, dtype=np.int64), np.arange(10**6, 10**6 + n_add, dtype=np.int64)
    A = PQIndex.from_index(_f32(X0, ids0), dsub=8, n_iter=1, frozen_updates=True)
    assert A.index.nlist == 1 and (A.assign_lists(_dev(Xa)).cpu().numpy() == 0).all()
    assert A.add_items_device(_dev(Xa), add_ids) == n_add
    m = _Corpus(X0, ids0)
    m.add(Xa, add_ids)
    B = _scratch(m, None, A, False)
    _same_files(A, B, tmp_path, "edge")
    np.testing.assert_array_equal(A.pq_codes(), B.pq_codes())
    np.testing.assert_array_equal(A.item_ids, m.ids)
    ref = PU.PqModel.from_corpus(m.X, m.ids, None, 1, *A.quantizer(), A.codebooks(), assign=P.assign_blas)
    np.testing.assert_array_equal(A.pq_codes(), ref.pq_codes())
    qd = _dev(np.concatenate([fx.unit_rows(rng, 20, d), Xa[:10]]))
    k = min(50, N0)
    _same_lists(_search(A, qd, k, mode="dense", return_int=True), _search(B, qd, k, mode="dense", return_int=True), "edge dense")
    assert A.update_stats()["last_distortion"] == ref.encode(Xa, None)[3]


# ---- 3. counters --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_residual", [False, True])
def test_counters_equal_the_models_integers(tmp_path, by_residual):
    """un-normalised rows through add_items_device: 3x scaled rows leave the SQ8 grid, -3x a list's centroid lands far from
    the centroid of whichever list takes it, so its residual leaves [-127, 127] as well.  A clamp is never a refusal."""
    from recommendit_amd import PQIndex
    rng = np.random.RandomState(97)
    d, N0, nlist, dsub = 64, 6000, 24, 8
    X0 = _clustered(rng, N0, d, 20)
    C = R.kmeans_ip(X0, nlist, n_iter=2, seed=7)
    a0 = R.ivf_assign(X0, C).astype(np.int32)
    ids0 = np.arange(N0, dtype=np.int64)
    src = _f32(X0, ids0, C, a0)
    A = PQIndex.from_index(src, dsub=dsub, n_iter=2, by_residual=by_residual, frozen_updates=True)
    del src
    mq, sq = A.quantizer()
    book = A.codebooks()
    Mdl = PU.PqModel.from_corpus(X0, ids0, a0, nlist, mq, sq, book, C if by_residual else None, assign=P.assign_blas)
    np.testing.assert_array_equal(A.pq_codes(), Mdl.pq_codes())
    by_size = np.argsort(-np.bincount(a0, minlength=nlist))
    calls = [np.ascontiguousarray(np.concatenate([3.0 * _clustered(rng, 50, d, 20), -3.0 * C[by_size[0]][None, :] + 0.05 * rng.randn(30, d)]),
                                  dtype=np.float32),
             np.ascontiguousarray(np.concatenate([-3.0 * C[by_size[1]][None, :] + 0.05 * rng.randn(20, d), 3.0 * X0[:40]]), dtype=np.float32)]
    total, next_id = dict(clamped=0, residual_clamped=0, distortion=0), 10**6
    m = _Corpus(X0, ids0, a0)
    for i, Xs in enumerate(calls):
        lists = A.assign_lists(_dev(Xs)).cpu().numpy()
        ids = np.arange(next_id, next_id + len(Xs))
        next_id += len(Xs)
        want = Mdl.update([], Xs, ids, lists)
        assert want["clamped"] > 0 and want["distortion"] > 0 and (want["residual_clamped"] > 0) == by_residual      # the model first
        assert A.add_items_device(_dev(Xs), ids) == len(Xs)                                                       # never a refusal
        m.add(Xs, ids, lists)
        for key in total:
            total[key] += want[key]
        st = A.update_stats()
        print(f"call {i}: clamped {st['last_clamped']}, residual clamped {st['last_residual_clamped']}, distortion {st['last_distortion']}")
        assert (st["last_clamped"], st["last_residual_clamped"], st["last_distortion"]) == (want["clamped"], want["residual_clamped"],
                                                                                          want["distortion"])
        assert (st["clamped"], st["residual_clamped"], st["distortion_added"]) == (total["clamped"], total["residual_clamped"],
                                                                                  total["distortion"])
        assert st["updates"] == i + 1 and st["added"] == next_id - 10**6 and st["dropped"] == 0
        np.testing.assert_array_equal(A.pq_codes(), Mdl.pq_codes())
    assert [st["updates"], st["dropped"], st["added"], st["clamped"], st["residual_clamped"], st["distortion_added"]] == Mdl.stats
    _same_files(A, _scratch(m, C, A, False), tmp_path, "drift")
    # the drift signal reads as the docstring says: the scaled rows sit far worse in the codebooks than the build's rows
    assert st["distortion_added"] / st["added"] > A.train_stats()["distortion"][-1] / N0


# ---- 4. equivalences ------------------------------------------------------------------------------------------------------------
def _ivf_case(seed, d=64, N0=6000, nlist=24, extra=900):
    rng = np.random.RandomState(seed)
    Xall = _clustered(rng, N0 + extra, d, 20)
    X0, pool = Xall[:N0], Xall[N0:]
    ids0 = np.arange(N0, dtype=np.int64) * 3
    C = R.kmeans_ip(X0, nlist, n_iter=2, seed=7)
    a0 = R.ivf_assign(X0, C).astype(np.int32)
    return rng, X0, pool, ids0, C, a0


@pytest.mark.parametrize("by_residual", [False, True])
def test_update_items_equals_remove_then_add(tmp_path, by_residual):
    from recommendit_amd import PQIndex
    rng, X0, pool, ids0, C, a0 = _ivf_case(89)
    N0, d = X0.shape
    tags0 = rng.randint(0, 64, N0).astype(np.uint32)
    src = _f32(X0, ids0, C, a0, 4)
    A = PQIndex.from_index(src, dsub=8, n_iter=2, keep_vectors=True, by_residual=by_residual, frozen_updates=True)
    A.set_item_tags(tags0)
    B = PQIndex.from_index(src, dsub=8, ranges=A.quantizer(), codebooks=A.codebooks(), keep_vectors=True, by_residual=by_residual,
                           frozen_updates=True)
    B.set_item_tags(tags0)
    del src
    E = 2.0 * pool[:700]
    ids = rng.permutation(np.concatenate([rng.choice(ids0, 450, replace=False), np.arange(1, 750, 3)]))    # 450 stored, 250 not
    assert A.update_items(E, ids) == (450, 250)
    words = np.where(np.isin(ids, ids0), tags0[np.minimum(ids // 3, N0 - 1)], 0).astype(np.uint32)
    assert B.remove_items(ids) == 450
    assert B.add_items(E, ids, tags=words) == 700         # (remove forgets the words; an upsert without tags= keeps them)
    qd = _dev(np.concatenate([fx.unit_rows(rng, 50, d), _unit(E[:14])]))
    _assert_same_state(A, B, tmp_path, qd, "upsert", k=50)
    assert A.update_items(np.empty((0, d), np.float32), []) == (0, 0)
    sa, sb = A.update_stats(), B.update_stats()
    assert (sa["updates"], sb["updates"]) == (1, 2) and sa["distortion_added"] == sb["distortion_added"] > 0


@pytest.mark.parametrize("by_residual", [False, True])
def test_lockstep_with_the_f32_index_then_attach(by_residual):
    """the PQ index follows an f32 index update by update without vectors, then attaches that index's: accepted (same rows,
    same order, same lists), and e_j / a_j are those of a handle that carried its vectors through the same updates"""
    from recommendit_amd import PQIndex
    rng, X0, pool, ids0, C, a0 = _ivf_case(87)
    F = _f32(X0, ids0, C, a0)
    Q = PQIndex.from_index(F, dsub=16, n_iter=2, by_residual=by_residual, frozen_updates=True)
    V = PQIndex.from_index(F, dsub=16, ranges=Q.quantizer(), codebooks=Q.codebooks(), by_residual=by_residual, keep_vectors=True,
                           frozen_updates=True)
    rm = rng.choice(ids0, 500, replace=False)
    stay = ids0[~np.isin(ids0, rm)]
    ups = [("remove", rm, None),
           ("add", np.arange(10**6, 10**6 + 600), pool[:600]),
           ("update", np.concatenate([stay[1000:1200], np.arange(2 * 10**6, 2 * 10**6 + 100)]), 2.0 * pool[600:])]
    for op, ids, X in ups:
        for idx in (F, Q, V):
            if op == "remove":
                assert idx.remove_items(ids) == 500
            elif op == "add":
                assert idx.add_items(X, ids) == 600
            else:
                assert idx.update_items(X, ids) == (200, 100)
    np.testing.assert_array_equal(Q.item_ids, F.item_ids)
    assert not Q.has_vectors and V.has_vectors
    Q.attach_vectors(F)
    _same_lists(Q.refine_ranges(), V.refine_ranges(), "ranges: attached after against carried through")
    fresh = PQIndex.from_index(F, dsub=16, ranges=Q.quantizer(), codebooks=Q.codebooks(), by_residual=by_residual, keep_vectors=True)
    _same_lists(Q.refine_ranges(), fresh.refine_ranges(), "ranges against from scratch")
    np.testing.assert_array_equal(Q.pq_codes(), fresh.pq_codes())
    np.testing.assert_array_equal(V.pq_codes(), fresh.pq_codes())
    _same_lists(Q.refine_ranges(), RF.ranges(F.reconstruct(), Q.codes(), *Q.quantizer()), "ranges against NumPy")


@pytest.mark.parametrize("by_residual", [False, True])
def test_a_loaded_index_opts_in_and_updates_like_the_one_never_saved(tmp_path, by_residual):
    from recommendit_amd import PQIndex
    rng, X0, pool, ids0, C, a0 = _ivf_case(85)
    src = _f32(X0, ids0, C, a0)
    A = PQIndex.from_index(src, dsub=8, n_iter=2, by_residual=by_residual, frozen_updates=True)
    del src
    A.save(str(tmp_path / "saved.pq"))
    Lo = PQIndex.load(str(tmp_path / "saved.pq"))
    assert Lo.frozen_updates is False and Lo.by_residual == by_residual           # the flag is in no file
    with pytest.raises(NotImplementedError, match="rebuild"):
        Lo.remove_items([0])
    Lo.frozen_updates = True
    rm = rng.choice(ids0, 300, replace=False)
    for idx in (A, Lo):
        assert idx.update_items(pool[:400], np.concatenate([rm[:100], np.arange(10**6, 10**6 + 300)])) == (100, 300)
        assert idx.remove_items(rm) == 300               # (the 100 replaced ids are stored again, under their new rows)
    data = _same_files(A, Lo, tmp_path, "loaded")
    assert len(data) > 0
    qd = _dev(np.concatenate([fx.unit_rows(rng, 40, X0.shape[1]), pool[:10]]))
    _same_lists(_search(A, qd, 50, return_int=True), _search(Lo, qd, 50, return_int=True), "loaded")
    sa, sl = A.update_stats(), Lo.update_stats()
    assert sa == sl and sa["updates"] == 2
    assert len(Lo.train_stats()["distortion"]) == 0 and len(A.train_stats()["distortion"]) == 3     # after load: the first half only


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_rejected_updates_leave_the_index_as_it_was(tmp_path, exact):
    from recommendit_amd import PQIndex, SQ8Index, _lib as L
    rng = np.random.RandomState(93)
    d, N0 = 64, 5000
    X0 = _clustered(rng, N0, d, 10)
    ids0 = np.arange(100, 100 + N0, dtype=np.int64)
    C = R.kmeans_ip(X0, 10, n_iter=2, seed=3)
    src = _f32(X0, ids0) if exact else _f32(X0, ids0, C, R.ivf_assign(X0, C), 4)
    A = PQIndex.from_index(src, dsub=8, n_iter=2, keep_vectors=True, by_residual=not exact, frozen_updates=True)
    A.set_item_tags(rng.randint(0, 64, N0).astype(np.uint32))
    sq = SQ8Index.from_index(src)
    del src
    qd = _dev(fx.unit_rows(rng, 30, d))

    def snapshot():
        return _search(A, qd, 40, return_int=True) + _search(A, qd, 40, refine=2, return_cert=True) + [A.pq_codes(), A.item_tags()]
    before, stats0 = snapshot(), A.update_stats()
    A.save(str(tmp_path / "before.pq"))
    gen0 = int(_gen())
    new = fx.unit_rows(rng, 4, d)
    with pytest.raises(ValueError, match="item id 103 is already stored"):          # stored and not dropped in the same call
        A.add_items(new, [9001, 9002, 103, 9003])
    with pytest.raises(ValueError, match="item id 9002 is repeated inside one update"):
        A.add_items(new, [9001, 9002, 9003, 9002])
    with pytest.raises(ValueError, match="item id 9002 is repeated inside one update"):
        A.update_items(new, [9001, 9002, 9003, 9002])
    with pytest.raises(ValueError, match="item id 177 is repeated inside one update"):
        A.remove_items([150, 177, 160, 177])
    with pytest.raises(ValueError, match="the update would leave the index empty"):
        A.remove_items(ids0)
    with pytest.raises(ValueError):                                   # wrong width
        A.add_items(fx.unit_rows(rng, 4, d // 2), [9001, 9002, 9003, 9004])
    with pytest.raises(ValueError):                                   # ids and rows do not pair up
        A.add_items(new, [9001, 9002])
    assert A.remove_items([]) == 0 and A.remove_items([1, 2, 10**9]) == 0     # nothing to do: nothing changes
    assert A.add_items(np.empty((0, d), np.float32), []) == 0
    assert int(_gen()) == gen0
    assert A.index.ntotal == N0 and A.update_stats() == stats0 and stats0["updates"] == 0
    np.testing.assert_array_equal(A.item_ids, ids0)
    _same_lists(snapshot(), before, "after the refusals")
    A.save(str(tmp_path / "after.pq"))
    assert (tmp_path / "after.pq").read_bytes() == (tmp_path / "before.pq").read_bytes()
    # the flag off: the calls raise as they always did, the SQ8 entry point still refuses the handle in C
    A.frozen_updates = False
    for call in (lambda: A.add_items(new, [9001, 9002, 9003, 9004]), lambda: A.remove_items([150]), lambda: A.update_items(new, [1, 2, 3, 4]),
                 lambda: A.add_items_device(_dev(new), [9001, 9002, 9003, 9004])):
        with pytest.raises(NotImplementedError, match="rebuild"):
            call()
    with pytest.raises(RuntimeError, match="not updated in place"):
        SQ8Index.remove_items(A, [150])
    # and the PQ entry point refuses an SQ8 handle, by name
    out = torch.empty(N0, dtype=torch.int64, device="cuda")
    drop = torch.tensor([150], dtype=torch.int64, device="cuda")
    w = [C_.c_int64(0) for _ in range(4)]
    kind = C_.c_int(0)
    rc = L.lib().rihip_pq_update_apply(sq.index._h, sq._item_ids_dev.data_ptr(), drop.data_ptr(), 1, None, None, None, 0, out.data_ptr(),
                                       C_.byref(w[0]), C_.byref(w[1]), C_.byref(w[2]), C_.byref(w[3]), C_.byref(kind), L.stream_ptr())
    assert rc != 0 and b"rihip_pq_update_apply" in L.lib().rihip_last_error() and sq.index.ntotal == N0
    stats8 = (C_.c_int64 * 8)()
    assert L.lib().rihip_pq_update_stats(sq.index._h, stats8) != 0
    assert int(_gen()) == gen0 and A.index.ntotal == N0
    _same_lists(snapshot(), before, "after the refused entry points")
    A.frozen_updates = True
    assert A.remove_items([150]) == 1 and int(_gen()) > gen0          # an accepted update is seen by graph holders
    assert A.update_stats()["updates"] == 1


# ---- 6. serving ------------------------------------------------------------------------------------------------------------------
def test_serving_follows_the_catalogue(tmp_path):
    """test_serving_follows_the_catalogue of tests/test_gpu_sq8_update.py over a residual PQIndex pipeline"""
    from recommendit_amd import FAISSIndex, PQIndex, TwoTowerModel
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
    index = PQIndex.from_index(src, dsub=8, n_iter=2, by_residual=True, frozen_updates=True)
    del src
    users = list(range(1, 65))
    uid = torch.tensor(users, device="cuda")
    q = model.get_user_embeddings(uid, as_tensor=True)
    pipe = T._pipeline(tmp_path, index, model, nu, ni, genres)
    ids0 = pipe.recommend_batch(users)[0].cpu().numpy()
    removed = np.unique(ids0[:8, 0])                        # items that were recommended
    chosen = np.array([4, 9, 23])                           # query rows whose near-duplicates become new items
    new_ids = np.arange(ni + 1, ni + 1 + len(chosen))
    new_vec = q[chosen].cpu().numpy()
    assert index.remove_items(removed) == len(removed)
    assert index.add_items(new_vec, new_ids) == len(chosen)
    ids1, sc1, rs1 = [t.cpu().numpy() for t in pipe.recommend_batch(users)]
    assert not np.isin(ids1, removed).any()
    cs, cand = index.batch_search_device(q, k=200, normalized=True)
    cand = cand.cpu().numpy()
    assert not np.isin(cand, removed).any()
    for row, nid in zip(chosen, new_ids):
        # the query's own direction: inner product 1 before quantisation, in the list the query probes first
        assert nid in cand[row], (row, nid, cand[row, :5])
    # a fresh pipeline over the from-scratch PQ index of the final catalogue with the same frozen state
    keep = ~np.isin(np.array(item_ids), removed)
    nn = _unit(new_vec)
    m = _Corpus(np.concatenate([_unit(E)[keep], nn]), np.concatenate([np.array(item_ids)[keep], new_ids]),
                np.concatenate([a0[keep], index.assign_lists(_dev(nn)).cpu().numpy()]))
    fresh = _scratch(m, C, index, False, 4)
    (tmp_path / "b").mkdir()
    pipe_b = T._pipeline(tmp_path / "b", fresh, model, nu, ni, genres)
    want = [t.cpu().numpy() for t in pipe_b.recommend_batch(users)]
    _same_lists([ids1, sc1, rs1], want, "served")
