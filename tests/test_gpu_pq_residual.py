"""GPU: the product-quantised index with residual codes against the IVF centroids (PQIndex.from_index(by_residual=True)).

Build: list codes, codebooks, entry numbers, distortion trace, clamp count, the int16 decoded matrix and the
reconstruction are bitwise tests/pq_residual_reference.py's.  Search: a residual PQ index is the exact-integer-score index
of its own int16 reconstruction, so rows and integer scores equal tests/sq8_reference.py over that matrix exactly, float
scores lie within 1 f32 ulp of (float32)(b + t S), the modes return the same bytes and the re-do counts lie within
redo_bounds; one case each for a tag filter, both exclusion routes, the refined search with its certificate (code bound
254) and serving; persistence and refusals.  Every test first asserts from the references alone that its inputs reach the
path it is about."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_reference as P  # noqa: E402
import pq_residual_reference as PR  # noqa: E402
import sq8_filtered_reference as FR  # noqa: E402
import sq8_reference as S  # noqa: E402
import sq8_refine_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ("dense", "thresholded", "auto")


def _flat(X):
    from recommendit_amd import FAISSIndex
    idx = FAISSIndex(embed_dim=X.shape[1], exact=True)
    idx.build_from_device(torch.from_numpy(np.ascontiguousarray(X)).cuda(), np.arange(X.shape[0]))
    return idx


def _ivf(X, C, assign, nprobe, ids=None):
    from recommendit_amd import FAISSIndex
    idx = FAISSIndex(embed_dim=X.shape[1], n_lists=C.shape[0], n_probe=nprobe)
    idx.build_from_device(torch.from_numpy(np.ascontiguousarray(X)).cuda(),
                          np.arange(X.shape[0]) if ids is None else np.asarray(ids, dtype=np.int64), centroids=C,
                          assign=np.asarray(assign, dtype=np.int32))
    return idx


def _same_bytes(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ---- 1. build ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1500, 100])
@pytest.mark.parametrize("dsub", [8, 16])
@pytest.mark.parametrize("du", [40, 64, 128])
def test_build_is_bitwise_the_restatement(du, dsub, n, tmp_path):
    from recommendit_amd import PQIndex
    n_iter, nlist, centres = 3, 6, 40
    rng = np.random.default_rng(2000 + du + dsub + n)
    Cc0 = rng.standard_normal((centres, du)).astype(np.float32)
    X = (Cc0[rng.integers(0, centres, n)] + 0.15 * rng.standard_normal((n, du))).astype(np.float32)
    X[:, 2] = -0.75                                            # a constant column: its codes are 0
    # six ragged lists, list 3 empty, one of a single row (the existing build test's)
    assign = rng.integers(0, nlist, n).astype(np.int32)
    assign[assign == 3] = 4
    assign[assign == 1] = 0
    assign[7] = 1
    lens = np.bincount(assign, minlength=nlist)
    assert lens[3] == 0 and lens[1] == 1 and len(set(lens.tolist())) >= 4 and (lens % 64 != 0).any()
    # centroids off the code grid: the lists' means plus noise (the empty list: noise alone)
    Cc = (0.1 * rng.standard_normal((nlist, du))).astype(np.float32)
    for l in range(nlist):
        if lens[l]:
            Cc[l] += X[assign == l].mean(axis=0)
    # one residual that clamps: row `hot` of list 4 sits at column 5's minimum, its centroid far above the maximum
    hot = int(np.nonzero(assign == 4)[0][3])
    X[hot, 5] = X[:, 5].min() - 0.5
    Cc[4, 5] = X[:, 5].max() + 1.0
    dpad = P.dpad_of(du)
    M = dpad // dsub
    m_, s_ = S.train_quantizer(X)
    c = P.pad_codes(S.encode(X, m_, s_), dpad)
    K = PR.list_codes(Cc, m_, s_, dpad)
    grid = (Cc.astype(np.float32) - m_[None, :]) / s_[None, :]
    assert (np.abs(grid - np.rint(grid)) > 1e-3).mean() > 0.9   # off the grid
    assert c[hot, 5] == -127 and K[4, 5] == 127
    book, codes, trace, clamped = PR.train(c, K, assign, dsub, n_iter)
    assert clamped >= 1 and trace.shape == (n_iter + 1,) and trace[-1] <= trace[0]
    dec = PR.decode(codes, book, K, assign)
    assert dec.dtype == np.int16
    if n == 1500:                                              # (at 100 rows every row is its own entry: decoded = code)
        assert np.abs(dec.astype(np.int32)).max() > 127        # genuinely 16-bit
    assert int(dec[hot, 5]) >= 0 > int(c[hot, 5])              # K = 127 plus an entry: the clamped value is not recovered
    src = _ivf(X, Cc, assign, 2)
    pq = PQIndex.from_index(src, dsub=dsub, n_iter=n_iter, by_residual=True)
    assert pq.by_residual
    qm, qs = pq.quantizer()
    np.testing.assert_array_equal(qm, m_)
    np.testing.assert_array_equal(qs, s_)
    np.testing.assert_array_equal(pq.list_codes(), K)
    np.testing.assert_array_equal(pq.codebooks(), book)
    np.testing.assert_array_equal(pq.pq_codes(), codes)
    ts = pq.train_stats()
    np.testing.assert_array_equal(ts["distortion"], trace)
    assert ts["residual_clamped"] == clamped and ts["by_residual"] is True
    got = pq.codes()
    assert got.dtype == np.int16
    np.testing.assert_array_equal(got, dec[:, :du])
    np.testing.assert_array_equal(pq.reconstruct(), PR.reconstruct(dec, m_, s_))
    st = pq.stats()
    assert st["by_residual"] is True and st["bytes_per_vector"] == M and st["n_lists"] == nlist
    plain = PQIndex.from_index(src, dsub=dsub, n_iter=0)
    assert not plain.by_residual and plain.train_stats()["residual_clamped"] == 0
    assert st["device_bytes"] == plain.stats()["device_bytes"] + nlist * dpad      # the list codes are counted
    assert ts["peak_bytes"] > st["device_bytes"]
    # injected ranges= + codebooks= reproduce the handle
    again = PQIndex.from_index(src, dsub=dsub, ranges=(m_, s_), codebooks=book, by_residual=True)
    _same_bytes((again.list_codes(), again.codebooks(), again.pq_codes(), again.codes()),
                (pq.list_codes(), pq.codebooks(), pq.pq_codes(), got))
    assert again.train_stats()["distortion"].tolist() == [int(trace[-1])] and again.train_stats()["residual_clamped"] == clamped
    # save -> load -> save
    p1, p2 = tmp_path / "a.pqr", tmp_path / "b.pqr"
    pq.save(str(p1))
    back = PQIndex.load(str(p1))
    back.save(str(p2))
    assert p1.read_bytes() == p2.read_bytes() and p1.read_bytes()[:8] == b"RIHIPPR1"
    assert back.by_residual and back.dsub == dsub
    _same_bytes((back.list_codes(), back.codes()), (K, got))


# ---- 2. search -----------------------------------------------------------------------------------------------------------
# The existing PQ search case's lists: list 0 empty, list 1 one row, list 2 65 rows, three long ragged ones.  Every
# centroid carries 1024 on its own axis (columns 0 .. 5), so the first six query columns decide the probes of every query
# but two: queries 0 and 1 probe lists 1 and 2 (66 rows); queries 2 and 3 (all +1 / all -1: the score extremes) see the
# same coarse score on every list (column 6 evens the centroids' column sums out) and probe the lowest lists.  Beyond the
# axis the centroids are list codes / 128, random and so strongly different between lists; list 1's are all 127.
S_LENS = [0, 1, 65, 64000, 48001, 35555]
S_NQ, S_KS = 70, (1, 10, 100)


def _sign_book(du, dsub):
    """entry e of every sub-space: +-127 by the bits of e (bit j set: column j negative; at dsub 16 columns j and j + 8
    share bit j).  Entry 0 is all +127, all entries have the same norm, padding columns hold 0"""
    dpad = P.dpad_of(du)
    M = dpad // dsub
    bits = (np.arange(256)[:, None] >> np.arange(8)[None, :]) & 1
    pat = np.where(bits == 1, -127, 127).astype(np.int8)                           # [256, 8]
    entry = pat if dsub == 8 else np.concatenate([pat, pat], axis=1)
    book = np.broadcast_to(entry[None], (M, 256, dsub)).copy()
    col = np.arange(dpad).reshape(M, 1, dsub)
    return np.where(col < du, book, 0).astype(np.int8)


def _sign_assign(r, dsub):
    """the entry of the smallest D under _sign_book, lowest entry on a tie: D = |r|^2 + |b|^2 - 2 <r, b> with |b| the same
    for every entry, so bit j is set exactly where the (summed) residual of its columns is negative"""
    N, dpad = r.shape
    t = r.astype(np.int32).reshape(N, dpad // dsub, dsub)
    if dsub == 16:
        t = t[:, :, :8] + t[:, :, 8:]
    return ((t < 0).astype(np.int64) << np.arange(8)[None, None, :]).sum(axis=2).astype(np.uint8)


def _search_case(du, dsub, nprobe):
    rng = np.random.default_rng(9000 + du + dsub)
    N, nlist = sum(S_LENS), len(S_LENS)
    dpad = P.dpad_of(du)
    book = _sign_book(du, dsub)
    assign = np.concatenate([np.full(n, l, np.int32) for l, n in enumerate(S_LENS)])[rng.permutation(N)]
    c = rng.integers(-127, 128, (N, du)).astype(np.int8)
    plus = int(np.nonzero(assign == 1)[0][0])
    c[plus] = 127                                              # list 1's one row: residual 0, every entry ties, entry 0 wins
    dup = np.nonzero(assign == 3)[0]
    c[dup[30000:30300]] = c[dup[100:400]]                      # ties inside a list across its splits
    X = c.astype(np.float32) / np.float32(128.0)
    m_, s_ = np.zeros(du, np.float32), np.full(du, 1.0 / 128.0, np.float32)
    np.testing.assert_array_equal(S.encode(X, m_, s_), c)
    Kr = rng.integers(-127, 128, (nlist, du)).astype(np.int32)
    Kr[1] = 127
    Cc = (Kr / 128.0).astype(np.float32)
    Cc[np.arange(nlist), np.arange(nlist)] = 1024.0            # the axis: decides the probes
    Cc[:, 6] = 0.0
    Cc[:, 6] = (Cc[1].sum() + np.float32(127.0 / 128.0)) - Cc.sum(axis=1)          # equal column sums; list 1 keeps 127 / 128
    assert len(set(Cc.astype(np.float64).sum(axis=1).tolist())) == 1
    K = PR.list_codes(Cc, m_, s_, dpad)
    assert (K[1, :du] == 127).all() and (K[np.arange(nlist), np.arange(nlist)] == 127).all() and (K[:, du:] == 0).all()
    r, clamped = PR.residuals(P.pad_codes(c, dpad), K, assign)
    codes = _sign_assign(r, dsub)
    got_codes, _ = P.assign(r[:600], book)                     # (the restatement agrees on a sample)
    np.testing.assert_array_equal(got_codes, codes[:600])
    assert clamped > 0 and (codes[plus] == 0).all()
    dec = PR.decode(codes, book, K, assign)
    assert (dec[plus, :du] == 254).all()
    Q = (rng.integers(-16, 17, (S_NQ, du)) / 8.0).astype(np.float32)
    Q[:, :3] = -1.0
    pat = np.array([[1, 1, -1], [1, -1, 1], [-1, 1, 1]], np.float32)
    Q[:, 3:6] = pat[np.arange(S_NQ) % 3]
    Q[0, :6] = [-1, 1, 1, -1, -1, -1]
    Q[1, :6] = [-1, 1, 1, -1, -1, -1]
    Q[2] = 1.0
    Q[3] = -1.0
    # every coarse score is exact in f32 in any order (multiples of 2^-10 below 2^13) and the probes have no tie but the
    # intended ones: the axis term moves a score by 2048, the rest by less than 2 * (du + |column 6|) in all
    rest = 2.0 * (np.abs(Cc).sum(axis=1) - 1024.0).max()
    assert rest < 1024.0, rest
    return dict(N=N, nlist=nlist, book=book, codes=codes, K=K, dec=dec[:, :du], X=X, m=m_, s=s_, Cc=Cc, Q=Q, assign=assign,
                plus=plus, c=c)


class _Expect:
    """tests/test_gpu_pq_index.py's: top-kmax rows and scores of the reference, the query transform, the re-do verdicts"""

    def __init__(self, Q, c, m, s, ks, allowed=None, rule=None):
        self.n, self.t, self.b = S.encode_queries(Q, m, s)
        self.Sc = S.int_scores_blas(self.n, c)
        assert np.abs(self.Sc).max() <= PR.SCORE_BOUND
        self.rows, self.sc = S.topk_fast(self.Sc, max(ks), allowed)
        self.redo = {k: rule(self.Sc, k) for k in ks} if rule else {}

    def check(self, got, k, rows=None, sc=None, id_of=None):
        gs, gr, gi = got
        rows = self.rows[:, :k] if rows is None else rows
        sc = self.sc[:, :k] if sc is None else sc
        pad = rows < 0
        np.testing.assert_array_equal(gr, rows if id_of is None else np.where(pad, -1, id_of[np.maximum(rows, 0)]))
        if gi is not None:
            np.testing.assert_array_equal(gi[~pad], sc[~pad])
            assert (gi[pad] == -2 ** 31).all()
        assert np.isneginf(gs[pad]).all()
        ref64 = (self.b[:, None] + self.t.astype(np.float64)[:, None] * sc.astype(np.float64))[~pad]
        ref32 = ref64.astype(np.float32)
        assert (np.abs(gs[~pad].astype(np.float64) - ref32.astype(np.float64))
                <= np.spacing(np.abs(ref32)).astype(np.float64)).all()


def _search(pq, Q, k, mode):
    before = pq.search_stats()
    s, r, i = pq.search_rows_device(torch.from_numpy(np.ascontiguousarray(Q)).cuda(), k, mode=mode, return_int=True)
    torch.cuda.synchronize()
    after = pq.search_stats()
    return (s.cpu().numpy(), r.cpu().numpy(), i.cpu().numpy()), (after[0] - before[0], after[1] - before[1])


@pytest.mark.parametrize("du,dsub,nprobe", [(128, 8, 2), (128, 16, 6), (64, 16, 2), (40, 8, 6)],
                         ids=["d128-pq8-probe2", "d128-pq16-probe6", "d64-pq16-probe2", "d40-pq8-probe6"])
def test_search_equals_the_reference_over_the_int16_decoded_matrix(du, dsub, nprobe):
    from recommendit_amd import PQIndex
    cs = _search_case(du, dsub, nprobe)
    Q, N, nlist, assign = cs["Q"], cs["N"], cs["nlist"], cs["assign"]
    # -- the path, from the references alone
    assert S_NQ % 32 != 0 and (S_NQ + 31) // 32 == 3            # three query groups, the last partial
    probes = S.probed_lists(Q, cs["Cc"], nprobe)
    per_list = np.bincount(probes.ravel(), minlength=nlist)
    allowed = FR.probed_mask(assign, probes, nlist)
    if nprobe < nlist:
        assert sorted(probes[0].tolist()) == [1, 2] and sorted(probes[2].tolist()) == [0, 1] and sorted(probes[3].tolist()) == [0, 1]
        assert (np.sort(probes[4:], axis=1) >= 3).all()
        assert allowed[0].sum() == 66 and allowed[2].sum() == 1 and max(S_KS) > 66
    else:
        assert allowed.all()
    tpi, n_seq, splits = S.plan(S_LENS, per_list, 1)
    assert tpi >= 3, tpi
    assert any(p > 0 and s % tpi != 0 for p, s in zip(per_list, n_seq))             # a ragged last split
    assert any(l % S.TILE != 0 and p > 0 for p, l in zip(per_list, S_LENS))         # a short last tile: n_ok
    assert S.dense_chunk(S_LENS, nprobe) >= S_NQ
    rule = lambda Sc, k: S.ivf_thresholded_redo(Sc, k, assign, probes, nlist)       # noqa: E731
    ex = _Expect(Q, cs["dec"], cs["m"], cs["s"], list(S_KS), allowed=allowed, rule=rule)
    # the score extremes: list 1's row against the all +1 and the all -1 query
    smax = 32512 * 254 * du
    assert (du < 128 or smax == PR.SCORE_BOUND) and ex.Sc[2, cs["plus"]] == smax and ex.Sc[3, cs["plus"]] == -smax
    assert ex.sc[2, 0] == smax and ex.rows[2, 0] == cs["plus"] and allowed[3, cs["plus"]]
    if nprobe < nlist:
        assert ex.sc[3, 0] == -smax and ex.rows[3, 1] == -1                         # (its one probed row)
    else:
        assert ex.Sc[3].min() == -smax
    # a padding row of list 1 (entry 0 under K = 127: the score smax) would tie the best row if n_ok let it through
    assert (cs["book"][:, 0][:, :1] >= 0).all() and (cs["K"][1, :du] == 127).all() and S_LENS[1] % S.TILE != 0
    # T matters: without it, or with the next list's, the top k changes for most queries
    split = PR.split_scores(ex.n, cs["codes"], cs["book"], cs["K"], assign)
    np.testing.assert_array_equal(split, ex.Sc)
    T = (ex.n.astype(np.int64) @ cs["K"][:, :du].astype(np.int64).T)
    no_t = S.topk_fast(ex.Sc - T[:, assign], 10, allowed)[0]
    wrong_t = S.topk_fast(ex.Sc - T[:, assign] + T[:, (assign + 1) % nlist], 10, allowed)[0]
    assert (no_t != ex.rows[:, :10]).any(axis=1).mean() > 0.5 and (wrong_t != ex.rows[:, :10]).any(axis=1).mean() > 0.5
    # -- the index
    src = _ivf(cs["X"], cs["Cc"], assign, nprobe)
    pq = PQIndex.from_index(src, dsub=dsub, ranges=(cs["m"], cs["s"]), codebooks=cs["book"], by_residual=True)
    del src
    np.testing.assert_array_equal(pq.list_codes(), cs["K"])
    np.testing.assert_array_equal(pq.pq_codes(), cs["codes"])
    np.testing.assert_array_equal(pq.codes(), cs["dec"])
    for k in S_KS:
        dense, d_dense = _search(pq, Q, k, "dense")
        thr, d_thr = _search(pq, Q, k, "thresholded")
        auto, d_auto = _search(pq, Q, k, "auto")
        ex.check(dense, k)
        _same_bytes(dense, thr)
        _same_bytes(dense, auto)
        assert d_dense == (0, 0)
        lo, hi = S.redo_bounds(ex.redo[k])
        print("k", k, "re-done", d_thr[1], "bounds", lo, hi)
        assert d_thr[0] == S_NQ and lo <= d_thr[1] <= hi, (d_thr, lo, hi)
        assert d_auto == (d_thr if S.auto_is_thresholded(S_NQ, k, S_LENS, nprobe) else (0, 0))
        if nprobe < nlist and k > 66:
            assert (dense[1][0, 66:] == -1).all() and (dense[1][0, :66] >= 0).all() and (dense[1][2, 1:] == -1).all()
    if nprobe < nlist:
        assert max(S.redo_bounds(ex.redo[k])[1] for k in S_KS) > 0                  # the re-do is reached
    if du == 64:
        # the refine side over codes that leave int8: e_j from the int16 range pass, the bound with 254
        src = _ivf(cs["X"], cs["Cc"], assign, nprobe)
        pq.attach_vectors(src)
        del src
        ea = R.ranges(cs["X"], cs["dec"], cs["m"], cs["s"])
        assert np.abs(cs["dec"].astype(np.int32)).max() == 254 and ea[0].min() >= 127.0 / 128   # (the plus row: |127 - 254| / 128)
        e, a = pq.refine_ranges()
        np.testing.assert_array_equal(e, ea[0])
        np.testing.assert_array_equal(a, ea[1])
        want = PR.refine(Q, cs["X"], cs["dec"], cs["m"], cs["s"], 10, 20, allowed, ea)
        gs, gr, gc, gb = [t.cpu().numpy() for t in pq.search_rows_device(torch.from_numpy(Q).cuda(), 10, refine=2, return_cert=True)]
        np.testing.assert_array_equal(gr, want["rows"])
        np.testing.assert_array_equal(gs.view(np.uint32), want["scores"].view(np.uint32))
        np.testing.assert_array_equal(gc, want["cert"])
        np.testing.assert_allclose(gb, want["bound"], rtol=1e-12, atol=0)


# ---- 3. one case each: filter, both exclusion routes, refine ------------------------------------------------------------
E_N, E_D, E_NQ, E_NLIST, E_NPROBE, E_DSUB, E_ITER = 6000, 64, 70, 8, 3, 8, 2


@pytest.fixture(scope="module")
def trained_case():
    """an IVF index with residual codebooks trained on unit rows, vectors attached; the decoded matrix from the restatement"""
    from recommendit_amd import PQIndex
    X, Q = R.unit_rows(41, E_N, E_D), R.unit_rows(42, E_NQ, E_D)
    Cc, assign = R.ivf_layout(43, E_N, E_D, E_NLIST)
    ids = np.arange(E_N) + 1000
    src = _ivf(X, Cc, assign, E_NPROBE, ids=ids)
    pq = PQIndex.from_index(src, dsub=E_DSUB, n_iter=E_ITER, keep_vectors=True, by_residual=True)
    m_, s_ = S.train_quantizer(X)
    K = PR.list_codes(Cc, m_, s_, 64)
    assert len({k.tobytes() for k in K}) == E_NLIST and np.abs(K.astype(np.int32)).max() == 127
    book, codes, trace, clamped = PR.train(P.pad_codes(S.encode(X, m_, s_), 64), K, assign, E_DSUB, E_ITER)
    dec = PR.decode(codes, book, K, assign)[:, :E_D]
    # (centroids of +-1/2 clamp to list codes of +-127, so the residuals are one-sided and trained entries keep the decoded
    # code inside int8 here; codes beyond 127 are the search case's, which also checks the int16 range pass)
    assert clamped > 0 and dec.dtype == np.int16
    np.testing.assert_array_equal(pq.codes(), dec)
    assert pq.train_stats()["residual_clamped"] == clamped
    probed = R.probe_mask(Q, Cc, assign, E_NPROBE)
    ex = _Expect(Q, dec, m_, s_, [200], allowed=probed)
    return dict(pq=pq, src=src, X=X, Q=Q, qd=torch.from_numpy(Q).cuda(), ids=ids, m=m_, s=s_, dec=dec, probed=probed, ex=ex,
                assign=assign, Cc=Cc)


def _restricted(case, k, ok):
    return S.topk_fast(case["ex"].Sc, k, case["probed"] & ok)


def test_tag_filter_inside_the_residual_scan(trained_case):
    c, k = trained_case, 20
    pq = c["pq"]
    rng = np.random.default_rng(5)
    tags = rng.integers(0, 16, E_N).astype(np.uint32)
    flt = (3, 0, 4)
    ok = FR.passes(tags, FR.words(flt, E_NQ))
    assert 0.2 < ok.mean() < 0.8
    rows, sc = _restricted(c, k, ok)
    pq.set_item_tags(tags)
    before = pq.filtered_stats()[0]
    try:
        for mode in MODES:
            s_, i_, n_ = pq.batch_search_device(c["qd"], k=k, normalized=True, mode=mode, return_int=True, item_filter=flt)
            c["ex"].check((s_.cpu().numpy(), i_.cpu().numpy(), n_.cpu().numpy()), k, rows, sc, id_of=c["ids"])
        assert pq.filtered_stats()[0] - before == 3 * E_NQ
    finally:
        pq.clear_item_tags()


def _seen_of(case):
    """every other one of each query's best 2 * count rows, count 0 / 5 / 40 by query"""
    from recommendit_amd import SeenItems
    top = case["ex"].rows
    counts = np.array([0] * 20 + [5] * 25 + [40] * (E_NQ - 45))
    seen = np.zeros((E_NQ, E_N), dtype=bool)
    users, items = [], []
    for q in range(E_NQ):
        mine = top[q, 1:2 * counts[q]:2]
        assert (mine >= 0).all()
        seen[q, mine] = True
        users += [q] * len(mine)
        items += (mine + 1000).tolist()
    return SeenItems.from_pairs(np.array(users), np.array(items), E_NQ), seen


def test_seen_items_excluded_inside_the_residual_scan(trained_case):
    c, k = trained_case, 20
    store, seen = _seen_of(c)
    rows, sc = _restricted(c, k, ~seen)
    assert (rows != c["ex"].rows[:, :k]).any()
    for mode in MODES:
        s_, i_, n_ = c["pq"].batch_search_device(c["qd"], k=k, normalized=True, mode=mode, exclude=store,
                                                 user_ids=list(range(E_NQ)), exclusion="scan", return_int=True)
        c["ex"].check((s_.cpu().numpy(), i_.cpu().numpy(), n_.cpu().numpy()), k, rows, sc, id_of=c["ids"])


def test_seen_items_excluded_by_over_fetch(trained_case):
    c, k = trained_case, 20
    store, seen = _seen_of(c)
    rows, sc = _restricted(c, k, ~seen)
    s_, i_ = c["pq"].batch_search_device(c["qd"], k=k, normalized=True, exclude=store, user_ids=list(range(E_NQ)))
    c["ex"].check((s_.cpu().numpy(), i_.cpu().numpy(), None), k, rows, sc, id_of=c["ids"])
    assert c["pq"].exclusion_deficit() == 0


def test_refined_search_and_certificate_with_the_code_bound_254(trained_case):
    c, k = trained_case, 10
    pq = c["pq"]
    assert pq.has_vectors
    ea = R.ranges(c["X"], c["dec"], c["m"], c["s"])
    e, a = pq.refine_ranges()
    np.testing.assert_array_equal(e, ea[0])
    np.testing.assert_array_equal(a, ea[1])
    want = PR.refine(c["Q"], c["X"], c["dec"], c["m"], c["s"], k, 2 * k, c["probed"], ea)
    b127 = R.bound(c["Q"], c["m"], c["s"], c["ex"].n, c["ex"].t, ea[0], ea[1])
    assert (want["rows"] >= 0).all() and (want["bound"] > b127 * (1 + 1e-9)).all()   # the factor is visible in the bound
    print("certified by the reference:", int(want["cert"].sum()), "of", E_NQ)
    br, bs = R.brute_force(c["Q"], c["X"], k, c["probed"])
    for mode in ("dense", "thresholded"):
        gs, gr, gc, gb = [t.cpu().numpy() for t in pq.search_rows_device(c["qd"], k, mode=mode, refine=2, return_cert=True)]
        np.testing.assert_array_equal(gr, want["rows"])
        np.testing.assert_array_equal(gs.view(np.uint32), want["scores"].view(np.uint32))
        np.testing.assert_array_equal(gc, want["cert"])
        np.testing.assert_allclose(gb, want["bound"], rtol=1e-12, atol=0)
        sure = gc == 1
        np.testing.assert_array_equal(gr[sure], br[sure])       # every certified query: the brute force over its probed lists
        assert gs[sure].tobytes() == bs[sure].tobytes()
    # the certificate's other branch: k_scan beyond every query's probed rows, so stage 1 returns them all
    k_scan = 4096
    assert c["probed"].sum(axis=1).max() < k_scan
    want = PR.refine(c["Q"], c["X"], c["dec"], c["m"], c["s"], k, k_scan, c["probed"], ea)
    assert (want["cert"] == 1).all()
    np.testing.assert_array_equal(want["rows"], br)
    gs, gr, gc, gb = [t.cpu().numpy() for t in pq.search_rows_device(c["qd"], k, refine=k_scan / k, return_cert=True)]
    np.testing.assert_array_equal(gr, br)
    assert gs.tobytes() == bs.tobytes() and (gc == 1).all()
    np.testing.assert_allclose(gb, want["bound"], rtol=1e-12, atol=0)


# ---- 4. persistence and refusals -----------------------------------------------------------------------------------------
def test_the_three_loaders_refuse_each_others_files_and_the_refusals(trained_case, tmp_path):
    from recommendit_amd import PQIndex, SQ8Index
    from recommendit_amd import _lib as L
    import ctypes as C
    c, k = trained_case, 15
    pq = c["pq"]
    want = [t.cpu().numpy() for t in pq.batch_search_device(c["qd"], k=k, normalized=True, return_int=True)]
    c["ex"].check(want, k, id_of=c["ids"])
    files = {"residual": tmp_path / "a.pqr", "pq": tmp_path / "b.pq", "sq8": tmp_path / "c.sq8"}
    pq.save(str(files["residual"]))
    plain = PQIndex.from_index(c["src"], dsub=E_DSUB, n_iter=0)
    plain.save(str(files["pq"]))
    SQ8Index.from_index(c["src"]).save(str(files["sq8"]))
    assert [files[n].read_bytes()[:8] for n in ("residual", "pq", "sq8")] == [b"RIHIPPR1", b"RIHIPPQ1", b"RIHIPSQ8"]
    loaders = {"residual": ("rihip_pq_index_load_residual", b"not a residual PQ index file"),
               "pq": ("rihip_pq_index_load", b"not a PQ index file"), "sq8": ("rihip_sq8_index_load", b"not an SQ8 index file")}
    for kind, (fn, msg) in loaders.items():
        for other, path in files.items():
            h = C.c_void_p()
            rc = getattr(L.lib(), fn)(str(path).encode(), C.byref(h))
            if other == kind:
                assert rc == 0 and h.value
                L.lib().rihip_sq8_index_destroy(h)
            else:
                assert rc != 0 and not h.value and msg in L.lib().rihip_last_error(), (kind, other)
    # load picks the format; the loaded index searches as the built one
    back = PQIndex.load(str(files["residual"]))
    assert back.by_residual and back.n_probe == E_NPROBE and back.train_stats()["distortion"].size == 0
    _same_bytes(want, [t.cpu().numpy() for t in back.batch_search_device(c["qd"], k=k, normalized=True, return_int=True)])
    assert not PQIndex.load(str(files["pq"])).by_residual
    with pytest.raises(RuntimeError, match="not an SQ8 index file"):
        SQ8Index.load(str(files["residual"]))
    # the int8 accessor and the SQ8 writer refuse the handle; a plain handle has no list codes
    buf = np.empty((E_N, E_D), dtype=np.int8)
    assert L.lib().rihip_sq8_index_get_codes(pq.index._h, buf.ctypes.data) != 0
    assert b"rihip_pq_index_get_decoded16" in L.lib().rihip_last_error()
    assert L.lib().rihip_sq8_index_save(pq.index._h, str(tmp_path / "d.sq8").encode()) != 0 and not (tmp_path / "d.sq8").exists()
    with pytest.raises(RuntimeError, match="not a residual index"):
        plain.list_codes()
    # a flat source is refused, in Python and under it
    flat = _flat(c["X"][:500])
    with pytest.raises(ValueError, match="IVF"):
        PQIndex.from_index(flat, by_residual=True)
    h = C.c_void_p()
    assert L.lib().rihip_pq_index_from_ip_index_residual(flat.index._h, None, None, 8, 1, None, 1, C.byref(h), L.stream_ptr()) != 0
    assert b"IVF" in L.lib().rihip_last_error() and not h.value
    # no live updates, as on every PQ index
    x = c["X"][:2].copy()
    for call in (lambda: pq.add_items(x, [1, 2]), lambda: pq.remove_items([1000]), lambda: pq.update_items(x, [1000, 5])):
        with pytest.raises(NotImplementedError, match="rebuild"):
            call()
    with pytest.raises(RuntimeError, match="not updated in place"):
        SQ8Index.remove_items(pq, [1000])
    _same_bytes(want, [t.cpu().numpy() for t in pq.batch_search_device(c["qd"], k=k, normalized=True, return_int=True)])


# ---- 5. serving ------------------------------------------------------------------------------------------------------------
def test_pipeline_over_a_residual_pq_index_equals_its_stages_run_by_hand(tmp_path):
    from oracle import fixtures as fx
    from oracle import gbdt_np as G
    from recommendit_amd import FAISSIndex, LightGBMRanker, PQIndex, TwoTowerModel
    from recommendit_amd import _lib as L
    from recommendit_amd.recommender import (GpuFeatureStore, GpuRecommendationPipeline, build_ranking_features_device,
                                             feature_columns)
    nu, ni, d, H, kc, k = 120, 900, 64, 128, 100, 10
    sd = fx.make_state(nu, ni, d, H, seed=21)
    model = TwoTowerModel(nu, ni, d, H)
    model.load_state_dict({key: torch.from_numpy(v.copy()) for key, v in sd.items()})
    rng = np.random.RandomState(2)
    item_ids = list(range(1, ni + 1))
    genres = (rng.rand(ni, 18) < 0.15).astype(np.float32)
    E = model.get_item_embeddings(item_ids, genres)
    src = FAISSIndex(embed_dim=d, n_lists=6, n_probe=2)
    src.build_ivf_index(E, item_ids)
    pq = PQIndex.from_index(src, dsub=16, n_iter=2, by_residual=True)
    plain = PQIndex.from_index(src, dsub=16, n_iter=2)
    del src
    assert pq.by_residual and np.abs(pq.list_codes().astype(np.int32)).max() > 0
    forest = G.random_forest_model(30, 15, 50, seed=5, names=feature_columns())
    p = tmp_path / "r.lgbm"
    p.write_text(G.write_text_model(forest))
    ranker = LightGBMRanker.load(str(p))
    store = GpuFeatureStore(nu, ni)
    ut, it = store.user.copy(), store.item.copy()
    ut[1:, :6] = rng.rand(nu, 6) * [5, 8, 1, 1, 1, 1]; ut[1:, 6:] = rng.rand(nu, 18)
    it[1:, :5] = rng.rand(ni, 5) * [5, 9, 1, 1.5, 1]; it[1:, 5:] = genres
    store.load_arrays(ut, it)
    pipe = GpuRecommendationPipeline(model, pq, ranker, store, top_k_candidates=kc, top_k_results=k)
    users = [1, 7, 120, 42, 3]
    ids, sc, rs = pipe.recommend_batch(users)
    uid = torch.tensor(users, dtype=torch.long, device="cuda")
    q = model.get_user_embeddings(uid, as_tensor=True)
    r_s, cand = pq.batch_search_device(q, k=kc, normalized=True)
    assert (cand >= 0).any() and not torch.equal(cand, plain.batch_search_device(q, k=kc, normalized=True)[1])
    Xf = build_ranking_features_device(store, uid, cand, ranker.feature_names)
    scores = ranker.predict_device(Xf)
    h_ids = torch.empty((len(users), k), dtype=torch.int64, device="cuda")
    h_top = torch.empty((len(users), k), dtype=torch.float64, device="cuda")
    h_rs = torch.empty((len(users), k), dtype=torch.float32, device="cuda")
    L.check(L.lib().rihip_rank_topk(scores.data_ptr(), cand.data_ptr(), r_s.data_ptr(), len(users), kc, k, h_ids.data_ptr(),
                                    h_top.data_ptr(), h_rs.data_ptr(), L.stream_ptr()), "rank_topk")
    torch.cuda.synchronize()
    assert torch.equal(ids, h_ids) and torch.equal(sc, h_top) and torch.equal(rs, h_rs)
