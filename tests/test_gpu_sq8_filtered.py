"""GPU: the SQ8 index's filtered search (tag predicates inside the int8 scan), its refined and certified form, seen-item
exclusion on the index, and the serve chain over a tagged SQ8 index.

The contract is tests/test_gpu_sq8_paths.py's: rows and integer scores equal the NumPy restatement exactly
(sq8_reference.int_scores_blas + topk_fast(..., allowed = passes & probed)), padding is -1 / -2^31 / -inf, float scores
within 1 f32 ulp of (float32)(b + t S) evaluated in f64, and the modes return the same bytes.  Every test first asserts
from the reference alone that its inputs reach the path it is about, then checks the filtered_stats() delta against
sq8_reference.redo_bounds of sq8_filtered_reference.thresholded_redo (the re-do rule on passing rows only)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_filtered_reference as FR  # noqa: E402
import sq8_reference as S  # noqa: E402
import sq8_refine_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ("dense", "thresholded", "auto")
NONE_BIT = 1 << 15      # carried by the rows of the IVF list whose rows all fail


def _flat(X, ids=None):
    from recommendit_amd import FAISSIndex
    idx = FAISSIndex(embed_dim=X.shape[1], exact=True)
    idx.build_from_device(torch.from_numpy(np.ascontiguousarray(X)).cuda(),
                          np.arange(X.shape[0]) if ids is None else np.asarray(ids, dtype=np.int64))
    return idx


def _ivf(X, C, assign, nprobe, ids=None):
    from recommendit_amd import FAISSIndex
    idx = FAISSIndex(embed_dim=X.shape[1], n_lists=C.shape[0], n_probe=nprobe)
    idx.build_from_device(torch.from_numpy(np.ascontiguousarray(X)).cuda(),
                          np.arange(X.shape[0]) if ids is None else np.asarray(ids, dtype=np.int64), centroids=C,
                          assign=np.asarray(assign, dtype=np.int32))
    return idx


def _rows(seed, n, du):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, du)) * rng.uniform(0.05, 2.0, du)).astype(np.float32)
    X[:, 2] = -0.75
    return X, rng


def _tags(rng, n):
    """bit 0 on every row, bit 1 on half, bit 2 on a tenth, bit 3 on 3 %, bit 4 on 1 %, bits 5 - 7 on half each"""
    t = np.zeros(n, dtype=np.uint32)
    for b, p in enumerate([1.0, 0.5, 0.1, 0.03, 0.01, 0.5, 0.5, 0.5]):
        t |= (rng.random(n) < p).astype(np.uint32) << np.uint32(b)
    return t


def _same_bytes(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


class _Case:
    """one index with tags and one batch of queries: the reference's integer scores (computed once, never changed), the
    probed rows, and the SQ8Index under test"""

    def __init__(self, X, Q, tags, ranges=None, C=None, assign=None, nprobe=1, keep_vectors=False, ids=None):
        from recommendit_amd import SQ8Index
        self.X, self.Q, self.tags = X, np.ascontiguousarray(Q), np.asarray(tags, dtype=np.uint32)
        self.m, self.s = ranges if ranges is not None else S.train_quantizer(X)
        self.c = S.encode(X, self.m, self.s)
        self.n, self.t, self.b = S.encode_queries(self.Q, self.m, self.s)
        self.Sc = S.int_scores_blas(self.n, self.c)
        self.Sc.setflags(write=False)
        self.nq, self.N = self.Sc.shape
        if C is None:
            self.nlist, self.assign, self.probes = 1, np.zeros(self.N, np.int64), np.zeros((self.nq, 1), np.int64)
        else:
            self.nlist, self.assign, self.probes = C.shape[0], np.asarray(assign), S.probed_lists(self.Q, C, nprobe)
        self.lens = np.bincount(self.assign, minlength=self.nlist).tolist()
        self.probed = FR.probed_mask(self.assign, self.probes, self.nlist)
        self.src = _flat(X, ids) if C is None else _ivf(X, C, assign, nprobe, ids)
        self.sq = SQ8Index.from_index(self.src, ranges=ranges, keep_vectors=keep_vectors)
        np.testing.assert_array_equal(self.sq.codes(), self.c)
        self.sq.set_item_tags(self.tags)

    def ok(self, preds):
        return FR.passes(self.tags, FR.words(preds, self.nq))

    def expect(self, preds, k, also=None):
        allowed = self.ok(preds) & self.probed
        return S.topk_fast(self.Sc, k, allowed if also is None else allowed & also)

    def redo(self, preds, k):
        return FR.thresholded_redo(self.Sc, k, self.assign, self.probes, self.nlist, self.ok(preds))

    def search(self, k, mode, flt):
        """((scores, rows, integer scores), filtered_stats() delta)"""
        before = self.sq.filtered_stats()
        out = self.sq.search_rows_device(torch.from_numpy(self.Q).cuda(), k, mode=mode, return_int=True, item_filter=flt)
        torch.cuda.synchronize()
        after = self.sq.filtered_stats()
        return tuple(x.cpu().numpy() for x in out), (after[0] - before[0], after[1] - before[1])

    def check(self, got, rows, sc, id_of=None):
        """ids and integer scores exact, padding as specified, float scores within 1 ulp of the f64 evaluation"""
        gs, gr = got[0], got[1]
        pad = rows < 0
        np.testing.assert_array_equal(gr, rows if id_of is None else np.where(pad, -1, id_of[np.maximum(rows, 0)]))
        assert np.isneginf(gs[pad]).all()
        if len(got) > 2:
            np.testing.assert_array_equal(got[2][~pad], sc[~pad])
            assert (got[2][pad] == -2 ** 31).all()
        ref32 = (self.b[:, None] + self.t.astype(np.float64)[:, None] * sc.astype(np.float64))[~pad].astype(np.float32)
        assert (np.abs(gs[~pad].astype(np.float64) - ref32.astype(np.float64))
                <= np.spacing(np.abs(ref32)).astype(np.float64)).all()

    def all_modes(self, preds, k, flt=None):
        """every mode against the reference; the thresholded delta against the reference's verdicts; -> dense result"""
        flt = preds if flt is None else flt
        rows, sc = self.expect(preds, k)
        res = {}
        for mode in MODES:
            res[mode], delta = self.search(k, mode, flt)
            thresholded = mode == "thresholded" or (mode == "auto" and S.auto_is_thresholded(self.nq, k, self.lens, self.probes.shape[1]))
            if thresholded:
                lo, hi = S.redo_bounds(self.redo(preds, k))
                assert delta[0] == self.nq and lo <= delta[1] <= hi, (mode, delta, lo, hi)
            else:
                assert delta == (self.nq, 0), (mode, delta)
        self.check(res["dense"], rows, sc)
        _same_bytes(res["dense"], res["thresholded"])
        _same_bytes(res["dense"], res["auto"])
        return res["dense"], rows


# ---- 1. dense, flat ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("du", [24, 100])
def test_dense_flat_per_query_predicates(du):
    """2 500 rows = 79 tiles, the last of 4 rows; 40 queries = a group of 32 and one of 8; dpad 64 and 128"""
    N, nq, k = 2500, 40, 50
    assert (N + S.TILE - 1) // S.TILE == 79 and N % S.TILE == 4 and nq % 32 == 8
    X, rng = _rows(10 + du, N, du)
    tags = _tags(rng, N)
    tags[rng.choice(N, 20, replace=False)] |= 1 << 9
    tags[N - 3:] |= 1 << 2                                   # rows of the ragged last tile pass the 10 % predicate
    menu = [(1, 0, 0), (2, 0, 0), (4, 0, 0), (8, 0, 0), (0, 0x60, 0), (6, 0x20, 0x80), (0, 0, 2)]
    preds = np.array([menu[i % len(menu)] for i in range(nq)], dtype=np.uint32)
    preds[0] = (0, 0, 0)
    preds[1] = (0, 1 << 31, 0)
    preds[2] = (1 << 9, 0, 0)
    preds[35] = (4, 0, 0)                                    # in the short last group
    case = _Case(X, rng.standard_normal((nq, du)).astype(np.float32), tags)
    n_pass = case.ok(preds).sum(axis=1)
    assert n_pass[0] == N and n_pass[1] == 0 and n_pass[2] == 20 < k and (n_pass[3:] > k).all()
    assert not S.auto_is_thresholded(nq, k, [N], 1)
    got, rows = case.all_modes(preds, k)
    assert (got[1][1] == -1).all() and (got[1][2, :20] >= 0).all() and (got[1][2, 20:] == -1).all()
    assert (rows[35] >= N - 3).any() or (case.Sc[35, N - 3:] < case.Sc[35, rows[35, k - 1]]).all()
    # the device form of the predicates and the plain search for (0, 0, 0)
    dev = torch.from_numpy(preds.view(np.int32)).cuda()
    again, _ = case.search(k, "dense", dev)
    _same_bytes(got, again)
    plain = case.sq.search_rows_device(torch.from_numpy(case.Q[:1]).cuda(), k, mode="dense", return_int=True)
    _same_bytes([x[:1] for x in got], [x.cpu().numpy() for x in plain])


# ---- 2 / 3b. IVF --------------------------------------------------------------------------------------------------------
IVF_LENS = [0, 700, 3000, 1500, 2500, 65, 1900, 2335]
IVF_NPROBE, IVF_NQ = 3, 96
ALL_FAIL = 3


def _ivf_inputs(du, nq, seed):
    N, nlist = sum(IVF_LENS), len(IVF_LENS)
    X, rng = _rows(seed, N, du)
    C = (rng.integers(-16, 17, (nlist, du)) / 8.0).astype(np.float32)
    Q = (rng.integers(-16, 17, (nq, du)) / 8.0).astype(np.float32)
    assign = np.concatenate([np.full(n, l, np.int32) for l, n in enumerate(IVF_LENS)])[rng.permutation(N)]
    tags = _tags(rng, N)
    tags[assign == ALL_FAIL] |= NONE_BIT
    return X, C, Q, assign, tags, rng


def _ivf_preds(nq, rng):
    menu = [(1, 0, NONE_BIT), (2, 0, NONE_BIT), (4, 0, NONE_BIT), (8, 0, NONE_BIT), (16, 0, NONE_BIT),
            (0, 0x60, NONE_BIT), (6, 0x20, 0x80 | NONE_BIT)]
    preds = np.array([menu[i] for i in rng.integers(0, len(menu), nq)], dtype=np.uint32)
    preds[0] = (0, 0, 0)
    return preds


@pytest.fixture(scope="module", params=[24, 100])
def ivf_case(request):
    du = request.param
    assert sum(IVF_LENS) == 12000
    X, C, Q, assign, tags, rng = _ivf_inputs(du, IVF_NQ, 20 + du)
    case = _Case(X, Q, tags, C=C, assign=assign, nprobe=IVF_NPROBE)
    assert case.lens == IVF_LENS
    assert (case.probes == 0).any() and (case.probes == ALL_FAIL).any()        # the empty list and the all-fail list are probed
    return case, _ivf_preds(IVF_NQ, rng)


def test_dense_ivf_shared_and_per_query_predicates(ivf_case):
    case, preds = ivf_case
    k = 50
    shared = (0x0F, 0, NONE_BIT)
    ok = case.ok(shared)
    assert not ok[:, case.assign == ALL_FAIL].any() and ok[:, case.assign == 2].any()
    only_fail = [q for q in range(case.nq) if set(case.probes[q]) <= {0, ALL_FAIL}]
    got, rows = case.all_modes(shared, k)
    for q in only_fail:
        assert (got[1][q] == -1).all()
    assert not np.isin(got[1], np.nonzero(case.assign == ALL_FAIL)[0]).any()
    got, rows = case.all_modes(preds, k)
    probing = np.nonzero((case.probes == ALL_FAIL).any(axis=1))[0]
    assert 0 in probing or (rows[probing[0]] >= 0).any()
    assert not np.isin(got[1][1:], np.nonzero(case.assign == ALL_FAIL)[0]).any()      # query 0 is (0, 0, 0)


def test_thresholded_ivf_at_every_pass_rate(ivf_case):
    """k = 16 (rank 9) on the IVF shape: per-query predicates from 100 % to 1 %, the verdicts are the reference's"""
    case, preds = ivf_case
    k = 16
    assert S.threshold_rank(k) == 9
    state = case.redo(preds, k)
    assert (state == S.KEPT).any()
    got, delta = case.search(k, "thresholded", preds)
    lo, hi = S.redo_bounds(state)
    assert delta[0] == case.nq and lo <= delta[1] <= hi
    case.check(got, *case.expect(preds, k))
    dense, _ = case.search(k, "dense", preds)
    _same_bytes(got, dense)


# ---- 3. thresholded, flat ------------------------------------------------------------------------------------------------
T_N, T_NQ, T_K = 20000, 64, 16


@pytest.fixture(scope="module")
def thr_case():
    """bit 0: every row; bit 1: half; bit 2: 3 % of the rows, only five of them sampled; bit 3: exactly k - 1 rows"""
    X, rng = _rows(31, T_N, 64)
    samp = S.flat_sample_rows(T_N)
    assert len(samp) == 40 * S.TILE
    tags = np.ones(T_N, dtype=np.uint32)
    tags |= (rng.random(T_N) < 0.5).astype(np.uint32) << np.uint32(1)
    few = (rng.random(T_N) < 0.03)
    few[samp] = False
    few[rng.choice(samp, 5, replace=False)] = True
    tags |= few.astype(np.uint32) << np.uint32(2)
    tags[rng.choice(T_N, T_K - 1, replace=False)] |= 1 << 3
    preds = np.array([[(1, 0, 0), (2, 0, 0), (4, 0, 0), (8, 0, 0)][q % 4] for q in range(T_NQ)], dtype=np.uint32)
    return _Case(X, rng.standard_normal((T_NQ, 64)).astype(np.float32), tags), preds, samp


def test_thresholded_flat_at_100_50_and_3_percent(thr_case):
    case, preds, samp = thr_case
    rank, cap = S.threshold_rank(T_K), S.threshold_cap(T_K, [T_N], 1)
    assert rank == 9 and cap == 4096
    ok = case.ok(preds)
    n_pass, n_samp = ok.sum(axis=1), ok[:, samp].sum(axis=1)
    assert (n_pass[0::4] == T_N).all() and (n_samp[1::4] >= rank).all() and (0.4 * T_N < n_pass[1::4]).all()
    assert (n_samp[2::4] == 5).all() and (n_samp[2::4] < rank).all() and (T_K < n_pass[2::4]).all() and (n_pass[2::4] <= cap).all()
    assert (n_pass[3::4] == T_K - 1).all()
    state = case.redo(preds, T_K)
    assert (state[2::4] == S.KEPT).all()                      # no threshold: every passing row is a candidate
    got, delta = case.search(T_K, "thresholded", preds)
    lo, hi = S.redo_bounds(state)
    assert delta[0] == T_NQ and lo <= delta[1] <= hi, (delta, lo, hi)
    rows, sc = case.expect(preds, T_K)
    case.check(got, rows, sc)
    assert (got[1][3::4, T_K - 1] == -1).all() and (got[1][3::4, :T_K - 1] >= 0).all()
    dense, d_dense = case.search(T_K, "dense", preds)
    assert d_dense == (T_NQ, 0)
    _same_bytes(got, dense)


# ---- 7. identity ---------------------------------------------------------------------------------------------------------
def _identity(case, k):
    qd = torch.from_numpy(case.Q).cuda()
    zeros = np.zeros((case.nq, 3), dtype=np.uint32)
    for mode in MODES:
        plain = [x.cpu().numpy() for x in case.sq.search_rows_device(qd, k, mode=mode, return_int=True)]
        for flt in ((0, 0, 0), zeros):
            got, _ = case.search(k, mode, flt)
            _same_bytes(got, plain)


def test_identity_predicate_returns_the_plain_searchs_bytes(thr_case, ivf_case):
    _identity(thr_case[0], 100)
    _identity(ivf_case[0], 100)


# ---- 4. steady loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("du", [24, 100])
def test_steady_loop_flat_on_the_filtered_instantiation(du):
    """tpi = 3: tile i + 1's codes and tag words are loaded under tile i's chain twice in a row; ragged last split"""
    N, nq, k = 8300, 1040, 10
    tpi, n_seq, splits = S.plan([N], [nq], 1)
    assert (tpi, n_seq, splits) == (3, [260], [87]) and n_seq[0] % tpi == 2 and N - (n_seq[0] - 1) * S.TILE == 12
    assert S.dense_chunk([N], 1) >= nq
    X, rng = _rows(40 + du, N, du)
    tags = _tags(rng, N)
    preds = np.array([[(1, 0, 0), (2, 0, 0), (4, 0, 0), (0, 0x60, 0x80), (8, 0, 0)][q % 5] for q in range(nq)], dtype=np.uint32)
    case = _Case(X, rng.standard_normal((nq, du)).astype(np.float32), tags)
    rows, sc = case.expect(preds, k)
    got, delta = case.search(k, "dense", preds)
    assert delta == (nq, 0)
    case.check(got, rows, sc)
    assert ((rows // S.TILE) % tpi == tpi - 1).any() and (rows >= (n_seq[0] - 1) * S.TILE).any()
    thr, d_thr = case.search(k, "thresholded", preds)
    lo, hi = S.redo_bounds(case.redo(preds, k))
    assert d_thr[0] == nq and lo <= d_thr[1] <= hi
    _same_bytes(got, thr)


@pytest.mark.parametrize("du", [24, 100])
def test_steady_loop_ivf_on_the_filtered_instantiation(du):
    nq, k, nprobe = 1024, 10, 6
    X, C, Q, assign, tags, rng = _ivf_inputs(du, nq, 50 + du)
    probes = S.probed_lists(Q, C, nprobe)
    per_list = np.bincount(probes.ravel(), minlength=len(IVF_LENS))
    tpi, n_seq, splits = S.plan(IVF_LENS, per_list, 1)
    assert tpi >= 3, tpi
    assert any(per_list[l] > 0 and n_seq[l] % tpi != 0 for l in range(len(IVF_LENS)))
    case = _Case(X, Q, tags, C=C, assign=assign, nprobe=nprobe)
    preds = _ivf_preds(nq, rng)
    rows, sc = case.expect(preds, k)
    got, delta = case.search(k, "dense", preds)
    assert delta == (nq, 0)
    case.check(got, rows, sc)
    thr, d_thr = case.search(k, "thresholded", preds)
    lo, hi = S.redo_bounds(case.redo(preds, k))
    assert d_thr[0] == nq and lo <= d_thr[1] <= hi
    _same_bytes(got, thr)


# ---- 5. re-do ------------------------------------------------------------------------------------------------------------
def test_redo_by_overflow_carries_each_querys_own_predicate():
    """every row identical, so all scores of a query tie: a predicate that more than 4 096 rows pass overflows the
    candidate slots.  100 queries overflow under six different predicates (two re-do chunks: 64 + 36), 50 do not"""
    N, d, nq, k = 6000, 64, 150, 10
    rng = np.random.default_rng(61)
    m = rng.uniform(-0.5, 0.5, d).astype(np.float32)
    s = np.full(d, 0.05, np.float32)
    X = np.tile((m + s * rng.integers(-100, 101, d)).astype(np.float32), (N, 1))
    tags = np.zeros(N, dtype=np.uint32)
    for b in range(6):
        tags |= (rng.random(N) < 0.8).astype(np.uint32) << np.uint32(b)
    tags |= (rng.random(N) < 0.4).astype(np.uint32) << np.uint32(6)
    preds = np.array([(1 << (q % 6), 0, 0) if q < 100 else (1 << 6, 0, 0) for q in range(nq)], dtype=np.uint32)
    case = _Case(X, rng.standard_normal((nq, d)).astype(np.float32), tags, ranges=(m, s))
    cap = S.threshold_cap(k, [N], 1)
    n_pass = case.ok(preds).sum(axis=1)
    assert cap == 4096 and (n_pass[:100] > cap).all() and (n_pass[100:] <= cap).all() and (n_pass[100:] >= k).all()
    state = case.redo(preds, k)
    assert (state[:100] == S.REDO).all() and (state[100:] == S.KEPT).all()
    rows, sc = case.expect(preds, k)
    assert len({tuple(r) for r in rows[:6]}) == 6             # the failed queries' answers differ by predicate
    got, delta = case.search(k, "thresholded", preds)
    assert delta == (nq, 100)
    case.check(got, rows, sc)
    dense, _ = case.search(k, "dense", preds)
    _same_bytes(got, dense)


def test_redo_by_deficit_under_a_real_threshold():
    """the sampled rows score far above the others: at least rank passing sampled rows give a real threshold that fewer
    than k passing rows reach, and no list overflows.  70 queries, four predicates: two re-do chunks"""
    N, d, nq, k = 16384, 64, 70, 200
    rng = np.random.default_rng(62)
    X = rng.integers(-3, 4, (N, d)).astype(np.float32)
    Q = rng.uniform(-0.01, 0.01, (nq, d)).astype(np.float32)
    Q[:, 0] = rng.uniform(0.5, 2.0, nq).astype(np.float32)
    samp = S.flat_sample_rows(N)
    X[:, 0] = rng.integers(-20, 21, N)
    X[samp, 0] = rng.integers(60, 128, len(samp))
    tags = np.zeros(N, dtype=np.uint32)
    for b in range(4):
        tags |= (rng.random(N) < 0.5).astype(np.uint32) << np.uint32(b)
    preds = np.array([(1 << (q % 4), 0, 0) for q in range(nq)], dtype=np.uint32)
    m, s = np.zeros(d, np.float32), np.ones(d, np.float32)
    case = _Case(X, Q, tags, ranges=(m, s))
    rank, cap = S.threshold_rank(k), S.threshold_cap(k, [N], 1)
    ok = case.ok(preds)
    for q in range(nq):
        ps = np.sort(case.Sc[q, samp[ok[q, samp]]])[::-1]
        assert len(ps) >= rank
        cnt = int((case.Sc[q, ok[q]] >= ps[rank - 1]).sum())
        assert rank <= cnt < k and cnt <= cap
    assert (case.redo(preds, k) == S.REDO).all()
    rows, sc = case.expect(preds, k)
    got, delta = case.search(k, "thresholded", preds)
    assert delta == (nq, nq)
    case.check(got, rows, sc)
    assert (got[1] >= 0).all()
    dense, _ = case.search(k, "dense", preds)
    _same_bytes(got, dense)


# ---- 6. ties -------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_passing_row():
    """rows r and r + 300 hold the same codes; odd rows below 300 fail, so their twin must be taken in their place"""
    N, d, nq, k = 600, 16, 8, 40
    rng = np.random.default_rng(63)
    X = rng.integers(-3, 4, (N, d)).astype(np.float32)
    X[300:] = X[:300]
    tags = np.ones(N, dtype=np.uint32)
    tags[1:300:2] = 0
    Q = rng.integers(-8, 9, (nq, d)).astype(np.float32)
    case = _Case(X, Q, tags, ranges=(np.zeros(d, np.float32), np.ones(d, np.float32)))
    assert (case.Sc[:, :300] == case.Sc[:, 300:]).all()
    rows, sc = case.expect((1, 0, 0), k)
    twin_taken = (rows >= 300) & ((rows - 300) % 2 == 1)
    both = (rows < 300) & (rows % 2 == 0)
    assert twin_taken.any() and both.any() and not ((rows < 300) & (rows % 2 == 1)).any()
    for q in range(nq):
        pos = {int(r): i for i, r in enumerate(rows[q])}
        pairs = [(pos[r], pos[r + 300]) for r in pos if r < 300 and r + 300 in pos]
        assert all(lo < hi for lo, hi in pairs)               # where both twins pass, the lower row comes first
    case.all_modes((1, 0, 0), k)


# ---- 8 / 9. refined + filtered, exclusion --------------------------------------------------------------------------------
E_N, E_D, E_NPROBE = 3000, 64, 3


@pytest.fixture(scope="module")
def ref_case():
    X = R.unit_rows(71, E_N, E_D)
    C, assign = R.ivf_layout(72, E_N, E_D)
    rng = np.random.default_rng(73)
    tags = _tags(rng, E_N)
    tags[rng.choice(E_N, 12, replace=False)] |= 1 << 9
    Q = R.dyadic_rows(74, 612, E_D)
    ids = np.arange(E_N, dtype=np.int64) + 1000
    return _Case(X, Q, tags, C=C, assign=assign, nprobe=E_NPROBE, keep_vectors=True, ids=ids), ids


def test_refined_filtered_search_and_its_certificate(ref_case):
    case, _ = ref_case
    nq, k, k_scan = 24, 10, 20
    Q = case.Q[:nq]
    preds = np.array([[(1, 0, 0), (2, 0, 0), (4, 0, 0), (0, 0x60, 0x80)][q % 4] for q in range(nq)], dtype=np.uint32)
    preds[5] = (1 << 9, 0, 0)
    preds[6] = (0, 1 << 31, 0)
    allowed = FR.passes(case.tags, preds) & case.probed[:nq]
    assert allowed[5].sum() < k_scan and allowed[6].sum() == 0 and (allowed[[0, 1, 2, 3]].sum(axis=1) > k_scan).all()
    ref = R.refine(Q, case.X, case.c, case.m, case.s, k, k_scan, allowed=allowed)
    e, a = case.sq.refine_ranges()
    re_, ra = R.ranges(case.X, case.c, case.m, case.s)
    assert e.tobytes() == re_.tobytes() and a.tobytes() == ra.tobytes()
    qd = torch.from_numpy(Q).cuda()
    outs = {}
    for mode in ("dense", "thresholded"):
        s_, r_, c_, b_ = [x.cpu().numpy() for x in case.sq.search_rows_device(qd, k, mode=mode, refine=2, return_cert=True,
                                                                                item_filter=preds)]
        outs[mode] = (s_, r_, c_, b_)
        np.testing.assert_array_equal(r_, ref["rows"])
        assert s_.tobytes() == ref["scores"].tobytes()
        np.testing.assert_array_equal(c_, ref["cert"])
        np.testing.assert_allclose(b_, ref["bound"], rtol=1e-12, atol=0)
    _same_bytes(outs["dense"], outs["thresholded"])
    s_, r_, c_, _ = outs["dense"]
    assert c_[5] == 1 and c_[6] == 1 and (r_[6] == -1).all() and c_.sum() >= nq // 2
    br, bs = R.brute_force(Q, case.X, k, allowed=allowed)
    sure = c_ == 1
    np.testing.assert_array_equal(r_[sure], br[sure])
    assert s_[sure].tobytes() == bs[sure].tobytes()
    # search_certified carries the unfinished queries' predicates into its repeats
    s2, i2, c2 = [x.cpu().numpy() for x in case.sq.search_certified(qd, k=k, start=1.0, normalized=True, item_filter=preds)]
    assert (c2 == 1).all()
    np.testing.assert_array_equal(i2, np.where(br >= 0, br + 1000, -1))


def test_exclusion_on_the_index_with_filter_and_refine(ref_case):
    from recommendit_amd import SeenItems
    from recommendit_amd.seen import plan_overfetch
    case, ids = ref_case
    nq, k = case.nq, 20
    top, _ = S.topk_fast(case.Sc, 150, case.probed)
    assert (top >= 0).all()
    counts = np.array([0] * 256 + [10] * 256 + [100] * (nq - 512))
    users, items = [], []
    seen_mask = np.zeros((nq, E_N), dtype=bool)
    for q in range(nq):
        mine = top[q, 1:2 * counts[q]:2]                      # every other one of its best rows
        seen_mask[q, mine] = True
        users += [q] * len(mine)
        items += (mine + 1000).tolist()
    store = SeenItems.from_pairs(np.array(users), np.array(items), nq)
    assert len(plan_overfetch(store.counts_of(np.arange(nq)), k, E_N, 16384)) == 3
    qd = torch.from_numpy(case.Q).cuda()
    rows, sc = case.expect((0, 0, 0), k, also=~seen_mask)
    host = list(range(nq))
    for uid in (host, torch.arange(nq, device="cuda"), None):
        s_, i_ = case.sq.batch_search_device(qd, k=k, normalized=True, exclude=store, user_ids=uid)
        case.check((s_.cpu().numpy(), i_.cpu().numpy()), rows, sc, id_of=ids)
    # with a filter: filter AND not seen
    flt = (2, 0, 0)
    rows, sc = case.expect(flt, k, also=~seen_mask)
    s_, i_ = case.sq.batch_search_device(qd, k=k, normalized=True, exclude=store, user_ids=host, item_filter=flt,
                                         mode="thresholded")
    case.check((s_.cpu().numpy(), i_.cpu().numpy()), rows, sc, id_of=ids)
    # refined: what a certificate proves of the over-fetched list holds for its unseen entries
    sub = np.r_[0:20, 256:276, 512:532]
    sub_store = SeenItems.from_pairs(np.searchsorted(sub, np.array(users)[np.isin(users, sub)]),
                                     np.array(items)[np.isin(users, sub)], len(sub))
    s_, i_, c_, _ = case.sq.batch_search_device(qd[torch.from_numpy(sub).cuda()].contiguous(), k=k, normalized=True,
                                                exclude=sub_store, user_ids=None, refine=2, return_cert=True, item_filter=flt)
    c_ = c_.cpu().numpy()
    allowed = (FR.passes(case.tags, FR.words(flt, nq)) & case.probed & ~seen_mask)[sub]
    br, bs = R.brute_force(case.Q[sub], case.X, k, allowed=allowed)
    sure = c_ == 1
    assert sure.sum() >= len(sub) // 2
    np.testing.assert_array_equal(i_.cpu().numpy()[sure], np.where(br >= 0, br + 1000, -1)[sure])
    assert s_.cpu().numpy()[sure].tobytes() == bs[sure].tobytes()
    assert case.sq.exclusion_deficit() == 0
    # the one-query host entry
    d_, got = case.sq.search(case.Q[600], k=k, exclude_items=items[-100:], item_filter=flt)
    want, _ = S.topk_fast(case.Sc[600:601], k, (FR.passes(case.tags, FR.words(flt, 1)) & case.probed[600:601]
                                                & ~np.isin(np.arange(E_N) + 1000, items[-100:])[None, :]))
    np.testing.assert_array_equal(got, want[0][want[0] >= 0] + 1000)


# ---- 10. API edges -------------------------------------------------------------------------------------------------------
def test_api_edges(tmp_path):
    from recommendit_amd import SQ8Index
    from recommendit_amd import _lib as L
    N, d, k = 700, 32, 10
    X, rng = _rows(81, N, d)
    ids = np.arange(N, dtype=np.int64) * 3 + 7
    tags = _tags(rng, N)
    src = _flat(X, ids)
    sq = SQ8Index.from_index(src)
    qd = torch.from_numpy(rng.standard_normal((4, d)).astype(np.float32)).cuda()
    assert sq.has_item_tags is False and sq.item_tags() is None and sq.filtered_stats() == (0, 0)
    with pytest.raises(ValueError, match="set_item_tags"):
        sq.batch_search_device(qd, k=k, item_filter=(1, 0, 0))
    out = torch.empty((4, k), dtype=torch.float32, device="cuda")
    rows = torch.empty((4, k), dtype=torch.int64, device="cuda")
    pred = torch.zeros(3, dtype=torch.int32, device="cuda")
    rc = L.lib().rihip_sq8_filter_search(sq.index._h, qd.data_ptr(), 4, k, 0, pred.data_ptr(), 0, out.data_ptr(), rows.data_ptr(),
                                         None, L.stream_ptr())
    assert rc != 0 and b"no tags" in L.lib().rihip_last_error()
    with pytest.raises(ValueError, match="tag words for"):
        sq.set_item_tags(tags[:-1])
    with pytest.raises(ValueError, match="is not stored"):
        sq.set_item_tags([1, 2], item_ids=[7, 8])
    assert sq.has_item_tags is False
    before = sq.stats()["device_bytes"]
    sq.set_item_tags([4, 6], item_ids=[10, 7])               # rows 1 and 0; every other row 0
    assert sq.has_item_tags and sq.item_tags()[:3].tolist() == [6, 4, 0] and sq.stats()["device_bytes"] == before + 4 * 704
    s_, i_ = sq.batch_search_device(qd, k=k, item_filter=(4, 0, 0))
    assert (np.sort(i_.cpu().numpy()[:, :2], axis=1) == [7, 10]).all() and (i_[:, 2:] == -1).all()      # set_id_map honoured
    sq.set_item_tags(tags)
    np.testing.assert_array_equal(sq.item_tags(), tags)
    with pytest.raises(ValueError, match="3-tuple"):
        sq.batch_search_device(qd, k=k, item_filter=np.zeros((5, 3), dtype=np.uint32))
    with pytest.raises(ValueError, match="return_int"):
        sq.batch_search_device(qd, k=k, refine=None, return_int=True, exclude=object(), user_ids=[0, 1, 2, 3])
    # tags are not saved; a new index of an untagged source has none; a tagged source hands them on
    sq.save(str(tmp_path / "t.sq8"))
    back = SQ8Index.load(str(tmp_path / "t.sq8"))
    assert back.has_item_tags is False and back.item_tags() is None
    assert SQ8Index.from_index(src).has_item_tags is False
    src.set_item_tags(tags)
    again = SQ8Index.from_index(src)
    assert again.has_item_tags
    np.testing.assert_array_equal(again.item_tags(), tags)
    a = sq.batch_search_device(qd, k=k, item_filter=(2, 0, 0), return_int=True)
    b = again.batch_search_device(qd, k=k, item_filter=(2, 0, 0), return_int=True)
    _same_bytes([x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b])
    assert np.isin(a[1].cpu().numpy(), ids[(tags & 2) != 0]).all()
    sq.clear_item_tags()
    assert sq.has_item_tags is False and sq.stats()["device_bytes"] == before
    with pytest.raises(ValueError, match="set_item_tags"):
        sq.search(X[0], k=k, item_filter=(1, 0, 0))


# ---- 11. serve chain -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [None, 2.0])
def test_pipeline_with_item_filter_equals_its_stages_run_by_hand(tmp_path, refine):
    from oracle import fixtures as fx
    from oracle import gbdt_np as G
    from recommendit_amd import FAISSIndex, LightGBMRanker, SQ8Index, TwoTowerModel
    from recommendit_amd import _lib as L
    from recommendit_amd.faiss_index import genre_tags
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
    untagged = SQ8Index.from_index(src)
    src.set_item_tags(genre_tags(genres))
    sq = SQ8Index.from_index(src, keep_vectors=refine is not None)
    sq.set_refine(refine)
    del src
    forest = G.random_forest_model(30, 15, 50, seed=5, names=feature_columns())
    p = tmp_path / "r.lgbm"
    p.write_text(G.write_text_model(forest))
    ranker = LightGBMRanker.load(str(p))
    store = GpuFeatureStore(nu, ni)
    ut, it = store.user.copy(), store.item.copy()
    ut[1:, :6] = rng.rand(nu, 6) * [5, 8, 1, 1, 1, 1]; ut[1:, 6:] = rng.rand(nu, 18)
    it[1:, :5] = rng.rand(ni, 5) * [5, 9, 1, 1.5, 1]; it[1:, 5:] = genres
    store.load_arrays(ut, it)
    pipe = GpuRecommendationPipeline(model, sq, ranker, store, top_k_candidates=kc, top_k_results=k)
    users = [1, 7, 120, 42, 3]
    uid = torch.tensor(users, dtype=torch.long, device="cuda")
    per_user = np.array([(1, 0, 0), (6, 0, 0), (0, 0, 1), (0, 1 << 30, 0), (0, 0, 0)], dtype=np.uint32)
    for flt in ((0b101, 0, 0b10), per_user):
        n0 = sq.filtered_stats()[0]
        ids, sc, rs = pipe.recommend_batch(users, item_filter=flt)
        assert sq.filtered_stats()[0] == n0 + len(users)
        q = model.get_user_embeddings(uid, as_tensor=True)
        r_s, cand = sq.batch_search_device(q, k=kc, normalized=True, item_filter=flt)
        Xf = build_ranking_features_device(store, uid, cand, ranker.feature_names)
        scores = ranker.predict_device(Xf)
        h_ids = torch.empty((len(users), k), dtype=torch.int64, device="cuda")
        h_top = torch.empty((len(users), k), dtype=torch.float64, device="cuda")
        h_rs = torch.empty((len(users), k), dtype=torch.float32, device="cuda")
        L.check(L.lib().rihip_rank_topk(scores.data_ptr(), cand.data_ptr(), r_s.data_ptr(), len(users), kc, k, h_ids.data_ptr(),
                                        h_top.data_ptr(), h_rs.data_ptr(), L.stream_ptr()), "rank_topk")
        torch.cuda.synchronize()
        assert torch.equal(ids, h_ids) and torch.equal(sc, h_top) and torch.equal(rs, h_rs)
        got = ids.cpu().numpy()
        w = FR.words(flt, len(users))
        passing = FR.passes(genre_tags(genres), w)
        for u in range(len(users)):
            assert passing[u, got[u][got[u] >= 0] - 1].all()
        if flt is per_user:
            assert (got[3] == -1).all() and (got[0] >= 1).any()
    # an SQ8 index without tags is still refused, by name, before anything runs
    plain = GpuRecommendationPipeline(model, untagged, ranker, store, top_k_candidates=kc, top_k_results=k)
    with pytest.raises(ValueError, match="SQ8"):
        plain.recommend_batch(users, item_filter=(1, 0, 0))
    assert untagged.filtered_stats() == (0, 0)
