"""GPU: the SQ8 index at the shapes that reach its steady tile loop, its chunked dense pass, auto -> thresholded, every
way the thresholded pass fails and is re-done, the coarse quantiser at every width, the float carrier of the integer score
around zero and around 2^23, an index built from an updated FAISSIndex, and the column ranges over 1 024 blocks.

The contract is tests/test_gpu_sq8_index.py's: rows and integer scores equal the NumPy restatement exactly, padding is
-1 / -2^31 / -inf, float scores within 1 f32 ulp of (float32)(b + t S) evaluated in f64; the modes return the same bytes.
Every test first asserts, from tests/sq8_reference.py alone, that its inputs reach the path it is about (tiles per work
item, ragged split, dense chunk, auto's rule, which queries must be re-done), and then the search_stats() deltas."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ("dense", "thresholded", "auto")


# ---- helpers (restated from tests/test_gpu_sq8_index.py) -----------------------------------------------------------------
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


def _search(sq, Q, k, mode):
    """((scores, rows, integer scores), search_stats() delta)"""
    before = sq.search_stats()
    s, r, i = sq.search_rows_device(torch.from_numpy(np.ascontiguousarray(Q)).cuda(), k, mode=mode, return_int=True)
    torch.cuda.synchronize()
    after = sq.search_stats()
    return (s.cpu().numpy(), r.cpu().numpy(), i.cpu().numpy()), (after[0] - before[0], after[1] - before[1])


def _case_rows(seed, n, du):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, du)) * rng.uniform(0.05, 2.0, du)).astype(np.float32)
    X[:, 2] = -0.75            # a constant column: s = 1, codes 0
    return X, rng


class _Expect:
    """the reference of one (queries, codes) case: top-kmax rows and scores (a smaller k is their prefix: the order is
    strict), the query transform, and per k which queries the thresholded pass must re-do.  Computed in query chunks so
    that the [nq, N] score matrix never exists whole"""

    def __init__(self, Q, c, m, s, ks, allowed=None, rules=None, chunk=256):
        """rules: {name: f(Sc, k, q0, q1) -> int8 [q1 - q0]}: which queries a thresholded pass must re-do, must keep, or
        may do either with (S.REDO / S.KEPT / S.EITHER); results in self.redo[name][k]"""
        self.n, self.t, self.b = S.encode_queries(Q, m, s)
        nq, kmax = Q.shape[0], max(ks)
        rules = rules or {}
        self.rows = np.empty((nq, kmax), dtype=np.int64)
        self.sc = np.empty((nq, kmax), dtype=np.int64)
        self.redo = {name: {k: np.empty(nq, dtype=np.int8) for k in ks} for name in rules}
        for q0 in range(0, nq, chunk):
            q1 = min(nq, q0 + chunk)
            Sc = S.int_scores_blas(self.n[q0:q1], c)
            self.rows[q0:q1], self.sc[q0:q1] = S.topk_fast(Sc, kmax, None if allowed is None else allowed[q0:q1])
            for name, rule in rules.items():
                for k in ks:
                    self.redo[name][k][q0:q1] = rule(Sc, k, q0, q1)

    def check(self, got, k):
        """ids and integer scores exact, padding as specified, float scores within 1 ulp of the f64 evaluation"""
        gs, gr, gi = got
        rows, sc = self.rows[:, :k], self.sc[:, :k]
        np.testing.assert_array_equal(gr, rows)
        pad = rows < 0
        np.testing.assert_array_equal(gi[~pad], sc[~pad])
        assert (gi[pad] == -2 ** 31).all() and np.isneginf(gs[pad]).all()
        ref64 = (self.b[:, None] + self.t.astype(np.float64)[:, None] * sc.astype(np.float64))[~pad]
        ref32 = ref64.astype(np.float32)
        assert (np.abs(gs[~pad].astype(np.float64) - ref32.astype(np.float64))
                <= np.spacing(np.abs(ref32)).astype(np.float64)).all()


def _flat_rule(Sc, k, q0, q1):
    return S.flat_thresholded_redo(Sc, k)


def _ivf_rule(assign, probes, nlist):
    return lambda Sc, k, q0, q1: S.ivf_thresholded_redo(Sc, k, assign, probes[q0:q1], nlist)


FLAT = {"flat": _flat_rule}


def _redo_within(delta, nq, state):
    """the search_stats() delta of one thresholded search against the reference's verdicts"""
    lo, hi = S.redo_bounds(state)
    assert delta[0] == nq and lo <= delta[1] <= hi, (delta, nq, lo, hi)


def _same_bytes(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ---- a. steady loop, flat ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_steady_loop_flat_three_tiles_and_a_ragged_last_split(d):
    """tpi = 3: a wave loads tile i + 1 under the chain of tile i twice in a row; the last split holds 2 tiles, the last
    tile 12 rows, the last query group 16 queries"""
    from recommendit_amd import SQ8Index
    N, nq, k = 8300, 1040, 10
    tpi, n_seq, splits = S.plan([N], [nq], 1)
    assert (tpi, n_seq, splits) == (3, [260], [87]) and n_seq[0] % tpi == 2
    assert N - (n_seq[0] - 1) * S.TILE == 12 and nq % 32 == 16
    assert S.dense_chunk([N], 1) >= nq                        # one dense pass
    X, rng = _case_rows(100 + d, N, d)
    X[4000:4400] = X[0:400]                                   # ties across tiles and splits (a split is 96 rows)
    X[8200:8300] = X[100:200]                                 # and in the short last split
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q[1030] = 0.0                                             # in the short last group: rows 0 .. 9
    m, s = S.train_quantizer(X)
    c = S.encode(X, m, s)
    ex = _Expect(Q, c, m, s, [k], rules=FLAT)
    sq = SQ8Index.from_index(_flat(X))
    got, delta = _search(sq, Q, k, "dense")
    assert delta == (0, 0)
    ex.check(got, k)
    assert (got[1][1030] == np.arange(k)).all()
    # rows of the last tile of a split and of the last, short tile are among the results
    last_of_split = (ex.rows // S.TILE) % tpi == tpi - 1
    assert last_of_split.any() and (ex.rows >= (n_seq[0] - 1) * S.TILE).any()


# ---- b. workload-shaped flat case --------------------------------------------------------------------------------------
B_N, B_NQ, B_KS = 40000, 2048, (10, 500)


@pytest.fixture(scope="module", params=[64, 128])
def workload_case(request):
    from recommendit_amd import SQ8Index
    d = request.param
    X, rng = _case_rows(200 + d, B_N, d)
    X[17990:21990] = X[0:4000]                                # ties across tiles and across the 640-row splits
    Q = rng.standard_normal((B_NQ, d)).astype(np.float32)
    Q[7] = 0.0                                                # every score 0: overflows its candidate list, re-done
    m, s = S.train_quantizer(X)
    c = S.encode(X, m, s)
    ex = _Expect(Q, c, m, s, list(B_KS), rules=FLAT)
    sq = SQ8Index.from_index(_flat(X))
    np.testing.assert_array_equal(sq.codes(), c)
    return sq, Q, ex


@pytest.mark.parametrize("k", B_KS)
def test_workload_shaped_flat_case_in_every_mode(workload_case, k):
    """sample pass tpi = 2 (tile step 16), full pass tpi = 20, the dense pass in two query chunks, auto -> thresholded"""
    sq, Q, ex = workload_case
    assert S.plan([B_N], [B_NQ], S.SAMPLE_STEP)[:2] == (2, [79])
    assert S.plan([B_N], [B_NQ], 1)[:2] == (20, [1250])
    assert 1 <= S.dense_chunk([B_N], 1) < B_NQ
    assert S.auto_is_thresholded(B_NQ, k, [B_N], 1)
    state = ex.redo["flat"][k]
    assert state[7] == S.REDO and (state == S.KEPT).sum() > B_NQ // 2
    dense, d_dense = _search(sq, Q, k, "dense")
    thr, d_thr = _search(sq, Q, k, "thresholded")
    auto, d_auto = _search(sq, Q, k, "auto")
    assert d_dense == (0, 0)
    _redo_within(d_thr, B_NQ, state)
    assert d_auto == d_thr
    ex.check(dense, k)
    _same_bytes(dense, thr)
    _same_bytes(dense, auto)
    assert (dense[1][7] == np.arange(k)).all()


# ---- c. steady loop, IVF -----------------------------------------------------------------------------------------------
C_LENS = [0, 1, 63, 64, 65, 2049, 9001, 7777, 6203, 4999, 3131, 2500, 1501, 1111, 777, 333]
C_NPROBE, C_NQ, C_KS = 4, 1024, (20, 500)


def _ivf_big_case(du):
    """16 lists; lists 0 - 4 have unit-axis centroids and the others no weight on those axes, so queries 0 and 1 probe
    short lists only.  Dyadic centroids and queries: the f32 coarse scores are exact"""
    nlist, N = len(C_LENS), sum(C_LENS)
    X, rng = _case_rows(300 + du, N, du)
    Cc = (rng.integers(-16, 17, (nlist, du)) / 8.0).astype(np.float32)
    Cc[:, :5] = 0.0
    Cc[:5] = 0.0
    Cc[np.arange(5), np.arange(5)] = 2.0
    Q = (rng.integers(-16, 17, (C_NQ, du)) / 8.0).astype(np.float32)
    Q[0] = 0.0; Q[0, [0, 1, 2, 3]] = 1.0                      # lists 0, 1, 2, 3: 128 rows
    Q[1] = 0.0; Q[1, [0, 1, 2, 4]] = 1.0                      # lists 0, 1, 2, 4: 129 rows
    assign = np.concatenate([np.full(n, l, np.int32) for l, n in enumerate(C_LENS)])[rng.permutation(N)]
    dup = np.nonzero(assign == 6)[0]
    X[dup[3000:3300]] = X[dup[0:300]]                         # ties inside one list across its splits
    return N, nlist, X, Cc, Q, assign


@pytest.mark.parametrize("du", [20, 64, 100, 128])
def test_steady_loop_ivf_at_every_coarse_and_code_width(du):
    """dk = 32 / 64 / 128 / 128 (the coarse quantiser's width), dpad = 64 / 64 / 128 / 128 (the scan's)"""
    from recommendit_amd import SQ8Index
    N, nlist, X, Cc, Q, assign = _ivf_big_case(du)
    assert np.bincount(assign, minlength=nlist).tolist() == C_LENS
    probes = S.probed_lists(Q, Cc, C_NPROBE)
    per_list = np.bincount(probes.ravel(), minlength=nlist)
    tpi, n_seq, splits = S.plan(C_LENS, per_list, 1)
    assert tpi >= 3, tpi
    assert any(per_list[l] > 0 and n_seq[l] % tpi != 0 for l in range(nlist))
    assert any(per_list[l] > 0 and splits[l] >= 3 for l in range(nlist))
    assert sorted(probes[0].tolist()) == [0, 1, 2, 3] and sorted(probes[1].tolist()) == [0, 1, 2, 4]
    assert S.dense_chunk(C_LENS, C_NPROBE) >= C_NQ
    on = np.zeros((C_NQ, nlist), dtype=bool)
    np.put_along_axis(on, probes, True, axis=1)
    allowed = on[:, assign]
    assert allowed[0].sum() == 128 and allowed[1].sum() == 129
    m, s = S.train_quantizer(X)
    c = S.encode(X, m, s)
    ex = _Expect(Q, c, m, s, list(C_KS), allowed=allowed, rules={"ivf": _ivf_rule(assign, probes, nlist)})
    sq = SQ8Index.from_index(_ivf(X, Cc, assign, C_NPROBE))
    st = sq.stats()
    assert st["bytes_per_vector"] == (64 if du <= 64 else 128) and st["n_lists"] == nlist
    np.testing.assert_array_equal(sq.codes(), c)
    for k in C_KS:
        dense, d_dense = _search(sq, Q, k, "dense")
        thr, d_thr = _search(sq, Q, k, "thresholded")
        ex.check(dense, k)
        _same_bytes(dense, thr)
        assert d_dense == (0, 0)
        _redo_within(d_thr, C_NQ, ex.redo["ivf"][k])
        assert (dense[1][0, 128:] == -1).all() and (dense[1][1, 129:] == -1).all()
        if k > 129:
            assert (dense[1][:2, :128] >= 0).all()
    # nprobe = nlist: the flat result of the same vectors, byte for byte
    sq.set_n_probe(nlist)
    flat = SQ8Index.from_index(_flat(X))
    k = 50
    assert S.auto_is_thresholded(C_NQ, k, C_LENS, nlist) and S.auto_is_thresholded(C_NQ, k, [N], 1)
    a, d_a = _search(sq, Q, k, "auto")
    b, d_b = _search(flat, Q, k, "auto")
    _same_bytes(a, b)
    every = np.tile(np.arange(nlist), (C_NQ, 1))
    exf = _Expect(Q, c, m, s, [k], rules={"flat": _flat_rule, "ivf": _ivf_rule(assign, every, nlist)})
    exf.check(a, k)
    _redo_within(d_a, C_NQ, exf.redo["ivf"][k])
    _redo_within(d_b, C_NQ, exf.redo["flat"][k])


# ---- d. thresholded failure by deficit ---------------------------------------------------------------------------------
def _column_case(N, d, nq, seed):
    """codes given directly (ranges (0, 1)); queries load column 0 with +1 and the others with at most 0.01"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, (N, d)).astype(np.float32)
    Q = rng.uniform(-0.01, 0.01, (nq, d)).astype(np.float32)
    Q[:, 0] = rng.uniform(0.5, 2.0, nq).astype(np.float32)
    return X, Q, rng


def test_thresholded_fails_by_deficit_under_a_real_threshold():
    """the 1 024 sampled rows score far above every other row, so fewer than k = 2 000 rows reach the 174th best sampled
    score and no list overflows: every query is re-done because it holds too few candidates"""
    from recommendit_amd import SQ8Index
    N, d, nq, k = 16384, 64, 70, 2000
    X, Q, rng = _column_case(N, d, nq, 401)
    samp = S.flat_sample_rows(N)
    X[:, 0] = rng.integers(-20, 21, N)
    X[samp, 0] = rng.integers(60, 128, len(samp))
    assert len(samp) == 1024 and S.threshold_rank(k) == 174 <= len(samp)
    m, s = np.zeros(d, np.float32), np.ones(d, np.float32)
    c = S.encode(X, m, s)
    np.testing.assert_array_equal(c, X.astype(np.int8))
    ex = _Expect(Q, c, m, s, [k], rules=FLAT)
    n, cap = ex.n, S.threshold_cap(k, [N], 1)
    Sc = S.int_scores_blas(n, c)
    thr = -np.partition(-Sc[:, samp], 173, axis=1)[:, 173]
    cnt = (Sc >= thr[:, None]).sum(axis=1)
    assert (cnt >= 174).all() and (cnt < k).all() and (cnt <= cap).all()        # deficit, never overflow
    assert (ex.redo["flat"][k] == S.REDO).all()
    sq = SQ8Index.from_index(_flat(X), ranges=(m, s))
    np.testing.assert_array_equal(sq.codes(), c)
    thr_got, d_thr = _search(sq, Q, k, "thresholded")
    dense, d_dense = _search(sq, Q, k, "dense")
    assert d_thr == (nq, nq) and d_dense == (0, 0)
    ex.check(thr_got, k)
    _same_bytes(thr_got, dense)
    assert (thr_got[1] >= 0).all()


def test_threshold_is_inclusive_exactly_k_rows_reach_it():
    """174 sampled rows tie at the best score H, 40 more sampled rows score H - 1, and 1 826 rows outside the sample score
    H: the threshold can only be H itself, exactly k rows have S >= H and the k-th of them equals it.  Nobody is re-done
    (S > threshold would keep none of them), and no row with H - 1 is returned"""
    from recommendit_amd import SQ8Index
    N, d, nq, k = 16384, 64, 40, 2000
    rng = np.random.default_rng(402)
    rank = S.threshold_rank(k)
    samp = S.flat_sample_rows(N)
    rest = np.setdiff1d(np.arange(N), samp)
    X = np.zeros((N, d), dtype=np.float32)
    X[:, 0] = rng.integers(-50, 51, N)
    pick = rng.choice(samp, rank + 40, replace=False)
    top = np.concatenate([pick[:rank], rng.choice(rest, k - rank, replace=False)])
    X[top, 0] = 100.0
    X[pick[rank:], 0] = 100.0
    X[pick[rank:], 1] = -1.0                                   # H - 1: column 1 of every query is n = 1
    Q = np.zeros((nq, d), dtype=np.float32)
    Q[:, 0] = rng.uniform(0.5, 2.0, nq).astype(np.float32)
    Q[:, 1] = Q[:, 0] / np.float32(S.QMAX)                     # the same f32 division as t: w_1 / t == 1
    m, s = np.zeros(d, np.float32), np.ones(d, np.float32)
    c = S.encode(X, m, s)
    ex = _Expect(Q, c, m, s, [k], rules=FLAT)
    assert (ex.n[:, 0] == S.QMAX).all() and (ex.n[:, 1] == 1).all() and (ex.n[:, 2:] == 0).all()
    Sc = S.int_scores_blas(ex.n, c)
    H = 100 * S.QMAX
    assert ((Sc == H).sum(axis=1) == k).all() and Sc.max() == H and ((Sc == H - 1).sum(axis=1) == 40).all()
    assert ((Sc[:, samp] == H).sum(axis=1) == rank).all()
    assert (ex.redo["flat"][k] == S.KEPT).all()
    sq = SQ8Index.from_index(_flat(X), ranges=(m, s))
    got, delta = _search(sq, Q, k, "thresholded")
    assert delta == (nq, 0)
    ex.check(got, k)
    np.testing.assert_array_equal(got[1], np.tile(np.sort(top), (nq, 1)))


# ---- e. no threshold: the sample is shorter than rank ------------------------------------------------------------------
@pytest.mark.parametrize("N,d,k", [(510, 64, 500), (520, 64, 500), (3000, 128, 2500), (3000, 64, 500)])
def test_thresholded_pass_with_a_sample_shorter_than_rank(N, d, k):
    """(510, 500): one sampled tile, 32 rows and 32 sample slots < rank 58.  (520, 500): two sampled tiles, 64 slots >= 58
    but only 40 real rows in them, so the rank-th best slot is an empty one.  (3000, 2500): 192 sampled rows < rank 211.
    Every probed row is then a candidate and nobody is re-done.  (3000, 500) holds 192 >= 58 sampled rows: a real
    threshold, the re-done queries are the reference's"""
    from recommendit_amd import SQ8Index
    nq = 70
    n_samp, rank = len(S.flat_sample_rows(N)), S.threshold_rank(k)
    X, rng = _case_rows(500 + N + k, N, d)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    m, s = S.train_quantizer(X)
    c = S.encode(X, m, s)
    ex = _Expect(Q, c, m, s, [k], rules=FLAT)
    if (N, k) != (3000, 500):
        assert n_samp < rank and S.threshold_cap(k, [N], 1) == N
        assert (ex.redo["flat"][k] == S.KEPT).all()
    else:
        assert n_samp == 192 >= rank == 58
    sq = SQ8Index.from_index(_flat(X))
    got, delta = _search(sq, Q, k, "thresholded")
    _redo_within(delta, nq, ex.redo["flat"][k])
    ex.check(got, k)
    dense, _ = _search(sq, Q, k, "dense")
    _same_bytes(got, dense)


# ---- f. re-do chunks and the second internal pass ----------------------------------------------------------------------
@pytest.mark.parametrize("nq", [130, 4100])
def test_every_query_redone_in_chunks_and_in_the_second_pass(nq):
    """every row identical: all 6 000 scores of a query tie and overflow its 4 096 candidate slots.  130 failed queries
    are three re-do chunks (64, 64, 2); 4 100 queries fail in two internal passes (4 096 + 4).  Integer score, t and b
    differ from query to query, so a result written to another query's row, or decoded with another pass's base,
    is wrong in all three outputs"""
    from recommendit_amd import SQ8Index
    N, d, k = 6000, 64, 10
    rng = np.random.default_rng(600 + nq)
    m = rng.uniform(-0.5, 0.5, d).astype(np.float32)
    s = np.full(d, 0.05, np.float32)
    row = (m + s * rng.integers(-100, 101, d)).astype(np.float32)
    X = np.tile(row, (N, 1))
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q[S.PASS_QUERIES:] = 16.0 * Q[S.PASS_QUERIES:] + 3.0      # the second pass: other t and b by an order of magnitude
    c = S.encode(X, m, s)
    assert (c == c[0]).all() and np.abs(c[0]).max() > 50
    ex = _Expect(Q, c, m, s, [k], rules=FLAT)
    assert S.threshold_cap(k, [N], 1) == 4096 < N and (ex.redo["flat"][k] == S.REDO).all()
    assert (nq - 1) // 64 + 1 >= 3 and (nq > S.PASS_QUERIES or nq % 64 == 2)
    assert len(np.unique(ex.sc[:, 0])) > 0.9 * nq and len(np.unique(ex.t)) > 0.9 * nq
    if nq > S.PASS_QUERIES:
        assert ex.t[S.PASS_QUERIES:].min() > 2 * ex.t[:S.PASS_QUERIES].max()
    sq = SQ8Index.from_index(_flat(X), ranges=(m, s))
    got, delta = _search(sq, Q, k, "thresholded")
    assert delta == (nq, nq)
    assert (got[1] == np.arange(k)[None, :]).all()
    ex.check(got, k)
    dense, d_dense = _search(sq, Q, k, "dense")
    assert d_dense == (0, 0)
    _same_bytes(got, dense)


# ---- g. the float carrier of the integer score -------------------------------------------------------------------------
def test_score_carrier_around_zero_and_around_two_to_the_23():
    """S travels from the select to the decode as the bits of a float: S = -1 is -0.0f, S = 0 is +0.0f, |S| < 2^23 a
    denormal.  Query 0 is (32512, -533, 32512, 32512, 1, 256, 0 ...): t = 1 and n = q exactly, so rows are chosen by hand
    to score -1, 0, +1, +-(2^23 - 1), +-2^23, +-(2^23 + 1); k = N returns them all, in strict order"""
    from recommendit_amd import SQ8Index
    d, N = 16, 48
    rng = np.random.default_rng(700)
    X = rng.integers(-2, 3, (N, d)).astype(np.float32)
    X[:, 6:] = 0.0
    special = {3: ([1, 61, 0, 0, 0, 0], -1), 40: ([0, 0, 0, 0, 0, 0], 0), 5: ([-1, -61, 0, 0, 0, 0], 1),
               33: ([0, 0, 0, 0, 0, 0], 0), 20: ([1, 61, 0, 0, 0, 0], -1), 9: ([0, 0, 0, 0, 1, 0], 1),
               11: ([127, 0, 127, 4, -1, 2], 2 ** 23 - 1), 12: ([127, 0, 127, 4, 0, 2], 2 ** 23),
               13: ([127, 0, 127, 4, 1, 2], 2 ** 23 + 1), 35: ([-127, 0, -127, -4, 1, -2], -(2 ** 23 - 1)),
               36: ([-127, 0, -127, -4, 0, -2], -(2 ** 23)), 37: ([-127, 0, -127, -4, -1, -2], -(2 ** 23 + 1))}
    for r, (v, _) in special.items():
        X[r, :6] = v
    q0 = np.zeros(d, dtype=np.float32)
    q0[:6] = [32512, -533, 32512, 32512, 1, 256]
    Q = np.stack([q0, 0.5 * q0, -q0, 3.0 * q0] + [rng.integers(-40, 41, d).astype(np.float32) for _ in range(4)])
    Q[4:, 6:] = 0.0
    nq = Q.shape[0]
    m, s = np.zeros(d, np.float32), np.ones(d, np.float32)
    c = S.encode(X, m, s)
    n, t, b = S.encode_queries(Q, m, s)
    np.testing.assert_array_equal(n[0], q0.astype(np.int32))
    np.testing.assert_array_equal(n[1], n[0])
    assert t[0] == 1.0 and t[1] == 0.5 and t[3] == 3.0 and (b == 0).all()
    Sc = S.int_scores(n, c)
    for r, (_, want) in special.items():
        assert Sc[0, r] == want and Sc[2, r] == -want
    assert np.nonzero(np.abs(Sc[0]) <= 1)[0].tolist() == [3, 5, 9, 20, 33, 40]
    assert {-1, 0, 1} <= set(Sc[0].tolist()) and (np.abs(Sc[0]) < 2 ** 23).sum() > 20       # mostly denormal carriers
    ex = _Expect(Q, c, m, s, [N], rules=FLAT)
    sq = SQ8Index.from_index(_flat(X), ranges=(m, s))
    np.testing.assert_array_equal(sq.codes(), c)
    results = {}
    for mode in MODES:
        got, delta = _search(sq, Q, N, mode)
        results[mode] = got
        if mode == "thresholded":
            _redo_within(delta, nq, ex.redo["flat"][N])
        else:
            assert delta == (0, 0)
        ex.check(got, N)
        gs, gr, gi = got
        assert (np.sort(gr, axis=1) == np.arange(N)[None, :]).all()
        # strict order: S descending, ties to the lower row
        assert ((gi[:, :-1] > gi[:, 1:]) | ((gi[:, :-1] == gi[:, 1:]) & (gr[:, :-1] < gr[:, 1:]))).all()
        for q in range(4):
            pos = {int(r): i for i, r in enumerate(gr[q])}
            sgn = -1 if q == 2 else 1
            plus, zero, minus = ([5, 9], [33, 40], [3, 20]) if sgn > 0 else ([3, 20], [33, 40], [5, 9])
            assert pos[plus[0]] < pos[plus[1]] < pos[zero[0]] < pos[zero[1]] < pos[minus[0]] < pos[minus[1]]
            assert pos[minus[0]] == pos[zero[1]] + 1 and pos[zero[0]] == pos[plus[1]] + 1      # nothing between -1, 0, 1
            assert gi[q, pos[minus[0]]] == -1 and gi[q, pos[zero[0]]] == 0 and gi[q, pos[plus[0]]] == 1
            # b = 0: the score of S = -1 is -t, not b
            assert gs[q, pos[minus[0]]] == -t[q] and gs[q, pos[plus[0]]] == t[q] and gs[q, pos[zero[0]]] == 0.0
        big = {int(r): int(v) for r, v in zip(gr[0], gi[0])}
        assert [big[r] for r in (11, 12, 13, 35, 36, 37)] == [2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, -(2 ** 23 - 1), -(2 ** 23),
                                                             -(2 ** 23 + 1)]
        assert gr[0, :3].tolist() == [13, 12, 11] and gr[0, -3:].tolist() == [35, 36, 37]
    assert not S.auto_is_thresholded(nq, N, [N], 1)
    _same_bytes(results["dense"], results["thresholded"])
    _same_bytes(results["dense"], results["auto"])


# ---- h. built from an updated index ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ivf", "flat"])
def test_built_from_an_updated_index_and_saved(tmp_path, kind):
    """remove 300, add 400, upsert 200 stored + 150 new ids; the SQ8 index of the updated FAISSIndex equals, file bytes
    included, the SQ8 index of a FAISSIndex built from scratch on the final catalogue with the same centroids and lists.
    The IVF case is d = 128 (dpad 128), the flat one d = 64; both are saved and loaded back"""
    from recommendit_amd import SQ8Index
    ivf = kind == "ivf"
    d, N0, nlist, nprobe, k, nq = (128 if ivf else 64), 5000, 12, 3, 60, 64
    Xall, rng = _case_rows(800 + d, N0 + 1000, d)
    X0, pool = Xall[:N0], Xall[N0:]
    ids0 = np.arange(1000, 1000 + N0, dtype=np.int64)
    pool_ids = np.arange(500000, 500000 + len(pool), dtype=np.int64)
    Cc = (rng.integers(-16, 17, (nlist, d)) / 8.0).astype(np.float32)
    Q = (rng.integers(-16, 17, (nq, d)) / 8.0).astype(np.float32)
    a0 = rng.integers(0, nlist, N0).astype(np.int32)
    A = _ivf(X0, Cc, a0, nprobe, ids0) if ivf else _flat(X0, ids0)

    def lists_of(E):
        if not ivf:
            return np.zeros(len(E), np.int32)
        return A.assign_lists(torch.from_numpy(np.ascontiguousarray(E)).cuda()).cpu().numpy().astype(np.int32)

    mX, mid, ml = X0.copy(), ids0.copy(), (a0.copy() if ivf else np.zeros(N0, np.int32))

    def drop(ids):
        nonlocal mX, mid, ml
        gone = np.isin(mid, ids)
        mX, mid, ml = mX[~gone], mid[~gone], ml[~gone]
        return int(gone.sum())

    def add(E, ids):
        nonlocal mX, mid, ml
        mX, mid, ml = np.concatenate([mX, E]), np.concatenate([mid, ids]), np.concatenate([ml, lists_of(E)])

    rm = rng.choice(ids0, 300, replace=False)
    assert A.remove_items(rm) == 300 == drop(rm)
    assert A.add_items_device(torch.from_numpy(pool[:400]).cuda(), pool_ids[:400]) == 400
    add(pool[:400], pool_ids[:400])
    stored = rng.choice(mid, 200, replace=False)
    fresh = pool_ids[400:550]
    E = (3.0 * pool[400:750]).astype(np.float32)              # the host entry normalises its rows
    En = np.ascontiguousarray(E / np.maximum(np.linalg.norm(E, axis=1, keepdims=True), 1e-8), dtype=np.float32)
    up_ids = np.concatenate([stored[:100], fresh, stored[100:]])
    assert A.update_items(E, up_ids) == (200, 150)
    assert drop(stored) == 200
    add(En, up_ids)
    np.testing.assert_array_equal(A.item_ids, mid)
    B = _ivf(mX, Cc, ml, nprobe, mid) if ivf else _flat(mX, mid)
    sqA, sqB = SQ8Index.from_index(A), SQ8Index.from_index(B)
    m, s = S.train_quantizer(mX)
    c = S.encode(mX, m, s)
    for sq in (sqA, sqB):
        gm, gs_ = sq.quantizer()
        np.testing.assert_array_equal(gm, m)
        np.testing.assert_array_equal(gs_, s)
        np.testing.assert_array_equal(sq.codes(), c)
        np.testing.assert_array_equal(sq.item_ids, mid)
    # the search against the reference (rows) and A against B (item ids), in both emissions
    allowed = None
    if ivf:
        probes = S.probed_lists(Q, Cc, nprobe)
        on = np.zeros((nq, nlist), dtype=bool)
        np.put_along_axis(on, probes, True, axis=1)
        allowed = on[:, ml]
    ex = _Expect(Q, c, m, s, [k], allowed=allowed)
    qd = torch.from_numpy(Q).cuda()
    res = {}
    for name, sq in (("A", sqA), ("B", sqB)):
        for mode in ("dense", "thresholded"):
            got, _ = _search(sq, Q, k, mode)
            ex.check(got, k)
            out = [x.cpu().numpy() for x in sq.batch_search_device(qd, k=k, normalized=True, mode=mode, return_int=True)]
            np.testing.assert_array_equal(out[1], mid[got[1]])
            np.testing.assert_array_equal(out[2], got[2])
            assert out[0].tobytes() == got[0].tobytes()
            res[name, mode] = out
    for mode in ("dense", "thresholded"):
        _same_bytes(res["A", mode], res["B", mode])
    _same_bytes(res["A", "dense"], res["A", "thresholded"])
    # files: updated == from scratch; the loaded index is the saved one
    pa, pb = tmp_path / "a.sq8", tmp_path / "b.sq8"
    sqA.save(str(pa))
    sqB.save(str(pb))
    raw = pa.read_bytes()
    assert raw == pb.read_bytes()
    hdr = np.frombuffer(raw[8:72], dtype=np.int64)
    assert hdr[1] == d and hdr[2] == d and hdr[3] == (128 if ivf else 64) and hdr[4] == len(mid)
    assert hdr[6] == (nlist if ivf else 1) and hdr[7] == (nprobe if ivf else 1) == sqA.n_probe
    back = SQ8Index.load(str(pa))
    assert back.n_probe == sqA.n_probe and back.index.ntotal == len(mid)
    np.testing.assert_array_equal(back.codes(), c)
    for x, y in zip(back.quantizer(), (m, s)):
        np.testing.assert_array_equal(x, y)
    for mode in ("dense", "thresholded"):
        out = [x.cpu().numpy() for x in back.batch_search_device(qd, k=k, normalized=True, mode=mode, return_int=True)]
        _same_bytes(out, res["A", mode])
    p2 = tmp_path / "again.sq8"
    back.save(str(p2))
    assert p2.read_bytes() == raw


# ---- i. quantiser ranges across many blocks ----------------------------------------------------------------------------
def test_column_ranges_over_1024_blocks_with_trailing_empty_blocks():
    """262 400 rows: the range kernel runs 1 024 blocks of 257 rows; blocks 1 022 and 1 023 own no rows, block 1 021 three.
    The minimum and maximum of every column sit in different blocks, the first, the last and the 3-row one among them"""
    from recommendit_amd import SQ8Index
    du, N = 16, 262400
    nb = min(1024, (N + 255) // 256)
    per = (N + nb - 1) // nb
    assert N == 1025 * 256 and nb == 1024 and per == 257
    assert 1021 * per < N <= 1022 * per and N - 1021 * per == 3
    rng = np.random.default_rng(900)
    X = rng.uniform(-1.0, 1.0, (N, du)).astype(np.float32)
    lo_rows = np.array([0, N - 1, 1021 * per, 1020 * per + 256] + [(37 * j + 5) * per + 11 * j for j in range(4, du)])
    hi_rows = np.array([N - 2, 256, 1, 512 * per] + [(61 * j + 17) * per + 200 - j for j in range(4, du)])
    assert lo_rows.max() < N and hi_rows.max() < N and ((lo_rows // per) != (hi_rows // per)).all()
    assert {0, 1020, 1021} <= set((np.concatenate([lo_rows, hi_rows]) // per).tolist())
    X[lo_rows, np.arange(du)] = -(2.0 + np.arange(du, dtype=np.float32) / 8)
    X[hi_rows, np.arange(du)] = 3.0 + np.arange(du, dtype=np.float32) / 4
    m, s = S.train_quantizer(X)
    assert (X.min(axis=0) == X[lo_rows, np.arange(du)]).all() and (X.max(axis=0) == X[hi_rows, np.arange(du)]).all()
    sq = SQ8Index.from_index(_flat(X))
    gm, gs = sq.quantizer()
    np.testing.assert_array_equal(gm, m)
    np.testing.assert_array_equal(gs, s)
    sample = np.unique(np.concatenate([lo_rows, hi_rows, rng.integers(0, N, 4096 - 2 * du), [N - 1, N - 2, N - 3]]))
    codes = sq.codes()
    assert codes.shape == (N, du)
    np.testing.assert_array_equal(codes[sample], S.encode(X[sample], m, s))
    assert (codes[lo_rows, np.arange(du)] == -127).all() and (codes[hi_rows, np.arange(du)] == 127).all()
