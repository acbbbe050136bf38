"""GPU: every path of the inner-product index search (csrc/topk.hip search_pass) at the shapes that reach it.

Every case first asserts, from tests/search_reference.py alone, that its inputs reach the path it is about ("inputs no
longer reach the path"), runs the search, asserts the search_stats() delta and the number of queries re-done against the
reference's verdicts, and compares scores and rows with the exact reference bit for bit, padding included.  All inputs
are integers in [-8, 8] held in float32: every inner product is exact in bf16 operands, in f32 and in any order.

Level data: a corpus column holds a designed level per row and a query is a multiple of that column's unit vector, so
its score against a row is level * multiple: the sampled rows, the threshold and the survivors are known by construction.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
MISS = "inputs no longer reach the path"
WIDTHS = (32, 64, 128)          # kernel widths
NARROW = {32: 20, 64: 33, 128: 100}   # a caller width below each kernel width


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _flat(X, two=True, ids=None):
    from recommendit_amd import FAISSIndex
    idx = FAISSIndex(embed_dim=X.shape[1], exact=True)
    idx.build_from_device(_dev(X), np.arange(X.shape[0]) if ids is None else ids)
    _set_two(idx, two)
    return idx


def _set_two(idx, two):
    from recommendit_amd import _lib
    _lib.check(_lib.lib().rihip_ip_index_set_two_precision(idx.index._h, 1 if two else 0))


def _ivf(X, C, assign, nprobe):
    from recommendit_amd import FAISSIndex
    idx = FAISSIndex(embed_dim=X.shape[1], n_lists=C.shape[0], n_probe=nprobe)
    idx.build_from_device(_dev(X), np.arange(X.shape[0]), centroids=C, assign=np.asarray(assign, dtype=np.int32))
    return idx


def _search(idx, Q, k, ids=False):
    """(scores, rows, search_stats() delta)"""
    before = idx.search_stats()
    s, r = idx._search_device(_dev(Q), k, item_ids=ids)
    torch.cuda.synchronize()
    after = idx.search_stats()
    return s.cpu().numpy(), r.cpu().numpy(), {n: after[n] - before[n] for n in after}


def _same(got_s, got_r, exp_s, exp_r):
    """bitwise: rows, scores (as their int32 patterns), -1 / -inf padding"""
    assert got_r.dtype == np.int64 and got_s.dtype == np.float32
    np.testing.assert_array_equal(got_r, exp_r)
    np.testing.assert_array_equal(got_s.view(np.int32), np.ascontiguousarray(exp_s, dtype=np.float32).view(np.int32))


def _check_stats(delta, exp, states=None, ivf=False):
    """delta against R.expected_stats(); states: the verdict arrays of the internal passes, one per pass (None: a search
    without a thresholded pass re-does nobody).  Re-done queries and re-do chunks within the reference's bounds (exact
    when no verdict is EITHER)"""
    exp = dict(exp)
    lo = hi = c_lo = c_hi = small = 0
    ch = R.IVF_REDO_CHUNK if ivf else R.FLAT_REDO_CHUNK
    for st in states or []:
        l, h = R.redo_bounds(st)
        lo, hi, c_lo, c_hi = lo + l, hi + h, c_lo + -(-l // ch), c_hi + -(-h // ch)
        small += R.redo_stats([l], ivf)[2]
    assert lo <= delta["redone"] <= hi, (delta, lo, hi)
    assert c_lo <= delta["redo_chunks"] <= c_hi, (delta, c_lo, c_hi)
    if lo == hi:
        exp["prepare_small"] += small
    else:
        exp.pop("prepare_small")
    for name in ("redone", "redo_chunks"):
        exp.pop(name)
    assert {n: delta[n] for n in exp} == exp, (delta, exp)


def _rand_ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def _du_cases():
    return [(d, d) for d in WIDTHS] + [(d, NARROW[d]) for d in WIDTHS]


# ======================================================================================================================
# flat dense
# ======================================================================================================================
DENSE_NQ = 130
# N -> tiles per split at 130 queries (two query blocks: 256 splits; one block would have 512).  8 212 is the smallest N
# whose splits hold 2 tiles with a 1-tile last split and empty splits behind it
DENSE_N = {500: 1, 8212: 2, 16416: 3, 39990: 5, 65536: 8}


@pytest.fixture(scope="module")
def dense_case():
    """per (N, du): (index, X, Q, expected scores and rows at k = 70) -- built on first use, shared read-only"""
    made = {}

    def get(N, du, nq=DENSE_NQ):
        if (N, du, nq) not in made:
            rng = np.random.default_rng(1000 + N + du)
            X = _rand_ints(rng, (N, du))
            Q = _rand_ints(rng, (nq, du))
            X[N // 2:N // 2 + 40] = X[0:40]                 # ties across splits: the lower row first
            Q[nq - 1] = 0.0                                 # in the second block's 2 queries: all scores tie, rows 0 ..
            per = R.plan(N, R.kernel_width(du), nq, 70)["scan"]["per"]
            sgn = lambda v: np.where(v < 0, -8.0, 8.0).astype(np.float32)      # noqa: E731
            X[N - 3] = sgn(Q[0])                            # query 0's best row: in the last tile
            X[per * R.TRS - 5] = sgn(Q[1])                  # query 1's best row: in the last tile of split 0
            kk = 70
            made[(N, du, nq)] = (_flat(X), X, Q) + R.topk_chunked(Q, X, kk)
        return made[(N, du, nq)]
    return get


@pytest.mark.parametrize("N,d,du", [(N, d, d) for N in sorted(DENSE_N) for d in WIDTHS]
                         + [(N, d, NARROW[d]) for N in (500, 16416) for d in WIDTHS])
def test_flat_dense_tiles_per_split(dense_case, N, d, du):
    """scan_kernel's three-buffer pipeline at 1, 2, 3, 5 and 8 tiles per split: empty trailing splits, a short last
    split, a short last tile; two query blocks, the second with 2 queries"""
    nq, k = DENSE_NQ, 70
    p = R.plan(N, d, nq, k)
    sc = p["scan"]
    assert p["route"] == "flat_dense" and sc["per"] == DENSE_N[N] and R.kernel_width(du) == d, MISS
    assert -(-nq // R.QB) == 2 and nq % R.QB == 2, MISS
    if N == 8212:
        assert sc["used"] < sc["nsplit"] and sc["last_split_tiles"] == 1 and sc["last_tile_rows"] == 20, MISS
    if N == 16416:
        assert sc["used"] == 171 < sc["nsplit"] == 256, MISS
    if N == 39990:
        assert sc["last_tile_rows"] == 22, MISS
    if N == 65536:
        assert N == 4 * R.SAMPLE, MISS
    idx, X, Q, es, er = dense_case(N, du)
    # rows of the last tile of a split and of the last (short) tile are among the expected results
    tile = er // R.TRS
    assert ((tile % sc["per"] == sc["per"] - 1) & (er >= 0)).any() and (er >= (sc["tiles"] - 1) * R.TRS).any(), MISS
    gs, gr, delta = _search(idx, Q, k)
    _check_stats(delta, R.expected_stats(N, d, nq, k))
    assert delta["flat_dense"] == 1 and delta["thr_queries"] == 0
    _same(gs, gr, es[:, :k], er[:, :k])
    assert (gr[nq - 1] == np.arange(k)).all()


@pytest.mark.parametrize("N,nq,lds", [(16320, 130, True), (16321, 130, False), (500, 513, False), (500, 512, True)])
def test_flat_dense_finalize_selects_in_lds_or_in_global_memory(dense_case, N, nq, lds):
    """launch_finalize: n <= 2 NCU workgroups and P + cap <= K_MAX key slots, both sides of both conditions"""
    d, k = 64, 64
    p = R.plan(N, d, nq, k)
    assert p["route"] == "flat_dense" and p["fin_lds"] is lds, MISS
    assert 64 + 16320 == R.K_MAX and 2 * R.RIHIP_NCU == 512, MISS
    idx, X, Q, es, er = dense_case(N, d, nq)
    gs, gr, delta = _search(idx, Q, k)
    _check_stats(delta, R.expected_stats(N, d, nq, k))
    _same(gs, gr, es[:, :k], er[:, :k])


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("N,k", [(500, 1), (500, 64), (500, 65), (500, 500), (500, 507), (20000, 16384)])
def test_flat_dense_k_edges(N, k, d):
    """k = 1, the sort buffer's 64 / 65 boundary, k = N, k > N (padded with -inf / -1), k = K_MAX"""
    nq = 5
    p = R.plan(N, d, nq, k)
    assert p["route"] == "flat_dense" and k <= R.K_MAX, MISS
    rng = np.random.default_rng(1100 + N + k + d)
    X, Q = _rand_ints(rng, (N, d)), _rand_ints(rng, (nq, d))
    es, er = R.topk(R.int_scores(Q, X), k)
    if k > N:
        assert (er[:, N:] == -1).all() and np.isneginf(es[:, N:]).all()
    gs, gr, delta = _search(_flat(X), Q, k)
    _check_stats(delta, R.expected_stats(N, d, nq, k))
    _same(gs, gr, es, er)


@pytest.mark.parametrize("d", WIDTHS)
def test_flat_dense_every_candidate_carries_one_score(d):
    """3 000 rows score exactly the same: the radix select runs all 8 passes (the keys differ in the row bits only), the
    k-th key is found among equal scores and the result is rows 0 .. k-1 of the tied set; 10 rows score strictly more
    and come first"""
    N, nq, k = 3000, 7, 100
    assert R.plan(N, d, nq, k)["route"] == "flat_dense", MISS
    X = np.zeros((N, d), dtype=np.float32)
    X[:, 0] = 3.0
    better = np.array([2999, 2500, 2000, 1500, 1000, 999, 64, 63, 32, 31])
    X[better, 0] = 4.0
    Q = np.zeros((nq, d), dtype=np.float32)
    Q[:, 0] = 1.0 + np.arange(nq)
    es, er = R.topk(R.int_scores(Q, X), k)
    tied = np.setdiff1d(np.arange(N), better)[:k - 10]
    assert (er[0] == np.concatenate([np.sort(better), tied])).all()
    gs, gr, delta = _search(_flat(X), Q, k)
    _check_stats(delta, R.expected_stats(N, d, nq, k))
    _same(gs, gr, es, er)


# ======================================================================================================================
# flat thresholded: level data
# ======================================================================================================================
FT_N = 66000
BACKGROUND_TOP = 1      # levels of the undesigned rows: -8 .. 1


def _spread(pool, n):
    """n entries of pool, evenly spread, the last one included"""
    assert n <= len(pool)
    return pool[np.unique(np.linspace(0, len(pool) - 1, n).round().astype(np.int64))] if n else pool[:0]


def _design(rng, p, kind):
    """int levels [N] of one design column for the pass plan p.  Every design keeps levels 7 / 8 for the rows that must
    be returned, 5 for the rows that set the threshold and at most 3 below"""
    N, k, stride, rank, cap = p["N"], p["k"], p["stride"], p["rank"], p["cap"]
    lev = rng.integers(-8, BACKGROUND_TOP + 1, N)
    rows = np.arange(N)
    sampled, unsampled = rows[rows % stride == 0][:p["S"]], rows[rows % stride != 0]
    if kind == "zeros":                                    # a column no row has weight on: it adds to |q| only
        return np.zeros(N, dtype=np.int64)
    if kind in ("kept", "seg_over", "many_survivors", "stream_overflow", "gap_one"):
        top = _spread(unsampled, k)
        assert len(top) == k and top[-1] == unsampled[-1]
        n_l1 = rank + 11
        if kind == "many_survivors":
            n_l1 = R.REFINE_LDS_SLOTS + 300 - k
        if kind == "stream_overflow":
            lev[_spread(rows, 1000)] = 3
            n_l1 = rank + 10
            # 48 consecutive sampled rows of one sample stage: 24 in each of its two streams (a stream takes every
            # other run of 4 rows), and with the stage's other survivors still within one filter segment
            stage = sampled[64 * 5:64 * 5 + 48]
            l1 = np.unique(np.concatenate([stage, _spread(sampled, n_l1 - 48)]))
        else:
            l1 = _spread(sampled, n_l1)
        lev[l1] = 5
        if kind == "seg_over":                             # 128 consecutive rows of one filter split reach the threshold
            per = p["filter"]["per"] * R.TRB
            assert per >= 128 > p["seg_cap"]
            lev[7 * per:7 * per + 128] = 5
        lev[top[0::2]] = 8 if kind != "gap_one" else 6     # gap_one: the results one level above the threshold
        lev[top[1::2]] = 7 if kind != "gap_one" else 6
    elif kind == "over_cap":                               # more than cap rows tie at the top
        lev[_spread(rows, cap + 1)] = 8
    elif kind == "top_is_threshold":                       # enough candidates, all of them AT the threshold
        n = max(k, rank + 1)
        lev[np.concatenate([_spread(sampled, rank + 1), _spread(unsampled, n - (rank + 1))])] = 8
    else:
        raise ValueError(kind)
    return lev


class _LevelCorpus:
    """One corpus per caller width; design columns are added before the index is built."""

    def __init__(self, du, seed):
        self.du, self.rng = du, np.random.default_rng(seed)
        self.X = _rand_ints(self.rng, (FT_N, du))
        self.levels, self.col = [], {}
        self.idx = None

    def add(self, name, p, kind):
        assert self.idx is None
        self.col[name] = len(self.levels)
        self.levels.append(_design(self.rng, p, kind))

    def build(self):
        L = np.stack(self.levels, axis=1)
        assert L.shape[1] <= self.du and np.abs(L).max() <= 8
        self.X[:, :L.shape[1]] = L
        self.L = L.T.astype(np.int64)                      # [designs, N]
        R.check_exact_inputs(self.X)
        self.eps = R.eps_scale(self.X)
        self.idx = _flat(self.X)
        self._top = {}

    def queries(self, names, mult, ballast=None):
        """ballast bool [nq]: those queries also put 8 on each of the three all-zero columns (|q| grows, no score does)"""
        cols = np.array([self.col[n] for n in names])
        Q = np.zeros((len(names), self.du), dtype=np.float32)
        Q[np.arange(len(names)), cols] = mult
        if ballast is not None:
            for z in ("zero0", "zero1", "zero2"):
                Q[np.asarray(ballast), self.col[z]] = 8.0
        return Q, cols

    def expect(self, cols, mult, k):
        if k not in self._top:
            self._top[k] = R.topk(self.L, k)
        s, r = self._top[k]
        with np.errstate(invalid="ignore"):
            return (s[cols] * np.asarray(mult, dtype=np.float32)[:, None]).astype(np.float32), r[cols]

    def verdicts(self, cols, mult, p, ballast=None):
        extra = np.zeros(len(cols), dtype=np.int64) if ballast is None else 192 * np.asarray(ballast, dtype=np.int64)
        pairs, inv = np.unique(np.stack([cols, mult, extra], axis=1), axis=0, return_inverse=True)
        Sc = self.L[pairs[:, 0]] * pairs[:, 1][:, None]
        qnorm = np.sqrt((pairs[:, 1] ** 2 + pairs[:, 2]).astype(np.float64))
        return R.flat_verdicts(Sc, p, qnorm=qnorm, eps=self.eps, inv=inv.ravel())


# (name of the design column, k, queries of the pass it is planned for, two-precision, kind)
FT_DESIGNS = [
    ("i_kept", 500, 9, True, "kept"),
    ("ii_unfused", 2049, 9, True, "kept"),
    ("iii_dense_unfused", 4000, 9, True, "kept"),
    ("iv_dense_fused", 2000, 257, True, "kept"),
    ("v_many", 500, 9, True, "many_survivors"),
    ("vi_seg", 500, 9, True, "seg_over"),
    ("vii_cap", 500, 9, True, "over_cap"),
    ("viii_proof", 500, 9, True, "top_is_threshold"),
    ("ix_stream", 500, 9, True, "stream_overflow"),
    ("f32_kept", 500, 20, False, "kept"),
    ("f32_kept10", 10, 20, False, "kept"),
    ("f32_incl", 500, 20, False, "top_is_threshold"),
    ("f32_incl10", 10, 20, False, "top_is_threshold"),
    ("kept10", 10, 9, True, "kept"),
    ("cap10", 10, 9, True, "over_cap"),
    ("iv_cap", 2000, 265, True, "over_cap"),
    ("proof_gap", 500, 9, True, "gap_one"),
    ("zero0", 500, 9, True, "zeros"), ("zero1", 500, 9, True, "zeros"), ("zero2", 500, 9, True, "zeros"),
]


@pytest.fixture(scope="module")
def level_corpus():
    made = {}

    def get(du):
        if du not in made:
            c = _LevelCorpus(du, 2000 + du)
            d = R.kernel_width(du)
            for name, k, nq, two, kind in FT_DESIGNS:
                c.add(name, R.plan(FT_N, d, nq, k, two_precision=two), kind)
            c.build()
            made[du] = c
        return made[du]
    return get


def _run_levels(c, names, k, two, want_route, want=None, mult=None, ballast=None, **plan_checks):
    """search the level corpus with one query per entry of names; returns (delta, verdicts, results)"""
    nq, d = len(names), R.kernel_width(c.du)
    mult = 1 + np.arange(nq) % 8 if mult is None else np.asarray(mult)
    Q, cols = c.queries(names, mult, ballast)
    p = R.plan(FT_N, d, nq, k, two_precision=two)
    assert p["route"] == want_route, MISS
    for key, val in plan_checks.items():
        assert p[key] == val, (MISS, key, p[key])
    st = c.verdicts(cols, mult, p, ballast)
    if want is not None:
        assert (st == np.asarray(want)).all(), (MISS, st)
    es, er = c.expect(cols, mult, k)
    _set_two(c.idx, two)
    try:
        gs, gr, delta = _search(c.idx, Q, k)
    finally:
        _set_two(c.idx, True)                              # the corpus is shared: it stays two-precision
    _check_stats(delta, R.expected_stats(FT_N, d, nq, k, two_precision=two), [st])
    _same(gs, gr, es, er)
    return delta, st, p


FT_WIDTHS = [(d, d) for d in WIDTHS] + [(32, 20)]


@pytest.mark.parametrize("d,du", FT_WIDTHS)
def test_two_precision_top_t_sample_fused_refine(level_corpus, d, du):
    """(i) k = 500, 9 queries: register top-T sample, fused refine in LDS; (x) the corpus is no multiple of 64 and the
    last expected row lies in the 16-row last stage"""
    c = level_corpus(du)
    delta, st, p = _run_levels(c, ["i_kept"] * 9, 500, True, "flat_fused", want=[R.KEPT] * 9, sample_top=True,
                               stride=2, seg_cap=64)
    assert FT_N % R.TRB == 16 and c.expect(np.array([c.col["i_kept"]]), [1], 500)[1][0, -1] == FT_N - 1, MISS
    assert delta["flat_fused"] == 1 and delta["sample_top"] == 1 and delta["redone"] == 0


@pytest.mark.parametrize("d,du", FT_WIDTHS)
def test_two_precision_top_t_sample_unfused(level_corpus, d, du):
    """(ii) k = 2049: compact_segments -> rerank -> finalize behind a register top-T sample"""
    delta, st, p = _run_levels(level_corpus(du), ["ii_unfused"] * 9, 2049, True, "flat_unfused", want=[R.KEPT] * 9,
                               sample_top=True, fin_lds=False, fin_kth_lds=True)
    assert delta["flat_unfused"] == 1 and delta["sample_top"] == 1 and delta["redone"] == 0


@pytest.mark.parametrize("d,du", FT_WIDTHS)
def test_two_precision_dense_sample_unfused(level_corpus, d, du):
    """(iii) k = 4000: the dense bf16 sample (rank too large for the streams), unfused"""
    delta, st, p = _run_levels(level_corpus(du), ["iii_dense_unfused"] * 9, 4000, True, "flat_unfused",
                               want=[R.KEPT] * 9, sample_top=False, cap=16384)
    assert delta["flat_unfused"] == 1 and delta["sample_top"] == 0 and delta["redone"] == 0


@pytest.mark.parametrize("d,du", FT_WIDTHS)
def test_two_precision_dense_sample_fused_refine(level_corpus, d, du):
    """(iv) k = 2000 over two query blocks: the streams halve, so the sample is dense, and k <= 2048 keeps the fused
    refine -- with 2000 + rank + 11 > 2048 survivors in the global scratch list.  A full block of queries with that many
    common survivors overruns the filter's wave queues (64 queries x 3.6 survivors per stage against 192 entries), so
    the first block holds 256 queries that are re-done for sure (more than cap rows tie at their top) and the 9 queries
    of the second block are the ones kept for sure: 256 re-done, in 32 chunks"""
    names = ["iv_cap"] * 256 + ["iv_dense_fused"] * 9
    want = [R.REDO] * 256 + [R.KEPT] * 9
    delta, st, p = _run_levels(level_corpus(du), names, 2000, True, "flat_fused", want=want, sample_top=False, fused=True)
    assert 2000 + p["rank"] + 11 > R.REFINE_LDS_SLOTS and 2000 + p["rank"] + 11 <= p["cap"], MISS
    assert delta["flat_fused"] == 1 and delta["sample_top"] == 0 and delta["redone"] == 256 and delta["redo_chunks"] == 32


@pytest.mark.parametrize("d,du", FT_WIDTHS)
def test_refine_in_global_scratch(level_corpus, d, du):
    """(v) 2 348 survivors, none of the segments over seg_cap: refine_kernel works in the global scratch slice"""
    c = level_corpus(du)
    delta, st, p = _run_levels(c, ["v_many"] * 9, 500, True, "flat_fused", want=[R.KEPT] * 9)
    n_surv = int((c.L[c.col["v_many"]] >= 5).sum())
    assert R.REFINE_LDS_SLOTS < n_surv <= p["cap"], MISS
    assert delta["redone"] == 0


@pytest.mark.parametrize("d,du", FT_WIDTHS)
def test_two_precision_every_way_to_fail(level_corpus, d, du):
    """(vi) a segment over seg_cap, (vii) more than cap survivors, (viii) the k-th exact score equal to the threshold:
    each re-does its own query only; the 9 queries hold 3 failures (one query with the 128-row run: two would bring
    2 x 64 entries per stage to the wave's queue and could take their neighbours with them)"""
    names = ["i_kept", "vi_seg", "i_kept", "vii_cap", "viii_proof", "i_kept", "i_kept", "i_kept", "i_kept"]
    want = [R.REDO if n != "i_kept" else R.KEPT for n in names]
    delta, st, p = _run_levels(level_corpus(du), names, 500, True, "flat_fused", want=want)
    assert delta["redone"] == 3 and delta["redo_chunks"] == 1


@pytest.mark.parametrize("d,du", FT_WIDTHS)
def test_proof_fails_by_its_eps_term_alone(level_corpus, d, du):
    """the k-th exact score lies one level above the threshold.  For a query that is the column's unit vector
    eps_scale * |q| < 1 and the proof holds; with 8 on each of three all-zero columns |q| = sqrt(193) and
    eps_scale * |q| > 1: the same scores, the same result, but the proof fails and the query is re-done"""
    c = level_corpus(du)
    ballast = np.arange(9) % 2 == 1
    assert 1e-3 + c.eps < 1.0 < c.eps * np.sqrt(193.0) - 1e-2, MISS
    want = np.where(ballast, R.REDO, R.KEPT)
    delta, st, p = _run_levels(c, ["proof_gap"] * 9, 500, True, "flat_fused", want=want, mult=np.ones(9, dtype=np.int64),
                               ballast=ballast)
    assert delta["redone"] == 4


@pytest.mark.parametrize("d,du", FT_WIDTHS)
def test_top_t_stream_overflow_keeps_the_result_exact(level_corpus, d, du):
    """(ix) one sample stage holds 48 of the sample's best rank + 10: its two streams keep 8 each, the threshold falls
    to the next level and 1 000 more rows survive -- still within cap, and the result is the same"""
    c = level_corpus(du)
    p = R.plan(FT_N, d, 9, 500)
    lev = c.L[c.col["ix_stream"]]
    # the sample's rank-th best is level 5, but one split holds 48 of them: the streams keep fewer than rank scores of
    # level 5 and at least rank of level 3 (no split crowded there beyond what 8 slots hold of the lower level)
    samp = lev[np.arange(p["S"]) * p["stride"]]
    assert -np.sort(-samp)[p["rank"] - 1] == 5 and set(np.unique(samp[samp >= 3]).tolist()) == {3, 5}, MISS
    least5, most5, crowd5 = R.top_t_kept(lev, p, 5)
    least3, most3, _ = R.top_t_kept(lev, p, 3)
    assert crowd5 >= 48 > 2 * R.SAMPLE_T and most5 < p["rank"] < least3, (MISS, most5, least3, p["rank"])
    assert int((lev >= 3).sum()) <= p["cap"], MISS
    delta, st, p = _run_levels(c, ["ix_stream"] * 9, 500, True, "flat_fused", want=[R.EITHER] * 9, sample_top=True)


@pytest.mark.parametrize("d,du", FT_WIDTHS)
def test_two_precision_partial_last_query_block(level_corpus, d, du):
    """(x) 700 queries at k = 10: three query blocks, the last of 188 with a wave of 60; the last expected row lies in
    the 16-row last stage.  One whole wave (queries 256 - 319) overflows its candidate lists and is re-done in 8 chunks;
    the waves of kept queries bring at most 2 x 64 entries per stage to their queues"""
    c = level_corpus(du)
    names = ["kept10"] * 700
    names[256:320] = ["cap10"] * 64
    want = [R.REDO if n == "cap10" else R.KEPT for n in names]
    delta, st, p = _run_levels(c, names, 10, True, "flat_fused", want=want, sample_top=True)
    assert 700 % R.QBB == 188 and c.expect(np.array([c.col["kept10"]]), [1], 10)[1][0, -1] == FT_N - 1, MISS
    assert delta["redone"] == 64 and delta["redo_chunks"] == 8


@pytest.mark.parametrize("d,du", FT_WIDTHS)
@pytest.mark.parametrize("k", [10, 500])
def test_all_f32_kept_redone_in_chunks_and_inclusive_threshold(level_corpus, d, du, k):
    """set_two_precision(0), stride 4.  KEPT for all; more than cap rows tie at the top for all 20 queries: re-done in
    chunks of 8, 8 and 4; the k-th candidate EQUALS the threshold and is kept (`acc >= thr`)"""
    c = level_corpus(du)
    kept, incl = ("f32_kept", "f32_incl") if k == 500 else ("f32_kept10", "f32_incl10")
    delta, st, p = _run_levels(c, [kept] * 20, k, False, "flat_f32", want=[R.KEPT] * 20, stride=4, fin_lds=True,
                               fin_thr_lds=False)
    assert delta["flat_f32"] == 1 and delta["redone"] == 0
    delta, st, p = _run_levels(c, ["vii_cap"] * 20, k, False, "flat_f32", want=[R.REDO] * 20)
    assert delta["redone"] == 20 and delta["redo_chunks"] == 3
    delta, st, p = _run_levels(c, [incl] * 20, k, False, "flat_f32", want=[R.KEPT] * 20)
    assert delta["redone"] == 0


@pytest.mark.parametrize("N", [65537, 66000])
@pytest.mark.parametrize("d,du", [(32, 32), (64, 33), (128, 128)])
def test_flat_thresholded_random_integers(N, d, du):
    """random integers in [-8, 8], all-f32 and two-precision, k = 10 and 500: interval verdicts"""
    nq = 20
    rng = np.random.default_rng(3000 + N + du)
    X, Q = _rand_ints(rng, (N, du)), _rand_ints(rng, (nq, du))
    X[N - 40:] = X[100:140]                                   # ties with the last rows (the short last tile)
    Sc = R.int_scores(Q, X)
    qn = np.sqrt((Q.astype(np.float64) ** 2).sum(axis=1))
    idx = _flat(X)
    for two in (False, True):
        for k in (10, 500):
            p = R.plan(N, d, nq, k, two_precision=two)
            assert p["route"] == ("flat_fused" if two else "flat_f32") and p["stride"] == (2 if two else 4), MISS
            st = R.flat_verdicts(Sc, p, qnorm=qn, eps=R.eps_scale(X))
            es, er = R.topk(Sc, k)
            _set_two(idx, two)
            gs, gr, delta = _search(idx, Q, k)
            _check_stats(delta, R.expected_stats(N, d, nq, k, two_precision=two), [st])
            _same(gs, gr, es, er)


# ---- passes, re-dos and id_map -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,du", [(64, 64), (32, 20)])
def test_second_internal_pass_redo_chunks_and_id_map(level_corpus, d, du):
    """4 100 queries at k = 10 on the two-precision index: passes of 4 096 and 4.  Two whole waves of the first pass
    (128 queries, 16 chunks) and 2 queries of the second (1 chunk) must be re-done; the results come back as item ids
    (id_map), padding stays -1"""
    from recommendit_amd import _lib
    c = level_corpus(du)
    nq, k = 4100, 10
    names = ["kept10"] * nq
    for q in list(range(192, 256)) + list(range(2560, 2624)) + [4097, 4099]:
        names[q] = "cap10"
    mult = 1 + np.arange(nq) % 8
    Q, cols = c.queries(names, mult)
    assert R.passes(nq) == [4096, 4], MISS
    states = []
    for q0, n in ((0, 4096), (4096, 4)):
        p = R.plan(FT_N, d, n, k)
        assert p["route"] == "flat_fused", MISS
        states.append(c.verdicts(cols[q0:q0 + n], mult[q0:q0 + n], p))
    assert (states[0] == R.REDO).sum() == 128 and (states[1] == R.REDO).sum() == 2, MISS
    assert (np.concatenate(states) == R.EITHER).sum() == 0, MISS
    es, er = c.expect(cols, mult, k)
    ids = (3 * np.arange(FT_N) + 7).astype(np.int64)
    old_ids, old_dev = c.idx.item_ids, c.idx._item_ids_dev
    c.idx.item_ids, c.idx._item_ids_dev = ids, _dev(ids)
    try:
        gs, gr, delta = _search(c.idx, Q, k, ids=True)
    finally:
        c.idx.item_ids, c.idx._item_ids_dev = old_ids, old_dev
        _lib.check(_lib.lib().rihip_ip_index_set_id_map(c.idx.index._h, None))
    _check_stats(delta, R.expected_stats(FT_N, d, nq, k), states)
    assert delta["passes"] == 2 and delta["redone"] == 130 and delta["redo_chunks"] == 17
    _same(gs, gr, es, np.where(er >= 0, ids[np.maximum(er, 0)], -1))
    # k > N on the dense path with the map: padding is not mapped
    X = c.X[:300]
    small = _flat(X, ids=ids[:300])
    s2, r2 = small._search_device(_dev(Q[:6]), 307, item_ids=True)
    e2s, e2r = R.topk(R.int_scores(Q[:6], X), 307)
    _same(s2.cpu().numpy(), r2.cpu().numpy(), e2s, np.where(e2r >= 0, ids[np.maximum(e2r, 0)], -1))


# ======================================================================================================================
# IVF
# ======================================================================================================================
IVF_LENS = [0, 1, 2, 3, 63, 64, 65, 2049, 9001, 8800, 8600, 8400, 5000, 3000, 1500, 700]
IVF_NPROBE = 4
IVF_TINY = 7            # lists 0 .. 6 have unit-axis centroids
IVF_TINY_Q = [0, 1, 2] + list(range(41, 138))     # the 100 queries that probe those lists only


def _ivf_case(du, nq, seed):
    """16 injected lists.  Centroid l < 7 is 8 e_l and the other centroids have no weight on axes 0 .. 6; a query with
    weight on those axes only probes tiny lists (ties at coarse score 0 go to the lower list id), the others probe the
    large lists"""
    nlist, N = len(IVF_LENS), sum(IVF_LENS)
    rng = np.random.default_rng(seed)
    X = _rand_ints(rng, (N, du))
    C = _rand_ints(rng, (nlist, du))
    C[:, :IVF_TINY] = 0.0
    C[:IVF_TINY] = 0.0
    C[np.arange(IVF_TINY), np.arange(IVF_TINY)] = 8.0
    Q = _rand_ints(rng, (nq, du), -2, 2)
    Q[:, :IVF_TINY] = 0.0
    tiny = [(0, 1, 2, 3), (1, 2, 4, 5), (0, 1, 2), (3, 4, 5, 6), (2, 4, 5, 6), (0, 4, 5, 6), (1, 3, 5, 6)]
    for t, q in enumerate(IVF_TINY_Q):                        # these queries probe tiny lists only
        Q[q] = 0.0
        Q[q, list(tiny[t % len(tiny)])] = 1.0 + (t // len(tiny)) % 2
    assign = np.concatenate([np.full(n, l, np.int32) for l, n in enumerate(IVF_LENS)])[rng.permutation(N)]
    big = np.nonzero(assign == 8)[0]
    X[big[4000:4200]] = X[big[0:200]]                         # ties inside one list, across its tiles
    R.check_exact_inputs(X, C, Q)
    return N, nlist, X, C, Q, assign


@pytest.fixture(scope="module")
def ivf_case():
    made = {}

    def get(du):
        if du not in made:
            N, nlist, X, C, Q, assign = _ivf_case(du, 1024, 4000 + du)
            probes = R.probed_lists(Q, C, IVF_NPROBE)
            allowed = R.allowed_by_lists(probes, assign, nlist)
            Sc = R.int_scores(Q, X)
            es, er = R.topk(Sc, 500, allowed)
            Sc = Sc.astype(np.int16)                          # (|score| <= 2 * 8 * 128; kept small: six widths share a module)
            made[du] = dict(N=N, nlist=nlist, X=X, C=C, Q=Q, assign=assign, probes=probes, Sc=Sc, es=es, er=er,
                            idx=_ivf(X, C, assign, IVF_NPROBE))
        return made[du]
    return get


@pytest.mark.parametrize("d,du", _du_cases())
def test_ivf_unfiltered_small_batches(ivf_case, d, du):
    """1, 4, 5, 8 queries take the one-launch prepare, 9 and 40 the four launches; the shared queries of 8 and 9 return
    the same bytes.  Queries 0 - 2 probe lists 0 - 3 (6 rows: results padded); query 2 reaches list 3 by the tie rule.
    Both levels of the select work in LDS at these sizes (the next test takes them to global memory)"""
    c = ivf_case(du)
    assert sorted(c["probes"][0].tolist()) == [0, 1, 2, 3] == sorted(c["probes"][2].tolist()), MISS
    assert (c["er"][0, 6:] == -1).all() and (c["er"][0, :6] >= 0).all(), MISS
    got = {}
    for k in (20, 500):
        for nq in (1, 4, 5, 8, 9, 40):
            p = R.plan(c["N"], d, nq, k, list_lens=IVF_LENS, nprobe=IVF_NPROBE)
            assert p["route"] == "ivf_unfiltered" and p["prepare"] == ("small" if nq <= 8 else "four"), MISS
            assert p["fin_pairs_lds"] and p["fin_lds"], MISS
            gs, gr, delta = _search(c["idx"], c["Q"][:nq], k)
            _check_stats(delta, R.expected_stats(c["N"], d, nq, k, list_lens=IVF_LENS, nprobe=IVF_NPROBE), ivf=True)
            assert delta["ivf_unfiltered"] == 1 and delta["prepare_small"] == int(nq <= 8)
            _same(gs, gr, c["es"][:nq, :k], c["er"][:nq, :k])
            got[k, nq] = (gs, gr)
        assert got[k, 8][0].tobytes() == got[k, 9][0][:8].tobytes() and got[k, 8][1].tobytes() == got[k, 9][1][:8].tobytes()


@pytest.mark.parametrize("nq,k,pairs_lds,lds", [(129, 20, False, True), (3, 5000, False, False), (3, 2000, True, True)])
def test_ivf_unfiltered_finalize_in_lds_and_in_global_memory(ivf_case, nq, k, pairs_lds, lds):
    """both levels of the two-level select on both sides of launch_finalize's rule: 516 pair workgroups (global), a
    pair list of 9 024 keys behind an 8 192-key sort buffer (global), nprobe * k = 20 000 keys (global)"""
    d = 64
    c = ivf_case(d)
    p = R.plan(c["N"], d, nq, k, list_lens=IVF_LENS, nprobe=IVF_NPROBE)
    assert p["route"] == "ivf_unfiltered" and p["fin_pairs_lds"] is pairs_lds and p["fin_lds"] is lds, MISS
    gs, gr, delta = _search(c["idx"], c["Q"][40:40 + nq], k)
    _check_stats(delta, R.expected_stats(c["N"], d, nq, k, list_lens=IVF_LENS, nprobe=IVF_NPROBE), ivf=True)
    es, er = R.topk(c["Sc"][40:40 + nq].astype(np.int64), k, R.allowed_by_lists(c["probes"][40:40 + nq], c["assign"], c["nlist"]))
    _same(gs, gr, es, er)


@pytest.mark.parametrize("d,du", _du_cases())
@pytest.mark.parametrize("k", [20, 500])
def test_ivf_thresholded_deficit_redo_chunks_and_deferred(ivf_case, d, du, k):
    """1 024 queries: nq * cap_df > 2^23, sample at tile step 16.  The 100 queries that probe tiny lists hold fewer than
    500 rows: under a real threshold they fail by deficit (ivf_thr) and are re-done in two chunks (k = 500); those with
    fewer sampled rows than rank have no threshold and keep every probed row.  Then the deferred form: same bytes,
    search_finish re-does within the same bounds"""
    c = ivf_case(du)
    nq = 1024
    p = R.plan(c["N"], d, nq, k, list_lens=IVF_LENS, nprobe=IVF_NPROBE)
    assert p["route"] == "ivf_thresholded" and nq * p["cap_df"] > 2 ** 23 and p["tile_step"] == 16, MISS
    st = R.ivf_verdicts(c["Sc"], p, c["assign"], c["probes"], c["nlist"])
    lo, hi = R.redo_bounds(st)
    n_rows = R.allowed_by_lists(c["probes"][IVF_TINY_Q], c["assign"], c["nlist"]).sum(axis=1)
    assert (n_rows < 500).all() and n_rows[0] == 6 < p["rank"] and st[0] == R.KEPT, MISS
    if k == 500:
        assert lo > R.IVF_REDO_CHUNK and (st[IVF_TINY_Q] == R.REDO).sum() > R.IVF_REDO_CHUNK, MISS
    exp = R.expected_stats(c["N"], d, nq, k, list_lens=IVF_LENS, nprobe=IVF_NPROBE)
    gs, gr, delta = _search(c["idx"], c["Q"], k)
    _check_stats(delta, exp, [st], ivf=True)
    assert delta["ivf_thresholded"] == 1 and delta["thr_queries"] == nq
    _same(gs, gr, c["es"][:, :k], c["er"][:, :k])
    # deferred
    idx = c["idx"]
    idx.set_deferred_check(True)
    try:
        before = idx.search_stats()
        s2, r2 = idx._search_device(_dev(c["Q"]), k)
        assert idx.search_pending()
        n_redone = idx.finish_search()
        torch.cuda.synchronize()
        after = idx.search_stats()
    finally:
        idx.set_deferred_check(False)
    assert lo <= n_redone <= hi and after["redone"] - before["redone"] == n_redone == delta["redone"]
    assert s2.cpu().numpy().tobytes() == gs.tobytes() and r2.cpu().numpy().tobytes() == gr.tobytes()


@pytest.mark.parametrize("d,du", [(64, 64), (32, 20)])
def test_ivf_every_list_probed_equals_the_flat_search(ivf_case, d, du):
    """nprobe = 16 on the thresholded route against the flat result of the same rows, byte for byte"""
    c = ivf_case(du)
    nq, k = 1024, 50
    every = np.tile(np.arange(c["nlist"]), (nq, 1))
    p = R.plan(c["N"], d, nq, k, list_lens=IVF_LENS, nprobe=16)
    assert p["route"] == "ivf_thresholded" and R.plan(c["N"], d, nq, k)["route"] == "flat_dense", MISS
    st = R.ivf_verdicts(c["Sc"], p, c["assign"], every, c["nlist"])
    es, er = R.topk(c["Sc"].astype(np.int64), k)
    c["idx"].set_n_probe(16)
    try:
        gs, gr, delta = _search(c["idx"], c["Q"], k)
    finally:
        c["idx"].set_n_probe(IVF_NPROBE)
    _check_stats(delta, R.expected_stats(c["N"], d, nq, k, list_lens=IVF_LENS, nprobe=16), [st], ivf=True)
    _same(gs, gr, es, er)
    fs, fr, fd = _search(_flat(c["X"]), c["Q"], k)
    assert fd["flat_dense"] == 1 and fs.tobytes() == gs.tobytes() and fr.tobytes() == gr.tobytes()


def test_ivf_second_internal_pass(ivf_case):
    """4 100 queries: the first pass of 4 096 is thresholded, the second of 4 is unfiltered (4 * cap_df <= 2^23 -- no
    corpus of this size sends a 4-query pass down the thresholded route), with the one-launch prepare; the re-done
    queries of the first pass and the second pass's outputs land in their own rows"""
    d, k = 64, 20
    c = ivf_case(d)
    nq = 4100
    mult = np.array([1, 2, 3, 4, 1])[np.arange(nq) // 1024].astype(np.float32)
    Q = np.tile(c["Q"], (5, 1))[:nq] * mult[:, None]
    R.check_exact_inputs(Q)
    p1 = R.plan(c["N"], d, 4096, k, list_lens=IVF_LENS, nprobe=IVF_NPROBE)
    p2 = R.plan(c["N"], d, 4, k, list_lens=IVF_LENS, nprobe=IVF_NPROBE)
    assert (p1["route"], p2["route"], p2["prepare"]) == ("ivf_thresholded", "ivf_unfiltered", "small"), MISS
    st1 = R.ivf_verdicts(c["Sc"], p1, c["assign"], c["probes"], c["nlist"])       # a positive multiple changes no verdict
    st = np.tile(st1, 4)
    gs, gr, delta = _search(c["idx"], Q, k)
    _check_stats(delta, R.expected_stats(c["N"], d, nq, k, list_lens=IVF_LENS, nprobe=IVF_NPROBE), [st], ivf=True)
    assert delta["passes"] == 2 and delta["ivf_thresholded"] == 1 and delta["ivf_unfiltered"] == 1
    with np.errstate(invalid="ignore"):
        es = (np.tile(c["es"][:, :k], (5, 1))[:nq] * mult[:, None]).astype(np.float32)
    _same(gs, gr, es, np.tile(c["er"][:, :k], (5, 1))[:nq])


# ======================================================================================================================
# filtered searches (the FILT instantiations): per-query predicates on the same integer data
# ======================================================================================================================
PREDS = [(0, 0, 0), (0b00001, 0, 0), (0, 0b00011, 0), (0b00110, 0, 0b01000), (0, 0b00111, 0b01000), (0, 0b11111, 0),
         (0b00001, 0, 0b00001)]            # the last one passes no row


def _tags_and_preds(rng, N, nq):
    tags = rng.integers(0, 32, N).astype(np.uint32)
    preds = np.array([PREDS[q % len(PREDS)] for q in range(nq)], dtype=np.uint32)
    passing = np.stack([R.pred_pass(tags, pr) for pr in PREDS])[np.arange(nq) % len(PREDS)]
    return tags, preds, passing


def _search_filtered(idx, Q, k, preds, tags):
    """the indexes are shared with the other cases: the tags are set for this search only"""
    idx.set_item_tags(tags)
    try:
        before, fb = idx.search_stats(), idx.filtered_stats()
        s, r = idx._search_device(_dev(Q), k, item_filter=preds)
        torch.cuda.synchronize()
        after, fa = idx.search_stats(), idx.filtered_stats()
    finally:
        idx.clear_item_tags()
    return s.cpu().numpy(), r.cpu().numpy(), {n: after[n] - before[n] for n in after}, (fa[0] - fb[0], fa[1] - fb[1])


@pytest.mark.parametrize("d,du", [(32, 32), (64, 33), (128, 128)])
def test_filtered_flat_dense_and_thresholded(dense_case, level_corpus, d, du):
    """flat index: the dense path at 8 212 rows (2 tiles per split) and the thresholded path, which a filtered search
    takes all-f32 whatever set_two_precision says"""
    N, nq, k = 8212, DENSE_NQ, 70
    idx, X, Q, _, _ = dense_case(N, du)
    rng = np.random.default_rng(5000 + du)
    tags, preds, passing = _tags_and_preds(rng, N, nq)
    assert R.plan(N, d, nq, k, filtered=True)["route"] == "flat_dense", MISS
    es, er = R.topk(R.int_scores(Q, X), k, passing)
    assert passing[6].sum() == 0 and (er[6] == -1).all() and 0 < passing[5].sum() < N // 16, MISS
    gs, gr, delta, fd = _search_filtered(idx, Q, k, preds, tags)
    _check_stats(delta, R.expected_stats(N, d, nq, k, filtered=True))
    assert fd == (nq, 0) and delta["flat_dense"] == 1
    _same(gs, gr, es, er)
    # thresholded
    c = level_corpus(du)
    assert R.kernel_width(c.du) == d, MISS
    nq, k = 20, 10
    p = R.plan(FT_N, R.kernel_width(c.du), nq, k, filtered=True)
    assert p["route"] == "flat_f32" and p["stride"] == 4, MISS
    tags, preds, passing = _tags_and_preds(rng, FT_N, nq)
    mult = 1 + np.arange(nq) % 8
    Q, cols = c.queries(["f32_kept10"] * 10 + ["vii_cap"] * 10, mult)
    Sc = c.L[cols] * mult[:, None]
    samp = np.arange(p["S"]) * p["stride"]
    st = np.array([R.filtered_verdict(Sc[q, passing[q]], Sc[q, samp][passing[q, samp]], p, p["S"]) for q in range(nq)])
    # (the pass-all predicate on the tie-heavy column overflows; under the others its passing rows fit the list)
    assert (st == R.REDO).sum() >= 1 and (st == R.KEPT).sum() >= 8, (MISS, st)
    es, er = R.topk(Sc, k, passing)
    gs, gr, delta, fd = _search_filtered(c.idx, Q, k, preds, tags)
    _check_stats(delta, R.expected_stats(FT_N, R.kernel_width(c.du), nq, k, filtered=True), [st])
    assert fd == (nq, delta["redone"]) and delta["flat_f32"] == 1 and delta["thr_queries"] == nq
    _same(gs, gr, es, er)


@pytest.mark.parametrize("d,du", [(32, 20), (64, 64), (128, 100)])
def test_filtered_ivf_unfiltered_and_thresholded(ivf_case, d, du):
    """IVF index: 40 queries on the unfiltered route, 1 024 on the thresholded one (passing rows of the probed lists are
    counted first: all within cap means no threshold)"""
    c = ivf_case(du)
    idx, N, nlist = c["idx"], c["N"], c["nlist"]
    rng = np.random.default_rng(6000 + du)
    tags, preds, passing = _tags_and_preds(rng, N, 1024)
    allowed = R.allowed_by_lists(c["probes"], c["assign"], nlist) & passing
    rows_of = [np.nonzero(c["assign"] == l)[0] for l in range(nlist)]
    samp_of = [r[R.ivf_sampled_positions(len(r))] for r in rows_of]
    for nq, k in ((40, 20), (1024, 20)):
        p = R.plan(N, d, nq, k, filtered=True, list_lens=IVF_LENS, nprobe=IVF_NPROBE)
        assert p["route"] == ("ivf_unfiltered" if nq == 40 else "ivf_thresholded"), MISS
        states = None
        if nq == 1024:
            st = np.empty(nq, dtype=np.int8)
            for q in range(nq):
                samp = np.concatenate([samp_of[l] for l in c["probes"][q]])
                samp = samp[passing[q, samp]]
                st[q] = R.filtered_verdict(c["Sc"][q, allowed[q]], c["Sc"][q, samp], p, p["cap_s"])
            states = [st]
        es, er = R.topk(c["Sc"][:nq].astype(np.int64), k, allowed[:nq])
        gs, gr, delta, fd = _search_filtered(idx, c["Q"][:nq], k, preds[:nq], tags)
        _check_stats(delta, R.expected_stats(N, d, nq, k, filtered=True, list_lens=IVF_LENS, nprobe=IVF_NPROBE), states,
                     ivf=True)
        assert fd == (nq, delta["redone"])
        _same(gs, gr, es, er)
