"""GPU: seen-item exclusion inside the index scan (exclusion="scan"; csrc/search_exclude.hip, the masked instantiations of
scan_kernel, ivf_scan_lm_kernel and sq8_scan_lm_kernel (csrc/sq8_scan.hip), the drivers in csrc/topk.hip and csrc/sq8.hip).

Every comparison is EQUALITY of ids and score bits on every query.  Vectors, queries and injected centroids are small
integers searched with normalized=True, so every f32 inner product is exact and the expected rows and scores come from
tests/search_reference.py (f32 index) and tests/sq8_reference.py (SQ8: integer scores), with the excluded rows taken out
of the candidate set by tests/exclusion_reference.py.  An SQ8 float score is a function of (query, integer score) alone,
so the float the plain search reports for the same (query, row) is the expected one, bit for bit.  The over-fetch route
("overfetch", the parent's path) is the second yardstick wherever it can serve the batch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exclusion_reference as XR  # noqa: E402
import search_reference as SR  # noqa: E402
import sq8_reference as S8  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_STATE = 5          # RIHIP_ERR_STATE (csrc/common.h)
LENS = [700, 613, 500, 431, 333, 250, 129, 45]      # 8 lists, none a multiple of 32 or 64
NPROBE, K, NQ, N_USERS = 3, 50, 70, 40               # 70 queries: three 32-query groups, the last ragged


def _ints(rng, n, d):
    return rng.randint(-3, 4, size=(n, d)).astype(np.float32)


def _store(lists):
    from recommendit_amd import SeenItems
    return SeenItems.from_dict({u: [int(x) for x in l] for u, l in enumerate(lists)}, n_users=len(lists))


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, exp, what=""):
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(_bits(g), _bits(e), err_msg=what)


class Case:
    """one corpus with its queries, seen store and expected candidates, host side; the indexes are built on demand"""

    def __init__(self, d):
        rng = np.random.RandomState(1000 + d)
        self.d, self.N, self.nlist = d, sum(LENS), len(LENS)
        N = self.N
        self.X, self.Q, self.C = _ints(rng, N, d), _ints(rng, NQ, d), _ints(rng, self.nlist, d)
        self.assign = rng.permutation(np.repeat(np.arange(self.nlist), LENS)).astype(np.int32)
        self.item_ids = rng.permutation(7 * np.arange(N) + 3).astype(np.int64)      # a sparse, shuffled id map
        self.pos, self.Np = XR.ivf_positions(self.assign, self.nlist)
        # query 5 is one of two identical vectors of one list: both tie at the top, the lower row first
        l0 = np.nonzero(self.assign == 1)[0]
        self.twin = (int(l0[3]), int(l0[40]))
        self.X[self.twin[0]] = np.where(self.X[self.twin[0]] == 0, 1, self.X[self.twin[0]]) * 3
        self.X[self.twin[1]] = self.X[self.twin[0]]
        self.Q[5] = self.X[self.twin[0]]
        self.C[1] = self.X[self.twin[0]]             # list 1 is query 5's first probe
        self.S = SR.int_scores(self.Q, self.X)
        self.probes = SR.probed_lists(self.Q, self.C, NPROBE)
        assert self.probes[5, 0] == 1
        self.cand_ivf = SR.allowed_by_lists(self.probes, self.assign, self.nlist)
        self.tags = rng.randint(0, 64, N).astype(np.uint32)
        self.preds = np.array([((1, 0, 0), (0, 2, 4), (0, 0, 0), (3, 0, 8))[q % 4] for q in range(NQ)], np.uint32)
        # the SQ8 side: codes, the query transform and integer scores
        self.m, self.s = S8.train_quantizer(self.X)
        self.codes = S8.encode(self.X, self.m, self.s)
        self.n8, self.t8, self.b8 = S8.encode_queries(self.Q, self.m, self.s)
        self.S8 = S8.int_scores_blas(self.n8, self.codes)
        self._seen()
        self._idx = {}

    def _seen(self):
        rng = np.random.RandomState(7)
        ids, N = self.item_ids, self.N
        plain_rows = SR.topk(self.S, K, self.cand_ivf)[1]
        lists = [np.sort(rng.choice(ids, rng.randint(0, 200), replace=False)) for _ in range(N_USERS)]
        uq = np.arange(NQ) % N_USERS                 # query q -> user
        uq[:12] = np.arange(12)
        lists[0] = ids[:0]                                                        # empty
        lists[1] = ids[[int(plain_rows[1, 0])]]                                   # one item: the query's best row
        lists[2] = ids[~self.cand_ivf[2]][:150]                                   # only rows of lists the query does not probe
        lists[3] = ids[plain_rows[3]]                                             # the entire unexcluded top k
        c = int(self.probes[4, 0])                                                # first / last row of a tile and of a list
        in_c = np.nonzero(self.assign == c)[0]
        p0 = self.pos[in_c].min()
        edge = [p0, p0 + 31, p0 + 32, p0 + 63, p0 + LENS[c] - 1]                   # bits 0 and 31; the last real row
        lists[4] = ids[[int(np.nonzero(self.pos == p)[0][0]) for p in edge]]
        self.edge_pos = edge
        lists[5] = ids[[self.twin[0]]]                                            # one of two identical vectors
        probed6 = np.nonzero(self.cand_ivf[6])[0]
        lists[6] = ids[probed6[:-20]]                                             # all but 20 < k probed rows: a padded answer
        lists[7] = np.concatenate([ids[plain_rows[7, :5]], [1, 2, 10 ** 6]])      # ids absent from the index (and its table)
        uq[8] = N_USERS + 5                                                       # a user outside the store
        uq[9] = -1
        uq[10] = uq[11] = 3                                                       # the same user twice in a batch
        self.lists = [np.unique(np.asarray(l, dtype=np.int64)) for l in lists]
        self.user_ids = uq.astype(np.int64)
        self.seen = _store(self.lists)
        per_q = XR.seen_lists(self.seen._offsets, self.seen._items, self.user_ids, NQ)
        self.excluded = XR.excluded_rows(per_q, ids)
        assert not self.excluded[8].any() and not self.excluded[9].any() and self.excluded[10].sum() == K

    # -- expected -------------------------------------------------------------------------------------------------
    def passing(self, preds):
        if preds is None:
            return None
        if isinstance(preds, tuple):
            return SR.pred_pass(self.tags, preds)
        return np.stack([SR.pred_pass(self.tags, p) for p in preds])

    def expect(self, ivf, preds=None, excluded=None):
        """(scores f32, item ids) of the f32 index"""
        ok = XR.allowed_rows(self.excluded if excluded is None else excluded, self.cand_ivf if ivf else None,
                             self.passing(preds))
        sc, rows = XR.topk_excluding(self.S, K, ok)
        return sc, np.where(rows >= 0, self.item_ids[np.maximum(rows, 0)], -1)

    def expect8(self, ivf, preds=None, k=K):
        """(rows, integer scores i32 with INT32_MIN padding) of the SQ8 index (a flat one is one list: every row probed)"""
        ok = XR.allowed_rows(self.excluded, self.cand_ivf if ivf else None, self.passing(preds))
        rows = XR.first_k((-self.S8) * (1 << 24) + np.arange(self.N)[None, :], ok, k)
        sc = np.where(rows >= 0, np.take_along_axis(self.S8, np.maximum(rows, 0), axis=1), -2 ** 31).astype(np.int32)
        return rows, sc

    # -- indexes ----------------------------------------------------------------------------------------------------
    def faiss(self, ivf, tagged=True):
        key = ("f", ivf)
        if key not in self._idx:
            from recommendit_amd import FAISSIndex
            xd = torch.from_numpy(self.X).cuda()
            if ivf:
                idx = FAISSIndex(embed_dim=self.d, n_lists=self.nlist, n_probe=NPROBE)
                idx.build_from_device(xd, self.item_ids, centroids=self.C, assign=self.assign)
            else:
                idx = FAISSIndex(embed_dim=self.d, exact=True)
                idx.build_from_device(xd, self.item_ids)
            self._idx[key] = idx
        return self._idx[key]

    def sq8(self, ivf):
        key = ("s", ivf)
        if key not in self._idx:
            from recommendit_amd import SQ8Index
            self._idx[key] = SQ8Index.from_index(self.faiss(ivf), keep_vectors=True)
        return self._idx[key]

    @property
    def qd(self):
        return torch.from_numpy(self.Q).cuda()


@pytest.fixture(scope="module", params=[64, 128])
def case(request):
    return Case(request.param)     # (computed once per width: shared by the tests below, never changed)


def _positions(case, ivf):
    pos = case.pos if ivf else np.arange(case.N)
    return [pos[np.nonzero(e)[0]] for e in case.excluded], (case.Np if ivf else case.N)


# ---- 1. the mask ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ivf", [True, False])
def test_mask_equals_reference_and_scratch_is_zero_after_a_search(case, ivf):
    idx = case.faiss(ivf)
    ps, Np = _positions(case, ivf)
    want = XR.mask_words(ps, Np)
    got = idx.exclusion_mask(case.seen, case.user_ids)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, want)
    if ivf:     # bits 0 and 31 of a word, and the last real row of a list, are among them
        row4 = want[4]
        assert all((row4[p >> 5] >> (p & 31)) & 1 for p in case.edge_pos)
    np.testing.assert_array_equal(got[10], got[11])                 # one user twice: a mask row each
    assert not got[8].any() and not got[9].any() and not got[0].any()
    # user_ids on the device, and None = row q of the store
    np.testing.assert_array_equal(idx.exclusion_mask(case.seen, torch.from_numpy(case.user_ids).cuda()), want)
    by_row = idx.exclusion_mask(case.seen, None, nq=N_USERS)
    ex_rows = XR.excluded_rows(XR.seen_lists(case.seen._offsets, case.seen._items, None, N_USERS), case.item_ids)
    pos = case.pos if ivf else np.arange(case.N)
    np.testing.assert_array_equal(by_row, XR.mask_words([pos[np.nonzero(e)[0]] for e in ex_rows], Np))
    idx.batch_search_device(case.qd, k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids, exclusion="scan")
    assert idx.exclusion_scratch_nonzero() == 0                     # set, search, clear the touched words
    # the SQ8 handle keeps the same physical order (a flat one is one list padded to 64 rows)
    sq = case.sq8(ivf)
    got8 = sq.exclusion_mask(case.seen, case.user_ids)
    if ivf:
        np.testing.assert_array_equal(got8, want)
    else:
        np.testing.assert_array_equal(got8, XR.mask_words(ps, (case.N + 63) // 64 * 64))
    sq.batch_search_device(case.qd, k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids, exclusion="scan")
    assert sq.exclusion_scratch_nonzero() == 0


# ---- 2. the f32 index: reference, over-fetch, item filters, chunks -----------------------------------------------------------
@pytest.mark.parametrize("ivf", [True, False])
def test_f32_scan_equals_reference_and_overfetch(case, ivf):
    idx = case.faiss(ivf)
    kw = dict(k=K, normalized=True, exclude=case.seen)
    exp = case.expect(ivf)
    if ivf:
        assert 0 < (exp[1][6] >= 0).sum() < K                       # a padded answer
        assert case.item_ids[case.twin[1]] == exp[1][5, 0]          # the surviving twin leads
    b = idx.exclusion_stats()
    for uid in (case.user_ids, torch.from_numpy(case.user_ids).cuda()):
        _same(idx.batch_search_device(case.qd, user_ids=uid, exclusion="scan", **kw), exp, "scan vs reference")
    a = idx.exclusion_stats()
    assert a["queries"] - b["queries"] == 2 * NQ and a["chunks"] - b["chunks"] == 2
    d0 = idx.exclusion_deficit()
    over = idx.batch_search_device(case.qd, user_ids=case.user_ids, **kw)
    _same(over, exp, "overfetch vs reference")
    assert idx.exclusion_deficit() == d0 == 0
    # host entries
    hs, hi = idx.batch_search(case.Q, k=K, exclude=case.seen, user_ids=case.user_ids, exclusion="scan")
    os_, oi = idx.batch_search(case.Q, k=K, exclude=case.seen, user_ids=case.user_ids)
    np.testing.assert_array_equal(hi, oi)
    np.testing.assert_array_equal(hs.view(np.uint32), os_.view(np.uint32))
    ds, di = idx.search(case.Q[3], k=K, exclude_items=case.lists[3], exclusion="scan")
    ds2, di2 = idx.search(case.Q[3], k=K, exclude_items=case.lists[3])
    np.testing.assert_array_equal(di, di2)
    np.testing.assert_array_equal(ds.view(np.uint32), ds2.view(np.uint32))
    assert not set(di.tolist()) & set(case.lists[3].tolist())


@pytest.mark.parametrize("ivf", [True, False])
def test_f32_scan_with_item_filters(case, ivf):
    idx = case.faiss(ivf)
    kw = dict(k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids)
    with pytest.raises(ValueError, match="tags"):
        idx.batch_search_device(case.qd, item_filter=(1, 0, 0), exclusion="scan", **kw)
    _same(idx.batch_search_device(case.qd, exclusion="scan", **kw), case.expect(ivf), "untagged index")
    idx.set_item_tags(case.tags)
    try:
        for flt in ((1, 0, 0), (0, 0, 0), case.preds, torch.from_numpy(case.preds.view(np.int32)).cuda()):
            host = flt.cpu().numpy().view(np.uint32) if isinstance(flt, torch.Tensor) else flt
            exp = case.expect(ivf, host)
            got = idx.batch_search_device(case.qd, item_filter=flt, exclusion="scan", **kw)
            _same(got, exp, f"scan + filter {type(flt).__name__}")
            _same(idx.batch_search_device(case.qd, item_filter=flt, **kw), got, "overfetch + filter")
        assert idx.exclusion_scratch_nonzero() == 0
    finally:
        idx.clear_item_tags()


@pytest.mark.parametrize("ivf", [True, False])
def test_several_mask_chunks_give_the_same_bytes(case, ivf):
    idx = case.faiss(ivf)
    sq = case.sq8(ivf)
    kw = dict(k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids, exclusion="scan")
    for obj, n_words in ((idx, ((case.Np if ivf else case.N) + 31) // 32),
                         (sq, ((case.Np if ivf else (case.N + 63) // 64 * 64) + 31) // 32)):
        one = obj.batch_search_device(case.qd, **kw)
        try:
            for per, chunks in ((32, 3), (1, NQ)):
                obj.set_exclusion_budget(4 * n_words * per)
                b = obj.exclusion_stats()["chunks"]
                _same(obj.batch_search_device(case.qd, **kw), one, f"{per} queries per chunk")
                assert obj.exclusion_stats()["chunks"] - b == chunks
                assert obj.exclusion_scratch_nonzero() == 0
        finally:
            obj.set_exclusion_budget(0)


# ---- 3. the SQ8 index ------------------------------------------------------------------------------------------------------
def _plain8_scores(sq, case, ivf):
    """float bits of the plain search per (query, row): the score the same index reports for the same row"""
    kk = min(case.N, 3000)
    s, r, i = sq.search_rows_device(case.qd, kk, mode="dense", return_int=True)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    out = np.full((NQ, case.N), -np.inf, np.float32)
    for q in range(NQ):
        ok = r[q] >= 0
        out[q, r[q][ok]] = s[q][ok]
    return out


@pytest.mark.parametrize("ivf", [True, False])
def test_sq8_scan_equals_reference_in_every_mode(case, ivf):
    sq = case.sq8(ivf)
    plain = _plain8_scores(sq, case, ivf)
    kw = dict(k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids)
    rows, isc = case.expect8(ivf)
    ids = np.where(rows >= 0, case.item_ids[np.maximum(rows, 0)], -1)
    fsc = np.where(rows >= 0, np.take_along_axis(plain, np.maximum(rows, 0), axis=1), np.float32(-np.inf)).astype(np.float32)
    first = None
    for mode in ("dense", "thresholded", "auto"):
        got = sq.batch_search_device(case.qd, mode=mode, return_int=True, exclusion="scan", **kw)
        _same(got, (fsc, ids, isc), f"sq8 scan, {mode}")
        first = got if first is None else first
        _same(got, first, "the modes give the same bytes")
    over = sq.batch_search_device(case.qd, **kw)
    _same(over, first[:2], "overfetch")
    assert sq.exclusion_stats()["queries"] >= 3 * NQ and sq.exclusion_scratch_nonzero() == 0
    # item filters, shared and per query
    sq.set_item_tags(case.tags)
    try:
        for flt in ((1, 0, 0), case.preds):
            r2, i2 = case.expect8(ivf, flt)
            id2 = np.where(r2 >= 0, case.item_ids[np.maximum(r2, 0)], -1)
            for mode in ("dense", "thresholded"):
                got = sq.batch_search_device(case.qd, mode=mode, return_int=True, item_filter=flt, exclusion="scan", **kw)
                np.testing.assert_array_equal(got[1].cpu().numpy(), id2)
                np.testing.assert_array_equal(got[2].cpu().numpy(), i2)
            _same(sq.batch_search_device(case.qd, item_filter=flt, **kw), got[:2], "overfetch + filter")
    finally:
        sq.clear_item_tags()
    ds, di = sq.search(case.Q[3], k=K, exclude_items=case.lists[3], exclusion="scan")
    ds2, di2 = sq.search(case.Q[3], k=K, exclude_items=case.lists[3])
    np.testing.assert_array_equal(di, di2)
    np.testing.assert_array_equal(ds.view(np.uint32), ds2.view(np.uint32))


@pytest.mark.parametrize("ivf", [True, False])
def test_sq8_refined_scan_is_certified_and_equals_the_overfetch_route(case, ivf):
    """The certificate of a refined search speaks of its own stage 1, and the two routes have different ones (over-fetch:
    k_scan = ceil(factor * k_eff) of all rows; scan: ceil(factor * k) of the unseen rows).  They are compared where both
    prove their list: a certified list is THE top k by (f, row) of the probed rows the user has not seen, whatever stage
    1 was.  With a factor that takes every probed row into stage 1 both routes certify every query ("fewer than k_scan
    valid rows"); with a small factor every query certified on both sides must still agree, and every certified query
    equals the brute force."""
    sq = case.sq8(ivf)
    kw = dict(k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids, return_cert=True)
    ok = XR.allowed_rows(case.excluded, case.cand_ivf if ivf else None)
    bs, br = XR.topk_excluding(case.S, K, ok)                        # integer inputs: f is the exact inner product
    bi = np.where(br >= 0, case.item_ids[np.maximum(br, 0)], -1)
    for factor, all_certified in ((400.0, True), (1.5, False)):
        got = sq.batch_search_device(case.qd, refine=factor, exclusion="scan", **kw)
        over = sq.batch_search_device(case.qd, refine=factor, **kw)
        gc, oc = got[2].cpu().numpy().astype(bool), over[2].cpu().numpy().astype(bool)
        if all_certified:
            assert gc.all() and oc.all()
            _same(got[:3], over[:3], "refined outputs and certificates")
        both = gc & oc
        _same([t[torch.from_numpy(both).cuda()] for t in got[:2]], [t[torch.from_numpy(both).cuda()] for t in over[:2]])
        np.testing.assert_array_equal(got[1].cpu().numpy()[gc], bi[gc])
        np.testing.assert_array_equal(got[0].cpu().numpy()[gc].view(np.uint32), bs[gc].view(np.uint32))
    cs, ci, cc = sq.search_certified(case.qd, k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids,
                                     exclusion="scan")
    cc = cc.cpu().numpy().astype(bool)
    assert cc.all()
    np.testing.assert_array_equal(ci.cpu().numpy(), bi)
    np.testing.assert_array_equal(cs.cpu().numpy().view(np.uint32), bs.view(np.uint32))
    with pytest.raises(ValueError, match="scan"):
        sq.search_certified(case.qd, k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids)


# ---- 4. updates ----------------------------------------------------------------------------------------------------------
def test_excluded_search_after_updates_equals_a_fresh_index():
    from recommendit_amd import FAISSIndex, SQ8Index
    case = Case(64)
    rng = np.random.RandomState(5)
    xd = torch.from_numpy(case.X).cuda()
    idx = FAISSIndex(embed_dim=64, n_lists=case.nlist, n_probe=NPROBE)
    idx.build_from_device(xd, case.item_ids, centroids=case.C, assign=case.assign)
    sq = SQ8Index.from_index(idx)
    kw = dict(k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids, exclusion="scan")
    idx.batch_search_device(case.qd, **kw)                           # (the row -> position table exists before the update)
    sq.batch_search_device(case.qd, **kw)
    gone = case.lists[3][:20]                                        # ids of a seen list leave the index: ignored afterwards
    repl = case.item_ids[rng.choice(case.N, 40, replace=False)]
    repl = repl[~np.isin(repl, gone)]
    new_ids = np.array([5, 12, 10 ** 5 + 1, 10 ** 5 + 8], np.int64)
    case.lists[2] = np.concatenate([case.lists[2], new_ids[:2]])     # ... and two of the new ids are seen by user 2
    seen = _store(case.lists)
    kw["exclude"] = seen
    Xr, Xn = _ints(rng, repl.shape[0], 64), _ints(rng, 4, 64)
    for obj in (idx, sq):
        assert obj.remove_items(gone) == 20
        obj._apply_update(repl, torch.from_numpy(Xr).cuda(), repl)   # (update_items without its normalisation: integer rows)
        obj.add_items_device(torch.from_numpy(Xn).cuda(), new_ids)
    final_ids = idx.item_ids.copy()
    Xf, af = idx.reconstruct(), idx.list_assignment()
    assert Xf.shape[0] == case.N - 20 + 4 and (Xf == np.rint(Xf)).all()
    fresh = FAISSIndex(embed_dim=64, n_lists=case.nlist, n_probe=NPROBE)
    fresh.build_from_device(torch.from_numpy(Xf).cuda(), final_ids, centroids=case.C, assign=af)
    got = idx.batch_search_device(case.qd, **kw)
    _same(got, fresh.batch_search_device(case.qd, **kw), "updated vs fresh")
    _same(got, idx.batch_search_device(case.qd, **{**kw, "exclusion": "overfetch"}), "updated: scan vs overfetch")
    per_q = XR.seen_lists(seen._offsets, seen._items, case.user_ids, NQ)
    ok = XR.allowed_rows(XR.excluded_rows(per_q, final_ids),
                         SR.allowed_by_lists(SR.probed_lists(case.Q, case.C, NPROBE), af, case.nlist))
    es, er = XR.topk_excluding(SR.int_scores(case.Q, Xf), K, ok)
    _same(got, (es, np.where(er >= 0, final_ids[np.maximum(er, 0)], -1)), "updated vs reference")
    assert not np.isin(got[1].cpu().numpy()[2], new_ids[:2]).any()
    # the SQ8 handle: its updated state against a handle encoded from the fresh index with the same quantiser
    np.testing.assert_array_equal(sq.item_ids, final_ids)
    fresh8 = SQ8Index.from_index(fresh, ranges=sq.quantizer())
    np.testing.assert_array_equal(sq.codes(), fresh8.codes())
    g8 = sq.batch_search_device(case.qd, return_int=True, **kw)
    _same(g8, fresh8.batch_search_device(case.qd, return_int=True, **kw), "sq8 updated vs fresh")
    _same(g8[:2], sq.batch_search_device(case.qd, **{**kw, "exclusion": "overfetch"}), "sq8 updated: scan vs overfetch")
    assert idx.exclusion_scratch_nonzero() == 0 and sq.exclusion_scratch_nonzero() == 0


# ---- 5. the wall is gone -------------------------------------------------------------------------------------------------
def test_a_history_longer_than_the_select_buffer():
    from recommendit_amd import FAISSIndex, SQ8Index
    rng = np.random.RandomState(11)
    N, d, nlist, k = 20480, 32, 4, 500
    X, Q, C = _ints(rng, N, d), _ints(rng, 3, d), _ints(rng, nlist, d)
    assign = rng.randint(0, nlist, N).astype(np.int32)
    ids = rng.permutation(3 * np.arange(N) + 1).astype(np.int64)
    idx = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=nlist)
    idx.build_from_device(torch.from_numpy(X).cuda(), ids, centroids=C, assign=assign)
    heavy = np.sort(rng.choice(ids, 16100, replace=False))
    seen = _store([heavy, ids[:3]])
    uid = np.array([0, 1, 0])
    qd = torch.from_numpy(Q).cuda()
    with pytest.raises(ValueError, match="exceeds the search limit"):
        idx.batch_search_device(qd, k=k, normalized=True, exclude=seen, user_ids=uid)
    ex = XR.excluded_rows(XR.seen_lists(seen._offsets, seen._items, uid, 3), ids)
    Sx = SR.int_scores(Q, X)
    es, er = XR.topk_excluding(Sx, k, ~ex)
    assert (er >= 0).all()
    exp = (es, ids[er])
    _same(idx.batch_search_device(qd, k=k, normalized=True, exclude=seen, user_ids=uid, exclusion="scan"), exp)
    sq = SQ8Index.from_index(idx)
    with pytest.raises(ValueError, match="exceeds the search limit"):
        sq.batch_search_device(qd, k=k, normalized=True, exclude=seen, user_ids=uid)
    m, s = S8.train_quantizer(X)
    n8 = S8.encode_queries(Q, m, s)[0]
    S8x = S8.int_scores_blas(n8, S8.encode(X, m, s))
    r8 = XR.first_k((-S8x) * (1 << 24) + np.arange(N)[None, :], ~ex, k)
    g = sq.batch_search_device(qd, k=k, normalized=True, exclude=seen, user_ids=uid, exclusion="scan", return_int=True)
    np.testing.assert_array_equal(g[1].cpu().numpy(), ids[r8])
    np.testing.assert_array_equal(g[2].cpu().numpy(), np.take_along_axis(S8x, r8, axis=1).astype(np.int32))


# ---- 6. the thresholded passes ---------------------------------------------------------------------------------------------
def _big_seen(rng, ids, nq, plain_rows):
    """per query (user q): its own best 40 rows plus random ids; query 0 nothing, query 1 everything but 30 rows"""
    lists = [np.concatenate([ids[plain_rows[q, :40]], rng.choice(ids, 300, replace=False)]) for q in range(nq)]
    lists[0] = ids[:0]
    lists[1] = ids[rng.permutation(ids.shape[0])[30:]]
    return [np.unique(l) for l in lists]


@pytest.mark.parametrize("ties", [False, True])
def test_ivf_thresholded_pass_with_a_real_threshold_and_a_forced_redo(ties):
    """the shape of tests/test_gpu_filtered_search.py (ivf_large): cap_full > 16 384, 4 k <= cap_full / 16 and
    nq * cap_df > 2^23, so pass A and pass B run; ties: nine rows in ten are copies of one vector, far more rows tie at the
    threshold than the candidate list holds, and those queries are re-done exactly -- through their own mask rows"""
    from recommendit_amd import FAISSIndex, SQ8Index
    rng = np.random.RandomState(404 + ties)
    N, d, nq, k, nlist, nprobe = 200_000, 32, 96, 64, 16, 8
    X, Q, C = _ints(rng, N, d), _ints(rng, nq, d), _ints(rng, nlist, d)
    if ties:
        X[rng.rand(N) < 0.9] = 3.0
    assign = rng.randint(0, nlist, N).astype(np.int32)
    ids = np.arange(N, dtype=np.int64) + 11
    idx = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=nprobe)
    idx.build_from_device(torch.from_numpy(X).cuda(), ids, centroids=C, assign=assign)
    Sx = SR.int_scores(Q, X)
    cand = SR.allowed_by_lists(SR.probed_lists(Q, C, nprobe), assign, nlist)
    seen = _store(_big_seen(rng, ids, nq, SR.topk(Sx, k, cand)[1]))
    ok = XR.allowed_rows(XR.excluded_rows(XR.seen_lists(seen._offsets, seen._items, None, nq), ids), cand)
    es, er = XR.topk_excluding(Sx, k, ok)
    assert 0 < (er[1] >= 0).sum() <= 30
    exp = (es, np.where(er >= 0, ids[np.maximum(er, 0)], -1))
    qd = torch.from_numpy(Q).cuda()
    uid = np.arange(nq)
    s0, x0 = idx.search_stats(), idx.exclusion_stats()
    got = idx.batch_search_device(qd, k=k, normalized=True, exclude=seen, user_ids=uid, exclusion="scan")
    s1, x1 = idx.search_stats(), idx.exclusion_stats()
    assert s1["ivf_thresholded"] - s0["ivf_thresholded"] == 1 and s1["thr_queries"] - s0["thr_queries"] == nq
    redone = x1["redone"] - x0["redone"]
    assert redone == s1["redone"] - s0["redone"]
    print(f"IVF thresholded, ties={ties}: {redone} of {nq} queries re-done exactly")
    if ties:
        assert redone > 0                                            # the tied corpus forces re-dos
    _same(got, exp, "ivf thresholded")
    sel = np.arange(nq) != 1                                         # (over-fetch cannot serve query 1's history)
    _same(idx.batch_search_device(qd[torch.from_numpy(sel).cuda()].contiguous(), k=k, normalized=True, exclude=seen,
                                  user_ids=uid[sel]), (exp[0][sel], exp[1][sel]), "overfetch")
    assert idx.exclusion_scratch_nonzero() == 0
    # the SQ8 index over the same lists: thresholded by choice and by auto's rule
    sq = SQ8Index.from_index(idx)
    m, s = S8.train_quantizer(X)
    S8x = S8.int_scores_blas(S8.encode_queries(Q, m, s)[0], S8.encode(X, m, s))
    r8 = XR.first_k((-S8x) * (1 << 24) + np.arange(N)[None, :], ok, k)
    i8 = np.where(r8 >= 0, np.take_along_axis(S8x, np.maximum(r8, 0), axis=1), -2 ** 31).astype(np.int32)
    id8 = np.where(r8 >= 0, ids[np.maximum(r8, 0)], -1)
    assert S8.auto_is_thresholded(nq, k, np.bincount(assign, minlength=nlist), nprobe)
    t0, y0 = sq.search_stats(), sq.exclusion_stats()
    outs = [sq.batch_search_device(qd, k=k, normalized=True, mode=mode, return_int=True, exclude=seen, user_ids=uid,
                                   exclusion="scan") for mode in ("thresholded", "auto", "dense")]
    t1, y1 = sq.search_stats(), sq.exclusion_stats()
    assert t1[0] - t0[0] == 2 * nq and y1["redone"] - y0["redone"] == t1[1] - t0[1]
    if ties:
        assert t1[1] - t0[1] > 0
    for o in outs:
        np.testing.assert_array_equal(o[1].cpu().numpy(), id8)
        np.testing.assert_array_equal(o[2].cpu().numpy(), i8)
        _same(o, outs[0], "sq8 modes")


@pytest.mark.parametrize("ties", [False, True])
def test_flat_all_f32_thresholded_pass(ties):
    """N > 65 536 and no multiple of 32 (tests/test_gpu_filtered_search.py, flat_large): the strided sample reads each
    row's own bit, the stride-1 filter one word per tile; nq crosses the 128-query workgroup"""
    from recommendit_amd import FAISSIndex
    rng = np.random.RandomState(202 + ties)
    N, d, nq, k = 70001, 32, 130, 100
    X, Q = _ints(rng, N, d), _ints(rng, nq, d)
    if ties:
        X[rng.rand(N) < 0.9] = 3.0
    ids = rng.permutation(2 * np.arange(N) + 5).astype(np.int64)
    idx = FAISSIndex(embed_dim=d, exact=True)
    idx.build_from_device(torch.from_numpy(X).cuda(), ids)
    Sx = SR.int_scores(Q, X)
    seen = _store(_big_seen(rng, ids, nq, SR.topk(Sx, k)[1]))
    ok = XR.allowed_rows(XR.excluded_rows(XR.seen_lists(seen._offsets, seen._items, None, nq), ids))
    es, er = XR.topk_excluding(Sx, k, ok)
    assert (er[1] >= 0).sum() == 30
    exp = (es, np.where(er >= 0, ids[np.maximum(er, 0)], -1))
    qd = torch.from_numpy(Q).cuda()
    uid = np.arange(nq)
    s0, x0 = idx.search_stats(), idx.exclusion_stats()
    got = idx.batch_search_device(qd, k=k, normalized=True, exclude=seen, user_ids=uid, exclusion="scan")
    s1, x1 = idx.search_stats(), idx.exclusion_stats()
    assert s1["flat_f32"] - s0["flat_f32"] == 1 and s1["flat_fused"] == s0["flat_fused"]
    redone = x1["redone"] - x0["redone"]
    print(f"flat all-f32 thresholded, ties={ties}: {redone} of {nq} queries re-done exactly")
    if ties:
        assert redone > 0
    _same(got, exp, "flat thresholded")
    sel = np.arange(nq) != 1                                         # (over-fetch cannot serve query 1's history)
    _same(idx.batch_search_device(qd[torch.from_numpy(sel).cuda()].contiguous(), k=k, normalized=True, exclude=seen,
                                  user_ids=uid[sel]), (exp[0][sel], exp[1][sel]), "overfetch")
    assert idx.exclusion_scratch_nonzero() == 0


# ---- 7. refusals, and the over-fetch route after scan calls -------------------------------------------------------------------
def test_refusals_leave_the_handle_searchable(case):
    from recommendit_amd import _lib as L
    idx, sq = case.faiss(True), case.sq8(True)
    kw = dict(k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids)
    ref = idx.batch_search_device(case.qd, exclusion="scan", **kw)
    ref8 = sq.batch_search_device(case.qd, exclusion="scan", **kw)
    stats = idx.exclusion_stats()
    for obj in (idx, sq):
        for bad in ("Scan", "mask", None, 1):
            with pytest.raises(ValueError, match="exclusion"):
                obj.batch_search_device(case.qd, exclusion=bad, **kw)
            with pytest.raises(ValueError, match="exclusion"):
                obj.batch_search_device(case.qd, k=K, normalized=True, exclusion=bad)      # even with nothing to exclude
            with pytest.raises(ValueError, match="exclusion"):
                obj.batch_search(case.Q, k=K, exclusion=bad)
            with pytest.raises(ValueError, match="exclusion"):
                obj.search(case.Q[0], k=K, exclusion=bad)
    uid = torch.from_numpy(case.user_ids).cuda()
    wrong = idx._row_of_device().to(torch.int64)
    with pytest.raises(ValueError, match="row_of"):
        idx._search_scan_excluding(case.qd, K, case.seen, uid, row_of=wrong)
    with pytest.raises(ValueError, match="row_of"):
        sq._scan_excluding(case.qd, K, case.seen, uid, None, 0, False, None, False, row_of=wrong.cpu())
    with pytest.raises(ValueError, match="user ids"):
        idx.batch_search_device(case.qd, k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids[:5], exclusion="scan")
    with pytest.raises(ValueError, match="user_ids"):
        idx.batch_search_device(case.qd, k=K, normalized=True, exclude=case.seen, exclusion="scan")
    assert idx.exclusion_stats() == stats
    # a pending deferred search: refused by the wrapper and by the C entry point
    big = _DeferredCase.get()
    bidx, bq, bseen, bk = big
    plain_ref = bidx.batch_search_device(bq, k=bk, normalized=True)
    scan_ref = bidx.batch_search_device(bq, k=bk, normalized=True, exclude=bseen, user_ids=np.arange(bq.shape[0]), exclusion="scan")
    bidx.set_deferred_check(True)
    try:
        bidx.batch_search_device(bq, k=bk, normalized=True)
        assert bidx.search_pending()
        before = bidx.exclusion_stats()
        with pytest.raises(RuntimeError, match="pending"):
            bidx.batch_search_device(bq, k=bk, normalized=True, exclude=bseen, user_ids=np.arange(bq.shape[0]), exclusion="scan")
        nq = bq.shape[0]
        s = torch.empty((nq, bk), dtype=torch.float32, device="cuda")
        r = torch.empty((nq, bk), dtype=torch.int64, device="cuda")
        row_of = bidx._row_of_device()
        rc = L.lib().rihip_ip_index_search_excluding(bidx.index._h, bq.data_ptr(), nq, bk, None, bseen.offsets.data_ptr(),
                                                     bseen.n_users, bseen.items.data_ptr(), row_of.data_ptr(), row_of.shape[0],
                                                     None, 0, s.data_ptr(), r.data_ptr(), L.stream_ptr())
        assert rc == ERR_STATE and bidx.search_pending() and bidx.exclusion_stats() == before
        bidx.finish_search()
        got = bidx.batch_search_device(bq, k=bk, normalized=True, exclude=bseen, user_ids=np.arange(nq), exclusion="scan")
        assert not bidx.search_pending()                             # synchronous even with the deferred check on
        _same(got, scan_ref)
    finally:
        bidx.set_deferred_check(False)
    _same(bidx.batch_search_device(bq, k=bk, normalized=True), plain_ref)
    _same(idx.batch_search_device(case.qd, exclusion="scan", **kw), ref)
    _same(sq.batch_search_device(case.qd, exclusion="scan", **kw), ref8)


class _DeferredCase:
    """a thresholded IVF shape (a deferred check exists on that path only), built once"""
    _it = None

    @classmethod
    def get(cls):
        if cls._it is None:
            from recommendit_amd import FAISSIndex
            rng = np.random.RandomState(99)
            N, d, nq, k, nlist, nprobe = 200_000, 32, 96, 64, 16, 8
            X, Q, C = _ints(rng, N, d), _ints(rng, nq, d), _ints(rng, nlist, d)
            idx = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=nprobe)
            idx.build_from_device(torch.from_numpy(X).cuda(), np.arange(N), centroids=C,
                                  assign=rng.randint(0, nlist, N).astype(np.int32))
            seen = _store([rng.choice(N, 50, replace=False) for _ in range(nq)])
            cls._it = (idx, torch.from_numpy(Q).cuda(), seen, k)
        return cls._it


def test_overfetch_after_scan_is_the_parents(case, monkeypatch):
    """the default route after scan calls: same bytes and the same exclusion_deficit as on an index that never ran one;
    MIN_GROUP = 16 makes the host plan split the batch into several over-fetch groups"""
    import recommendit_amd.seen as seen_mod
    from recommendit_amd import FAISSIndex
    monkeypatch.setattr(seen_mod, "MIN_GROUP", 16)
    plan = seen_mod.plan_overfetch(case.seen.counts_of(case.user_ids), K, case.N, 16384)
    assert len(plan) > 1
    virgin = FAISSIndex(embed_dim=case.d, n_lists=case.nlist, n_probe=NPROBE)
    virgin.build_from_device(torch.from_numpy(case.X).cuda(), case.item_ids, centroids=case.C, assign=case.assign)
    idx = case.faiss(True)
    kw = dict(k=K, normalized=True, exclude=case.seen, user_ids=case.user_ids)
    scan = idx.batch_search_device(case.qd, exclusion="scan", **kw)
    d0 = idx.exclusion_deficit()
    over = idx.batch_search_device(case.qd, exclusion="overfetch", **kw)
    _same(over, virgin.batch_search_device(case.qd, **kw))
    _same(over, scan)
    assert idx.exclusion_deficit() - d0 == virgin.exclusion_deficit() == 0
    # a short over-fetch by hand: filter_excluded counts its deficit exactly as before
    s, c = idx.batch_search_device(case.qd, k=K, normalized=True)
    outs = []
    for obj in (idx, virgin):
        o = (torch.empty((NQ, K), dtype=torch.float32, device="cuda"), torch.empty((NQ, K), dtype=torch.int64, device="cuda"))
        b = obj.exclusion_deficit()
        obj.filter_excluded(s, c, K, case.seen, torch.from_numpy(case.user_ids).cuda(), *o)
        outs.append((o, obj.exclusion_deficit() - b))
    assert outs[0][1] == outs[1][1] > 0
    _same(outs[0][0], outs[1][0])
