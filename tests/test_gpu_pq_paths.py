"""GPU: the product-quantised index at the shapes that reach every instantiation of its scan and every branch of the search
driver that PQ storage changes, and its trainer across workgroups and at the edges of the update rule.

A. sq8_scan_lm_kernel<DP, FM, PQ, RES> for FM in {TAGS, MASK, TAGS_MASK} x DP in {64, 128} x PQ in {8, 16} x RES: 24 cases over
   an IVF index whose plan gives tpi = 3, ragged splits, short last tiles and partial query groups.
B. the re-do in chunks and in a second internal pass over plain and residual handles (renumbered pairs and their T), with
   mask rows and with per-query predicates; the deficit re-do with T in the compared score; the refined search at dpad 128,
   dsub 16, filtered and excluding.
C. the build across six workgroups per sub-space, flat, IVF and residual; half-way means, negative sums, an entry
   without rows, a tie between identical seeds.

The contract is tests/test_gpu_pq_index.py's: rows and integer scores equal the restatement exactly, padding is
-1 / -2^31 / -inf, float scores within 1 f32 ulp of (float32)(b + t S) evaluated in f64, the modes return the same bytes,
the stats deltas lie within the reference's re-do bounds.  The inputs, the expectations and the assertions that a case
reaches its path are tests/pq_paths_cases.py's; tests/test_pq_paths_host.py runs them without a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_paths_cases as PC  # noqa: E402
import sq8_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ("dense", "thresholded", "auto")


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


def _same_bytes(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def _check(got, rows, sc, ref32, id_of=None):
    """ids and integer scores exact, padding as specified, float scores within 1 ulp of ref32 = (float32)(b + t S)"""
    gs, gr, gi = got
    pad = rows < 0
    np.testing.assert_array_equal(gr, rows if id_of is None else np.where(pad, -1, id_of[np.maximum(rows, 0)]))
    np.testing.assert_array_equal(gi[~pad], sc[~pad])
    assert (gi[pad] == -2 ** 31).all() and np.isneginf(gs[pad]).all()
    ref = ref32[~pad]
    assert (np.abs(gs[~pad].astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)).all()


class _Stats:
    """the deltas of search_stats(), filtered_stats() and exclusion_stats() over one search"""

    def __init__(self, pq):
        self.pq = pq
        self.before = self.read()

    def read(self):
        x = self.pq.exclusion_stats()
        return self.pq.search_stats() + self.pq.filtered_stats() + (x["queries"], x["redone"])

    def delta(self):
        torch.cuda.synchronize()
        d = tuple(a - b for a, b in zip(self.read(), self.before))
        return dict(search=d[0:2], filtered=d[2:4], excluded=d[4:6])


def _seen_store(pairs, nq):
    from recommendit_amd import SeenItems
    return SeenItems.from_pairs(pairs[0], pairs[1], nq)


# ---- A. the instantiation matrix -------------------------------------------------------------------------------------------
A_SHAPES = [(du, dsub, res) for du in (40, 100) for dsub in (8, 16) for res in (False, True)]


@pytest.fixture(scope="module", params=A_SHAPES, ids=lambda p: f"dp{64 if p[0] <= 64 else 128}-pq{p[1]}-{'res' if p[2] else 'plain'}")
def matrix(request):
    from recommendit_amd import PQIndex
    du, dsub, res = request.param
    case = PC.matrix_case(du, dsub, res)
    src = _ivf(case["X"], case["Cc"], case["assign"], PC.A_NPROBE, ids=case["ids"])
    pq = PQIndex.from_index(src, dsub=dsub, ranges=(case["m"], case["s"]), codebooks=case["book"], by_residual=res)
    del src
    np.testing.assert_array_equal(pq.pq_codes(), case["codes"])
    got = pq.codes()
    assert got.dtype == case["dec"].dtype
    np.testing.assert_array_equal(got, case["dec"])
    if res:
        np.testing.assert_array_equal(pq.list_codes(), case["K"])
    pq.set_item_tags(case["tags"])
    case["pq"], case["qd"] = pq, torch.from_numpy(case["Q"]).cuda()
    case["store"] = _seen_store(case["seen_pairs"], PC.A_NQ)
    return case


@pytest.mark.parametrize("fm", PC.FMS)
def test_scan_instantiation(matrix, fm):
    """sq8_scan_lm_kernel<dpad, FM, dsub, RES> in all three modes at k = 10 and 100: FM_TAGS through item_filter=, FM_MASK
    and FM_TAGS_MASK through exclusion="scan" without and with item_filter="""
    c, pq = matrix, matrix["pq"]
    rows, sc, redo = PC.matrix_expect(c, fm)
    ref32 = c["ex"].float_ref(sc)
    kw = {}
    if fm != "mask":
        kw["item_filter"] = c["preds"]
    if fm != "tags":
        kw.update(exclude=c["store"], user_ids=np.arange(PC.A_NQ), exclusion="scan")
    for k in PC.A_KS:
        out = {}
        for mode in MODES:
            st = _Stats(pq)
            res = pq.batch_search_device(c["qd"], k=k, normalized=True, mode=mode, return_int=True, **kw)
            d = st.delta()
            out[mode] = tuple(t.cpu().numpy() for t in res)
            thresholded = mode == "thresholded" or (mode == "auto" and S.auto_is_thresholded(PC.A_NQ, k, PC.A_LENS, PC.A_NPROBE))
            lo, hi = S.redo_bounds(redo[k]) if thresholded else (0, 0)
            assert d["search"][0] == (PC.A_NQ if thresholded else 0) and lo <= d["search"][1] <= hi, (mode, k, d, lo, hi)
            assert d["filtered"] == ((PC.A_NQ, d["search"][1]) if fm != "mask" else (0, 0)), (mode, k, d)
            assert d["excluded"] == ((PC.A_NQ, d["search"][1]) if fm != "tags" else (0, 0)), (mode, k, d)
        _check(out["dense"], rows[:, :k], sc[:, :k], ref32[:, :k], id_of=c["ids"])
        _same_bytes(out["dense"], out["thresholded"])
        _same_bytes(out["dense"], out["auto"])
    if fm != "tags":
        assert pq.exclusion_scratch_nonzero() == 0


# ---- B1. every query re-done, in chunks and in a second internal pass ----------------------------------------------------------
def _redo_index(case):
    from recommendit_amd import PQIndex
    src = _ivf(case["X"], case["Cc"], case["assign"], case["nlist"], ids=case["ids"]) if case["res"] else _flat(case["X"], case["ids"])
    pq = PQIndex.from_index(src, dsub=case["dsub"], ranges=(case["m"], case["s"]), codebooks=case["book"], by_residual=case["res"])
    np.testing.assert_array_equal(pq.pq_codes(), case["codes"])
    np.testing.assert_array_equal(pq.codes()[:3], np.tile(case["x"], (3, 1)))
    return pq


def _redo_expect(case, nq):
    sc = np.tile(case["score"][:, None], (1, PC.B1_K))
    return case["rows"], sc, np.tile(case["ref32"], (1, PC.B1_K))


@pytest.mark.parametrize("nq", [130, 4100])
@pytest.mark.parametrize("shape", list(PC.B1_SHAPES))
def test_every_query_redone_in_chunks_and_in_the_second_pass(shape, nq):
    """sq8_redo with f0 > 0 and the pass at q0 = 4096 over PQ storage; on a residual handle every re-do chunk refills pair_t
    for its renumbered queries, and a (t, b) or a T taken from the main pass shows in all three outputs"""
    case = PC.redo_case(shape, nq)
    pq = _redo_index(case)
    qd = torch.from_numpy(case["Q"]).cuda()
    rows, sc, ref32 = _redo_expect(case, nq)
    out = {}
    for mode in ("thresholded", "dense"):
        st = _Stats(pq)
        res = pq.search_rows_device(qd, PC.B1_K, mode=mode, return_int=True)
        d = st.delta()
        assert d["search"] == ((nq, nq) if mode == "thresholded" else (0, 0)), (mode, d)
        out[mode] = tuple(t.cpu().numpy() for t in res)
    _check(out["thresholded"], rows, sc, ref32)
    _same_bytes(out["thresholded"], out["dense"])


@pytest.mark.parametrize("variant", ["seen", "tags"])
@pytest.mark.parametrize("shape", ["res-64-16", "res-128-8"])
def test_redo_carries_mask_rows_and_predicates(shape, variant):
    """xrow (the mask rows of re-done queries) and launch_gather_pred (their predicates) over a residual handle: every query
    excludes other rows, so a chunk that reads the mask row or the predicate of its own position returns another query's"""
    nq = 130
    case = PC.redo_case(shape, nq, variant)
    pq = _redo_index(case)
    qd = torch.from_numpy(case["Q"]).cuda()
    rows, sc, ref32 = _redo_expect(case, nq)
    if variant == "seen":
        users, seen_rows = np.nonzero(~case["keep"])
        kw = dict(exclude=_seen_store((users, seen_rows + PC.ID0), nq), user_ids=np.arange(nq), exclusion="scan")
    else:
        pq.set_item_tags(case["tags"])
        kw = dict(item_filter=case["preds"])
    out = {}
    for mode in ("thresholded", "dense"):
        st = _Stats(pq)
        res = pq.batch_search_device(qd, k=PC.B1_K, normalized=True, mode=mode, return_int=True, **kw)
        d = st.delta()
        n_redone = nq if mode == "thresholded" else 0
        assert d["search"] == ((nq, nq) if mode == "thresholded" else (0, 0)), (mode, d)
        assert d["filtered" if variant == "tags" else "excluded"] == (nq, n_redone), (mode, d)
        out[mode] = tuple(t.cpu().numpy() for t in res)
    _check(out["thresholded"], rows, sc, ref32, id_of=case["ids"])
    _same_bytes(out["thresholded"], out["dense"])


# ---- B2. deficit re-do under a real threshold ----------------------------------------------------------------------------------
def test_thresholded_fails_by_deficit_with_t_in_the_compared_score():
    from recommendit_amd import PQIndex
    case = PC.deficit_case()
    nq, k = case["nq"], case["k"]
    src = _ivf(case["X"], case["Cc"], case["assign"], case["nlist"])
    pq = PQIndex.from_index(src, dsub=case["dsub"], ranges=(case["m"], case["s"]), codebooks=case["book"], by_residual=True)
    del src
    np.testing.assert_array_equal(pq.list_codes(), case["K"])
    np.testing.assert_array_equal(pq.pq_codes(), case["codes"])
    np.testing.assert_array_equal(pq.codes(), case["dec"])
    qd = torch.from_numpy(case["Q"]).cuda()
    out = {}
    for mode in ("thresholded", "dense"):
        st = _Stats(pq)
        res = pq.search_rows_device(qd, k, mode=mode, return_int=True)
        d = st.delta()
        assert d["search"] == ((nq, nq) if mode == "thresholded" else (0, 0)), (mode, d)
        out[mode] = tuple(t.cpu().numpy() for t in res)
    _check(out["thresholded"], case["rows"], case["sc"], case["ex"].float_ref(case["sc"]))
    _same_bytes(out["thresholded"], out["dense"])
    assert (out["thresholded"][1] >= 0).all()


# ---- B3. refined search and certificate at dpad 128, dsub 16 -------------------------------------------------------------------
def _refined_equals(got, want):
    gs, gr, gc, gb = got
    np.testing.assert_array_equal(gr, want["rows"])
    np.testing.assert_array_equal(gs.view(np.uint32), want["scores"].view(np.uint32))
    np.testing.assert_array_equal(gc, want["cert"])
    np.testing.assert_allclose(gb, want["bound"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
def test_refined_search_filtered_and_excluding_at_dpad_128_dsub_16(res):
    """pq_decode_all / pq_decode_all16 at dpad 128 with dsub 16 (attach_vectors' range pass), the refined search, the refined
    filtered search and rihip_sq8_refine_search_excluding over a PQ and a residual handle"""
    from recommendit_amd import PQIndex
    c = PC.refine_case(res)
    k, nq = PC.C3_K, PC.C3_NQ
    src = _ivf(c["X"], c["Cc"], c["assign"], PC.C3_NPROBE, ids=c["ids"])
    if res:
        pq = PQIndex.from_index(src, dsub=PC.C3_DSUB, codebooks=c["book"], keep_vectors=True, by_residual=True)
        np.testing.assert_array_equal(pq.list_codes(), c["K"])
    else:
        pq = PQIndex.from_index(src, dsub=PC.C3_DSUB, n_iter=2, keep_vectors=True)
        np.testing.assert_array_equal(pq.codebooks(), c["book"])
    del src
    np.testing.assert_array_equal(pq.pq_codes(), c["codes"])
    np.testing.assert_array_equal(pq.codes(), c["dec"])
    e, a = pq.refine_ranges()
    np.testing.assert_array_equal(e, c["ea"][0])
    np.testing.assert_array_equal(a, c["ea"][1])
    pq.set_item_tags(c["tags"])
    qd = torch.from_numpy(c["Q"]).cuda()
    store = _seen_store(c["seen_pairs"], nq)
    id_of = c["ids"]
    for name, want in c["want"].items():
        print(name, "certified by the reference at factor 2:", int(want["cert"].sum()), "of", nq)
    for mode in ("dense", "thresholded"):
        got = [t.cpu().numpy() for t in pq.search_rows_device(qd, k, mode=mode, refine=2, return_cert=True)]
        _refined_equals(got, c["want"]["plain"])
        got = [t.cpu().numpy() for t in pq.search_rows_device(qd, k, mode=mode, refine=2, return_cert=True, item_filter=c["preds"])]
        _refined_equals(got, c["want"]["filtered"])
        sure = got[2] == 1
        np.testing.assert_array_equal(got[1][sure], c["brute"]["filtered"][0][sure])
        assert got[0][sure].tobytes() == c["brute"]["filtered"][1][sure].tobytes()
        got = [t.cpu().numpy() for t in pq.batch_search_device(qd, k=k, normalized=True, mode=mode, refine=2, return_cert=True,
                                                               exclude=store, user_ids=np.arange(nq), exclusion="scan")]
        want = dict(c["want"]["excluding"])
        want["rows"] = id_of[want["rows"]]
        _refined_equals(got, want)
        sure = got[2] == 1
        np.testing.assert_array_equal(got[1][sure], id_of[c["brute"]["excluding"][0]][sure])
        assert got[0][sure].tobytes() == c["brute"]["excluding"][1][sure].tobytes()
    # the certificate's other branch on the two routes: k_scan beyond every query's rows, so every query is certified and
    # equals the brute force over its probed, passing / unseen rows
    factor = PC.C3_KSCAN_ALL / k
    got = [t.cpu().numpy() for t in pq.search_rows_device(qd, k, refine=factor, return_cert=True, item_filter=c["preds"])]
    assert (got[2] == 1).all()
    np.testing.assert_array_equal(got[1], c["brute"]["filtered"][0])
    assert got[0].tobytes() == c["brute"]["filtered"][1].tobytes()
    got = [t.cpu().numpy() for t in pq.batch_search_device(qd, k=k, normalized=True, refine=factor, return_cert=True, exclude=store,
                                                           user_ids=np.arange(nq), exclusion="scan")]
    assert (got[2] == 1).all()
    np.testing.assert_array_equal(got[1], id_of[c["brute"]["excluding"][0]])
    assert got[0].tobytes() == c["brute"]["excluding"][1].tobytes()


# ---- C1. the build across several workgroups -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dsub", [8, 16])
@pytest.mark.parametrize("du", [40, 100])
def test_build_across_workgroups_flat_ivf_and_residual(du, dsub):
    """10 277 rows: six workgroups per sub-space add their LDS sums into the same u64 words; the IVF layout has two
    consecutive empty lists and an empty last one (pq_list_of in the residual and the int16 decode kernels)"""
    from recommendit_amd import PQIndex
    c = PC.train_case(du, dsub)
    book, codes, trace = c["plain"]
    ivf_src = _ivf(c["X"], c["Cc"], c["assign"], 2)
    built = {"flat": PQIndex.from_index(_flat(c["X"]), dsub=dsub, n_iter=PC.C1_ITER),
             "ivf": PQIndex.from_index(ivf_src, dsub=dsub, n_iter=PC.C1_ITER)}
    for kind, pq in built.items():
        np.testing.assert_array_equal(pq.codebooks(), book, err_msg=kind)
        np.testing.assert_array_equal(pq.pq_codes(), codes, err_msg=kind)
        ts = pq.train_stats()
        np.testing.assert_array_equal(ts["distortion"], trace)
        assert ts["residual_clamped"] == 0
        np.testing.assert_array_equal(pq.codes(), c["dec"])
    _same_bytes((built["flat"].pq_codes(), built["flat"].codebooks()), (built["ivf"].pq_codes(), built["ivf"].codebooks()))
    rbook, rcodes, rtrace = c["resid"]
    pq = PQIndex.from_index(ivf_src, dsub=dsub, n_iter=PC.C1_ITER, by_residual=True)
    np.testing.assert_array_equal(pq.list_codes(), c["K"])
    np.testing.assert_array_equal(pq.codebooks(), rbook)
    np.testing.assert_array_equal(pq.pq_codes(), rcodes)
    ts = pq.train_stats()
    np.testing.assert_array_equal(ts["distortion"], rtrace)
    assert ts["residual_clamped"] == c["clamped"]
    got = pq.codes()
    assert got.dtype == np.int16
    np.testing.assert_array_equal(got, c["dec16"])


# ---- C2. the update rule's edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dsub", [8, 16])
def test_update_rule_half_way_means_negative_sums_and_an_entry_without_rows(dsub):
    """one Lloyd step whose means are 42.5, 83.5, -42.5 and -83.5 exactly (-> 42, 84, -42, -84), whose negative sums come
    from three or four workgroups, whose entry 5 ties with entry 1 on every row and keeps its seed, and whose column 1
    adds positive and negative workgroup sums into one word"""
    from recommendit_amd import PQIndex
    c = PC.edges_case(dsub)
    book, codes, trace = c["want"]
    pq = PQIndex.from_index(_flat(c["X"]), dsub=dsub, n_iter=1, ranges=(c["m"], c["s"]))
    got = pq.codebooks()
    assert got[0, 1:5, 0].tolist() == [42, 84, -42, -84]
    np.testing.assert_array_equal(got, book)
    np.testing.assert_array_equal(pq.pq_codes(), codes)
    np.testing.assert_array_equal(pq.train_stats()["distortion"], trace)
    assert (got[:, 5, 0] == 42).all() and (got[:, 5] == c["step"][:, 5]).all()      # entry 5 kept its seed
