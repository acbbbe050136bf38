"""GPU: the product-quantised index.

Build: codebooks, entry numbers and the distortion trace are bitwise tests/pq_reference.py's, for a flat and an IVF build
of the same rows.  Search: a PQ index is the SQ8 index of its own reconstruction, so rows and integer scores equal
tests/sq8_reference.py over the DECODED matrix exactly, padding is -1 / -2^31 / -inf, float scores lie within 1 f32 ulp
of (float32)(b + t S) evaluated in f64, the modes return the same bytes and the re-do counts lie within redo_bounds; one
case each for a tag filter, both exclusion routes and the refined search with its certificate; persistence, refusals and
serving.  Every test first asserts from the references alone that its inputs reach the path it is about."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_reference as P  # noqa: E402
import sq8_filtered_reference as FR  # noqa: E402
import sq8_reference as S  # noqa: E402
import sq8_refine_reference as R  # noqa: E402

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


# ---- 1. build ------------------------------------------------------------------------------------------------------------
def _clustered(seed, n, du, centres=40):
    rng = np.random.default_rng(seed)
    Cc = rng.standard_normal((centres, du)).astype(np.float32)
    X = (Cc[rng.integers(0, centres, n)] + 0.15 * rng.standard_normal((n, du))).astype(np.float32)
    X[:, 2] = -0.75                                            # a constant column: its codes are 0
    X[n // 2:n // 2 + 20] = X[:20]                             # identical rows: identical bytes
    return X, rng


@pytest.mark.parametrize("n", [1500, 100])
@pytest.mark.parametrize("dsub", [8, 16])
@pytest.mark.parametrize("du", [40, 64, 128])
def test_build_is_bitwise_the_restatement_flat_and_ivf(du, dsub, n):
    from recommendit_amd import PQIndex
    n_iter, nlist = 3, 6
    X, rng = _clustered(1000 + du + dsub + n, n, du)
    dpad = P.dpad_of(du)
    M = dpad // dsub
    assert (du == 40) == any(m * dsub < du < (m + 1) * dsub or m * dsub >= du for m in range(M))   # padded sub-spaces at 40 only
    m_, s_ = S.train_quantizer(X)
    c = P.pad_codes(S.encode(X, m_, s_), dpad)
    book, codes, trace = P.train(c, dsub, n_iter)
    assert trace.shape == (n_iter + 1,) and (trace[-1] < trace[0] if n == 1500 else trace[-1] <= trace[0])
    if n == 100:                                               # N < 256: repeated seeds, entries that stay empty
        assert (np.bincount(codes[:, 0], minlength=256) == 0).sum() >= 156
    # six ragged lists, list 3 empty, one of a single row
    assign = rng.integers(0, nlist, n).astype(np.int32)
    assign[assign == 3] = 4
    assign[assign == 1] = 0
    assign[7] = 1
    lens = np.bincount(assign, minlength=nlist)
    assert lens[3] == 0 and lens[1] == 1 and len(set(lens.tolist())) >= 4 and (lens % 64 != 0).any()
    Cc = (rng.integers(-4, 5, (nlist, du)) / 4.0).astype(np.float32)
    built = {"flat": PQIndex.from_index(_flat(X), dsub=dsub, n_iter=n_iter),
             "ivf": PQIndex.from_index(_ivf(X, Cc, assign, 2), dsub=dsub, n_iter=n_iter)}
    for kind, pq in built.items():
        qm, qs = pq.quantizer()
        np.testing.assert_array_equal(qm, m_)
        np.testing.assert_array_equal(qs, s_)
        np.testing.assert_array_equal(pq.codebooks(), book, err_msg=kind)
        np.testing.assert_array_equal(pq.pq_codes(), codes, err_msg=kind)
        ts = pq.train_stats()
        np.testing.assert_array_equal(ts["distortion"], trace)
        np.testing.assert_array_equal(pq.codes(), P.decode(codes, book)[:, :du])          # pq_decode_rows
        np.testing.assert_array_equal(pq.reconstruct(), S.decode(P.decode(codes, book)[:, :du], m_, s_))
        st = pq.stats()
        assert st["bytes_per_vector"] == M and st["dsub"] == dsub and st["n_vectors"] == n
        assert st["n_lists"] == (1 if kind == "flat" else nlist)
        assert ts["peak_bytes"] > st["device_bytes"] > n * M
    _same_bytes((built["flat"].pq_codes(), built["flat"].codebooks()), (built["ivf"].pq_codes(), built["ivf"].codebooks()))


# ---- 2. search -----------------------------------------------------------------------------------------------------------
# Six lists: list 0 empty, list 1 one row, list 2 65 rows, three long ragged ones.  The centroids are unit axes, so the
# coarse scores are exact and read off the first six query columns: queries 0 and 1 probe lists 1 and 2 (66 rows), queries
# 2 and 3 (all +1 / all -1: the score extremes) tie on every list and probe lists 0 and 1 (one row), every other query
# probes two of the three long lists.
S_LENS = [0, 1, 65, 64000, 48001, 35555]
S_NPROBE, S_NQ, S_KS = 2, 70, (1, 10, 100)


def _search_case(du, dsub, ivf):
    """rows that ARE codebook entries (x = c / 128 under the injected quantiser (0, 1/128)): the entry numbers, the SQ8
    codes and the decoded matrix are known by construction"""
    rng = np.random.default_rng(7000 + du + dsub)
    N, nlist = sum(S_LENS), len(S_LENS)
    dpad = P.dpad_of(du)
    M = dpad // dsub
    book = rng.integers(-127, 128, (M, 256, dsub)).astype(np.int8)
    book[:, 0] = 127                                           # entry 0: what a padding row decodes to -- the best score
    book[:, 1] = -127
    col = np.arange(dpad).reshape(M, 1, dsub)
    book = np.where(col < du, book, 0).astype(np.int8)         # padding columns hold 0
    real = np.array([m * dsub < du for m in range(M)])
    for m in np.nonzero(real)[0]:
        assert len({e.tobytes() for e in book[m]}) == 256      # distinct entries: a row's entry is its own at D = 0
    codes = rng.integers(0, 256, (N, M)).astype(np.uint8)
    codes[:, ~real] = 0                                        # a sub-space of padding columns: all entries 0, so entry 0
    assign = np.concatenate([np.full(n, l, np.int32) for l, n in enumerate(S_LENS)])[rng.permutation(N)]
    plus = [np.nonzero(assign == l)[0][0] for l in (1, 2, 3, 4, 5)]
    minus = [np.nonzero(assign == l)[0][1] for l in (2, 3, 4, 5)]
    codes[plus] = 0
    codes[minus] = 1
    codes[np.ix_(minus, np.nonzero(~real)[0])] = 0
    dup = np.nonzero(assign == 3)[0]
    codes[dup[30000:30300]] = codes[dup[100:400]]              # ties inside a list across its splits
    dec = P.decode(codes, book)
    X = (dec[:, :du].astype(np.float32) / np.float32(128.0))
    m_, s_ = np.zeros(du, np.float32), np.full(du, 1.0 / 128.0, np.float32)
    np.testing.assert_array_equal(S.encode(X, m_, s_), dec[:, :du])
    got_codes, dist = P.assign(P.pad_codes(dec[:1000, :du], dpad), book)
    np.testing.assert_array_equal(got_codes, codes[:1000])     # (the restatement agrees on a sample; D = 0)
    assert dist == 0
    Cc = np.zeros((nlist, du), np.float32)
    Cc[np.arange(nlist), np.arange(nlist)] = 2.0
    Q = (rng.integers(-16, 17, (S_NQ, du)) / 8.0).astype(np.float32)
    Q[:, :3] = -1.0
    pat = np.array([[1, 1, -1], [1, -1, 1], [-1, 1, 1]], np.float32)
    Q[:, 3:6] = pat[np.arange(S_NQ) % 3]
    Q[0, :6] = [-1, 1, 1, -1, -1, -1]
    Q[1, :6] = [-1, 1, 1, -1, -1, -1]
    Q[2] = 1.0
    Q[3] = -1.0
    return dict(N=N, nlist=nlist, book=book, codes=codes, dec=dec[:, :du], X=X, m=m_, s=s_, Cc=Cc, Q=Q, assign=assign,
                plus=plus, minus=minus)


class _Expect:
    """tests/test_gpu_sq8_paths.py's: top-kmax rows and scores of the reference, the query transform, the re-do verdicts"""

    def __init__(self, Q, c, m, s, ks, allowed=None, rule=None):
        self.n, self.t, self.b = S.encode_queries(Q, m, s)
        self.Sc = S.int_scores_blas(self.n, c)
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


@pytest.mark.parametrize("du,dsub,ivf", [(128, 8, True), (128, 16, True), (40, 8, True), (40, 16, True), (128, 8, False),
                                         (128, 16, False)],
                         ids=["d128-pq8-ivf", "d128-pq16-ivf", "d40-pq8-ivf", "d40-pq16-ivf", "d128-pq8-flat", "d128-pq16-flat"])
def test_search_equals_the_sq8_reference_over_the_decoded_matrix(du, dsub, ivf):
    from recommendit_amd import PQIndex
    cs = _search_case(du, dsub, ivf)
    Q, N, nlist, assign = cs["Q"], cs["N"], cs["nlist"], cs["assign"]
    # -- the path, from the references alone
    assert S_NQ % 32 != 0 and (S_NQ + 31) // 32 == 3            # three query groups, the last partial
    if ivf:
        probes = S.probed_lists(Q, cs["Cc"], S_NPROBE)
        per_list = np.bincount(probes.ravel(), minlength=nlist)
        lens = S_LENS
        assert sorted(probes[0].tolist()) == [1, 2] and sorted(probes[2].tolist()) == [0, 1] and sorted(probes[3].tolist()) == [0, 1]
        assert (np.sort(probes[4:], axis=1) >= 3).all()
        allowed = FR.probed_mask(assign, probes, nlist)
        assert allowed[0].sum() == 66 and allowed[2].sum() == 1 and max(S_KS) > 66
        rule = lambda Sc, k: S.ivf_thresholded_redo(Sc, k, assign, probes, nlist)   # noqa: E731
    else:
        per_list, lens, allowed = [S_NQ], [N], None
        rule = lambda Sc, k: S.flat_thresholded_redo(Sc, k)                          # noqa: E731
    tpi, n_seq, splits = S.plan(lens, per_list, 1)
    assert tpi >= 3, tpi
    assert any(p > 0 and s % tpi != 0 for p, s in zip(per_list, n_seq))             # a ragged last split
    assert any(l % S.TILE != 0 and p > 0 for p, l in zip(per_list, lens))           # a short last tile: n_ok
    assert S.dense_chunk(lens, S_NPROBE if ivf else 1) >= S_NQ
    ex = _Expect(Q, cs["dec"], cs["m"], cs["s"], list(S_KS), allowed=allowed, rule=rule)
    smax = 32512 * 127 * du
    assert ex.sc[2, 0] == smax and smax < 2 ** 31                                   # the score extremes are reached
    if ivf:
        assert ex.sc[3, 0] == -smax                                                 # (its one probed row)
    else:
        assert (ex.sc[2, :5] == smax).all() and (ex.sc[3, :4] == smax).all() and ex.Sc[3].min() == -smax
    # -- the index
    src = _ivf(cs["X"], cs["Cc"], assign, S_NPROBE) if ivf else _flat(cs["X"])
    pq = PQIndex.from_index(src, dsub=dsub, ranges=(cs["m"], cs["s"]), codebooks=cs["book"])
    del src
    np.testing.assert_array_equal(pq.codebooks(), cs["book"])
    np.testing.assert_array_equal(pq.pq_codes(), cs["codes"])
    np.testing.assert_array_equal(pq.codes(), cs["dec"])
    assert pq.train_stats()["distortion"].tolist() == [0]
    for k in S_KS:
        dense, d_dense = _search(pq, Q, k, "dense")
        thr, d_thr = _search(pq, Q, k, "thresholded")
        auto, d_auto = _search(pq, Q, k, "auto")
        ex.check(dense, k)
        _same_bytes(dense, thr)
        _same_bytes(dense, auto)
        assert d_dense == (0, 0)
        lo, hi = S.redo_bounds(ex.redo[k])
        assert d_thr[0] == S_NQ and lo <= d_thr[1] <= hi, (d_thr, lo, hi)
        assert d_auto == (d_thr if S.auto_is_thresholded(S_NQ, k, lens, S_NPROBE if ivf else 1) else (0, 0))
        if ivf and k > 66:
            assert (dense[1][0, 66:] == -1).all() and (dense[1][0, :66] >= 0).all() and (dense[1][2, 1:] == -1).all()


# ---- 3. one case each: filter, both exclusion routes, refine ------------------------------------------------------------
E_N, E_D, E_NQ, E_NLIST, E_NPROBE, E_DSUB, E_ITER = 6000, 64, 70, 8, 3, 8, 2


@pytest.fixture(scope="module")
def trained_case():
    """an IVF index trained on unit rows, vectors attached; the decoded matrix from the restatement"""
    from recommendit_amd import PQIndex
    X, Q = R.unit_rows(31, E_N, E_D), R.unit_rows(32, E_NQ, E_D)
    Cc, assign = R.ivf_layout(33, E_N, E_D, E_NLIST)
    ids = np.arange(E_N) + 1000
    src = _ivf(X, Cc, assign, E_NPROBE, ids=ids)
    pq = PQIndex.from_index(src, dsub=E_DSUB, n_iter=E_ITER, keep_vectors=True)
    m_, s_ = S.train_quantizer(X)
    book, codes, trace = P.train(P.pad_codes(S.encode(X, m_, s_), 64), E_DSUB, E_ITER)
    dec = P.decode(codes, book)[:, :E_D]
    np.testing.assert_array_equal(pq.codes(), dec)
    probed = R.probe_mask(Q, Cc, assign, E_NPROBE)
    ex = _Expect(Q, dec, m_, s_, [200], allowed=probed)
    return dict(pq=pq, src=src, X=X, Q=Q, qd=torch.from_numpy(Q).cuda(), ids=ids, m=m_, s=s_, dec=dec, probed=probed, ex=ex,
                assign=assign, Cc=Cc)


def _restricted(case, k, ok):
    return S.topk_fast(case["ex"].Sc, k, case["probed"] & ok)


def test_tag_filter_inside_the_pq_scan(trained_case):
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


def _seen_of(case, k):
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


def test_seen_items_excluded_inside_the_pq_scan(trained_case):
    c, k = trained_case, 20
    store, seen = _seen_of(c, k)
    rows, sc = _restricted(c, k, ~seen)
    assert (rows != c["ex"].rows[:, :k]).any()
    for mode in MODES:
        s_, i_, n_ = c["pq"].batch_search_device(c["qd"], k=k, normalized=True, mode=mode, exclude=store,
                                                 user_ids=list(range(E_NQ)), exclusion="scan", return_int=True)
        c["ex"].check((s_.cpu().numpy(), i_.cpu().numpy(), n_.cpu().numpy()), k, rows, sc, id_of=c["ids"])


def test_seen_items_excluded_by_over_fetch(trained_case):
    c, k = trained_case, 20
    store, seen = _seen_of(c, k)
    rows, sc = _restricted(c, k, ~seen)
    s_, i_ = c["pq"].batch_search_device(c["qd"], k=k, normalized=True, exclude=store, user_ids=list(range(E_NQ)))
    c["ex"].check((s_.cpu().numpy(), i_.cpu().numpy(), None), k, rows, sc, id_of=c["ids"])
    assert c["pq"].exclusion_deficit() == 0


def test_refined_search_and_certificate_over_the_decoded_matrix(trained_case):
    c, k = trained_case, 10
    pq = c["pq"]
    assert pq.has_vectors
    ea = R.ranges(c["X"], c["dec"], c["m"], c["s"])
    e, a = pq.refine_ranges()
    np.testing.assert_array_equal(e, ea[0])
    np.testing.assert_array_equal(a, ea[1])
    want = R.refine(c["Q"], c["X"], c["dec"], c["m"], c["s"], k, 2 * k, c["probed"], ea)
    assert (want["rows"] >= 0).all()
    print("certified by the reference:", int(want["cert"].sum()), "of", E_NQ)
    for mode in ("dense", "thresholded"):
        gs, gr, gc, gb = [t.cpu().numpy() for t in pq.search_rows_device(c["qd"], k, mode=mode, refine=2, return_cert=True)]
        np.testing.assert_array_equal(gr, want["rows"])
        np.testing.assert_array_equal(gs.view(np.uint32), want["scores"].view(np.uint32))
        np.testing.assert_array_equal(gc, want["cert"])
        np.testing.assert_allclose(gb, want["bound"], rtol=1e-12, atol=0)
    # the certificate's other branch: k_scan beyond every query's probed rows, so stage 1 returns them all and the
    # re-ranked list is the exact one (the decode error of a product quantiser is too large for the bound to certify above)
    k_scan = 4096
    assert c["probed"].sum(axis=1).max() < k_scan
    want = R.refine(c["Q"], c["X"], c["dec"], c["m"], c["s"], k, k_scan, c["probed"], ea)
    assert (want["cert"] == 1).all()
    br, bs = R.brute_force(c["Q"], c["X"], k, c["probed"])
    np.testing.assert_array_equal(want["rows"], br)
    gs, gr, gc, gb = [t.cpu().numpy() for t in pq.search_rows_device(c["qd"], k, refine=k_scan / k, return_cert=True)]
    np.testing.assert_array_equal(gr, br)
    assert gs.tobytes() == bs.tobytes() and (gc == 1).all()


# ---- 4. persistence and refusals -----------------------------------------------------------------------------------------
def test_save_load_save_and_the_refusals(trained_case, tmp_path):
    from recommendit_amd import PQIndex, SQ8Index
    c, k = trained_case, 15
    pq = c["pq"]
    want = [t.cpu().numpy() for t in pq.batch_search_device(c["qd"], k=k, normalized=True, return_int=True)]
    c["ex"].check(want, k, id_of=c["ids"])
    p1, p2, p3 = tmp_path / "a.pq", tmp_path / "b.pq", tmp_path / "c.sq8"
    pq.save(str(p1))
    back = PQIndex.load(str(p1))
    back.save(str(p2))
    assert p1.read_bytes() == p2.read_bytes() and p1.read_bytes()[:8] == b"RIHIPPQ1"
    assert isinstance(back, PQIndex) and back.dsub == E_DSUB and back.n_probe == E_NPROBE
    _same_bytes(want, [t.cpu().numpy() for t in back.batch_search_device(c["qd"], k=k, normalized=True, return_int=True)])
    np.testing.assert_array_equal(back.pq_codes(), pq.pq_codes())
    assert back.train_stats()["distortion"].size == 0
    # each loader refuses the other's file
    with pytest.raises(RuntimeError, match="not an SQ8 index file"):
        SQ8Index.load(str(p1))
    sq = SQ8Index.from_index(c["src"])
    sq.save(str(p3))
    with pytest.raises(RuntimeError, match="not a PQ index file"):
        PQIndex.load(str(p3))
    from recommendit_amd import _lib as L
    assert L.lib().rihip_sq8_index_save(pq.index._h, str(tmp_path / "d.sq8").encode()) != 0       # the SQ8 writer, too
    assert b"rihip_pq_index_save" in L.lib().rihip_last_error() and not (tmp_path / "d.sq8").exists()
    # no live updates: the three calls raise, so does the C entry point under them, and nothing changes
    x = c["X"][:2].copy()
    for call in (lambda: pq.add_items(x, [1, 2]), lambda: pq.remove_items([1000]), lambda: pq.update_items(x, [1000, 5])):
        with pytest.raises(NotImplementedError, match="rebuild"):
            call()
    with pytest.raises(RuntimeError, match="not updated in place"):
        SQ8Index.remove_items(pq, [1000])
    assert pq.index.ntotal == E_N
    _same_bytes(want, [t.cpu().numpy() for t in pq.batch_search_device(c["qd"], k=k, normalized=True, return_int=True)])


def test_the_loader_refuses_a_damaged_file_field_by_field(trained_case, tmp_path):
    """as test_gpu_sq8_index.py's refusals, over the PQ format: ten header words, one more payload block"""
    from recommendit_amd import PQIndex
    from recommendit_amd._lib import RihipError
    p = tmp_path / "a.pq"
    trained_case["pq"].save(str(p))
    raw = p.read_bytes()
    meta = p.with_suffix(".meta.pkl").read_bytes()
    assert isinstance(PQIndex.load(str(p)), PQIndex)           # the undamaged file loads

    def try_load(name, data):
        f = tmp_path / name
        f.write_bytes(data)
        f.with_suffix(".meta.pkl").write_bytes(meta)
        with pytest.raises(RihipError):
            PQIndex.load(str(f))

    try_load("short_header.pq", raw[:40])
    try_load("truncated.pq", raw[:len(raw) // 2])
    hdr = np.frombuffer(raw[8:88], dtype=np.int64)
    dk, dpad, Np, nlist, M = (int(hdr[i]) for i in (2, 3, 5, 6, 9))
    assert hdr.tolist() == [1, E_D, 64, 64, E_N, Np, E_NLIST, E_NPROBE, E_DSUB, 64 // E_DSUB]
    for field, value in ((0, 2), (1, 200), (2, 96), (3, 32), (4, -5), (4, 2 ** 40), (5, hdr[5] + 6400), (6, 0), (6, 10 ** 6), (7, 0),
                         (8, 12), (9, hdr[9] + 1)):
        h2 = hdr.copy()
        h2[field] = value
        try_load(f"field{field}_{abs(int(value))}.pq", raw[:8] + h2.tobytes() + raw[88:])
    lens_at = 88 + 8 * dpad + 4 * nlist * dk                   # list lengths: behind quantiser and centroids
    ll = np.frombuffer(raw[lens_at:lens_at + 8 * nlist], dtype=np.int64).copy()
    assert ll.sum() == E_N
    ll[0] += 1
    try_load("lists.pq", raw[:lens_at] + ll.tobytes() + raw[lens_at + 8 * nlist:])
    book_at = lens_at + 8 * nlist + 8 * Np                     # codebooks: behind list lengths and row ids
    assert len(raw) == book_at + 256 * dpad + Np * M
    try_load("book.pq", raw[:book_at + 5] + b"\x80" + raw[book_at + 6:])


# ---- 5. serving ------------------------------------------------------------------------------------------------------------
def test_pipeline_over_a_pq_index_equals_its_stages_run_by_hand(tmp_path):
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
    pq = PQIndex.from_index(src, dsub=16, n_iter=2)
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
    pipe = GpuRecommendationPipeline(model, pq, ranker, store, top_k_candidates=kc, top_k_results=k)
    users = [1, 7, 120, 42, 3]
    ids, sc, rs = pipe.recommend_batch(users)
    uid = torch.tensor(users, dtype=torch.long, device="cuda")
    q = model.get_user_embeddings(uid, as_tensor=True)
    r_s, cand = pq.batch_search_device(q, k=kc, normalized=True)
    assert (cand >= 0).any()
    Xf = build_ranking_features_device(store, uid, cand, ranker.feature_names)
    scores = ranker.predict_device(Xf)
    h_ids = torch.empty((len(users), k), dtype=torch.int64, device="cuda")
    h_top = torch.empty((len(users), k), dtype=torch.float64, device="cuda")
    h_rs = torch.empty((len(users), k), dtype=torch.float32, device="cuda")
    L.check(L.lib().rihip_rank_topk(scores.data_ptr(), cand.data_ptr(), r_s.data_ptr(), len(users), kc, k, h_ids.data_ptr(),
                                    h_top.data_ptr(), h_rs.data_ptr(), L.stream_ptr()), "rank_topk")
    torch.cuda.synchronize()
    assert torch.equal(ids, h_ids) and torch.equal(sc, h_top) and torch.equal(rs, h_rs)
