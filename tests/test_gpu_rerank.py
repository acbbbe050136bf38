"""GPU: the diversified top-k (csrc/rerank.hip, greedy MMR) -- the kernel against the sequential NumPy reference of its
definition (tests/mmr_reference.py; ids exact, scores bit for bit), against rihip_rank_topk at diversity 0, its status
codes, the serving pipeline (eager, hipGraph, seen store, item filter, caller's vectors) and the stand-alone entry."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmr_reference as M  # noqa: E402
from oracle import fixtures as fx  # noqa: E402
from oracle import gbdt_np as G  # noqa: E402

pytestmark = pytest.mark.gpu

DELTAS = (0.0, 0.3, 0.7, 1.0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _kernel(s, c, r, k, delta, Vd, n_rows, ld, col0, w):
    from recommendit_amd import _lib as L
    nq, kc = c.shape
    sd, cd, rd = _dev(s), _dev(c), _dev(r)
    ids = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    top = torch.full((nq, k), 7.0, dtype=torch.float64, device="cuda")
    trs = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    L.check(L.lib().rihip_rank_topk_diverse(sd.data_ptr(), cd.data_ptr(), rd.data_ptr(), nq, kc, k, Vd.data_ptr(), n_rows,
                                            ld, col0, w, delta, ids.data_ptr(), top.data_ptr(), trs.data_ptr(),
                                            L.stream_ptr()), "rank_topk_diverse")
    torch.cuda.synchronize()
    return ids.cpu().numpy(), top.cpu().numpy(), trs.cpu().numpy()


def _assert_same(got, exp, what=""):
    assert np.array_equal(got[0], exp[0]), (what, np.argwhere(got[0] != exp[0])[:5])
    assert np.array_equal(_bits(got[1]), _bits(exp[1])), what
    assert np.array_equal(_bits(got[2]), _bits(exp[2])), what


def _mixed_case(seed, nq, kc, k, w):
    """a strided table (ld > w, col0 > 0) with zero rows and duplicated vectors; scores with repeats, signed zeros,
    NaN and infinities; padding inside rows and as tails, ids beyond the table; one row of all-equal scores and one
    with fewer eligible candidates than k (when the batch has the rows for them)"""
    rng = np.random.default_rng(seed)
    n_rows, col0, ld = kc + 40, 3, w + 5
    V = np.full((n_rows, ld), 9.0)
    V[:, col0:col0 + w] = rng.standard_normal((n_rows, w)) * (rng.random((n_rows, w)) < 0.5)
    if w == 18:
        V[: n_rows // 2, col0:col0 + w] = (rng.random((n_rows // 2, w)) < 0.15)      # binary genre rows: many exact ties
    V[::7, col0:col0 + w] = 0.0
    V[3::11, col0:col0 + w] = V[5, col0:col0 + w]
    s = np.round(rng.standard_normal((nq, kc)), 1)
    for p, v in ((0.05, np.nan), (0.03, -0.0), (0.03, 0.0), (0.01, np.inf), (0.01, -np.inf)):
        s[rng.random((nq, kc)) < p] = v
    c = np.stack([rng.permutation(n_rows + 20)[:kc] for _ in range(nq)]).astype(np.int64)     # ids >= n_rows among them
    c[rng.random((nq, kc)) < 0.06] = -1
    for q in range(nq):
        if q % 2 and kc > 4:
            c[q, kc - (q % 5) - 1:] = -1
    if nq > 1:
        s[1, :] = 0.25                                  # all equal: relevance 0 for everyone
    if nq > 2 and kc > 8:
        c[2, 5:] = -1                                   # fewer eligible candidates than k
        s[2, 1] = np.nan
    r = rng.standard_normal((nq, kc)).astype(np.float32)
    return s, c, r, V, n_rows, ld, col0


SHAPES = [(3, 1, 1, 18), (5, 63, 20, 18), (4, 64, 64, 18), (7, 65, 20, 18), (6, 257, 20, 18), (3, 500, 20, 18),
          (2, 1000, 50, 128), (1, 4096, 20, 18), (3, 10, 25, 18)]          # the last one: k > kc


# ---- 1. kernel against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,kc,k,w", SHAPES)
def test_kernel_matches_reference(nq, kc, k, w):
    s, c, r, V, n_rows, ld, col0 = _mixed_case(100 + kc + w, nq, kc, k, w)
    Vd = _dev(V)
    for delta in DELTAS:
        exp = M.mmr_reference(s, c, r, k, delta, V, col0, w)
        _assert_same(_kernel(s, c, r, k, delta, Vd, n_rows, ld, col0, w), exp, f"delta={delta}")
    if kc >= 63:                                        # the inputs do what they are meant to: diversity changes lists
        assert not np.array_equal(M.mmr_reference(s, c, r, k, 0.7, V, col0, w)[0], M.plain_topk(s, c, r, k)[0])


def test_kernel_reads_vectors_from_the_table_when_lds_cannot_hold_them(monkeypatch):
    """the same answers with the candidates' vectors left in the table (the path of shapes too large for LDS) as with
    them staged in LDS"""
    s, c, r, V, n_rows, ld, col0 = _mixed_case(7, 4, 300, 20, 18)
    Vd = _dev(V)
    exp = M.mmr_reference(s, c, r, 20, 0.5, V, col0, 18)
    _assert_same(_kernel(s, c, r, 20, 0.5, Vd, n_rows, ld, col0, 18), exp, "staged")
    monkeypatch.setenv("RIHIP_RERANK_STAGE", "0")
    _assert_same(_kernel(s, c, r, 20, 0.5, Vd, n_rows, ld, col0, 18), exp, "table")


# ---- 2. diversity 0 is rihip_rank_topk ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", [64, 500])
def test_delta_zero_equals_rank_topk(kc):
    from recommendit_amd import _lib as L
    rng = np.random.default_rng(kc)
    nq, k = 9, 20
    s = np.round(rng.standard_normal((nq, kc)), 1)                 # many repeats
    s[rng.random((nq, kc)) < 0.1] = -0.0
    s[rng.random((nq, kc)) < 0.1] = 0.0
    s[0, :] = np.where(rng.random(kc) < 0.5, 0.0, -0.0)            # nothing but signed zeros
    s[1, : kc // 2] = 1.0
    s[1, kc // 2:] = np.nextafter(1.0, 2.0)                        # neighbours that normalise to 0 and 1
    s[2] = 1e300 + s[2]                                             # a span that swallows differences
    s[2, 0] = -1e300
    c = np.stack([rng.permutation(kc + 30)[:kc] for _ in range(nq)]).astype(np.int64)
    c[3, kc - 9:] = -1
    c[4, ::5] = -1
    r = rng.standard_normal((nq, kc)).astype(np.float32)
    V = rng.standard_normal((kc + 10, 18))
    sd, cd, rd = _dev(s), _dev(c), _dev(r)
    ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    top = torch.empty((nq, k), dtype=torch.float64, device="cuda")
    trs = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    L.check(L.lib().rihip_rank_topk(sd.data_ptr(), cd.data_ptr(), rd.data_ptr(), nq, kc, k, ids.data_ptr(), top.data_ptr(),
                                    trs.data_ptr(), L.stream_ptr()), "rank_topk")
    torch.cuda.synchronize()
    plain = (ids.cpu().numpy(), top.cpu().numpy(), trs.cpu().numpy())
    _assert_same(_kernel(s, c, r, k, 0.0, _dev(V), V.shape[0], 18, 0, 18), plain)
    _assert_same(M.plain_topk(s, c, r, k), plain)


# ---- 3. determinism ---------------------------------------------------------------------------------------------------
def test_two_launches_are_bitwise_equal():
    s, c, r, V, n_rows, ld, col0 = _mixed_case(11, 16, 500, 20, 18)
    Vd = _dev(V)
    a = _kernel(s, c, r, 20, 0.3, Vd, n_rows, ld, col0, 18)
    b = _kernel(s, c, r, 20, 0.3, Vd, n_rows, ld, col0, 18)
    _assert_same(a, b)


# ---- 4. status codes ----------------------------------------------------------------------------------------------------
def test_status_codes():
    from recommendit_amd import _lib as L
    lib = L.lib()
    z = torch.zeros((8, 64), dtype=torch.float64, device="cuda")
    zi = torch.zeros((8, 64), dtype=torch.int64, device="cuda")
    zf = torch.zeros((8, 64), dtype=torch.float32, device="cuda")
    V = torch.zeros((10, 256), dtype=torch.float64, device="cuda")
    oi = torch.full((8, 64), -7, dtype=torch.int64, device="cuda")
    od = torch.zeros((8, 64), dtype=torch.float64, device="cuda")
    of = torch.zeros((8, 64), dtype=torch.float32, device="cuda")

    def call(nq=2, kc=8, k=4, ld=256, col0=0, w=18, d=0.5, n_rows=10, null=None):
        p = [z.data_ptr(), zi.data_ptr(), zf.data_ptr(), V.data_ptr(), oi.data_ptr(), od.data_ptr(), of.data_ptr()]
        if null is not None:
            p[null] = None
        return lib.rihip_rank_topk_diverse(p[0], p[1], p[2], nq, kc, k, p[3], n_rows, ld, col0, w, d, p[4], p[5], p[6],
                                           L.stream_ptr())
    assert call() == 0 and call(nq=0) == 0 and call(d=0.0) == 0 and call(d=1.0) == 0 and call(w=256) == 0
    assert call(k=64) == 0 and call(n_rows=0) == 0
    torch.cuda.synchronize()
    oi.fill_(-7)
    bad = [dict(kc=0), dict(kc=4097), dict(k=0), dict(k=-1), dict(w=0), dict(w=257), dict(d=-1e-9), dict(d=1.0000001),
           dict(d=float("nan")), dict(d=float("inf")), dict(nq=-1), dict(col0=-1), dict(col0=250, w=18), dict(ld=17),
           dict(n_rows=-1)] + [dict(null=i) for i in range(7)]
    for kw in bad:
        assert call(**kw) == 1, kw                                  # RIHIP_ERR_ARG
        assert b"rank_topk_diverse" in lib.rihip_last_error(), kw
    torch.cuda.synchronize()
    assert (oi == -7).all()                                         # nothing was launched


# ---- 5. the serving pipeline --------------------------------------------------------------------------------------------
NU, NI, D, KC = 300, 6000, 64, 200


@pytest.fixture(scope="module")
def parts(tmp_path_factory):
    """model, exact index, ranker and feature store of a small catalogue (the set-up of tests/test_gpu_exclude.py)"""
    from recommendit_amd import FAISSIndex, LightGBMRanker, TwoTowerModel
    from recommendit_amd.recommender import GpuFeatureStore, feature_columns
    sd = fx.make_state(NU, NI, D, 128, seed=21)
    model = TwoTowerModel(NU, NI, D, 128)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    rng = np.random.RandomState(2)
    item_ids = list(range(1, NI + 1))
    genres = (rng.rand(NI, 18) < 0.15).astype(np.float32)
    E = model.get_item_embeddings(item_ids, genres)
    index = FAISSIndex(embed_dim=D, exact=True)
    index.build_ivf_index(E, item_ids)
    forest = G.random_forest_model(60, 31, 50, seed=5, names=feature_columns())
    p = tmp_path_factory.mktemp("rerank") / "r.lgbm"
    p.write_text(G.write_text_model(forest))
    ranker = LightGBMRanker.load(str(p))
    store = GpuFeatureStore(NU, NI)
    ut = store.user.copy(); it = store.item.copy()
    ut[1:, :6] = rng.rand(NU, 6) * [5, 8, 1, 1, 1, 1]; ut[1:, 6:] = rng.rand(NU, 18)
    it[1:, :5] = rng.rand(NI, 5) * [5, 9, 1, 1.5, 1]; it[1:, 5:] = genres
    store.load_arrays(ut, it)
    return dict(model=model, index=index, ranker=ranker, store=store, item=it, item_ids=item_ids)


def _pipe(parts, **kw):
    from recommendit_amd.recommender import GpuRecommendationPipeline
    return GpuRecommendationPipeline(parts["model"], parts["index"], parts["ranker"], parts["store"], top_k_candidates=KC,
                                     top_k_results=20, **kw)


def _host(out):
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


UIDS = list(range(1, 49))


def _expected(full, delta, V, col0, w, k=20):
    """the reference on a chain's own k = all-candidates output: `full` is in (score desc, position asc) order, so a
    tie in the objective resolves in it as it does in retrieval order"""
    ids, sc, rs = full
    return M.mmr_reference(sc, ids, rs, k, delta, V, col0, w)


def test_pipeline_matches_reference_and_none_is_unchanged(parts):
    pipe = _pipe(parts)
    full = _host(pipe.recommend_batch(UIDS, k=KC))
    plain = _host(pipe.recommend_batch(UIDS, k=20))
    _assert_same(plain, tuple(a[:, :20] for a in full))
    _assert_same(_host(pipe.recommend_batch(UIDS, k=20, diversity=None)), plain)
    for delta in (0.3, 1.0):
        exp = _expected(full, delta, parts["item"], 5, 18)
        assert not np.array_equal(exp[0], plain[0])
        _assert_same(_host(pipe.recommend_batch(UIDS, k=20, diversity=delta)), exp, f"delta={delta}")
    _assert_same(_host(pipe.recommend_batch(UIDS, k=20, diversity=0.0)), plain)
    # the constructor's value is the default of every call; None turns it off for one
    tuned = _pipe(parts, diversity=0.3)
    exp = _expected(full, 0.3, parts["item"], 5, 18)
    _assert_same(_host(tuned.recommend_batch(UIDS, k=20)), exp)
    _assert_same(_host(tuned.recommend_batch(UIDS, k=20, diversity=None)), plain)
    one = tuned.get_recommendations(UIDS[3], k=20)
    assert [d["item_id"] for d in one] == exp[0][3].tolist() and [d["rank"] for d in one] == list(range(1, 21))
    assert [d["item_id"] for d in tuned.get_recommendations(UIDS[3], k=20, diversity=None)] == plain[0][3].tolist()


def test_pipeline_value_errors(parts):
    pipe = _pipe(parts)
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            pipe.recommend_batch(UIDS, k=20, diversity=bad)
    with pytest.raises(ValueError):
        pipe.recommend_batch(UIDS, k=-2, diversity=0.3)
    from recommendit_amd.recommender import GpuRecommendationPipeline
    wide = GpuRecommendationPipeline(parts["model"], parts["index"], parts["ranker"], parts["store"],
                                     top_k_candidates=5000, diversity=0.3)
    with pytest.raises(ValueError, match="4096"):
        wide.recommend_batch(UIDS, k=20)
    with pytest.raises(ValueError):
        _pipe(parts, diversity=0.3, diversity_vectors=torch.zeros((NI + 1, 300), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        _pipe(parts, diversity_vectors=torch.zeros((NI + 1, 8), dtype=torch.float64)).recommend_batch(UIDS, diversity=0.3)


@pytest.mark.parametrize("nq", [1, 48])
def test_pipeline_graph_equals_eager(parts, nq):
    pipe = _pipe(parts)
    uids = UIDS[:nq]
    eager = {d: _host(pipe.recommend_batch(uids, k=20, diversity=d)) for d in (None, 0.3, 0.8)}
    assert not np.array_equal(eager[0.3][0], eager[0.8][0]) and not np.array_equal(eager[0.3][0], eager[None][0])
    for d in (0.3, 0.8, 0.3, None, 0.8):                 # back and forth: a replay never returns another weight's list
        _assert_same(_host(pipe.recommend_batch(uids, k=20, graph=True, diversity=d)), eager[d], f"graph, {d}")
    first = _host(pipe.recommend_batch(uids, k=20, graph=True, diversity=0.3))
    _assert_same(_host(pipe.recommend_batch(uids, k=20, graph=True, diversity=0.3)), first)
    keys = {key[3]: ent for key, ent in pipe._graphs.items() if key[0] == nq}
    assert set(keys) == {None, 0.3, 0.8} and all(ent is not False for ent in keys.values())     # captured, not eager
    other = [u + 100 for u in uids]
    _assert_same(_host(pipe.recommend_batch(other, k=20, graph=True, diversity=0.3)),
                 _host(pipe.recommend_batch(other, k=20, diversity=0.3)))


def test_pipeline_graph_sees_new_vectors(parts):
    """the vector table is part of the graph's state: other vectors never replay the graph of the old ones"""
    rng = np.random.default_rng(4)
    T1, T2 = (_dev(rng.standard_normal((NI + 1, 32))) for _ in range(2))
    pipe = _pipe(parts, diversity=0.6, diversity_vectors=T1)
    uids = UIDS[:4]
    a = _host(pipe.recommend_batch(uids, k=20, graph=True))
    _assert_same(a, _host(pipe.recommend_batch(uids, k=20)))
    pipe.diversity_vectors = T2
    b = _host(pipe.recommend_batch(uids, k=20, graph=True))
    _assert_same(b, _host(pipe.recommend_batch(uids, k=20)))
    assert not np.array_equal(a[0], b[0])


def test_pipeline_with_seen_store(parts):
    from recommendit_amd import SeenItems
    plain = _pipe(parts)
    head = _host(plain.recommend_batch(UIDS, k=60))[0]
    users = np.repeat(np.asarray(UIDS), 15)
    seen = SeenItems.from_pairs(users, head[:, ::3][:, :15].reshape(-1))      # items the plain chain would have served
    pipe = _pipe(parts, seen=seen)
    full = _host(pipe.recommend_batch(UIDS, k=KC))
    assert not any(np.isin(full[0][q], seen.items_of(u)).any() for q, u in enumerate(UIDS))
    exp = _expected(full, 0.3, parts["item"], 5, 18)
    got = _host(pipe.recommend_batch(UIDS, k=20, diversity=0.3))
    _assert_same(got, exp)
    assert not np.array_equal(got[0], full[0][:, :20])


def test_pipeline_with_item_filter(parts):
    pipe = _pipe(parts)
    idx, store = parts["index"], parts["store"]
    idx.set_item_tags(store.item_genre_tags(parts["item_ids"]))
    flt = (0b1111, 0, 1 << 7)                          # any of genres 0-3, not genre 7
    full = _host(pipe.recommend_batch(UIDS, k=KC, item_filter=flt))
    tags = store.item_genre_tags(full[0].reshape(-1)).reshape(full[0].shape)
    assert (((tags & 0b1111) != 0) & ((tags & (1 << 7)) == 0))[full[0] >= 0].all()
    exp = _expected(full, 0.3, parts["item"], 5, 18)
    got = _host(pipe.recommend_batch(UIDS, k=20, item_filter=flt, diversity=0.3))
    _assert_same(got, exp)
    assert not np.array_equal(got[0], full[0][:, :20])


def test_pipeline_with_callers_vectors(parts):
    rng = np.random.default_rng(9)
    T = rng.standard_normal((NI + 1, 32))
    pipe = _pipe(parts, diversity_vectors=_dev(T))
    full = _host(pipe.recommend_batch(UIDS, k=KC))
    got = _host(pipe.recommend_batch(UIDS, k=20, diversity=0.3))
    _assert_same(got, _expected(full, 0.3, T, 0, 32))
    assert not np.array_equal(got[0], _expected(full, 0.3, parts["item"], 5, 18)[0])


# ---- 6. the stand-alone entry -----------------------------------------------------------------------------------------
def test_standalone_equals_the_kernel_call():
    from recommendit_amd import mmr_rerank_device
    s, c, r, V, n_rows, ld, col0 = _mixed_case(5, 6, 130, 20, 18)
    Vd = _dev(V)
    exp = _kernel(s, c, r, 20, 0.4, Vd, n_rows, ld, col0, 18)
    got = mmr_rerank_device(_dev(s), _dev(c), _dev(r), 20, 0.4, Vd, col0=col0, width=18)
    _assert_same(_host(got), exp)
    _assert_same(exp, M.mmr_reference(s, c, r, 20, 0.4, V, col0, 18))
    sub = Vd[:, col0:col0 + 18]                          # a view with a row stride: every column of it
    _assert_same(_host(mmr_rerank_device(_dev(s), _dev(c), _dev(r), 20, 0.4, sub)), exp)
    with pytest.raises(ValueError):
        mmr_rerank_device(_dev(s), _dev(c), _dev(r), 20, 0.4, torch.from_numpy(V))       # host vectors
