"""Host: the 8-bit scalar quantiser -- invariants of its NumPy reference (tests/sq8_reference.py), the argument checks of
SQ8Index that need no device, and the C ABI's declarations."""
import os
import pickle
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_reference as S  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
ABI = ["from_ip_index", "destroy", "ntotal", "nlist", "set_nprobe", "set_id_map", "get_quantizer", "get_codes", "reconstruct",
       "encode_queries", "search", "stats", "save", "load"]


def _rows(seed, n, d):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32) * rng.uniform(0.01, 3.0, d).astype(np.float32)
    X[:, 3] = 0.25          # a constant column
    X[::7, 5] *= 40.0       # a column with outliers
    return X


@pytest.mark.parametrize("d", [16, 50, 128])
def test_reconstruction_error_inside_the_trained_range(d):
    X = _rows(1, 500, d)
    m, s = S.train_quantizer(X)
    assert m.dtype == np.float32 and s.dtype == np.float32
    assert s[3] == 1.0 and m[3] == np.float32(0.25)
    c = S.encode(X, m, s)
    assert c.dtype == np.int8 and c.min() >= -127 and c.max() <= 127
    assert (c[:, 3] == 0).all()
    assert np.abs(c).max(axis=0)[np.arange(d) != 3].min() >= 126       # every trained column uses its whole range
    xh = S.decode(c, m, s).astype(np.float64)
    bound = s.astype(np.float64)[None, :] * (0.5 + 2.0 ** -16)
    assert (np.abs(X.astype(np.float64) - xh) <= bound).all()


def test_clamp_outside_injected_ranges():
    X = _rows(2, 64, 16)
    m = np.zeros(16, np.float32)
    s = np.full(16, 1e-3, np.float32)
    c = S.encode(X, m, s)
    big = np.abs(X) > 0.2
    assert big.any() and (np.abs(c[big]) == 127).all() and (np.sign(c[big]) == np.sign(X[big])).all()


@pytest.mark.parametrize("d", [1, 64, 128])
def test_query_limbs_recombine_and_fit_int8(d):
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((40, d)).astype(np.float32)
    Q[5] = 0.0                                        # A == 0: t = 0 and every limb 0
    Q[6, 1:] = 0.0                                    # one non-zero component
    m = rng.standard_normal(d).astype(np.float32)
    s = rng.uniform(1e-3, 0.1, d).astype(np.float32)
    n, t, b = S.encode_queries(Q, m, s)
    assert n.dtype == np.int32 and t.dtype == np.float32 and b.dtype == np.float64
    assert np.abs(n).max() == S.QMAX and t[5] == 0 and (n[5] == 0).all() and b[5] == 0
    assert abs(n[6, 0]) == S.QMAX
    hi, lo = S.limbs(n)
    assert (256 * hi + lo == n).all()
    assert hi.min() >= -127 and hi.max() <= 127 and lo.min() >= -128 and lo.max() <= 127
    every = np.arange(-S.QMAX, S.QMAX + 1)
    h2, l2 = S.limbs(every)
    assert (256 * h2 + l2 == every).all() and np.abs(h2).max() == 127 and l2.min() == -128 and l2.max() == 127
    np.testing.assert_allclose(b, Q.astype(np.float64) @ m.astype(np.float64), rtol=0, atol=1e-12)


def test_integer_score_bound_at_128():
    n = np.full((1, 128), S.QMAX, dtype=np.int32)
    c = np.full((2, 128), 127, dtype=np.int8)
    c[1] = -127
    Sc = S.int_scores(n, c)
    assert Sc[0, 0] == 32512 * 127 * 128 == -Sc[0, 1] and Sc[0, 0] < 2 ** 31
    hi, lo = S.limbs(n)                               # the two chains the kernel accumulates, each inside int32
    assert abs(int(S.int_scores(hi, c)[0, 0])) * 256 < 2 ** 31 and abs(int(S.int_scores(lo, c)[0, 0])) < 2 ** 31


def test_topk_orders_ties_by_row_and_pads():
    Sc = np.array([[5, 9, 5, 9, -3]], dtype=np.int64)
    rows, sc = S.topk(Sc, 7)
    assert rows[0].tolist() == [1, 3, 0, 2, 4, -1, -1] and sc[0, :5].tolist() == [9, 9, 5, 5, -3]
    rows, _ = S.topk(Sc, 2, allowed=np.array([[True, False, True, False, True]]))
    assert rows[0].tolist() == [0, 2]
    assert S.probed_lists(np.array([[1.0, 0.0]]), np.array([[0.5, 0.0], [1.0, 0.0], [1.0, 9.0]]), 2)[0].tolist() == [1, 2]


def test_header_declares_and_binding_holds_the_sq8_abi():
    from recommendit_amd import _lib
    txt = (ROOT / "include" / "recommendit_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(rihip_sq8_index_\w+)\s*\(", txt))
    want = {f"rihip_sq8_index_{n}" for n in ABI}
    assert declared == want
    assert want <= set(_lib.SIGNATURES)
    assert re.search(r"#define\s+RIHIP_ABI_VERSION\s+1\b", txt)
    res, args = _lib.SIGNATURES["rihip_sq8_index_search"]
    assert len(args) == 9


def test_sq8index_argument_validation_without_a_device(tmp_path):
    import torch
    from recommendit_amd import FAISSIndex, SQ8Index
    from recommendit_amd.recommender import GpuRecommendationPipeline
    with pytest.raises(ValueError, match="embed_dim"):
        SQ8Index(embed_dim=129)
    with pytest.raises(ValueError, match="embed_dim"):
        SQ8Index(embed_dim=0)
    sq = SQ8Index(embed_dim=32)
    assert sq.stats() == {"status": "not built"}
    for call in (lambda: sq.search(np.zeros(32, np.float32)), lambda: sq.batch_search(np.zeros((2, 32), np.float32)),
                 lambda: sq.batch_search_device(torch.zeros((2, 32))), sq.codes, sq.reconstruct, sq.quantizer,
                 lambda: sq.save(str(tmp_path / "x.sq8"))):
        with pytest.raises(RuntimeError, match="not built"):
            call()
    with pytest.raises(ValueError, match="FAISSIndex"):
        SQ8Index.from_index(object())
    with pytest.raises(RuntimeError, match="not built"):
        SQ8Index.from_index(FAISSIndex(embed_dim=32))
    with pytest.raises(ValueError, match="n_probe"):
        sq.set_n_probe(0)
    sq.set_n_probe(7)
    assert sq.n_probe == 7
    with pytest.raises(FileNotFoundError):
        SQ8Index.load(str(tmp_path / "missing.sq8"))
    # the serve chain's calls on an index without a pending state
    assert sq.finish_search() == 0 and sq.search_pending() is False and sq.last_fail_count() == 0
    assert sq.exclusion_deficit() == 0
    # options the SQ8 chain does not serve are refused by name, before anything runs
    with pytest.raises(ValueError, match="SQ8"):
        GpuRecommendationPipeline(None, sq, None, None, diversity=0.2)
    pipe = GpuRecommendationPipeline(None, sq, None, None)
    with pytest.raises(ValueError, match="SQ8"):
        pipe.recommend_batch([1], graph=True)
    with pytest.raises(ValueError, match="SQ8"):
        pipe.recommend_batch([1], item_filter=(1, 0, 0))
    with pytest.raises(ValueError, match="SQ8"):
        pipe.recommend_batch([1], diversity=0.3)
    with pytest.raises(ValueError, match="SQ8"):
        pipe.recommend_batch([1], exclude_seen=True)
    with pytest.raises(ValueError, match="SQ8"):
        pipe.recommend_cold_batch(None)


def test_meta_sidecar_keys_match_faissindex(tmp_path, monkeypatch):
    """save() writes FAISSIndex's sidecar keys (the library call is stubbed: no device here)"""
    from recommendit_amd import SQ8Index
    from recommendit_amd import sq8_index as M

    class _Lib:
        def rihip_sq8_index_save(self, h, path):
            Path(path.decode()).write_bytes(b"RIHIPSQ8")
            return 0

        def rihip_sq8_index_destroy(self, h):
            return 0
    monkeypatch.setattr(M.L, "lib", lambda: _Lib())
    sq = SQ8Index(embed_dim=16, n_lists=4, n_probe=2)
    sq.index = M._SQ8Handle(1, sq)
    sq.item_ids = np.array([10, 11, 12], dtype=np.int64)
    sq._item_id_to_faiss_idx = {10: 0, 11: 1, 12: 2}
    sq.save(str(tmp_path / "a.sq8"))
    meta = pickle.loads((tmp_path / "a.meta.pkl").read_bytes())
    assert sorted(meta) == ["embed_dim", "item_id_to_faiss_idx", "item_ids", "n_lists", "n_probe"]
    assert meta["embed_dim"] == 16 and meta["n_probe"] == 2 and meta["item_ids"].tolist() == [10, 11, 12]
    sq.index._h = None


# ---- the additions behind tests/test_gpu_sq8_paths.py --------------------------------------------------------------------
def test_int_scores_blas_is_exact_at_the_extremes():
    rng = np.random.default_rng(11)
    for d in (1, 20, 64, 128):
        n = rng.integers(-S.QMAX, S.QMAX + 1, (37, d)).astype(np.int32)
        c = rng.integers(-127, 128, (211, d)).astype(np.int8)
        n[0], n[1], n[2] = S.QMAX, -S.QMAX, S.QMAX * np.where(np.arange(d) % 2, -1, 1)
        c[0], c[1], c[2] = 127, -127, 127 * np.where(np.arange(d) % 2, -1, 1)
        a, b = S.int_scores(n, c), S.int_scores_blas(n, c)
        assert b.dtype == np.int64
        np.testing.assert_array_equal(a, b)
        assert a[0, 0] == S.QMAX * 127 * d == -a[0, 1] == -a[1, 0] == a[2, 2]
    n16 = rng.integers(-S.QMAX, S.QMAX + 1, (5, 128)).astype(np.int16)
    c8 = rng.integers(-127, 128, (9, 128)).astype(np.int8)
    np.testing.assert_array_equal(S.int_scores_blas(n16, c8), S.int_scores(n16, c8))


def test_topk_fast_equals_topk():
    rng = np.random.default_rng(12)
    Sc = rng.integers(-6, 7, (300, 97)).astype(np.int64) * 1000003          # many ties
    Sc[5] = 0
    Sc[6] = -S.QMAX * 127 * 128
    Sc[7, ::2] = S.QMAX * 127 * 128
    allowed = rng.random((300, 97)) < 0.3
    allowed[9] = False
    for k in (1, 10, 97, 120):
        for al in (None, allowed):
            r1, s1 = S.topk(Sc, k, al)
            r2, s2 = S.topk_fast(Sc, k, al, chunk=64)
            np.testing.assert_array_equal(r1, r2)
            np.testing.assert_array_equal(s1, s2)
    assert (S.topk_fast(Sc, 3, allowed)[0][9] == -1).all()


def test_plan_arithmetic_of_the_path_cases():
    import test_gpu_sq8_paths as P
    # a: 260 tiles x 33 query groups = 8 580 > 2 * 4 096
    assert S.plan([8300], [1040], 1) == (3, [260], [87]) and 260 * 33 == 8580 and 260 % 3 == 2
    # b: the sample pass (every 16th tile) and the full pass
    assert S.plan([P.B_N], [P.B_NQ], S.SAMPLE_STEP) == (2, [79], [40]) and 79 * 64 == 5056
    assert S.plan([P.B_N], [P.B_NQ], 1) == (20, [1250], [63]) and 1250 % 20 != 0
    assert S.plan([32768], [2048], S.SAMPLE_STEP)[0] == 1 and S.plan([32769], [2048], S.SAMPLE_STEP)[:2] == (2, [65])
    assert S.dense_chunk([P.B_N], 1) == 2 ** 26 // 40000 == 1677
    for k in P.B_KS:
        assert S.auto_is_thresholded(P.B_NQ, k, [P.B_N], 1)
    # c: the probes of the dyadic case at every width
    for du in (20, 64, 100, 128):
        N, nlist, X, Cc, Q, assign = P._ivf_big_case(du)
        per_list = np.bincount(S.probed_lists(Q, Cc, P.C_NPROBE).ravel(), minlength=nlist)
        tpi, n_seq, splits = S.plan(P.C_LENS, per_list, 1)
        assert per_list.sum() == P.C_NQ * P.C_NPROBE and tpi >= 3
        assert n_seq[:6] == [0, 2, 2, 2, 4, 66] and any(p > 0 and s % tpi for p, s in zip(per_list, n_seq))
    # a list no query probes costs nothing; an empty list has no tiles
    assert S.plan([0, 640, 64], [5, 0, 33], 1) == (1, [0, 20, 2], [0, 20, 2])
    assert S.plan([64 * 4096], [64], 1, target=16) == (1024, [8192], [8])


def test_auto_rule_dense_chunk_and_threshold_arithmetic():
    assert S.geometry([40000], 1) == (1, 40000, 40000, 40000)
    assert S.geometry([100, 9001, 0, 65], 2) == (2, 9101, 9024, 18048)
    assert S.geometry([0], 7) == (1, 1, 32, 32)
    # each of the three ways auto stays dense, and none of them
    big = [40000]
    assert S.auto_is_thresholded(210, 10, big, 1) and not S.auto_is_thresholded(209, 10, big, 1)        # 209 * 40000 <= 2^23
    assert not S.auto_is_thresholded(4096, 10, [16384], 1) and S.auto_is_thresholded(4096, 10, [16385], 1)
    assert S.auto_is_thresholded(4096, 625, big, 1) and not S.auto_is_thresholded(4096, 626, big, 1)    # 4 k > 40000 / 16
    assert S.dense_chunk([1000], 1) == 4096 and S.dense_chunk([2 ** 27], 1) == 1
    assert S.threshold_rank(500) == 58 and S.threshold_rank(2000) == 174 and S.threshold_rank(2500) == 211
    assert S.threshold_rank(10) == 8 and S.threshold_rank(48) == 14
    assert S.threshold_cap(10, [6000], 1) == 4096 and S.threshold_cap(2000, [16384], 1) == 8192
    assert S.threshold_cap(2500, [3000], 1) == 3000 and S.threshold_cap(500, [510], 1) == 510
    assert len(S.flat_sample_rows(16384)) == 1024 and len(S.flat_sample_rows(3000)) == 192
    assert S.flat_sample_rows(520).tolist() == list(range(32)) + list(range(512, 520))


def test_redo_rules_on_hand_made_scores():
    R, K, E = S.REDO, S.KEPT, S.EITHER
    # 600 rows, k = 10 (rank 8): the sample is rows 0..31 and 512..543
    N, k = 600, 10
    base = np.zeros((5, N), dtype=np.int64)
    base[0, :8] = 5                                # threshold in (0, 5]: eight rows reach it, fewer than k
    base[1, :8] = 5; base[1, 100:102] = 5          # ten rows reach any threshold in (0, 5]
    base[2, :7] = 5                                # 8th and 9th best sampled score tie at 0: all 600 rows, cap = 600
    base[3, :8] = 5; base[3, 100:102] = 4          # threshold 5: eight rows; threshold <= 4: ten
    base[4, :8] = 5; base[4, 100:102] = 4; base[4, 8] = 4      # a sampled 4: the threshold can only be 5
    assert S.threshold_rank(k) == 8 and S.threshold_cap(k, [N], 1) == 600
    assert S.flat_thresholded_redo(base, k).tolist() == [R, K, K, E, R]
    assert S.redo_bounds(S.flat_thresholded_redo(base, k)) == (2, 3)
    assign = np.zeros(N, dtype=np.int32)
    assert S.ivf_thresholded_redo(base, k, assign, np.zeros((5, 1), dtype=np.int64), 1).tolist() == [R, K, K, E, R]
    # all rows tie in a list longer than its 4 096 candidate slots: overflow
    assert (S.flat_thresholded_redo(np.zeros((2, 6000), dtype=np.int64), k) == R).all()
    # overflow at the low end of the interval only
    over = np.zeros((1, 6000), dtype=np.int64)
    rest = np.setdiff1d(np.arange(6000), S.flat_sample_rows(6000))
    over[0, :8] = 9; over[0, rest[:12]] = 9; over[0, rest[12:4200]] = 3      # 20 rows at 9, 4 208 rows above 0
    assert S.flat_thresholded_redo(over, k).tolist() == [E]
    # a sample shorter than rank: no threshold, no failure while the rows fit
    assert (S.flat_thresholded_redo(np.arange(2 * 200).reshape(2, 200), 500) == K).all()
    # exactly rank sampled rows: nothing bounds the threshold from below
    few = np.zeros((1, 8), dtype=np.int64)
    assert S.flat_thresholded_redo(few, k).tolist() == [R]     # 8 rows < k under a real threshold
    # two lists, the query probes list 1 only: rows and sample are that list's
    assign = (np.arange(N) % 2).astype(np.int32)
    sc = np.zeros((1, N), dtype=np.int64)
    sc[0, 0:32:2] = 9                              # list 0's rows: not probed, must not matter
    sc[0, 1:16:2] = 5                              # eight rows of list 1, all in its first tile
    assert S.ivf_thresholded_redo(sc, k, assign, np.array([[1]]), 2).tolist() == [R]
    sc[0, 301] = 5; sc[0, 303] = 7
    assert S.ivf_thresholded_redo(sc, k, assign, np.array([[1]]), 2).tolist() == [K]
