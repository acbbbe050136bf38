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
