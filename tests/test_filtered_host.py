"""Host-side pieces of filtered retrieval (no GPU): tag words from a genre matrix, predicate normalisation, the sidecar
key that appears only with tags, and a clean import without a device."""
import pickle

import numpy as np
import pytest
import torch


def test_genre_tags_bit_layout():
    from recommendit_amd.faiss_index import genre_tags
    g = np.zeros((5, 18), np.float32)
    g[0, 0] = 1; g[1, 17] = 1; g[2, [3, 5]] = 1; g[3, :] = 0.5; g[4, 2] = -1.0       # > 0 sets the bit; <= 0 does not
    t = genre_tags(g)
    assert t.dtype == np.uint32
    assert t.tolist() == [1, 1 << 17, (1 << 3) | (1 << 5), (1 << 18) - 1, 0]
    assert genre_tags(torch.from_numpy(g)).tolist() == t.tolist()
    wide = np.ones((1, 32), np.int8)
    assert genre_tags(wide).tolist() == [0xFFFFFFFF]
    with pytest.raises(ValueError):
        genre_tags(np.ones((1, 33)))
    with pytest.raises(ValueError):
        genre_tags(np.ones(18))


def test_store_item_genre_tags():
    from recommendit_amd.recommender import GpuFeatureStore
    store = GpuFeatureStore(2, 4)
    store.set_item_features(1, {"genre_vector": [1.0] + [0.0] * 17})
    store.set_item_features(3, {"genre_vector": [0.0] * 16 + [1.0, 1.0]})
    assert store.item_genre_tags([1, 2, 3, 99, -1]).tolist() == [1, 0, (1 << 16) | (1 << 17), 0, 0]


def test_predicate_normalisation_reaches_the_same_words():
    from recommendit_amd.faiss_index import item_filter_words
    nq = 4
    want = np.tile(np.array([[5, 0x80000000, 0xFFFFFFFF]], np.uint32), (nq, 1))
    assert np.array_equal(item_filter_words((5, 0x80000000, 0xFFFFFFFF), nq), want)
    assert np.array_equal(item_filter_words((5, -(1 << 31), -1), nq), want)                   # negative = bit pattern
    assert np.array_equal(item_filter_words(want, nq), want)                                  # uint32 [nq,3]
    assert np.array_equal(item_filter_words(want.view(np.int32), nq), want)                   # int32 bit pattern
    assert np.array_equal(item_filter_words(torch.from_numpy(want.view(np.int32)), nq), want)  # tensor, read as bits
    assert np.array_equal(item_filter_words(want.astype(np.int64), nq), want)
    assert np.array_equal(item_filter_words(want[0], nq), want)                               # one row for the batch
    w = item_filter_words(want, nq)
    assert w.dtype == np.uint32 and w.shape == (nq, 3) and w.flags["C_CONTIGUOUS"]
    for bad in ((1, 2), (1, 2, 3, 4), np.zeros((nq, 2), np.uint32), np.zeros((nq + 1, 3), np.uint32),
                np.zeros((nq, 3), np.float32), (1 << 32, 0, 0), np.full((nq, 3), 1 << 32, np.int64)):
        with pytest.raises(ValueError):
            item_filter_words(bad, nq)


def test_sidecar_key_only_with_tags(tmp_path, monkeypatch):
    """save() without a device: the handle file is stubbed, the sidecar is the code under test"""
    from recommendit_amd import FAISSIndex
    from recommendit_amd import _lib as L

    class _Lib:
        @staticmethod
        def rihip_ip_index_save(h, path):
            open(path.decode(), "wb").write(b"stub")
            return 0

    monkeypatch.setattr(L, "lib", lambda: _Lib)

    class _H:
        _h = None
    idx = FAISSIndex(embed_dim=8, n_lists=4, n_probe=2)
    idx.index = _H()
    idx.item_ids = np.arange(3, dtype=np.int64)
    idx._item_id_to_faiss_idx = {0: 0, 1: 1, 2: 2}
    idx.save(str(tmp_path / "a.idx"))
    plain = (tmp_path / "a.meta.pkl").read_bytes()
    assert sorted(pickle.loads(plain)) == ["embed_dim", "item_id_to_faiss_idx", "item_ids", "n_lists", "n_probe"]
    idx._tags = torch.from_numpy(np.array([1, 2, 0x80000000], np.uint32).view(np.int32))
    idx.save(str(tmp_path / "b.idx"))
    meta = pickle.loads((tmp_path / "b.meta.pkl").read_bytes())
    assert sorted(meta) == ["embed_dim", "item_id_to_faiss_idx", "item_ids", "item_tags", "n_lists", "n_probe"]
    assert meta["item_tags"].dtype == np.uint32 and meta["item_tags"].tolist() == [1, 2, 0x80000000]
    idx._tags = None
    idx.save(str(tmp_path / "c.idx"))
    assert (tmp_path / "c.meta.pkl").read_bytes() == plain


def test_import_and_keywords_without_a_device():
    import inspect
    import recommendit_amd
    from recommendit_amd import FAISSIndex, _lib
    from recommendit_amd.recommender import GpuRecommendationPipeline
    for fn in (FAISSIndex.search, FAISSIndex.batch_search, FAISSIndex.batch_search_device,
               GpuRecommendationPipeline.recommend_batch, GpuRecommendationPipeline.get_recommendations):
        p = inspect.signature(fn).parameters
        assert "item_filter" in p and p["item_filter"].default is None
    for fn in (FAISSIndex.add_items, FAISSIndex.add_items_device, FAISSIndex.update_items):
        assert inspect.signature(fn).parameters["tags"].default is None
    for name in ("rihip_ip_index_set_tags", "rihip_ip_index_has_tags", "rihip_ip_index_search_filtered",
                 "rihip_ip_index_filtered_stats"):
        assert name in _lib.SIGNATURES
    idx = FAISSIndex(embed_dim=8)
    assert idx.item_tags() is None and not idx.has_item_tags
    with pytest.raises(RuntimeError, match="not built"):
        idx.set_item_tags(np.zeros(3, np.uint32))
