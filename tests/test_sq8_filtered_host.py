"""Host: the SQ8 index's filter API without a device -- predicate-word parsing, the Python-side tag state, the pipeline's
host-only refusal, the new exports, and the reference's re-do rule on passing rows against the existing rule."""
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_filtered_reference as FR  # noqa: E402
import sq8_reference as S  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


def _unbuilt_with_ids(monkeypatch, ids):
    """an SQ8Index whose handle is a stub: the library is never called (no device here)"""
    from recommendit_amd import SQ8Index
    from recommendit_amd import sq8_index as M
    sq = SQ8Index(embed_dim=16)
    sq.index = object()
    sq.item_ids = np.asarray(ids, dtype=np.int64)
    pushed = []
    monkeypatch.setattr(M.SQ8Index, "_push_tags", lambda self: pushed.append(None if self._tags is None else self._tags.copy()))
    return sq, pushed


def test_tag_state_lives_on_the_host(monkeypatch):
    from recommendit_amd import SQ8Index
    with pytest.raises(RuntimeError, match="not built"):
        SQ8Index(embed_dim=16).set_item_tags([1, 2])
    sq, pushed = _unbuilt_with_ids(monkeypatch, [10, 30, 20, 40])
    assert sq.item_tags() is None and sq._tags is None
    sq.set_item_tags(np.array([1, 2, 3, 0xFFFFFFFF], dtype=np.uint32))
    assert sq.item_tags().dtype == np.uint32 and sq.item_tags().tolist() == [1, 2, 3, 0xFFFFFFFF] and len(pushed) == 1
    sq.set_item_tags([8, -1], item_ids=[20, 10])             # named items only; -1 is the pattern of all ones
    assert sq.item_tags().tolist() == [0xFFFFFFFF, 2, 8, 0xFFFFFFFF]
    got = sq.item_tags()
    got[0] = 0                                               # a copy: the state is not the caller's to change
    assert sq.item_tags()[0] == 0xFFFFFFFF
    for bad, text in (([1, 2, 3], "3 tag words for 4 items"), (np.zeros(4, np.float32), "uint32 words"),
                      ([0, 0, 0, 1 << 32], "fit 32 bits")):
        with pytest.raises(ValueError, match=text):
            sq.set_item_tags(bad)
    with pytest.raises(ValueError, match="item id 99 is not stored"):
        sq.set_item_tags([1], item_ids=[99])
    assert sq.item_tags().tolist() == [0xFFFFFFFF, 2, 8, 0xFFFFFFFF] and len(pushed) == 2      # failed calls change nothing
    sq.clear_item_tags()
    assert sq.item_tags() is None and pushed[-1] is None
    sq.set_item_tags([5], item_ids=[30])                     # on an index without tags the others are 0
    assert sq.item_tags().tolist() == [0, 5, 0, 0]
    sq.index = None


def test_predicate_words_are_checked_on_the_host(monkeypatch):
    """every input form FAISSIndex takes is parsed by the same code, and a bad one fails before any device call"""
    import torch
    from recommendit_amd.faiss_index import item_filter_words
    sq, _ = _unbuilt_with_ids(monkeypatch, [1, 2, 3])
    with pytest.raises(ValueError, match="set_item_tags"):
        sq._pred((1, 0, 0), 2, "cpu")
    sq.set_item_tags([1, 2, 3])
    for bad, text in (((1, 2), "3-tuple"), (np.zeros((3, 3), np.uint32), "3-tuple"), (np.zeros((2, 3), np.float32), "integers"),
                      ((1 << 32, 0, 0), "32 bits")):
        with pytest.raises(ValueError, match=text):
            sq._pred(bad, 2, "cpu")
    w, stride = sq._pred((-1, 0, 1 << 31), 5, "cpu")
    assert stride == 0 and w.dtype == torch.int32 and w.flatten().tolist() == [-1, 0, -(1 << 31)]
    assert sq._pred((-1, 0, 1 << 31), 5, "cpu")[0] is w       # a shared predicate is uploaded once
    w, stride = sq._pred(np.array([[1, 2, 3], [4, 5, 6]], dtype=np.int64), 2, "cpu")
    assert stride == 3 and w.tolist() == [[1, 2, 3], [4, 5, 6]]
    assert item_filter_words(torch.tensor([[7, 0, 0]], dtype=torch.int32), 1).tolist() == [[7, 0, 0]]
    sq.index = None


def test_pipeline_refuses_an_untagged_sq8_index_on_the_host(monkeypatch):
    from recommendit_amd import SQ8Index
    from recommendit_amd.recommender import GpuRecommendationPipeline
    pipe = GpuRecommendationPipeline(None, SQ8Index(embed_dim=32), None, None)
    with pytest.raises(ValueError, match="SQ8Index.set_item_tags"):
        pipe.recommend_batch([1], item_filter=(1, 0, 0))
    # what stays out of scope on an SQ8 index is refused as before, tagged or not
    sq, _ = _unbuilt_with_ids(monkeypatch, [1, 2, 3])
    sq.set_item_tags([1, 2, 3])
    pipe = GpuRecommendationPipeline(None, sq, None, None)
    for call in (lambda: pipe.recommend_batch([1], graph=True, item_filter=(1, 0, 0)),
                 lambda: pipe.recommend_batch([1], exclude_seen=True), lambda: pipe.recommend_batch([1], diversity=0.3),
                 lambda: pipe.recommend_cold_batch(None), lambda: pipe.set_seen(object())):
        with pytest.raises(ValueError, match="SQ8"):
            call()
    sq.index = None


def test_header_declares_and_binding_holds_the_filter_abi():
    from recommendit_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "recommendit_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(rihip_sq8_filter_\w+)\s*\(", txt))
    assert declared == {"rihip_sq8_filter_set_tags", "rihip_sq8_filter_has_tags", "rihip_sq8_filter_search",
                        "rihip_sq8_filter_stats"}
    assert "rihip_sq8_refine_search_filtered" in txt and declared <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["rihip_sq8_filter_search"][1]) == len(_lib.SIGNATURES["rihip_sq8_index_search"][1]) + 2
    assert len(_lib.SIGNATURES["rihip_sq8_refine_search_filtered"][1]) == len(_lib.SIGNATURES["rihip_sq8_refine_search"][1]) + 2
    assert re.search(r"#define\s+RIHIP_ABI_VERSION\s+1\b", txt)


def test_predicate_restatement():
    tags = np.array([0b0000, 0b0001, 0b0110, 0b1111], dtype=np.uint32)
    preds = FR.words([(0, 0, 0), (0b0011, 0, 0), (0, 0b0110, 0), (0, 0, 0b1000), (0b0001, 0b0100, 0b1000), (0, 1 << 31, 0)], 6)
    assert FR.passes(tags, preds).tolist() == [[True] * 4, [False, True, True, True], [False, False, True, True],
                                               [True, True, True, False], [False] * 4, [False] * 4]
    assert FR.words((-1, 0, 0), 2).tolist() == [[0xFFFFFFFF, 0, 0]] * 2


def test_redo_rule_on_passing_rows_is_the_existing_rule_when_every_row_passes():
    rng = np.random.default_rng(5)
    N, nq, nlist, nprobe = 9000, 24, 6, 2
    Sc = rng.integers(-4000, 4000, (nq, N))
    Sc[3] = 7                                                 # every score ties: overflow
    every = np.ones((nq, N), dtype=bool)
    flat = (np.zeros(N, np.int64), np.zeros((nq, 1), np.int64), 1)
    assign = rng.integers(0, nlist, N)
    probes = np.stack([rng.choice(nlist, nprobe, replace=False) for _ in range(nq)])
    seen = set()
    for k in (10, 200, 1500):
        a = FR.thresholded_redo(Sc, k, *flat, every)
        np.testing.assert_array_equal(a, S.flat_thresholded_redo(Sc, k))
        b = FR.thresholded_redo(Sc, k, assign, probes, nlist, every)
        np.testing.assert_array_equal(b, S.ivf_thresholded_redo(Sc, k, assign, probes, nlist))
        seen |= set(a.tolist()) | set(b.tolist())
    assert {S.REDO, S.KEPT} <= seen
    # and it is a rule about passing rows: a row that fails can neither raise the threshold nor fill a slot
    ok = every.copy()
    ok[:, ::2] = False
    half = FR.thresholded_redo(Sc, 10, *flat, ok)
    samp = S.flat_sample_rows(N)
    for q in (0, 3):
        want = S._redo_state(Sc[q, ok[q]], Sc[q, samp[ok[q, samp]]], S.threshold_rank(10), S.threshold_cap(10, [N], 1), 10)
        assert half[q] == want
    assert half[3] == S.REDO                                  # 4 500 tied passing rows still overflow 4 096 slots
