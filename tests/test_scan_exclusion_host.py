"""Host: the NumPy reference of seen-item exclusion inside the scan (tests/exclusion_reference.py) against a per-query
Python loop over sets, and the mask layout against np.packbits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import exclusion_reference as XR  # noqa: E402


def _case(seed, nq=23, N=300, n_users=9):
    rng = np.random.RandomState(seed)
    item_ids = rng.permutation(7 * np.arange(N) + 3).astype(np.int64)
    S = rng.randint(-4, 5, size=(nq, N)).astype(np.int64)          # a handful of values: ties everywhere
    counts = rng.randint(0, 120, n_users)
    counts[0] = 0
    pool = np.concatenate([item_ids, [1, 2, 10 ** 6]])               # ids that are not stored as well
    rows = [np.sort(rng.choice(pool, c, replace=False)) for c in counts]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    items = np.concatenate(rows).astype(np.int64)
    user_ids = rng.randint(-1, n_users + 2, nq)                      # some outside the store
    user_ids[:2] = 3                                                 # one user twice
    cand = rng.rand(nq, N) < 0.6
    passing = rng.rand(N) < 0.7
    return S, item_ids, offsets, items, user_ids, cand, passing


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 50, 400])
def test_reference_equals_a_loop_over_sets(seed, k):
    S, item_ids, offsets, items, user_ids, cand, passing = _case(seed)
    nq, N = S.shape
    lists = XR.seen_lists(offsets, items, user_ids, nq)
    allowed = XR.allowed_rows(XR.excluded_rows(lists, item_ids), cand, passing)
    sc, rows = XR.topk_excluding(S, k, allowed)
    assert sc.dtype == np.float32 and rows.dtype == np.int64 and rows.shape == (nq, k)
    n_users = offsets.shape[0] - 1
    for q in range(nq):
        u = int(user_ids[q])
        seen = set(items[offsets[u]:offsets[u + 1]].tolist()) if 0 <= u < n_users else set()
        ok = [r for r in range(N) if cand[q, r] and passing[r] and int(item_ids[r]) not in seen]
        ok.sort(key=lambda r: (-S[q, r], r))
        want = ok[:k]
        assert rows[q, :len(want)].tolist() == want
        assert (rows[q, len(want):] == -1).all() and np.isneginf(sc[q, len(want):]).all()
        assert sc[q, :len(want)].tolist() == [float(S[q, r]) for r in want]


def test_seen_lists_by_position_and_out_of_range_users():
    offsets = np.array([0, 2, 2, 5], np.int64)
    items = np.array([4, 9, 1, 2, 3], np.int32)
    got = XR.seen_lists(offsets, items, None, 3)
    assert [g.tolist() for g in got] == [[4, 9], [], [1, 2, 3]]
    got = XR.seen_lists(offsets, items, [2, -1, 3, 0], 4)
    assert [g.tolist() for g in got] == [[1, 2, 3], [], [], [4, 9]]


@pytest.mark.parametrize("Np", [1, 31, 32, 33, 64, 1000])
def test_mask_words_equal_packbits_little(Np):
    rng = np.random.RandomState(Np)
    bits = rng.rand(5, Np) < 0.3
    bits[0] = False
    bits[1] = True
    got = XR.mask_words([np.nonzero(b)[0] for b in bits], Np)
    W = (Np + 31) // 32
    padded = np.zeros((5, W * 32), dtype=bool)
    padded[:, :Np] = bits
    want = np.packbits(padded, axis=1, bitorder="little").view("<u4")
    assert got.dtype == np.uint32 and got.shape == (5, W)
    np.testing.assert_array_equal(got, want)
    # a position given twice is one bit
    np.testing.assert_array_equal(XR.mask_words([[0, 0, Np - 1]], Np), XR.mask_words([[Np - 1, 0]], Np))


def test_ivf_positions_are_list_major_and_padded():
    assign = np.array([2, 0, 2, 1, 0, 2], np.int64)
    pos, Np = XR.ivf_positions(assign, 4)          # list 3 is empty
    assert Np == 192
    assert pos.tolist() == [128, 0, 129, 64, 1, 130]
    rng = np.random.RandomState(0)
    assign = rng.randint(0, 8, 3000)
    pos, Np = XR.ivf_positions(assign, 8)
    assert np.unique(pos).size == 3000 and Np % 64 == 0 and pos.max() < Np
    order = np.argsort(pos)
    assert (np.diff(assign[order]) >= 0).all()                       # lists ascending
    same = np.diff(assign[order]) == 0
    assert (np.diff(order)[same] > 0).all()                          # rows ascending inside a list
    first = np.array([pos[assign == c].min() for c in range(8)])
    assert (first % 64 == 0).all()
