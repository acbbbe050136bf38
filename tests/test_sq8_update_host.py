"""CPU: the NumPy model of an SQ8 index update (tests/sq8_update_reference.py) applied step by step equals the model
built from the final corpus -- the property the GPU tests then ask of the handle -- and refuses what the C ABI
refuses.  Also: the package exports the update calls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_reference as S  # noqa: E402
import sq8_update_reference as U  # noqa: E402


def _unit(rng, n, d):
    x = rng.randn(n, d).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _setup(d, N0, nlist, tagged, seed):
    rng = np.random.RandomState(seed)
    X0, pool = _unit(rng, N0, d), _unit(rng, 600, d)
    C = _unit(rng, nlist, d)
    assign = lambda X: np.argmax(X.astype(np.float64) @ C.astype(np.float64).T, axis=1)    # noqa: E731
    ids0 = rng.permutation(10 * N0)[:N0].astype(np.int64)
    tags0 = rng.randint(0, 2 ** 32, N0, dtype=np.uint64).astype(np.uint32) if tagged else None
    m, s = S.train_quantizer(X0)
    lists0 = assign(X0) if nlist > 1 else None
    return rng, X0, pool, ids0, tags0, lists0, assign, m, s


class _Corpus:
    """the plain model next to the physical one: rows, ids, lists and tags in insertion order"""

    def __init__(self, X, ids, lists, tags):
        self.X, self.ids, self.lists, self.tags = X.copy(), ids.copy(), None if lists is None else lists.copy(), tags

    def apply(self, drop, X_add, add_ids, add_lists, add_tags):
        keep = ~np.isin(self.ids, drop)
        self.X = np.concatenate([self.X[keep], X_add])
        self.ids = np.concatenate([self.ids[keep], add_ids])
        if self.lists is not None:
            self.lists = np.concatenate([self.lists[keep], add_lists])
        if self.tags is not None:
            self.tags = np.concatenate([self.tags[keep], np.zeros(len(add_ids), np.uint32) if add_tags is None else add_tags])


@pytest.mark.parametrize("d,nlist,tagged", [(8, 5, True), (72, 5, False), (8, 1, True)])
def test_step_by_step_equals_from_scratch(d, nlist, tagged):
    rng, X0, pool, ids0, tags0, lists0, assign, m, s = _setup(d, 700, nlist, tagged, 11 + d + nlist)
    A = U.Sq8Model.from_corpus(X0, ids0, lists0, nlist, m, s, tags0)
    c = _Corpus(X0, ids0, lists0, tags0)
    pool_ids = np.arange(10 ** 6, 10 ** 6 + len(pool), dtype=np.int64)
    pool_list = assign(pool) if nlist > 1 else np.zeros(len(pool), dtype=np.int64)
    used = [0]

    def step(drop, rows, add_ids=None, add_tags=None, X=None):
        X_add = pool[rows] if X is None else X
        add_ids = pool_ids[rows] if add_ids is None else add_ids
        al = (assign(X_add) if nlist > 1 else np.zeros(len(X_add), dtype=np.int64)) if len(X_add) else np.zeros(0, np.int64)
        n_gone, clamped = A.update(drop, X_add, add_ids, al if nlist > 1 else None, add_tags)
        assert n_gone == int(np.isin(c.ids, drop).sum()) and clamped == U.clamp_count(X_add, m, s)
        c.apply(drop, X_add, add_ids, al, add_tags)
        B = U.Sq8Model.from_corpus(c.X, c.ids, c.lists, nlist, m, s, c.tags)
        U.same_state(A, B)
        np.testing.assert_array_equal(A.codes_by_row(), S.encode(c.X, m, s))
        if nlist > 1:
            np.testing.assert_array_equal(A.lists(), c.lists)
        if tagged:
            np.testing.assert_array_equal(A.tags_by_row(), c.tags)
        assert (A.codes[A.row_ids < 0] == 0).all() and (A.codes[:, d:] == 0).all()
        assert int(A.poff[-1]) % 64 == 0 and (A.row_ids >= 0).sum() == len(c.ids)

    none = np.zeros(0, dtype=np.int64)
    if nlist > 1:
        # (a) a list emptied completely, unknown ids among the drop ids
        sizes = np.bincount(c.lists, minlength=nlist)
        victim = int(np.where(sizes > 0, sizes, 10 ** 9).argmin())
        step(np.concatenate([[-4, 10 ** 12], c.ids[c.lists == victim][::-1]]), none)
        assert A.list_len[victim] == 0 and A.poff[victim] == A.poff[victim + 1]
        T = int(np.bincount(pool_list, minlength=nlist).argmax())
    else:
        step(np.concatenate([[-4, 10 ** 12], c.ids[5:40]]), none)
        T = 0
    # (b) list T filled exactly to a granule, rows of other lists added in the same call
    of_T = np.nonzero(pool_list == T)[0]
    fill = int(-A.list_len[T] % 64) or 64
    assert len(of_T) >= fill + 3
    others = np.nonzero(pool_list != T)[0][:40]
    pick = np.sort(np.concatenate([of_T[:fill], others]))
    step(none, pick, add_tags=(np.arange(len(pick)) * 7 + 1).astype(np.uint32) if tagged else None)
    assert A.list_len[T] % 64 == 0
    np_before = int(A.poff[-1])
    # (c) three more rows: the list crosses the granule
    step(none, of_T[fill:fill + 3])
    assert A.list_len[T] % 64 == 3 and int(A.poff[-1]) == np_before + 64
    # (d) an upsert: 50 stored ids get new rows, 30 ids are new
    stored = rng.choice(c.ids, 50, replace=False)
    up_ids = np.concatenate([stored[:20], np.arange(5 * 10 ** 6, 5 * 10 ** 6 + 30), stored[20:]])
    step(up_ids, None, add_ids=up_ids, X=3.0 * _unit(rng, 80, d))       # scaled rows: some codes clamp
    assert A.stats[0] == 4 and A.stats[3] > 0 and A.stats[2] == len(pick) + 3 + 80


def test_refusals_leave_the_model_as_it_was():
    rng, X0, pool, ids0, tags0, lists0, assign, m, s = _setup(8, 300, 4, True, 5)
    A = U.Sq8Model.from_corpus(X0, ids0, lists0, 4, m, s, tags0)
    B = U.Sq8Model.from_corpus(X0, ids0, lists0, 4, m, s, tags0)
    new = np.array([10 ** 7, 10 ** 7 + 1, 10 ** 7 + 2], dtype=np.int64)
    cases = [
        (1, [], pool[:3], [new[0], new[1], new[0]]),                       # repeated among the add ids
        (1, [ids0[3], ids0[4], ids0[3]], pool[:0], []),                    # repeated among the drop ids
        (2, [ids0[1]], pool[:3], [new[0], ids0[2], new[1]]),               # stored and not dropped
        (3, ids0, pool[:0], []),                                           # would be empty
    ]
    for kind, drop, X, add in cases:
        with pytest.raises(U.Refused) as e:
            A.update(drop, X, add, assign(X) if len(X) else None)
        assert e.value.kind == kind
        U.same_state(A, B)
    assert A.update([ids0[3], ids0[3] + 10 ** 9][1:], pool[:0], []) == (0, 0)   # only unknown ids: nothing changes
    assert A.update([], pool[:0], []) == (0, 0)
    U.same_state(A, B)
    assert A.stats == [0, 0, 0, 0]
    # dropping a stored id and adding it again in one call is an upsert, not a refusal
    assert A.update([ids0[2]], pool[:1], [ids0[2]], assign(pool[:1]))[0] == 1


def test_clamp_count_is_the_unclamped_rint():
    m, s = np.array([0.0, 1.0], np.float32), np.array([0.01, 0.5], np.float32)
    X = np.array([[1.27, 1.0], [1.275, 64.5], [1.2751, 64.76], [-1.28, -62.76]], np.float32)
    v = np.rint((X - m) / s)
    assert U.clamp_count(X, m, s) == int((np.abs(v) > 127).sum()) >= 3
    assert U.clamp_count(X[:0], m, s) == 0
    assert (np.abs(S.encode(X, m, s).astype(np.int64)) <= 127).all()


def test_the_package_exports_the_update_calls():
    from recommendit_amd import SQ8Index, _lib
    for name in ("add_items", "add_items_device", "remove_items", "update_items", "assign_lists", "update_stats"):
        assert callable(getattr(SQ8Index, name)), name
    for name in ("rihip_sq8_update_apply", "rihip_sq8_update_assign", "rihip_sq8_update_stats"):
        assert name in _lib.SIGNATURES, name
    for call in (lambda e: e.add_items(np.zeros((1, 8), np.float32), [1]), lambda e: e.remove_items([1]),
                 lambda e: e.update_items(np.zeros((1, 8), np.float32), [1])):
        with pytest.raises(RuntimeError, match="Index not built."):
            call(SQ8Index(embed_dim=8))
