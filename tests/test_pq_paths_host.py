"""Host: every case of tests/test_gpu_pq_paths.py built on the CPU (tests/pq_paths_cases.py) -- the builders assert from
the references alone that the inputs reach the path each case is about -- and the reference helpers added for that file
against their slower, obviously correct forms."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_paths_cases as PC  # noqa: E402
import pq_reference as P  # noqa: E402
import sq8_reference as S  # noqa: E402


# ---- the new helpers -------------------------------------------------------------------------------------------------------
def _small_codes(n, du, seed):
    rng = np.random.default_rng(seed)
    Cc = rng.standard_normal((12, du)).astype(np.float32)
    X = (Cc[rng.integers(0, 12, n)] + 0.2 * rng.standard_normal((n, du))).astype(np.float32)
    X[n // 2:n // 2 + 9] = X[:9]                                 # identical rows: ties between entries seeded from them
    m, s = S.train_quantizer(X)
    return P.pad_codes(S.encode(X, m, s), P.dpad_of(du))


@pytest.mark.parametrize("n,du,dsub", [(600, 40, 8), (600, 40, 16), (90, 100, 8), (300, 100, 16)])
def test_the_blas_trainer_is_the_integer_trainer(n, du, dsub):
    c = _small_codes(n, du, 5 + n + dsub)
    a, b = P.train(c, dsub, 2), P.train_blas(c, dsub, 2)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    book = P.init_book(c, dsub)
    ca, da = P.assign(c, book)
    cb, db = P.assign_blas(c, book)
    assert da == db and ca.tobytes() == cb.tobytes()
    if n == 90:
        assert len({e.tobytes() for e in book[0]}) < 256          # repeated seeds: ties, the lowest entry in both


def test_entry_sums_are_what_the_lloyd_step_divides():
    c = _small_codes(500, 40, 77)
    book = P.init_book(c, 8)
    codes, _ = P.assign(c, book)
    step = P.lloyd_step(c, codes, book)
    for m in range(8):
        s, cnt = P.entry_sums(c, codes, m, 8)
        slow = np.zeros_like(s)
        for i in range(c.shape[0]):
            slow[codes[i, m]] += c[i, m * 8:(m + 1) * 8]
        np.testing.assert_array_equal(s, slow)
        has = cnt > 0
        np.testing.assert_array_equal(step[m][has], np.clip(np.rint(s[has] / cnt[has][:, None]), -127, 127).astype(np.int8))
        np.testing.assert_array_equal(step[m][~has], book[m][~has])


def test_list_layout_against_a_walk_over_the_lists():
    rng = np.random.default_rng(3)
    assign = rng.choice([0, 2, 5, 6], 700, p=[0.5, 0.01, 0.3, 0.19])
    pos, phys, lens = PC.list_layout(assign, 8)
    at, want_pos, want_phys = 0, np.empty(700, np.int64), np.empty(700, np.int64)
    for l in range(8):
        rows = [i for i in range(700) if assign[i] == l]         # ascending
        for j, i in enumerate(rows):
            want_pos[i], want_phys[i] = j, at + j
        at += (len(rows) + 63) // 64 * 64
    np.testing.assert_array_equal(pos, want_pos)
    np.testing.assert_array_equal(phys, want_phys)
    assert lens.tolist() == [len([i for i in range(700) if assign[i] == l]) for l in range(8)]


# ---- A ---------------------------------------------------------------------------------------------------------------------
def test_the_shape_chosen_for_the_instantiation_matrix():
    """r27's case c shrunk as far as the plan allows: one more halving of the long lists or of the queries gives tpi 2"""
    assert sum(PC.A_LENS) == 15442 and len(PC.A_LENS) == 16 and (PC.A_NPROBE, PC.A_NQ) == (4, 1000)
    case = PC.matrix_case(40, 8, False)
    per_list = np.bincount(case["probes"].ravel(), minlength=16)
    tpi, n_seq, splits = S.plan(PC.A_LENS, per_list, 1)
    assert tpi == 3 == case["tpi"]
    total = sum((int(p) + 31) // 32 * s for p, s in zip(per_list, n_seq))
    assert 2 * 4096 < total <= 3 * 4096
    halved = [l if l <= 65 else l // 2 for l in PC.A_LENS]
    assert S.plan(halved, per_list, 1)[0] == 2 and S.plan(PC.A_LENS, (per_list + 1) // 2, 1)[0] == 2
    assert max(splits) >= 30 and n_seq[2] == 4 and splits[2] == 2       # the 65-row list: tiles 0 - 2, then tile 3


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("dsub", [8, 16])
@pytest.mark.parametrize("du", [40, 100])
def test_matrix_cases_reach_their_paths(du, dsub, res):
    case = PC.matrix_case(du, dsub, res)
    assert case["dec"].dtype == (np.int16 if res else np.int8)
    for fm in PC.FMS:
        rows, sc, redo = PC.matrix_expect(case, fm)
        assert (rows[:2, 66:] == -1).all()                       # k = 100 is above the 66 rows queries 0 and 1 probe
        for k in PC.A_KS:
            lo, hi = S.redo_bounds(redo[k])
            assert (lo >= 4) == (k == 100)                       # at k = 100 the queries of the short lists are re-done by deficit
            assert not S.auto_is_thresholded(PC.A_NQ, k, PC.A_LENS, PC.A_NPROBE)


# ---- B ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [130, 4100])
@pytest.mark.parametrize("shape", list(PC.B1_SHAPES))
def test_redo_cases_reach_their_paths(shape, nq):
    case = PC.redo_case(shape, nq)
    assert (case["rows"] == np.arange(PC.B1_K)[None, :]).all()


@pytest.mark.parametrize("variant", ["seen", "tags"])
@pytest.mark.parametrize("shape", ["res-64-16", "res-128-8"])
def test_redo_variants_reach_their_paths(shape, variant):
    case = PC.redo_case(shape, 130, variant)
    assert len({r.tobytes() for r in case["rows"]}) >= 5 and (case["rows"] != np.arange(PC.B1_K)[None, :]).any(axis=1).mean() > 0.5


def test_deficit_case_reaches_its_path():
    case = PC.deficit_case()
    assert (case["rows"] >= 0).all()


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
def test_refine_cases(res):
    case = PC.refine_case(res)
    assert set(case["want"]) == {"plain", "filtered", "excluding"}


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dsub", [8, 16])
@pytest.mark.parametrize("du", [40, 100])
def test_train_cases_reach_the_cross_workgroup_sums(du, dsub):
    case = PC.train_case(du, dsub)
    assert case["dec16"].dtype == np.int16 and case["clamped"] >= 0


@pytest.mark.parametrize("dsub", [8, 16])
def test_edges_of_the_update_rule(dsub):
    case = PC.edges_case(dsub)
    assert case["want"][2].shape == (2,)
    np.testing.assert_array_equal(case["want"][0], case["step"])
