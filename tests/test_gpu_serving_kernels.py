"""GPU: the serving chain's kernels at the C ABI -- the forest predictor (csrc/gbdt.hip, all four kernels), the ranking
feature assembly and the final top-k (csrc/features.hip) -- each against an independent NumPy reference:
oracle/gbdt_np.py (pinned by tests/test_ranker_oracle.py), oracle/ranking_features_np.table_feature_matrix (pinned
bitwise to the per-row restatement in tests/test_ranking_features_oracle.py) and a stable sort.

Every forest case asserts the kernel it was written for (rihip_gbdt_predict_path); tests/test_serving_paths_host.py
checks the same expectation on the CPU against a host restatement of the chunk and record arithmetic.

Score bound (derived, not tuned): the kernels add the T reached leaves in another order than the reference, each of the
T - 1 additions rounds once, so |got - ref| <= (T - 1) * 2^-53 * sum_t |leaf_t| per row; average_output multiplies once
more (+ 2^-53 * |ref|).  Features and top-k are exact.  Worst ratios observed: profiles/r10_serving_kernel_tests.md.
"""
import ctypes
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import gbdt_np as G
from oracle import ranking_features_np as RF

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
FLT_MAX = float(np.finfo(np.float32).max)
OK, ERR_ARG, ERR_SHAPE = 0, 1, 3
ROOT = Path(__file__).resolve().parent.parent


def _L():
    from recommendit_amd import _lib as L
    return L, L.lib(), L.device(), L.stream_ptr()


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)                 # a copy: the shared inputs are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _report(name, value):
    print(f"[worst] {name}: {value:.3f}")


# =========================================================================================== forest predictor
def _load(model):
    """model dict -> recommendit_amd.ranker._Forest (owns the handle)"""
    from recommendit_amd.ranker import _Forest
    L, lib, _, _ = _L()
    text = G.write_text_model(model).encode()
    h = ctypes.c_void_p()
    L.check(lib.rihip_gbdt_create_from_text(text, len(text), ctypes.byref(h)), "gbdt_create_from_text")
    return _Forest(h.value)


def _assert_path(forest, want):
    assert forest.predict_path() == want


def _predict(forest, X):
    """raw ABI call on a contiguous float32 matrix"""
    L, lib, dev, st = _L()
    Xd = _dev(np.asarray(X, np.float32), dev)
    out = torch.full((X.shape[0],), float("nan"), dtype=torch.float64, device=dev)
    L.check(lib.rihip_gbdt_predict(forest._h, Xd.data_ptr(), X.shape[0], X.shape[1], out.data_ptr(), st), "gbdt_predict")
    return out.cpu().numpy()


def _one_leaf(v):
    return dict(num_leaves=1, num_cat=0, leaf_value=np.array([v]), shrinkage=1.0)


def _f32_floor(x):
    f = np.float32(x)
    return np.nextafter(f, np.float32(-np.inf)) if float(f) > x else f


ZERO_LO = _f32_floor(G.K_ZERO)                           # largest float32 <= 1e-35: still "zero" for a zero-missing node
ZERO_HI = np.nextafter(ZERO_LO, np.float32(np.inf))      # the next one: not zero any more
TINY = np.array([ZERO_LO, ZERO_HI, -ZERO_LO, -ZERO_HI, 1e-40, -1e-40, 1.4e-45, -1.4e-45, -0.0, 0.0, np.nan], np.float32)


def _edge_X(model, n, seed, extra=None):
    """N(0,1) features with the values a walk gets wrong: NaN, +-inf, +-0.0, and the float32 image of a node's own
    threshold in that node's feature (rounded to nearest: at, or one float32 above, the largest float32 <= threshold)"""
    rng = np.random.RandomState(seed)
    nf = len(model["feature_names"])
    X = rng.randn(n, nf).astype(np.float32)
    X[rng.rand(n, nf) < 0.03] = np.nan
    X[rng.rand(n, nf) < 0.01] = np.inf
    X[rng.rand(n, nf) < 0.01] = -np.inf
    X[rng.rand(n, nf) < 0.02] = 0.0
    X[rng.rand(n, nf) < 0.02] = -0.0
    if extra is not None:
        hit = rng.rand(n, nf) < 0.3
        X[hit] = rng.choice(extra, size=int(hit.sum()))
    nodes = [(t["split_feature"][i], t["threshold"][i]) for t in model["trees"] if t["num_leaves"] > 1
             for i in range(t["num_leaves"] - 1) if not (t["decision_type"][i] & 1)]
    if nodes:
        for r in range(n):                                # two exact threshold hits per row
            for j in rng.randint(len(nodes), size=2):
                with np.errstate(over="ignore"):
                    X[r, nodes[j][0]] = np.float32(nodes[j][1])
    return X


def _set_types(model, seed, types):
    rng = np.random.RandomState(seed)
    for t in model["trees"]:
        if t["num_leaves"] > 1:
            t["decision_type"] = rng.choice(types, size=t["num_leaves"] - 1).astype(np.int64)
    return model


def _with_one_leaf_trees(model):
    """one-leaf trees first, in the middle and last"""
    t = model["trees"]
    m = len(t) // 2
    model["trees"] = [_one_leaf(0.37)] + t[:m] + [_one_leaf(-1.25)] + t[m:] + [_one_leaf(0.011)]
    return model


def _categorical_forest():
    """9 trees of 8 leaves over 8 features; trees 0, 3, 6 carry three categorical splits each (bitsets of 1, 2 and 5
    words, different words per tree) on features 0..2; tree 3 keeps its other nodes numerical with zero- and
    NaN-missing types; the numerical trees mix all missing types."""
    model = _set_types(G.random_forest_model(9, 8, 8, seed=91), 92, [2, 0, 4, 6, 8, 10])
    rng = np.random.RandomState(93)
    for ti in (0, 3, 6):
        t = model["trees"][ti]
        cat_nodes = [0, 2, 5]                             # the root and two inner nodes
        words = []
        for ci, (node, nw) in enumerate(zip(cat_nodes, (1, 2, 5))):
            t["decision_type"][node] = 1
            t["threshold"][node] = float(ci)
            t["split_feature"][node] = ci                 # features 0..2 hold category codes
            words += [int(w) for w in rng.randint(0, 2 ** 32, size=nw, dtype=np.uint64)]
        others = [i for i in range(7) if i not in cat_nodes]
        t["decision_type"][others] = [4, 10, 6, 8] if ti == 3 else 2
        for i in others:
            t["split_feature"][i] = 3 + rng.randint(5)    # numerical nodes stay off the category columns
        t["num_cat"] = 3
        t["cat_boundaries"] = np.array([0, 1, 3, 8])
        t["cat_threshold"] = np.array(words, dtype=np.int64)
    return model


def _categorical_X(n, seed):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, 8).astype(np.float32)
    X[rng.rand(n, 8) < 0.1] = np.nan
    X[rng.rand(n, 8) < 0.1] = 0.0
    # category codes: in and out of the sets, past the 1-, 2- and 5-word bitsets (>= 32, 64, 160), negative, fractional
    # (3.7 reads as 3, -0.5 as 0), NaN and far above INT_MAX
    codes = np.concatenate([np.arange(0, 170, dtype=np.float32),
                            np.array([-1, -7, -0.5, 3.7, 31.9, 63.5, 159.9, 160, 1e6, 3e9, np.nan, np.nan], np.float32)])
    X[:, :3] = rng.choice(codes, size=(n, 3))
    return X


def _beyond_f32_forest():
    model = G.random_forest_model(6, 16, 4, seed=71)
    rng = np.random.RandomState(72)
    for t in model["trees"]:
        hit = rng.rand(15) < 0.6
        t["threshold"][hit] = rng.choice([1e300, -1e300, FLT_MAX, -FLT_MAX], size=int(hit.sum()))
    return model


def _global_forest(reverse):
    big = G.random_forest_model(1, 1300, 50, seed=81)["trees"] + G.random_forest_model(1, 1600, 50, seed=82)["trees"]
    model = G.random_forest_model(10, 31, 50, seed=83)
    model["trees"] = big + model["trees"]
    if reverse:
        model["trees"] = model["trees"][::-1]
    return _set_types(model, 84, [2, 2, 0, 6, 8])


def _ncu():
    """the library's workgroup-count constant, read from its source rather than restated here"""
    return int(re.search(r"#define\s+RIHIP_NCU\s+(\d+)", (ROOT / "recommendit_amd/csrc/common.h").read_text()).group(1))


def _striding_rows(model, per_cu):
    """smallest n (plus an odd tail) at which a compact kernel's workgroups stride over candidate tiles: the launch of
    rihip_gbdt_predict gives a chunk ceil(per_cu * NCU / n_chunks) workgroups, capped by the n_tiles = ceil(n / 64)"""
    n_chunks = len(G.predict_plan(model)["chunks"]) - 1
    per_chunk = -(-per_cu * _ncu() // n_chunks)
    return 64 * (per_chunk + 1) + 5, per_chunk


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """name -> (model, X, expected path), built once and never modified"""
    avg = False
    if name in ("simple8_32x65", "simple8_40x65"):
        model = G.random_forest_model(int(name[8:10]), 65, 50, seed=11)
        X, path = _edge_X(model, 4100, 12), G.PATH_COMPACT_SIMPLE
    elif name in ("walk_1_feature", "walk_2_features"):
        model = G.random_forest_model(8, 100, int(name[5]), seed=21)
        X, path = _edge_X(model, 700, 22), G.PATH_WALK
    elif name == "walk_record_cap":
        model = G.random_forest_model(64, 64, 20, seed=31)
        X, path = _edge_X(model, 1500, 32), G.PATH_WALK
    elif name == "walk_beyond_f32":
        model = _beyond_f32_forest()
        X = _edge_X(model, 600, 73, extra=np.array([np.inf, -np.inf, FLT_MAX, -FLT_MAX], np.float32))
        path = G.PATH_WALK
    elif name == "missing8_striding":
        model = _set_types(G.random_forest_model(400, 8, 12, seed=41), 42, [2, 0, 4, 6, 8, 10])
        rng = np.random.RandomState(43)
        for t in model["trees"]:                          # thresholds that make the tiny inputs decisive
            hit = rng.rand(7) < 0.25
            t["threshold"][hit] = rng.choice([0.0, 1e-40, -1e-40, 1e-35, -1e-35, 2e-35], size=int(hit.sum()))
        n, _ = _striding_rows(model, 3)
        X, path = _edge_X(model, n, 44, extra=TINY), G.PATH_COMPACT_MISSING
    elif name in ("global_memory", "global_memory_reversed"):
        model = _global_forest(name.endswith("reversed"))
        X, path = _edge_X(model, 1500, 85, extra=TINY), G.PATH_GENERAL
    elif name == "categorical":
        model = _categorical_forest()
        X, path = _categorical_X(900, 94), G.PATH_GENERAL
    elif name.startswith("one_leaf_"):
        path = int(name[-1])
        model = G.random_forest_model(9, 16, 5, seed=51)
        if path == G.PATH_COMPACT_MISSING:
            _set_types(model, 52, [2, 4, 10])
        if path == G.PATH_GENERAL:
            model["trees"][3:4] = G.random_forest_model(1, 200, 5, seed=53)["trees"]     # > 127 nodes: not compact
        _with_one_leaf_trees(model)
        X = _edge_X(model, 300, 54, extra=TINY)
    elif name == "only_one_leaf_trees":
        model = G.random_forest_model(1, 2, 3, seed=55)
        model["trees"] = [_one_leaf(v) for v in (0.5, -0.125, 3.0, 1e-3, -7.25)]
        X, path = np.random.RandomState(56).randn(130, 3).astype(np.float32), G.PATH_GENERAL
    elif name in ("average_path_0", "average_path_3"):
        avg = True
        path = int(name[-1])
        model = G.random_forest_model(7, 24, 6, seed=61)
        if path == G.PATH_GENERAL:
            model["trees"][2:3] = G.random_forest_model(1, 200, 6, seed=62)["trees"]
        X = _edge_X(model, 500, 63)
    else:
        raise KeyError(name)
    model["average_output"] = avg
    X.setflags(write=False)
    return model, X, path


@functools.lru_cache(maxsize=None)
def _case(name):
    """_inputs(name) + the oracle's scores and the sum of |leaf| every row reached, computed once for all tests"""
    model, X, path = _inputs(name)
    ref, ref_abs = G.predict_raw(model, X, return_abs=True)
    ref.setflags(write=False); ref_abs.setflags(write=False)
    return model, X, path, ref, ref_abs


FOREST_CASES = ["simple8_32x65", "simple8_40x65", "walk_1_feature", "walk_2_features", "walk_record_cap",
                "walk_beyond_f32", "missing8_striding", "global_memory", "global_memory_reversed", "categorical",
                "one_leaf_path_0", "one_leaf_path_1", "one_leaf_path_3", "only_one_leaf_trees", "average_path_0",
                "average_path_3"]


def expected_paths():
    """{case: (model, expected path)} for the host-side check of the path arithmetic"""
    return {name: (_inputs(name)[0], _inputs(name)[2]) for name in FOREST_CASES}


def _check_scores(name, model, got, ref, ref_abs):
    T = len(model["trees"])
    bound = (T - 1) * U53 * ref_abs
    if model.get("average_output"):
        bound = bound / T + U53 * np.abs(ref)
    err = np.abs(got - ref)
    assert np.isfinite(got).all()
    pos = bound > 0
    _report(f"forest {name} n={len(got)} |got-ref|/bound", float((err[pos] / bound[pos]).max()) if pos.any() else 0.0)
    assert (err <= bound).all(), (name, int(np.argmax(err - bound)), float(err.max()))


@functools.lru_cache(maxsize=None)
def _forest_of(name):
    return _load(_inputs(name)[0])


@pytest.mark.parametrize("name", FOREST_CASES)
def test_forest_case_against_oracle(name):
    """the case's kernel is the one it was written for; every row within the summation bound of the oracle; two calls
    bitwise equal; the first rows predicted alone bitwise equal to their part of the batch"""
    model, X, path, ref, ref_abs = _case(name)
    f = _forest_of(name)
    _assert_path(f, path)
    got = _predict(f, X)
    _check_scores(name, model, got, ref, ref_abs)
    assert _same_bits(got, _predict(f, X))
    for m in (1, 63, 65):
        assert _same_bits(_predict(f, X[:m]), got[:m]), m


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("name", ["simple8_32x65", "simple8_40x65"])
def test_compact_simple_kernel_batch_sizes(name, n):
    """gbdt_predict8_kernel<true> (a chunk of 32 trees x 65 leaves = 4160 walk records > 4096) on one lane, a tile
    short of one lane, a full tile and one lane more; n = 4100 is test_forest_case_against_oracle"""
    model, X, path, ref, ref_abs = _case(name)
    f = _forest_of(name)
    _assert_path(f, G.PATH_COMPACT_SIMPLE)
    _check_scores(name, model, _predict(f, X[:n]), ref[:n], ref_abs[:n])


def test_compact_missing_kernel_strides_over_tiles():
    """the case 'missing8_striding' has more candidate tiles than workgroups per chunk, by the launch rule of
    rihip_gbdt_predict, and its inputs hold both float32 neighbours of 1e-35 with both signs, denormals and -0.0"""
    model, X, path = _inputs("missing8_striding")
    n, per_chunk = _striding_rows(model, 3)
    assert X.shape[0] == n and (n + 63) // 64 > per_chunk
    assert float(ZERO_LO) <= G.K_ZERO < float(ZERO_HI)
    for v in TINY[:8]:
        assert (_bits(X) == _bits(np.array([v]))[0]).any(), v
    assert (_bits(X) == 0x80000000).any()
    types = np.concatenate([t["decision_type"] for t in model["trees"]])
    assert {0, 1, 2} <= set(((types >> 2) & 3).tolist())


@pytest.mark.parametrize("name", ["global_memory", "missing8_striding", "simple8_32x65", "walk_1_feature"])
def test_row_stride_wider_than_the_model(name):
    """ldx = n_features + 5 with NaN in the extra columns, through the base pointer of a strided view: bitwise the
    contiguous call"""
    L, lib, dev, st = _L()
    _, X, path = _inputs(name)
    X = X[:200]
    f = _forest_of(name)
    _assert_path(f, path)
    n, nf = X.shape
    wide = torch.full((n * (nf + 5),), float("nan"), dtype=torch.float32, device=dev)
    view = torch.as_strided(wide, (n, nf), (nf + 5, 1))
    view.copy_(_dev(X, dev))
    assert bool(torch.isnan(wide.view(n, nf + 5)[:, nf:]).all())
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    L.check(lib.rihip_gbdt_predict(f._h, view.data_ptr(), n, nf + 5, out.data_ptr(), st), "gbdt_predict")
    assert _same_bits(out.cpu().numpy(), _predict(f, X))


def test_forest_status_codes():
    L, lib, dev, st = _L()
    f = _forest_of("walk_2_features")
    X = torch.zeros((4, 2), dtype=torch.float32, device=dev)
    out = torch.full((4,), 7.5, dtype=torch.float64, device=dev)
    assert lib.rihip_gbdt_predict(f._h, X.data_ptr(), 4, 1, out.data_ptr(), st) == ERR_SHAPE     # ldx < n_features
    assert lib.rihip_gbdt_predict(f._h, X.data_ptr(), 0, 2, out.data_ptr(), st) == OK            # n = 0: nothing written
    assert (out.cpu().numpy() == 7.5).all()
    text = G.write_text_model(G.random_forest_model(2, 4, 129, seed=1)).encode()                 # 129 features > 128
    h = ctypes.c_void_p()
    assert lib.rihip_gbdt_create_from_text(text, len(text), ctypes.byref(h)) == ERR_SHAPE
    assert not h.value
    text = G.write_text_model(G.random_forest_model(2, 4, 128, seed=1)).encode()
    assert lib.rihip_gbdt_create_from_text(text, len(text), ctypes.byref(h)) == OK
    assert lib.rihip_gbdt_num_features(h) == 128 and lib.rihip_gbdt_destroy(h) == OK


def test_predict_path_of_a_null_handle():
    assert _L()[1].rihip_gbdt_predict_path(None) == G.PATH_GENERAL


# =========================================================================================== feature assembly
N_UROWS, N_IROWS, GUARD = 37, 53, 777.0
CANON = 50


@functools.lru_cache(maxsize=None)
def _tables():
    """general float64 tables (products and sums that round); row 0 = the serving defaults; one guard row of 777 behind
    each table (an id compared with > instead of >= reads it, instead of memory the test does not own).
    User 5 x item 7 is a contraction probe: genre products 1 * 1 and (2^-12 (1 + 2^-30))^2.  Rounded one by one the
    sum is 1 + 2^-24 exactly, a float32 tie that casts to 1.0; with the second product fused into the addition the
    float64 sum is 1 + 2^-24 + 2^-52, which casts to 1 + 2^-23."""
    rng = np.random.default_rng(7)
    ut = rng.standard_normal((N_UROWS + 1, RF.USER_WIDTH)) * 2.5
    it = rng.standard_normal((N_IROWS + 1, RF.ITEM_WIDTH)) * 2.5
    ut[0, :6] = [d for _, d in RF.USER_SCALARS]; ut[0, 6:] = 0.0
    it[0, :5] = [d for _, d in RF.ITEM_SCALARS]; it[0, 5:] = 0.0
    it[10:20, 5:] = rng.integers(0, 2, size=(10, RF.N_GENRES))           # genre flags, as real item rows have them
    p = 2.0 ** -12 * (1 + 2.0 ** -30)
    ut[5, 6:] = 0.0; it[7, 5:] = 0.0
    ut[5, 6:8] = [1.0, p]; it[7, 5:7] = [1.0, p]
    ut[N_UROWS], it[N_IROWS] = GUARD, GUARD
    ut.setflags(write=False); it.setflags(write=False)
    return ut, it


USER_IDS = np.array([-1, 0, N_UROWS - 1, N_UROWS, 2 ** 40, 5, 17], dtype=np.int64)
CAND_ROW = np.array([-1, 0, N_IROWS - 1, N_IROWS, 7, 3, 12, 41, N_IROWS + 1000, 2 ** 40, 19], dtype=np.int64)


def _build_features(user_ids, cand, col_map, tail=64):
    L, lib, dev, st = _L()
    ut, it = _tables()
    utd, itd = _dev(ut, dev), _dev(it, dev)
    cand = np.ascontiguousarray(cand, dtype=np.int64)
    nq, kc = cand.shape
    nf = len(col_map)
    X = torch.full((nq * kc * nf + tail,), float("nan"), dtype=torch.float32, device=dev)
    uidd, candd, mapd = _dev(np.asarray(user_ids, np.int64), dev), _dev(cand, dev), _dev(np.asarray(col_map, np.int32), dev)
    L.check(lib.rihip_rank_features_build(utd.data_ptr(), N_UROWS, itd.data_ptr(), N_IROWS, uidd.data_ptr(),
                                          candd.data_ptr(), nq, kc, mapd.data_ptr(), nf, X.data_ptr(), st),
            "rank_features_build")
    X = X.cpu().numpy()
    assert np.isnan(X[nq * kc * nf:]).all()                              # nothing written behind the matrix
    ref = RF.table_feature_matrix(ut[:N_UROWS], it[:N_IROWS], user_ids, cand, col_map)
    return X[:nq * kc * nf].reshape(nq * kc, nf), ref


def _col_maps():
    rng = np.random.RandomState(3)
    perm = rng.permutation(CANON)
    twice = np.arange(CANON); twice[[2, 40]] = 13; twice[49] = 12        # genre_affinity three times, the ratio twice
    holes = np.concatenate([[-1], perm[:30], [-1, -1], perm[30:], [-1] * 11])                     # 64 wide
    wide65 = np.concatenate([[-1], rng.randint(CANON, size=30), [-1, -1], perm, [13, 12], [-1]])  # 86 -> cut to 65
    wide128 = np.concatenate([[-1, 13], rng.randint(CANON, size=60), [-1], perm, np.arange(CANON)[:14], [-1]])
    assert len(holes) == 64 and len(wide128) == 128
    return {"canonical_50": np.arange(CANON), "shuffled_50": perm, "same_column_twice_50": twice,
            "affinity_only_1": np.array([13]), "ratio_only_1": np.array([12]), "unknown_columns_64": holes,
            "thread_65": wide65[:65], "thread_128": wide128}


@pytest.mark.parametrize("name", list(_col_maps()))
def test_rank_features_column_maps_and_ids(name):
    """1, 50 and 64 columns on the wave kernel, 65 and 128 on the thread kernel, bit-equal to the float64 reference:
    user ids -1, 0, last row, one past it and 2^40; candidate ids -1 (row of zeros), 0, last row, one past it (the
    defaults row) and far beyond; the contraction probe of _tables()"""
    col_map = _col_maps()[name]
    assert (col_map < CANON).all() and len(col_map) == int(name.rsplit("_", 1)[1])
    cand = np.stack([np.roll(CAND_ROW, q) for q in range(len(USER_IDS))])
    got, ref = _build_features(USER_IDS, cand, col_map)
    assert _same_bits(got, ref), np.argwhere(_bits(got) != _bits(ref))[:5]
    assert not got[cand.reshape(-1) < 0].any()
    if 13 in col_map:                                                    # the probe pair is in the batch and decisive
        row = 5 * cand.shape[1] + int(np.where(cand[5] == 7)[0][0])
        assert ref[row, list(col_map).index(13)] == 1.0


def test_rank_features_wave_and_thread_kernels_agree():
    """the same 50 canonical columns inside a 64-wide map (wave kernel) and a 65-wide map (thread kernel): both equal
    to the reference, hence to each other, bit for bit"""
    perm = np.random.RandomState(4).permutation(CANON)
    m64 = np.concatenate([[-1] * 5, perm, [-1] * 9])
    m65 = np.concatenate([m64, [-1]])
    cand = np.stack([np.roll(CAND_ROW, q) for q in range(len(USER_IDS))])
    g64, r64 = _build_features(USER_IDS, cand, m64)
    g65, r65 = _build_features(USER_IDS, cand, m65)
    assert _same_bits(g64, r64) and _same_bits(g65, r65)
    assert _same_bits(g64[:, 5:55], g65[:, 5:55])


@pytest.mark.parametrize("nf", [50, 65])
@pytest.mark.parametrize("nq,kc", [(1, 1), (3, 1), (1, 3), (2, 2), (4, 1), (5, 1), (1, 5)])
def test_rank_features_small_batches(nq, kc, nf):
    """1, 3, 4 and 5 rows (the wave kernel takes four rows per block), kc = 1"""
    col_map = np.concatenate([np.arange(CANON), [13] * 15])[:nf]
    user_ids = np.array([5, 17, 2 ** 40, 0, 36])[:nq]
    cand = np.array([7, 12, -1, N_IROWS, 52]).reshape(-1)[:nq * kc].reshape(nq, kc)
    got, ref = _build_features(user_ids, cand, col_map)
    assert _same_bits(got, ref)


def test_rank_features_wave_kernel_grid_stride():
    """2 x 33 000 candidates x 64 columns: more rows than the wave kernel's 4 x 16 384 per pass"""
    rng = np.random.RandomState(6)
    cand = rng.randint(-1, N_IROWS + 3, size=(2, 33000)).astype(np.int64)
    cand[1, -1] = 7
    got, ref = _build_features(np.array([17, 5]), cand, _col_maps()["unknown_columns_64"])
    assert 2 * 33000 > 4 * 16384
    assert _same_bits(got, ref)


# =========================================================================================== final top-k
def _topk_ref(s, cand, rs, k):
    """stable sort on (class, -score, position): numbers < NaN < padding; -0.0 orders as +0.0.  Slots past the kc
    candidates are filled with -1 / -inf; a padded candidate returns its id and -inf as its score."""
    nq, kc = s.shape
    ids = np.full((nq, k), -1, np.int64)
    sc = np.full((nq, k), -np.inf, np.float64)
    out_rs = np.full((nq, k), -np.inf, np.float32)
    m = min(k, kc)
    for q in range(nq):
        real = cand[q] >= 0
        cls = np.where(~real, 2, np.where(np.isnan(s[q]), 1, 0))
        neg = np.where(cls == 0, -np.where(s[q] == 0, 0.0, s[q]), 0.0)
        j = np.lexsort((np.arange(kc), neg, cls))[:m]
        ids[q, :m] = cand[q][j]
        sc[q, :m] = np.where(real[j], s[q][j], -np.inf)
        out_rs[q, :m] = rs[q][j]
    return ids, sc, out_rs


def _topk(s, cand, rs, k):
    L, lib, dev, st = _L()
    nq, kc = s.shape
    ids = torch.full((nq * k + 8,), -77, dtype=torch.int64, device=dev)
    top = torch.full((nq * k + 8,), 77.0, dtype=torch.float64, device=dev)
    trs = torch.full((nq * k + 8,), 77.0, dtype=torch.float32, device=dev)
    sd, candd, rsd = _dev(s, dev), _dev(cand, dev), _dev(rs, dev)
    L.check(lib.rihip_rank_topk(sd.data_ptr(), candd.data_ptr(), rsd.data_ptr(), nq, kc, k, ids.data_ptr(), top.data_ptr(),
                                trs.data_ptr(), st), "rank_topk")
    ids, top, trs = ids.cpu().numpy(), top.cpu().numpy(), trs.cpu().numpy()
    assert (ids[nq * k:] == -77).all() and (top[nq * k:] == 77.0).all() and (trs[nq * k:] == 77.0).all()
    return ids[:nq * k].reshape(nq, k), top[:nq * k].reshape(nq, k), trs[:nq * k].reshape(nq, k)


def _check_topk(s, cand, rs, k):
    s, cand, rs = np.asarray(s, np.float64), np.asarray(cand, np.int64), np.asarray(rs, np.float32)
    got = _topk(s, cand, rs, k)
    ref = _topk_ref(s, cand, rs, k)
    for g, r, what in zip(got, ref, ("ids", "scores", "retrieval scores")):
        assert _same_bits(g, r), (what, np.argwhere(_bits(g) != _bits(r))[:5])


def _topk_inputs(rng, nq, kc, values):
    s = rng.choice(np.asarray(values, np.float64), size=(nq, kc))
    cand = rng.permutation(nq * kc).reshape(nq, kc).astype(np.int64) + 3
    rs = rng.rand(nq, kc).astype(np.float32)
    return s, cand, rs


def _pad(cand, rs, mask):
    cand[mask] = -1
    rs[mask] = -np.inf
    return cand, rs


QNAN, QNAN_NEG, QNAN_PAYLOAD = (np.array([b], np.uint64).view(np.float64)[0]
                                for b in (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000123))


def test_rank_topk_five_distinct_scores():
    """a forest emits many exact ties: 500 candidates over 5 score values (both infinities among them), a few NaN of
    three bit patterns and a few padded slots anywhere in the list"""
    rng = np.random.RandomState(10)
    s, cand, rs = _topk_inputs(rng, 4, 500, [-np.inf, -1.5, 0.25, 0.25000000000000006, np.inf])
    s[rng.rand(4, 500) < 0.02] = QNAN
    s[0, 3], s[1, 499], s[2, 0] = QNAN_NEG, QNAN_PAYLOAD, QNAN_PAYLOAD
    _pad(cand, rs, rng.rand(4, 500) < 0.03)
    _check_topk(s, cand, rs, 20)
    _check_topk(s, cand, rs, 500)                                        # the whole order, NaN and padding at its end


def test_rank_topk_all_scores_equal():
    rng = np.random.RandomState(11)
    s, cand, rs = _topk_inputs(rng, 3, 200, [0.125])
    _check_topk(s, cand, rs, 20)
    _check_topk(s, cand, rs, 200)


def test_rank_topk_signed_zeros_tie():
    """-0.0 and +0.0 are equal to DataFrame.nlargest: retrieval order decides among them, and the score comes back with
    the sign it had"""
    rng = np.random.RandomState(12)
    s, cand, rs = _topk_inputs(rng, 3, 100, [0.0])
    s[:, ::2] = -0.0                                                     # -0.0 first: it must stay first
    s[1, 50:] = -1.0
    s[2, 7] = 1.0
    _check_topk(s, cand, rs, 20)
    _check_topk(s, cand, rs, 100)
    got_scores = _topk(s, cand, rs, 4)[1]
    assert _same_bits(got_scores[0], np.array([-0.0, 0.0, -0.0, 0.0]))


def test_rank_topk_all_padded_and_all_nan():
    rng = np.random.RandomState(13)
    s, cand, rs = _topk_inputs(rng, 2, 70, [1.0, 2.0])
    _pad(cand, rs, np.ones_like(cand, bool))
    _check_topk(s, cand, rs, 10)
    s, cand, rs = _topk_inputs(rng, 2, 70, [QNAN, QNAN_NEG, QNAN_PAYLOAD])
    _check_topk(s, cand, rs, 10)
    _check_topk(s, cand, rs, 80)


@pytest.mark.parametrize("kc", [1, 63, 64, 65, 200])
def test_rank_topk_edge_sizes(kc):
    """k = 1, kc, kc + 7 (more outputs than candidates) and 300; kc on both sides of the 64-slot sort width"""
    rng = np.random.RandomState(kc)
    s, cand, rs = _topk_inputs(rng, 3, kc, list(rng.randn(7)) + [0.0, -0.0, QNAN])
    _pad(cand, rs, rng.rand(3, kc) < 0.05)
    for k in (1, kc, kc + 7, 300):
        _check_topk(s, cand, rs, k)


def test_rank_topk_status_codes():
    L, lib, dev, st = _L()
    z = torch.zeros(16, dtype=torch.float64, device=dev)
    zi = torch.zeros(16, dtype=torch.int64, device=dev)
    zf = torch.zeros(16, dtype=torch.float32, device=dev)
    oi = torch.full((16,), -77, dtype=torch.int64, device=dev)

    def call(nq, kc, k):
        return lib.rihip_rank_topk(z.data_ptr(), zi.data_ptr(), zf.data_ptr(), nq, kc, k, oi.data_ptr(), z.data_ptr(),
                                   zf.data_ptr(), st)
    assert call(0, 4, 2) == OK                                           # nq = 0: nothing to do, nothing written
    assert (oi.cpu().numpy() == -77).all()
    assert call(1, 0, 1) == ERR_ARG and call(1, 4, 0) == ERR_ARG and call(1, 16385, 1) == ERR_ARG
    assert (oi.cpu().numpy() == -77).all()
