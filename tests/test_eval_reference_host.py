"""CPU-only checks of the evaluation-kernel tests' own infrastructure (tests/eval_reference.py):

* the restated reference reproduces every G10 case (the reference project's own outputs) and equals
  recommendit_amd.metrics per user, with ==, on the new cases -- the one place where metrics is imported;
* the exact-diversity generator: every row norm a power of two, and an f64 and an f32 evaluation of every per-user
  value agree bit for bit;
* every case of tests/test_gpu_eval_kernels.py reaches the kernel regions it names, through the mirrors of the loop
  structure of csrc/eval.hip -- without this nobody can tell whether a row leaves the first 512-id chunk at all;
* the comparison helpers go red for one dropped pair and name the first wrong (user, k-index, metric);
* the regression note: the older diversity comparison (1e-5 max(|d|, 1)) accepts structural errors;
* GroundTruth.csr_from_pairs (static, NumPy only).
"""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import eval_reference as R  # noqa: E402

from recommendit_amd import metrics as M  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------
# the reference against G10 and against recommendit_amd.metrics
# ---------------------------------------------------------------------------------------------------------------------
def _g10_case(case):
    users = [u for u, _ in case["recs"]]
    truth = {u: t for u, t in case["truth"]}
    K = max([len(r) for _, r in case["recs"]] + [1])
    rec = np.full((len(users), K), -1, np.int64)
    for i, (_, r) in enumerate(case["recs"]):
        rec[i, :len(r)] = r
    tab = present = None
    if case["vectors"]:
        rows = max(i for i, _ in case["vectors"]) + 1
        tab = np.zeros((rows, len(case["vectors"][0][1])), case["vec_dtype"])
        present = np.zeros(rows, np.uint8)
        for i, v in case["vectors"]:
            tab[i], present[i] = v, 1
    return R.Case("g10", rec, [list(truth.get(u) or []) for u in users], list(case["k_values"]),
                  catalog_size=case["catalog_size"], tab=tab, present=present), users


def test_reference_reproduces_g10(golden_dir):
    cases = json.loads((golden_dir / "g10_evaluate_model.json").read_text())
    seen = set()
    for case in cases:
        report = dict(case["report"])
        if "error" in report:
            assert len(case["recs"]) == 0
            continue
        c, users = _g10_case(case)
        ref = R.case_reference(c)
        nsc = int(ref.scored.sum())
        on = ref.scored.astype(bool)
        for j, k in enumerate(ref.ks):
            for m, name in enumerate(("ndcg", "recall", "precision")):
                want = math.fsum(ref.vals[on, j, m].tolist()) / nsc if nsc else 0.0
                assert abs(want - report[f"{name}@{k}"]) <= 1e-12, (name, k)
        want = math.fsum(ref.mrr[on].tolist()) / nsc if nsc else 0.0
        assert abs(want - report["mrr"]) <= 1e-12
        assert ("coverage" in report) == bool(c.catalog_size and nsc)
        if "coverage" in report:
            assert abs(ref.coverage - report["coverage"]) <= 1e-12
            seen.add("coverage")
        assert ("avg_diversity" in report) == (c.tab is not None and nsc > 0)
        if "avg_diversity" in report:
            # the fixture's values carry the float32 residue of the reference's pair arithmetic: the pairwise form
            divs = [R.user_diversity_pairwise(c.rec[i].tolist(), c.ks[-1], c.tab, c.present)
                    for i in np.nonzero(on)[0]]
            want = math.fsum(divs) / nsc
            assert abs(want - report["avg_diversity"]) <= 1e-6 * max(abs(report["avg_diversity"]), 1e-30)
            seen.add("diversity")
        for row in case["components"]:
            i = users.index(row["user"])
            rel = c.truth[i]
            ks = [pk["k"] for pk in row["per_k"]]
            if rel:
                v, rr = R.user_ranking(c.rec[i].tolist(), rel, ks)
            else:   # the component functions are also recorded for users without truth: all 0
                v, rr = [(0.0, 0.0, 0.0)] * len(ks), 0.0
            assert abs(rr - row["mrr"]) <= 1e-12
            for (nd, rc, pr), pk in zip(v, row["per_k"]):
                assert abs(nd - pk["ndcg"]) <= 1e-12 and abs(rc - pk["recall"]) <= 1e-12, (row["user"], pk)
                if rel:   # precision does not depend on the truth being non-empty only through the hits: 0 either way
                    assert abs(pr - pk["precision"]) <= 1e-12, (row["user"], pk)
                else:
                    assert pk["precision"] == 0.0
            if "ild" in row:
                got = R.user_diversity_pairwise(c.rec[i].tolist(), c.ks[-1], c.tab, c.present)
                assert got == pytest.approx(row["ild"], rel=1e-6, abs=1e-30)
                # and the vectorised f64 form used everywhere else is that value up to float32 rounding of a term
                f64 = R.user_diversity(c.rec[i].tolist(), c.ks[-1], c.tab.astype(np.float64), c.present)
                assert abs(f64 - got) <= 4 * 2.0 ** -24, (row["user"], f64, got)
                seen.add("ild")
    assert seen == {"coverage", "diversity", "ild"}


def _metrics_equal(case: R.Case, rows) -> None:
    ref = R.case_reference(case)
    for i in rows:
        lst, rel = R.listed(case.rec[i].tolist()), case.truth[i]
        if not rel:
            assert not ref.scored[i] and not ref.vals[i].any() and ref.mrr[i] == 0
            continue
        for j, k in enumerate(ref.ks):
            assert ref.vals[i, j, 0] == M.ndcg_at_k(lst, rel, k), (case.name, i, k)
            assert ref.vals[i, j, 1] == M.recall_at_k(lst, rel, k), (case.name, i, k)
            assert ref.vals[i, j, 2] == M.precision_at_k(lst, rel, k), (case.name, i, k)
        assert ref.mrr[i] == M.mrr(lst, rel), (case.name, i)


def test_reference_equals_metrics_per_user_on_the_new_cases():
    c = R.segment_case()
    _metrics_equal(c, range(c.rec.shape[0]))
    for K in (1, 65, 513, 1025, 2000):
        c = R.row_length_case(K)
        _metrics_equal(c, range(c.rec.shape[0]))
    c = R.row_length_case(1025, "wait")
    _metrics_equal(c, range(c.rec.shape[0]))
    _metrics_equal(R.k_list_case(29), range(0, 1100, 23))
    _metrics_equal(R.k_list_case(64, n=24, K=2000, kmax=2000), range(0, 24, 5))
    _metrics_equal(R.stride_case(), range(0, 70000, 97))
    c = R.diversity_case(7, 33)
    _metrics_equal(c, range(c.rec.shape[0]))


# ---------------------------------------------------------------------------------------------------------------------
# exact inputs for diversity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", sorted({g for g, _ in R.DIVERSITY_SHAPES}))
def test_exact_table_rows(g):
    tab = R.exact_table(100 + g, R.DIV_ROWS, g)
    assert tab.dtype == np.float32 and tab.shape == (R.DIV_ROWS, g)
    nz = (tab != 0).sum(axis=1)
    assert set(nz.tolist()) <= {0, 1, 4, 16, 64} and (nz == 0).any() and (nz > 0).sum() > 200
    mag = np.abs(tab).max(axis=1)
    assert ((np.abs(tab) == mag[:, None]) | (tab == 0)).all()            # one magnitude per row
    assert set(np.unique(mag[mag > 0]).tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0}
    sq = (tab.astype(np.float64) ** 2).sum(axis=1)
    e = np.log2(sq[sq > 0])
    assert (e == np.round(e)).all() and (e % 2 == 0).all() and sq.max() < 2 ** 24     # powers of four
    norm = np.sqrt(sq[sq > 0])
    assert (np.log2(norm) == np.round(np.log2(norm))).all()
    # the edge columns of the two lane halves are used, and the pair terms vary (a dropped pair moves a mean)
    H = (g + 1) // 2
    used = (tab != 0).any(axis=0)
    assert used[g - 1] and used[H - 1] and used[H % g] and used[0]
    if g > 1:
        X = tab[nz > 0].astype(np.float64)
        C = (X @ X.T) / np.sqrt(np.outer(sq[nz > 0], sq[nz > 0]))
        assert len(np.unique(C[np.triu_indices(len(X), 1)])) >= 3


@pytest.mark.parametrize("g,L", R.DIVERSITY_SHAPES)
def test_exact_diversity_is_the_same_in_f32_and_f64(g, L):
    c = R.diversity_case(g, L)
    for i in range(c.rec.shape[0]):
        row = c.rec[i].tolist()
        a, b = R.user_diversity(row, L, c.tab, c.present), R.user_diversity_f32(row, L, c.tab, c.present)
        assert a == b, (i, a, b)
        # every term is on the 2^-14 grid: the sum is exact, so the value is (integer / 2^14) / count
        assert 0.0 <= a <= 2.0


def test_exact_diversity_stride_case_in_f32_and_f64():
    c = R.diversity_stride_case()
    rows = np.unique(c.rec, axis=0)
    assert len(rows) == 4096
    vals = set()
    for row in rows.tolist():
        a = R.user_diversity(row, 4, c.tab, c.present)
        assert a == R.user_diversity_f32(row, 4, c.tab, c.present)
        vals.add(a)
    assert len(vals) >= 8


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases reach the regions they name
# ---------------------------------------------------------------------------------------------------------------------
def test_segment_case_reaches_both_searches_at_every_size():
    c = R.segment_case()
    assert c.rec.shape == (40, 96)
    reg = c.regions(cov=False)
    ref = R.case_reference(c)
    for cnt in R.SEGMENT_SIZES:
        for i in range(c.notes[cnt], c.notes[cnt] + 4):
            t = c.truth[i]
            assert len(set(t)) == cnt and len(t) > cnt                    # raw > cnt
            assert reg[i]["search"] == ("small" if cnt <= 64 else "global")
            assert ref.vals[i, :, 1].max() > 0                            # hits
        items = sorted(set(c.truth[c.notes[cnt]]))
        row = R.listed(c.rec[c.notes[cnt]].tolist())
        # below the smallest, above the largest, equal to the first and the last, one off each
        for x in (items[0] - 1, 0, items[-1] + 1, items[0], items[-1], items[0] + 1, items[-1] - 1):
            assert x in row
        assert items[0] - 1 not in items and (cnt == 1 or items[0] + 1 not in items) and items[-1] + 1 not in items
        # the second and third rows ask for the first 45 and the last 45 items, each next to a non-member
        row_b = R.listed(c.rec[c.notes[cnt] + 1].tolist())
        assert set(items[:45]) <= set(row_b) and any(x not in items for x in row_b)


def test_row_length_cases_reach_every_chunk_region():
    for K in R.ROW_LENGTHS:
        lists = ("mixed",) if K <= 512 else ("exit1", "wait", "never", "zero")
        for kl in lists:
            c = R.row_length_case(K, kl)
            no, cov = c.regions(cov=False), c.regions(cov=True)
            nt = c.notes
            trips = -(-K // 512)
            assert cov[nt["hits_at_chunk_edges"]]["trips"] == trips
            assert all(r["trips"] == (trips if r["search"] != "none" else 0) for r in cov)    # <true> never exits
            assert no[nt["no_truth"]]["search"] == "none"
            assert no[nt["all_holes"]]["nvalid"] == 0 and no[nt["all_holes"]]["trips"] == trips
            assert no[nt["no_hit"]]["trips"] == trips and not no[nt["no_hit"]]["early_exit"]
            ls = c.rec[nt["only_last_step"]]
            assert (ls[:(K - 1) // 64 * 64] < 0).all() and ls[K - 1] == 7
            if K > 512:
                assert cov[nt["hits_at_chunk_edges"]]["hit_after_first_chunk"]
                assert cov[nt["hits_at_chunk_edges_holes"]]["compacted_differs"]
            if K >= 516:
                r = c.rec[nt["raw515_compacted509"]]
                assert r[515] == 7 and (r[:515] >= 0).sum() == 509 and 510 in R.ROW_K_LISTS["exit1"](K)
                assert cov[nt["raw515_compacted509"]]["first"] == 509
                assert cov[nt["raw515_compacted509"]]["compacted_differs"]
                assert cov[nt["mixed_hits_holes"]]["compacted_differs"]
                assert cov[nt["first_hit_in_chunk_two"]]["first"] == 520
            if K >= 1024:
                assert cov[nt["only_last_chunk"]]["first"] == 200 and cov[nt["only_last_chunk"]]["compacted_differs"]
                assert (c.rec[nt["only_last_chunk"]][:K - 300] < 0).all()
            more = K > 512 and trips > 1
            if kl == "exit1":
                assert c.kmax == 510 and no[nt["hits_at_chunk_edges"]]["early_exit"]
            if kl == "exit1" and K >= 516:      # kmax = 510 <= nvalid after chunk one
                assert no[nt["exit_after_chunk_one"]]["early_exit"] and no[nt["exit_after_chunk_one"]]["trips"] == 1
                assert no[nt["hit_first"]]["early_exit"]
                # later hits exist beyond kmax: they must count for nothing
                assert (c.rec[nt["exit_after_chunk_one"]][512:] == 7).sum() == 3
                # the first hit only in chunk two: no exit after chunk one although nvalid >= kmax
                r = no[nt["first_hit_in_chunk_two"]]
                assert r["trips"] >= 2 and r["early_exit"] == (trips > 2)
                # 506 valid ids in chunk one < kmax: goes on and finds the hit at compacted 509
                assert no[nt["raw515_compacted509"]]["trips"] >= 2
            if kl == "wait" and K >= 516:       # kmax = 600 > 512: the exit waits for chunk two
                assert c.kmax == 600
                r = no[nt["exit_after_chunk_one"]]
                assert r["trips"] == min(2, trips) and r["early_exit"] == (trips > 2)
            if kl == "never":      # kmax above K
                assert c.kmax > K and not any(r["early_exit"] for r in no)
            if kl == "zero" and K >= 516:       # kmax = 0: out as soon as a chunk has seen a hit
                assert c.kmax == 0
                assert no[nt["hit_first"]]["trips"] == 1 and no[nt["hit_first"]]["early_exit"] == more
                assert no[nt["first_hit_in_chunk_two"]]["trips"] == 2
    # the three-trip shapes take the exit after the second trip somewhere
    assert any(r["early_exit"] and r["trips"] == 2 for r in R.row_length_case(2000, "wait").regions(cov=False))
    assert R.row_length_case(16384).rec.shape[0] <= 12
    assert max(r["trips"] for r in R.row_length_case(16384, "never").regions(cov=False)) == 32


def test_k_list_cases_cover_both_rpi_and_every_lane():
    assert [R.reduce_rpi(n) for n in R.K_LIST_SIZES] == [85, 2, 2, 1, 1]
    assert R.reduce_rpi(28) == 3 and R.reduce_rpi(42) == 2 and R.reduce_rpi(43) == 1      # the two edges
    for n_k in R.K_LIST_SIZES:
        c = R.k_list_case(n_k)
        K = c.rec.shape[1]
        d = R.distinct(c.ks)
        assert len(d) == n_k and len(c.ks) > n_k                           # repeats
        assert d != sorted(d) or n_k == 1
        if n_k > 1:
            assert 0 in d and 1 in d and max(d) > K
            valid = (c.rec >= 0).sum(axis=1)
            assert (valid < np.median(d)).any()                            # k above a row's valid count
        assert R.reduce_partition(c.rec.shape[0])["per"] == 3              # rpi = 2 and rpi = 1 walk 3 rows differently
    c = R.k_list_case(64, n=24, K=2000, kmax=2000)
    assert len(R.distinct(c.ks)) == 64 and c.kmax == 2000
    assert max(r["trips"] for r in c.regions(cov=False)) == 4


def test_stride_and_partition_cases():
    c = R.stride_case()
    n = c.rec.shape[0]
    assert n == 70000 and R.rank_grid_stride(n) and not R.rank_grid_stride(32768) and R.rank_grid_stride(32769)
    assert all((len(t) == 0) == (i % 5 == 2) for i, t in enumerate(c.truth))
    assert {len(set(t)) for t in c.truth if t} == {1, 2, 4, 8}
    assert any(len(t) > len(set(t)) for t in c.truth)
    ref = R.case_reference(c)
    assert set(np.unique(ref.mrr).tolist()) == {0.0, 1.0, 0.5, 0.25, 0.125}
    for j in range(4):
        assert R.all_dyadic(ref.vals[:, j, 1]) and R.all_dyadic(ref.vals[:, j, 2])
    assert R.all_dyadic(ref.mrr) and not R.all_dyadic(ref.vals[:, 3, 0])
    p = R.reduce_partition(n)
    assert p == dict(per=137, used=511, empty=1, last=130)
    assert [R.reduce_partition(m) for m in R.PARTITION_SIZES] == [
        dict(per=1, used=1, empty=511, last=1), dict(per=1, used=511, empty=1, last=1),
        dict(per=1, used=512, empty=0, last=1), dict(per=2, used=257, empty=255, last=1),
        dict(per=3, used=342, empty=170, last=2)]
    # the bound is far below one user's contribution to a mean: a dropped or doubled row is seen
    on = ref.scored.astype(bool)
    assert R.mean_bound(n, ref.vals[on, 3, 0], int(on.sum())) < 1e-3 * ref.vals[on, 3, 0][ref.vals[on, 3, 0] > 0].min() / n


def test_coverage_cases():
    for S in R.COVERAGE_SPACES:
        c = R.coverage_case(S)
        ids = [set(R.listed(r.tolist())) for r in c.rec]
        assert max(max(s) for s in ids if s) == S - 1 and 0 in ids[c.notes["ends"]]
        assert c.rec[c.notes["ends"]][5] == S - 1
        res = c.notes["reserved"]
        assert bool(res) == (S > 3)
        if res:
            a, b, e = res
            assert {a, b} <= ids[1] and not c.truth[1] and all(a not in s and b not in s for s in ids[:1] + ids[2:])
            row = c.rec[c.notes["second_chunk"]]
            assert row[700] == e and (row == e).sum() == 1 and all(e not in s for s in ids[:2])
            ref = R.case_reference(c)
            want = len(ids[0] | ids[2])
            assert ref.coverage == want / (S + 3) and e in (ids[0] | ids[2]) and a not in (ids[0] | ids[2])
        assert [r["trips"] for r in c.regions(cov=True)] == [2, 0, 2, 2]


def test_diversity_cases_reach_every_path():
    assert {g for g, _ in R.DIVERSITY_SHAPES} == {1, 2, 3, 7, 8, 18, 72, 128, 250, 256}
    assert {L for _, L in R.DIVERSITY_SHAPES} == {0, 1, 2, 31, 32, 33, 64, 65, 100, 511, 512}
    assert {(256, 512), (72, 65), (7, 33), (1, 2)} <= set(R.DIVERSITY_SHAPES)
    seen_m = set()
    for g, L in R.DIVERSITY_SHAPES:
        c = R.diversity_case(g, L)
        n, K = c.rec.shape
        assert K >= L + 40 and c.ks[-1] == L and 30 <= n <= 45
        reg = [R.diversity_regions(c.rec[i].tolist(), L, c.tab.shape[0], c.present, g) for i in range(n)]
        assert {r["path"] for r in reg} == {"vec" if g % 8 == 0 else "scalar"}
        for m in (2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512):
            if m <= L:
                r = reg[c.notes[f"m{m}"]]
                assert r["m"] == m and r["nvalid"] == L and r["cap_decides"] and r["tiles"] == -(-m // 32)
                assert (c.rec[c.notes[f"m{m}"]] < 0).any()                 # holes inside the first L
                seen_m.add(m)
        assert reg[c.notes["one_vector"]]["m"] == min(1, L) and not reg[c.notes["one_vector"]]["computed"]
        z = reg[c.notes["two_zero_vectors"]]
        assert z["m"] == min(2, L) and z["computed"] == (L >= 2)
        assert reg[c.notes["dense"]]["cap_decides"] and reg[c.notes["dense"]]["m"] == L
        assert reg[c.notes["all_holes"]]["nvalid"] == 0 and reg[c.notes["one_listed"]]["nvalid"] == min(1, L)
        # ids beyond the table, absent vectors, zero vectors, duplicates and holes all occur among the listed ids
        flat = c.rec[:, :].ravel()
        assert (flat >= c.tab.shape[0]).any() and (flat < 0).any()
        inside = flat[(flat >= 0) & (flat < c.tab.shape[0])]
        assert (c.present[inside] == 0).any() and (~c.tab[inside].any(axis=1)).any()
        assert any(len(set(R.listed(r.tolist())[:max(L, 2)])) < len(R.listed(r.tolist())[:max(L, 2)]) for r in c.rec)
        assert any(len(t) == 0 for t in c.truth)
    assert seen_m == {2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512}
    vec = {g: R.diversity_regions([0, 1], 2, 300, None, g) for g in (8, 72, 128, 256)}
    assert [vec[g]["s0_trips"] for g in (8, 72, 128, 256)] == [1, 2, 2, 4]
    assert vec[72]["partial_s0_trip"] and vec[8]["partial_s0_trip"] and not vec[256]["partial_s0_trip"]
    assert R.diversity_regions([0, 1], 2, 300, None, 8, aligned=False)["path"] == "scalar"
    assert all(R.diversity_regions([0, 1], 2, 300, None, g)["odd_g"] for g in (1, 3, 7))
    c = R.diversity_stride_case()
    assert c.rec.shape == (66000, 4) and R.diversity_grid_stride(66000) and not R.diversity_grid_stride(65536)


# ---------------------------------------------------------------------------------------------------------------------
# the helpers see what they are for
# ---------------------------------------------------------------------------------------------------------------------
def test_helpers_go_red_and_name_the_place():
    c = R.segment_case()
    ref = R.case_reference(c)
    per = dict(vals=ref.vals.copy(), mrr=ref.mrr.copy(), scored=ref.scored.copy())
    R.check_per_user("ok", per, ref)
    per["vals"][17, 2, 1] = np.nextafter(per["vals"][17, 2, 1], 2.0)
    with pytest.raises(AssertionError, match=r"user 17, k-index 2 \(k = 10\), metric recall"):
        R.check_per_user("bad", per, ref)
    # one pair dropped from one user's diversity: the exact comparison sees every one of them
    d = R.diversity_case(128, 64)
    i = d.notes["m64"]
    ids = [x for x in R.listed(d.rec[i].tolist())[:64] if x < 300 and d.present[x]]
    X = d.tab[ids].astype(np.float64)
    nr = np.sqrt((X * X).sum(axis=1))
    iu, ju = np.triu_indices(len(ids), 1)
    ok = (nr[iu] > 0) & (nr[ju] > 0)
    t = 1.0 - (X @ X.T)[iu[ok], ju[ok]] / (nr[iu[ok]] * nr[ju[ok]])
    full = math.fsum(t.tolist()) / len(t)
    assert full == R.user_diversity(d.rec[i].tolist(), 64, d.tab, d.present)
    dropped = (math.fsum(t.tolist()) - t) / (len(t) - 1)
    assert (dropped != full).mean() > 0.99
    # the report check: a mean one part short is outside the derived bound
    s = R.stride_case(513)
    rs = R.case_reference(s)
    on = rs.scored.astype(bool)
    nsc = int(on.sum())
    good = {"n_users": 513, "k_values": [1, 2, 4, 8]}
    for j, k in enumerate(rs.ks):
        for m, name in enumerate(("ndcg", "recall", "precision")):
            good[f"{name}@{k}"] = float(np.sum(rs.vals[on, j, m])) / nsc
        good[f"mrr@{k}"] = good[f"ap@{k}"] = 0.0
    good["mrr"] = float(np.sum(rs.mrr[on])) / nsc
    R.check_report("ok", good, s, rs)
    bad = dict(good)
    bad["ndcg@8"] = (float(np.sum(rs.vals[on, 3, 0])) - rs.vals[on, 3, 0].max()) / nsc
    with pytest.raises(AssertionError):
        R.check_report("bad", bad, s, rs)


def test_regression_note_old_comparison_accepts_structural_errors():
    """tests/test_gpu_eval_device.py compares diversity at 1e-5 max(|d|, 1).  On its own data (seed 10, g = 128,
    L = 100) more than a third of the pairs can each be dropped inside that.  At L = 500 on 18-column 0/1 genre
    vectors (the big_case generator, seed 6; 500 ids drawn with seed 100) EVERY single pair can; a whole diagonal
    32 x 32 tile (465 pairs) can for one of the sixteen tiles (the other fifteen move the mean by 1.1e-5 .. 1.4e-4,
    just outside), and in every diagonal tile the first 7 pairs can be dropped together."""
    import test_gpu_eval_device as T
    n, K, n_items, L, g = 2000, 160, 5000, 100, 128
    rec, users, truth = T._random_case(n, K, n_items, seed=9)
    E = np.random.default_rng(10).standard_normal((n_items, g)).astype(np.float32)
    E[::97] = 0.0

    def terms(ids, tab):
        X = tab[ids].astype(np.float64)
        nr = np.linalg.norm(X, axis=1)
        iu, ju = np.triu_indices(len(ids), 1)
        ok = (nr[iu] > 0) & (nr[ju] > 0)
        iu, ju = iu[ok], ju[ok]
        return iu, ju, 1.0 - (X[iu] * X[ju]).sum(axis=1) / (nr[iu] * nr[ju])

    fractions = []
    for i in range(40):
        if not truth.get(users[i]):
            continue
        _, _, t = terms([x for x in rec[i] if x >= 0][:L], E)
        d = t.mean()
        moved = np.abs((t.sum() - t) / (len(t) - 1) - d)
        fractions.append(float((moved <= 1e-5 * max(abs(d), 1.0)).mean()))
    print("fraction of single pairs that can be dropped, per user:", np.round(fractions, 3))
    assert float(np.mean(fractions)) > 1 / 3 and min(fractions) > 0.3

    G = (np.random.default_rng(6).random((3000, 18)) < 0.2).astype(np.float32)
    ids = np.random.default_rng(100).integers(0, 3000, 500)
    iu, ju, t = terms(ids, G)
    d = t.mean()
    tol = 1e-5 * max(abs(d), 1.0)
    assert (np.abs((t.sum() - t) / (len(t) - 1) - d) <= tol).all()       # any single pair of the 119 316
    whole, prefix = [], []
    for tile in range(16):
        idx = np.nonzero((iu // 32 == tile) & (ju // 32 == tile))[0]
        whole.append(abs(np.delete(t, idx).mean() - d))
        q = np.arange(1, len(idx) + 1)
        inside = np.nonzero(np.abs((t.sum() - np.cumsum(t[idx])) / (len(t) - q) - d) <= tol)[0]
        prefix.append(int(inside.max()) + 1 if len(inside) else 0)
    print("whole diagonal tile dropped, |change of the mean|:", np.array(whole), "tolerance", tol)
    print("pairs of each diagonal tile that can be dropped together:", prefix)
    assert sum(w <= tol for w in whole) >= 1 and max(whole) < 20 * tol
    assert min(prefix) >= 7
    # the exact inputs: the same structural errors on a (128, 64) case change the value (see the helper test above)


# ---------------------------------------------------------------------------------------------------------------------
# GroundTruth.csr_from_pairs
# ---------------------------------------------------------------------------------------------------------------------
def test_csr_from_pairs():
    from recommendit_amd.eval_device import GroundTruth
    users = [30, 10, 20, 40]                                               # not sorted; 40 has no pairs
    pu = [10, 30, 10, 99, 10, 20, 30, 10, 5]                               # 99 and 5 are not in users
    pi = [7, 3, 7, 1, 2, 9, 3, 8, 4]                                       # (10, 7) and (30, 3) twice
    off, items, raw = GroundTruth.csr_from_pairs(users, pu, pi)
    assert off.dtype == items.dtype == raw.dtype == np.int64
    assert off.tolist() == [0, 1, 4, 5, 5] and items.tolist() == [3, 2, 7, 8, 9] and raw.tolist() == [2, 4, 1, 0]
    # empty inputs
    off, items, raw = GroundTruth.csr_from_pairs([], [1], [2])
    assert off.tolist() == [0] and items.size == 0 and raw.size == 0
    off, items, raw = GroundTruth.csr_from_pairs([4, 2], [], [])
    assert off.tolist() == [0, 0, 0] and items.size == 0 and raw.tolist() == [0, 0]
    # only foreign pairs
    off, items, raw = GroundTruth.csr_from_pairs([4, 2], [9, 1, 3], [1, 1, 1])
    assert off.tolist() == [0, 0, 0] and items.size == 0 and raw.tolist() == [0, 0]
    # against the definition on random pairs
    rng = np.random.RandomState(3)
    users = rng.permutation(50)[:30]
    pu, pi = rng.randint(0, 60, size=2000), rng.randint(0, 40, size=2000)
    off, items, raw = GroundTruth.csr_from_pairs(users, pu, pi)
    for r, u in enumerate(users):
        mine = [int(i) for uu, i in zip(pu, pi) if uu == u]
        assert items[off[r]:off[r + 1]].tolist() == sorted(set(mine)) and raw[r] == len(mine)
    # the cases of the GPU tests go through from_dict's rows: the same segments
    c = R.segment_case()
    n = len(c.truth)
    rows = np.repeat(np.arange(n), [len(t) for t in c.truth])
    off, items, raw = GroundTruth.csr_from_pairs(np.arange(n), rows, np.concatenate(c.truth))
    for i, t in enumerate(c.truth):
        assert items[off[i]:off[i + 1]].tolist() == sorted(set(t)) and raw[i] == len(t)
