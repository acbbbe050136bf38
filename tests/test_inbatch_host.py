"""CPU-only checks of the in-batch pass tests' own infrastructure (tests/inbatch_reference.py):

* the mirror of the launch arithmetic against the library's host functions, and its tile schedule against brute force
  (every tile once; a steady tile is full, off the workgroup's diagonal, two full tiles before the split's end, in
  trips of six from ring position 0);
* which loop regions the cases of tests/test_gpu_inbatch_exact.py reach -- without this nobody can tell whether a
  shape runs the steady loop at all;
* that every comparison helper goes red for one pair dropped, doubled, swapped between owners, an unmasked diagonal, a
  zeroed 32x32 tile and a non-zero ragged slot;
* the regression note: the random-unit-row comparison of the older tests accepts the first three of those;
* that the realistic cases' derived bounds lie >= 100 x below one pair's contribution (r, dU, dI at one set of shapes,
  every loss part at a smaller one).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import inbatch_reference as R  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------
# mirror of nw / nsplit / loss parts / workspace / gmat sizes
# ---------------------------------------------------------------------------------------------------------------------
def test_mirror_matches_library_host_functions():
    from recommendit_amd import _lib as L
    lib = L.lib()
    sizes = [1, 31, 32, 33, 127, 128, 129, 257, 300, 700, 2500, 4095, 4096, 4196, 8192, 16383, 16384, 16400, 65536]
    for no in sizes:
        assert lib.rihip_inbatch_workspace_doubles(no) >= R.cdiv(no, R.OW) * 16
        for ns in sizes:
            assert lib.rihip_inbatch_loss_parts(no, ns) == R.loss_parts(no, ns), (no, ns)
            assert lib.rihip_inbatch_gmat_floats(no, ns) == R.gmat_floats(no, ns), (no, ns)
            for d in (16, 32, 128, 256):
                assert lib.rihip_inbatch_workspace_floats(no, ns, d) == R.workspace_floats(no, ns, d), (no, ns, d)
            # the sizes the library hands out cover every split count either workgroup shape can use
            for nw in (4, 8):
                assert R.sweep_nsplit(no, ns, nw) <= min(16, R.sweep_nsplit(no, ns, 4))
                assert R.cdiv(no, R.OW) * R.sweep_nsplit(no, ns, nw) <= lib.rihip_inbatch_workspace_doubles(no)


def test_steady_tables():
    assert [R.sweep_steady(d, mu, go, nw) for d in (64, 128) for mu in (0, 1) for go in (0, 1) for nw in (4, 8)] == \
        [False] * 8 + [False] * 7 + [True]
    assert [R.gt_steady(d, nw) for d in (32, 64, 128) for nw in (4, 8)] == [False] * 5 + [True]


def _diag_tiles(n_owner, o_goff, s_goff, nw, bx):
    """tiles that hold a diagonal element of an in-range owner of workgroup bx, by brute force"""
    owners = np.arange(bx * nw * 32, min((bx + 1) * nw * 32, n_owner))
    drow = o_goff + owners - s_goff
    return set((drow[drow >= 0] // 32).tolist())


def test_sweep_schedule_invariants_brute_force():
    rng = np.random.RandomState(5)
    seen = {k: 0 for k in R.REGIONS}
    for _ in range(400):
        nw = 8
        n_owner = int(rng.choice([256, 300, 512, 700, 1024]))
        n_swept = int(rng.randint(1, 5000))
        nsplit = int(rng.choice([1, 2, 3, 5]))
        o_goff, s_goff = int(rng.randint(0, 4000)), int(rng.choice([0, 0, 100, 1777]))
        nfull = n_swept // 32
        for bx in range(R.cdiv(n_owner, nw * 32)):
            diag = _diag_tiles(n_owner, o_goff, s_goff, nw, bx)
            for by in range(nsplit):
                t0, t1 = R.split_range(n_swept, nsplit, by)
                s = R.sweep_schedule(n_owner, o_goff, n_swept, s_goff, nw, nsplit, bx, by, True)
                tiles = sorted(t for k in R.REGIONS for t in s[k])
                assert tiles == list(range(t0, max(t0, t1))), "every tile of the split exactly once"
                for k in R.REGIONS:
                    seen[k] += len(s[k])
                for name in ("steady_pre", "steady_post"):
                    st = s[name]
                    assert len(st) % 6 == 0
                    for t in st:
                        assert t not in diag and t + 2 < min(t1, nfull) and (bx + 1) * nw * 32 <= n_owner
                    # trips start at ring position 0: runs of consecutive tiles, each a multiple of 6 long
                    runs = np.split(np.array(st), np.where(np.diff(st) != 1)[0] + 1) if st else []
                    for run in runs:
                        assert (run[0] - t0) % 3 == 0 and len(run) % 6 == 0
                assert all(t >= t0 + 3 for k in R.REGIONS[1:] for t in s[k])
                # without a steady loop: everything in the one-tile loop
                s0 = R.sweep_schedule(n_owner, o_goff, n_swept, s_goff, nw, nsplit, bx, by, False)
                assert s0["lead"] == list(range(t0, max(t0, t1))) and not any(s0[k] for k in R.REGIONS[1:])
    assert all(seen[k] > 0 for k in R.REGIONS), seen


def test_gt_schedule_invariants_brute_force():
    rng = np.random.RandomState(6)
    for _ in range(400):
        n_swept, nsplit = int(rng.randint(1, 6000)), int(rng.choice([1, 2, 3, 7, 16]))
        nfull = n_swept // 32
        for by in range(nsplit):
            t0, t1 = R.split_range(n_swept, nsplit, by)
            s = R.gt_schedule(1000, n_swept, nsplit, by, True)
            assert s["lead"] + s["steady_pre"] + s["tail"] == list(range(t0, max(t0, t1)))
            assert len(s["steady_pre"]) % 3 == 0 and all(t + 2 < min(t1, nfull) for t in s["steady_pre"])
            assert not s["steady_pre"] or (s["steady_pre"][0] - t0) == 3


# ---------------------------------------------------------------------------------------------------------------------
# which regions the GPU cases reach
# ---------------------------------------------------------------------------------------------------------------------
def test_large_user_cases_reach_every_region_of_the_steady_sweep():
    No, Ns = R.LARGE_OWNERS, R.LARGE_SWEPT
    nw = R.sweep_nw(No, Ns)
    assert nw == 8 and R.sweep_steady(128, True, True, nw) and not R.sweep_steady(64, True, True, nw)
    assert R.sweep_nw(No - 101, Ns) == 4 and R.sweep_nw(No, 16383) == 4, "the smallest 8-wave shape, plus the ragged part"
    nsplit = R.sweep_nsplit(No, Ns, nw)
    gx = R.cdiv(No, nw * 32)
    assert nsplit == 16 and No % (nw * 32) != 0 and Ns % 32 != 0      # several splits, ragged last workgroup and tile
    found = {off: set() for off in R.LARGE_USER_OFFSETS}
    for off in R.LARGE_USER_OFFSETS:
        assert 0 <= off <= Ns - No
        for bx in range(gx):
            ddw = off + bx * nw * 32
            blo, bhi = ddw >> 5, (ddw + nw * 32 + 31) >> 5
            for by in range(nsplit):
                t0, t1 = R.split_range(Ns, nsplit, by)
                s = R.sweep_schedule(No, off, Ns, 0, nw, nsplit, bx, by, True)
                if s["steady_pre"] and s["steady_post"] and t0 <= blo and bhi <= t1 and len(s["band"]) == bhi - blo:
                    found[off].add("steady trip on each side of a whole band")
                if not s["steady_pre"] and not s["steady_post"]:
                    found[off].add("split with no steady tile")
                if blo < t0 < bhi or blo < t1 < bhi:
                    found[off].add("band cut by a split boundary")
                if s["fill"]:
                    found[off].add("ring-alignment tiles between steady ranges")
                if bx == gx - 1 and (bx + 1) * nw * 32 > No:
                    found[off].add("ragged last workgroup")
                    assert not s["steady_pre"] and not s["steady_post"]
                if by == nsplit - 1 and t1 * 32 > Ns:
                    found[off].add("ragged last tile")
                    assert (t1 - 1) in s["tail"] + s["band"] + s["lead"]
    want = {"steady trip on each side of a whole band", "split with no steady tile", "band cut by a split boundary",
            "ragged last workgroup", "ragged last tile", "ring-alignment tiles between steady ranges"}
    assert set().union(*found.values()) == want, found
    # the first offset is mid-tile; the last is G - Bl: the band of the ragged last workgroup ends in the ragged tile
    assert R.LARGE_USER_OFFSETS[0] % 32 != 0 and R.LARGE_USER_OFFSETS[-1] == Ns - No


def test_large_item_case_reaches_the_steady_item_loop():
    No, Ns = R.LARGE_OWNERS, R.LARGE_SWEPT      # owners = items, swept = users
    nw = R.sweep_nw(No, Ns)
    nsplit = R.sweep_nsplit(No, Ns, nw)
    assert nw == 8 and R.gt_steady(128, nw) and not R.gt_steady(64, nw) and nsplit == 16
    last = R.gt_schedule(No, Ns, nsplit, nsplit - 1, True)
    full = R.gt_schedule(No, Ns, nsplit, 3, True)
    assert len(full["lead"]) == 3 and len(full["steady_pre"]) == 27 and len(full["tail"]) == 3
    assert len(last["steady_pre"]) == 12 and last["tail"][-1] * 32 + 32 > Ns       # ragged last tile in the tail


def test_small_cases_reach_the_one_tile_paths():
    """4-wave kernels: one workgroup and several, owners and swept rows ragged and full, splits of one tile and a
    split long enough (> 3 tiles) to wrap the three-buffer ring; slices with partners below, inside and above"""
    per_split, wgs = set(), set()
    partners = set()
    for nu, ni, uo, io in R.EXACT_SMALL_SHAPES:
        assert R.sweep_nw(nu, ni) == 4 and R.sweep_nw(ni, nu) == 4
        ns = R.sweep_nsplit(nu, ni, 4)
        t0, t1 = R.split_range(ni, ns, 0)
        per_split.add(t1 - t0)
        wgs.add(R.cdiv(nu, 128))
        drow = uo + np.arange(nu) - io
        partners |= {"below"} if (drow < 0).any() else set()
        partners |= {"inside"} if ((drow >= 0) & (drow < ni)).any() else set()
        partners |= {"above"} if (drow >= ni).any() else set()
    assert 1 in per_split and 2 in per_split and max(per_split) >= 4, per_split
    assert {1, 2, 3} <= wgs
    assert partners == {"below", "inside", "above"}
    counts = {n for s in R.EXACT_SMALL_SHAPES for n in s[:2]}
    assert {1, 31, 32, 33, 127, 128, 129} <= counts
    # the forced 8-wave child: at d = 128 the steady instantiation runs with too few tiles for a trip (lead-in and
    # one-tile code only) -- its large-shape regions are the large cases' business
    for nu, ni, uo, io in R.CHILD_SHAPES:
        ns = R.sweep_nsplit(nu, ni, R.sweep_nw(nu, ni, 8))
        for by in range(ns):
            s = R.sweep_schedule(nu, uo, ni, io, 8, ns, 0, by, True)
            assert not s["steady_pre"] and not s["steady_post"]


# ---------------------------------------------------------------------------------------------------------------------
# exact expectations: the gather against brute force, f32 products against integers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(33, 127, 94, 0), (129, 200, 300, 250), (97, 131, 0, 64)])
@pytest.mark.parametrize("d", [16, 128])
def test_exact_expectations_against_brute_force(shape, d):
    nu, ni, uo, io = shape
    cs = R.make_exact_case(7, nu, ni, d, uo, io)
    R.assert_distinguishable(cs.w2)
    s = cs.items.astype(np.float64) @ cs.users.astype(np.float64).T
    assert np.all(s % 256 == 0) and np.abs(s).max() <= 512
    w = np.where(s == 0, 0.5, (s > 0) * 1.0)
    w[(io + np.arange(ni))[:, None] == (uo + np.arange(nu))[None, :]] = 0
    assert np.array_equal(cs.weights(), w.astype(np.float32))
    r, du = R.expected_user_outputs(cs)
    r64 = 0.5 * w.sum(axis=0)
    du64 = 0.5 * (w.T @ cs.items.astype(np.float64))
    for i in range(nu):
        j = uo + i - io
        if 0 <= j < ni:
            du64[i] -= r64[i] * cs.items[j]
    assert np.array_equal(r.astype(np.float64), r64) and np.array_equal(du.astype(np.float64), du64)
    di = R.expected_item_outputs(cs.weights(), cs.users, r, uo, io)
    di64 = 0.5 * (w @ cs.users.astype(np.float64))
    for j in range(ni):
        i = io + j - uo
        if 0 <= i < nu:
            di64[j] -= r64[i] * cs.users[i]
    assert np.array_equal(di.astype(np.float64), di64)
    # every value is a multiple of 1/8 below 2^24 / 8: exact in f32 whatever the order of the sums
    for a in (r64, du64, di64):
        assert np.all(a * 8 == np.round(a * 8)) and np.abs(a).max() * 8 < 2 ** 24


def test_exact_large_case_partial_sums_fit_f32():
    """the worst partial sum of the large cases: |w| <= 1 times |y| = 16 over 16 400 rows, in units of 1/2 * 16 = 8"""
    assert R.LARGE_SWEPT * 16 * 2 < 2 ** 24 and R.LARGE_SWEPT * 3 * 8 * 8 < 2 ** 24     # ternary; synthetic 0..3 x +-8


def test_gmat_layout_roundtrip_and_formula():
    nu, ni = 300, 70
    full = np.arange(R.g_ub(ni) * 32 * R.g_ub(nu) * 32, dtype=np.float32).reshape(R.g_ub(ni) * 32, R.g_ub(nu) * 32)
    flat = R.encode_gmat(full, nu, ni)
    assert flat.size == R.gmat_floats(nu, ni) and np.array_equal(R.decode_gmat(flat, nu, ni), full)
    for j, i in [(0, 0), (5, 299), (69, 31), (33, 32), (64, 255)]:
        assert flat[((j // 32) * R.g_ub(nu) + i // 32) * 1024 + (j % 32) * 32 + i % 32] == full[j, i]


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity of the comparison helpers
# ---------------------------------------------------------------------------------------------------------------------
def _outputs(cs, w2):
    """what a device that computed the weights w2 [item, user] would write"""
    wrong = R.ExactCase(cs.d, cs.users, cs.items, cs.user_goff, cs.item_goff, w2)
    full = np.full((R.g_ub(cs.n_items) * 32, R.g_ub(cs.n_users) * 32), np.nan, dtype=np.float32)
    full[:R.cdiv(cs.n_items, 32) * 32, :R.cdiv(cs.n_users, 128) * 128] = 0
    full[:cs.n_items, :cs.n_users] = wrong.weights()
    r, du = R.expected_user_outputs(wrong)
    di = R.expected_item_outputs(wrong.weights(), cs.users, r, cs.user_goff, cs.item_goff)
    return R.encode_gmat(full, cs.n_users, cs.n_items), r, du, di


def _compare_all(cs, out):
    """the four comparisons of the GPU tests; returns the names of those that raised"""
    gm, r, du, di = out
    er, edu = R.expected_user_outputs(cs)
    edi = R.expected_item_outputs(cs.weights(), cs.users, er, cs.user_goff, cs.item_goff)
    red = []
    for name, fn in (("gmat", lambda: R.check_gmat(gm, cs.weights(), cs.n_users, cs.n_items)),
                     ("r", lambda: R.check_equal("r", r, er)), ("dU", lambda: R.check_equal("dU", du, edu)),
                     ("dI", lambda: R.check_equal("dI", di, edi))):
        try:
            fn()
        except AssertionError:
            red.append(name)
    return red


@pytest.fixture(scope="module")
def sens_case():
    return R.make_exact_case(11, 129, 300, 32, 77, 0)


def _pick(w2, value, skip=0):
    j, i = np.argwhere(w2 == value)[skip]
    return int(j), int(i)


def test_helpers_accept_the_expectation(sens_case):
    assert _compare_all(sens_case, _outputs(sens_case, sens_case.w2)) == []


def test_helpers_see_one_pair_dropped(sens_case):
    for value in (1, 2):
        w2 = sens_case.w2.copy()
        w2[_pick(w2, value, 5)] = 0
        assert _compare_all(sens_case, _outputs(sens_case, w2)) == ["gmat", "r", "dU", "dI"]


def test_helpers_see_one_pair_doubled(sens_case):
    for value in (1, 2):
        w2 = sens_case.w2.copy()
        w2[_pick(w2, value, 9)] *= 2
        assert _compare_all(sens_case, _outputs(sens_case, w2)) == ["gmat", "r", "dU", "dI"]


def test_helpers_see_two_pairs_swapped_between_owners(sens_case):
    w2 = sens_case.w2.copy()
    j = 40
    i1, i2 = int(np.flatnonzero(w2[j] == 2)[0]), int(np.flatnonzero(w2[j] == 0)[3])
    assert i1 != i2 and sens_case.user_goff + i2 != j       # not the diagonal zero
    w2[j, i1], w2[j, i2] = w2[j, i2], w2[j, i1]
    assert _compare_all(sens_case, _outputs(sens_case, w2)) == ["gmat", "r", "dU", "dI"]


def test_helpers_see_the_diagonal_unmasked(sens_case):
    w2 = sens_case.w2.copy()
    w2[sens_case.user_goff + 3, 3] = 1          # g_ii = 0.5 counted
    # in dU and dI the term cancels against the correction (c g_ii y_i - r_i y_i with g_ii inside r_i): only the
    # stored weights and r can show it, which is why both are compared
    assert _compare_all(sens_case, _outputs(sens_case, w2)) == ["gmat", "r"]


def test_helpers_see_one_tile_zeroed_for_one_wave(sens_case):
    w2 = sens_case.w2.copy()
    w2[64:96, 32:64] = 0
    assert _compare_all(sens_case, _outputs(sens_case, w2)) == ["gmat", "r", "dU", "dI"]


def test_helpers_see_a_nonzero_ragged_slot(sens_case):
    cs = sens_case
    for j, i in [(cs.n_items, 5), (7, cs.n_users), (cs.n_items + 3, cs.n_users + 2)]:     # ragged row, column, corner
        gm, r, du, di = _outputs(cs, cs.w2)
        assert j < R.cdiv(cs.n_items, 32) * 32 and i < R.cdiv(cs.n_users, 32) * 32
        gm[((j // 32) * R.g_ub(cs.n_users) + i // 32) * 1024 + (j % 32) * 32 + i % 32] = 0.5
        assert _compare_all(cs, (gm, r, du, di)) == ["gmat"]
    # a number (not 0, not the prefill) in a block nobody should write
    gm, r, du, di = _outputs(cs, cs.w2)
    gm[-1] = 1.0
    assert _compare_all(cs, (gm, r, du, di)) == ["gmat"]
    # and a NaN prefill left in a block the item pass multiplies
    gm, r, du, di = _outputs(cs, cs.w2)
    gm[3] = np.nan
    assert _compare_all(cs, (gm, r, du, di)) == ["gmat"]


def test_regression_note_old_comparison_accepts_structural_errors():
    """The comparison of the older in-batch tests -- random unit rows, assert_allclose(atol=3e-9, rtol=3e-4) against
    the fp64 closed form -- at 64 owners x 16 650 swept rows, d = 128 (the swept size of
    test_inbatch_stored_g_steady_loops_ragged): a pair dropped, doubled, or two pairs swapped between owners leave it
    green, because one pair carries 1 / 16 650 = 6e-5 of an element, five times under rtol.  (A CPU restatement: the
    stand-in for the device is the unperturbed closed form in f32; the older tests stay as they are.)"""
    rng = np.random.RandomState(16420)
    Bl, G, d, off = 64, 16650, 128, 77
    U, Y = R.rows_of_norm(rng, Bl, d, 1.0).astype(np.float64), R.rows_of_norm(rng, G, d, 1.0).astype(np.float64)
    pos = np.einsum("ij,ij->i", U, Y[off:off + Bl])
    c = 1.0 / (G * (G - 1.0))

    def closed_form(g):
        du = c * (g @ Y)
        du -= (c * g.sum(axis=1))[:, None] * Y[off:off + Bl]
        return du

    g = 1.0 / (1.0 + np.exp(-(U @ Y.T - pos[:, None])))
    g[np.arange(Bl), off + np.arange(Bl)] = 0
    device = closed_form(g).astype(np.float32)
    dropped, doubled, swapped = g.copy(), g.copy(), g.copy()
    dropped[5, 1000] = 0
    doubled[5, 1000] *= 2
    swapped[5, 1000], swapped[6, 1000] = g[6, 1000], g[5, 1000]
    for wrong in (dropped, doubled, swapped):
        np.testing.assert_allclose(device, closed_form(wrong), atol=3e-9, rtol=3e-4)      # the old check: green
    # the realistic bound of this file's GPU tests is not the tool for 16 650 rows either (n u is 1e-3); the exact
    # inputs are: the same three errors on an exact case turn every comparison red (tests above).


# ---------------------------------------------------------------------------------------------------------------------
# realistic cases: the derived bounds against one pair
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(R.REALISTIC_CASES))
def test_realistic_bounds_lie_100x_below_one_pair(key):
    """r, dU, dI at the shapes of REALISTIC_CASES; the loss parts at the smaller shapes of LOSS_CASES, where a part holds
    14 to 640 pairs (every pair's score error enters a part's bound unamplified, so the bound grows with the pairs)."""
    d, precision, norm = key
    users, items, pos, off = R.make_realistic_case(d, precision, norm)
    ref = R.realistic_reference(users, items, pos, off, 0, items.shape[0])
    ratios = R.one_pair_ratios(ref, R.bound_sums(ref, pos, d, precision), users, items)
    print(key, {k: round(v, 1) for k, v in ratios.items()})
    assert min(ratios["r"], ratios["dU"], ratios["dI"]) >= 100, ratios
    if precision == 0 and norm == 1:    # unit rows on the f32 MFMA: the derived bound is no looser than (n + d + 44) u M
        plain, mine = R.issue_form_bounds(ref, d), R.bound_sums(ref, pos, d, precision)
        assert all(np.all(mine[k] <= plain[k] * (1 + 1e-12)) for k in ("r", "dU", "dI"))
    # the weight bound does not depend on G and is far below the weight itself
    bg = R.bound_gmat(ref, pos, d, precision)
    assert (bg[ref["g"] > 0] / ref["g"][ref["g"] > 0]).max() < 1e-3
    assert np.abs(ref["z"]).max() <= 2 * norm * norm


@pytest.mark.parametrize("key", sorted(R.LOSS_CASES))
def test_realistic_loss_part_bounds_lie_100x_below_one_pair(key):
    d, precision, norm = key
    users, items, pos, off = R.make_realistic_case(d, precision, norm, R.LOSS_CASES)
    ref = R.realistic_reference(users, items, pos, off, 0, items.shape[0])
    ratios = R.one_pair_ratios(ref, R.bound_sums(ref, pos, d, precision), users, items)
    print(key, users.shape[0], "x", items.shape[0], "parts", len(ref["loss_part"]), {k: round(v, 1) for k, v in ratios.items()})
    assert min(ratios.values()) >= 100, ratios
