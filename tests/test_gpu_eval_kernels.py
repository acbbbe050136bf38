"""GPU: the evaluation-report kernels (recommendit_amd/csrc/eval.hip) against exact per-user references.

Every case comes from tests/eval_reference.py, which also holds the reference (written from the definitions, nothing
from eval_device or metrics), the exact inputs for diversity, the derived bound of the report's means and the
comparison helpers; tests/test_eval_reference_host.py shows on the CPU which kernel regions each case reaches.

Every user's vals (ndcg, recall, precision per k), mrr, scored and diversity are compared with ==.  The report's means
are held to (ceil(n/512) + 768) 2^-53 mean|v| against math.fsum, and with == where every per-user value is dyadic;
coverage and the key order with ==.  Calls go through evaluate_topk_device(per_user=True); the C ABI is used only for
the table that is not 16-byte aligned, which the wrapper cannot produce.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import eval_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

RATIOS = {}   # worst |device - reference| / bound of the report's means, per metric (printed with -s)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _truth(case):
    from recommendit_amd.eval_device import GroundTruth
    n = case.rec.shape[0]
    return GroundTruth.from_dict({i: t for i, t in enumerate(case.truth) if t}, range(n))


def run(case, rec=None, gt=None):
    """(report without per_user, {name: numpy copy of the per-user tensor})"""
    from recommendit_amd.eval_device import evaluate_topk_device
    dev = _dev()
    rec = torch.from_numpy(case.rec).to(dev) if rec is None else rec
    tab = pres = None
    if case.tab is not None:
        tab = torch.from_numpy(case.tab).to(dev)
        pres = torch.from_numpy(case.present).to(dev) if case.present is not None else None
    got = evaluate_topk_device(rec, gt or _truth(case), list(case.ks), catalog_size=case.catalog_size,
                               item_vectors=tab, item_present=pres, n_id_space=case.n_id_space, per_user=True)
    per = {k: v.cpu().numpy() for k, v in got.pop("per_user").items()}
    return got, per


def check(case, ref=None):
    ref = ref or R.case_reference(case)
    got, per = run(case)
    R.check_per_user(case.name, per, ref)
    R.check_report(case.name, got, case, ref, RATIOS)
    return got, per


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------------------------
# eval_rank_kernel
# ---------------------------------------------------------------------------------------------------------------------
def test_segment_sizes_on_both_sides_of_the_shuffle_search():
    """cnt in {1, 2, 3, 63, 64, 65, 127, 128, 129, 1000}: lane-held segments and the global binary search"""
    case = R.segment_case()
    ref = R.case_reference(case)
    _, a = check(case, ref)
    _, b = check(R.with_coverage(case), R.case_reference(R.with_coverage(case)))
    same_bits(a, b)


@pytest.mark.parametrize("K", R.ROW_LENGTHS)
def test_row_lengths_chunks_and_early_exit(K):
    """every k list without coverage (eval_rank_kernel<false>: the early exit) and with it (<true>: no exit); the
    per-user tensors of the two runs are bitwise equal"""
    for kl in (("mixed",) if K <= 512 else ("exit1", "wait", "never", "zero")):
        case = R.row_length_case(K, kl)
        ref = R.case_reference(case)
        _, a = check(case, ref)
        cov = R.with_coverage(case)
        cref = R.case_reference(cov)
        assert np.array_equal(cref.vals, ref.vals)
        _, b = check(cov, cref)
        same_bits(a, b)


@pytest.mark.parametrize("n_k", R.K_LIST_SIZES)
def test_k_lists(n_k):
    """1, 29, 42, 43 and 64 distinct k (rpi = 85, 2, 2, 1, 1; every lane), unsorted, repeated, with 0, 1 and values
    above K and above a row's valid count"""
    check(R.k_list_case(n_k))


def test_k_list_of_64_up_to_2000():
    """kmax = 2000: the discount tables grow to 2048 entries; four chunks per row"""
    check(R.k_list_case(64, n=24, K=2000, kmax=2000))


def test_grid_stride_partition_and_run_to_run():
    """70 000 users: waves take a third row, parts of 137 rows; recall, precision, mrr and n_scored == as means"""
    case = R.stride_case()
    ref = R.case_reference(case)
    rec = torch.from_numpy(case.rec).to(_dev())
    gt = _truth(case)
    got, per = run(case, rec, gt)
    R.check_per_user(case.name, per, ref)
    R.check_report(case.name, got, case, ref, RATIOS)
    for j, k in enumerate(ref.ks):                       # check_report did compare these with ==: say so here
        assert R.all_dyadic(ref.vals[:, j, 1]) and R.all_dyadic(ref.vals[:, j, 2])
    got2, per2 = run(case, rec, gt)
    assert got2 == got
    same_bits(per, per2)


@pytest.mark.parametrize("n", R.PARTITION_SIZES)
def test_partition_sizes(n):
    """n below, at and above 512: empty and ragged parts of the fixed 512-way reduction"""
    check(R.stride_case(n))


@pytest.mark.parametrize("S", R.COVERAGE_SPACES)
def test_coverage_flags(S):
    """ids 0 and n_id_space - 1, ids listed only by users without truth, ids seen only in the second chunk"""
    case = R.coverage_case(S)
    got, _ = check(case)
    assert got["coverage"] == R.case_reference(case).coverage


def test_id_beyond_the_id_space_in_the_second_chunk_raises():
    from recommendit_amd.eval_device import evaluate_topk_device
    case = R.coverage_case(513)
    rec = case.rec.copy()
    rec[0, 800] = 513
    with pytest.raises(RuntimeError, match="n_id_space"):
        evaluate_topk_device(torch.from_numpy(rec).to(_dev()), _truth(case), case.ks, catalog_size=case.catalog_size,
                             n_id_space=513)


# ---------------------------------------------------------------------------------------------------------------------
# eval_diversity_kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,L", R.DIVERSITY_SHAPES)
def test_diversity_exact(g, L):
    case = R.diversity_case(g, L)
    ref = R.case_reference(case)
    _, per = check(case, ref)
    if (g, L) == (256, 512):
        _, again = run(case)
        same_bits(per, again)


def _diversity_abi(case, scored, tab_view):
    """rihip_eval_diversity on a table view; returns the per-user values"""
    from recommendit_amd import _lib as L
    dev = _dev()
    n, K = case.rec.shape
    rec = torch.from_numpy(case.rec).to(dev)
    sc = torch.from_numpy(scored).to(dev)
    pres = torch.from_numpy(case.present).to(dev)
    div = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    L.check(L.lib().rihip_eval_diversity(rec.data_ptr(), n, K, sc.data_ptr(), int(case.ks[-1]), tab_view.data_ptr(),
                                         case.tab.shape[0], case.tab.shape[1], pres.data_ptr(), div.data_ptr(),
                                         L.stream_ptr()), "eval_diversity")
    torch.cuda.synchronize()
    return div.cpu().numpy()


def test_diversity_unaligned_table_takes_the_scalar_kernel():
    """g = 8 from a buffer offset by one float: eval_diversity_kernel<false> with g % 8 == 0, bitwise the aligned call"""
    case = R.diversity_case(8, 31)
    ref = R.case_reference(case)
    flat = torch.from_numpy(case.tab.reshape(-1)).to(_dev())
    buf = torch.zeros(flat.numel() + 8, dtype=torch.float32, device=_dev())
    aligned, shifted = buf[4:4 + flat.numel()], buf[1:1 + flat.numel()]
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    aligned.copy_(flat)
    a = _diversity_abi(case, ref.scored, aligned)
    buf.zero_()
    shifted.copy_(flat)
    b = _diversity_abi(case, ref.scored, shifted)
    R.check_equal("aligned table", a, ref.diversity)
    R.check_equal("table offset by one float", b, ref.diversity)
    assert a.tobytes() == b.tobytes()


def test_diversity_grid_stride():
    """66 000 users, K = L = g = 4: blocks take a second row; every user compared"""
    check(R.diversity_stride_case())


def test_zz_report_ratios():
    """prints the worst |device - reference| / bound of the means seen by this file's tests (run with -s)"""
    for key in sorted(RATIOS):
        print(f"worst ratio {key}: {RATIOS[key]:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())
