"""CPU: tests/search_reference.py against the sources of the search driver (its constants, read as text), the path every
shape of tests/test_gpu_search_paths.py claims, and the reference's own top-k order and verdict rule on hand-made
scores."""
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_reference as R  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "recommendit_amd" / "csrc"


def _const(src, name):
    m = re.search(rf"constexpr (?:int|int64_t) {name} = ([^;]+);", src)
    assert m, name
    return m.group(1).strip()


def test_constants_are_the_drivers():
    kern, idx, topk = ((CSRC / f).read_text() for f in ("search_kernels.h", "ip_index.h", "topk.hip"))
    for name in ("QB", "SAMPLE", "CSTRIDE", "QBB", "TRB", "SAMPLE_T"):
        assert int(_const(kern, name)) == getattr(R, name), name
    for name in ("TR", "TRS", "K_MAX", "NLIST_MAX"):
        assert int(_const(idx, name)) == getattr(R, name), name
    bf16 = (CSRC / "scan_bf16.hip").read_text()
    assert int(_const(bf16, "WQE")) == R.WQE and ">= (unsigned)(WQE - 64)) wave_flush();" in bf16
    assert int(re.search(r"#define RIHIP_NCU (\d+)", (CSRC / "common.h").read_text()).group(1)) == R.RIHIP_NCU
    assert _const(topk, "IVF_TARGET") == "16 * RIHIP_NCU" and R.IVF_TARGET == 16 * R.RIHIP_NCU
    assert int(_const(topk, "IVF_SS")) == R.IVF_SS
    assert int(_const(topk, "CH")) == R.PASS_QUERIES
    # the re-do chunks: `const int FCH = ..;` in flat_redo and in ivf_redo
    fch = {fn: int(re.search(rf"int {fn}\(.*?const int FCH = (\d+);", topk, flags=re.S).group(1))
           for fn in ("flat_redo", "ivf_redo")}
    assert fch == {"flat_redo": R.FLAT_REDO_CHUNK, "ivf_redo": R.IVF_REDO_CHUNK}
    assert f"r.lds_slots = {R.REFINE_LDS_SLOTS};" in topk
    assert f"if (two_prec && k <= {R.FUSED_K_MAX})" in topk
    assert f"if (n <= {R.IVF_SMALL_PREPARE}) {{" in topk
    assert f"g.cap_full <= {R.IVF_DENSE_ROWS} ||" in topk and "nq * g.cap_df <= (int64_t)(1 << 23)" in topk
    assert "if (h->N <= 4 * (int64_t)SAMPLE) return flat_dense(s);" in topk
    assert "(two_prec ? 1.5 : 1.0)" in topk and "2.5 * expect" in topk and "2.5 * rank * SS" in topk
    assert "(int64_t)rank * 4 <= streams * SAMPLE_T" in topk
    sel = (CSRC / "select.hip").read_text()
    assert "n <= 2u * RIHIP_NCU && f.cap > 0 && (size_t)(P + f.cap) <= (size_t)K_MAX" in sel
    # the slots of the stats export are the enum's
    enum = re.search(r"enum SearchStat \{(.*?)\};", idx, flags=re.S).group(1)
    names = [n.split("=")[0].strip()[3:].lower() for n in enum.split(",") if n.strip() and "ST_COUNT" not in n]
    assert names == list(R.STATS)
    from recommendit_amd.faiss_index import FAISSIndex
    assert FAISSIndex.SEARCH_STATS == R.STATS


# ---- plan: every exit of every rule, at the shapes of tests/test_gpu_search_paths.py ------------------------------------
def test_plan_flat_route_and_splits():
    assert R.plan(65536, 64, 130, 10)["route"] == "flat_dense" and R.plan(65537, 64, 130, 10)["route"] == "flat_fused"
    assert R.plan(65537, 64, 130, 10, two_precision=False)["route"] == "flat_f32"
    assert R.plan(65537, 64, 130, 10, filtered=True)["route"] == "flat_f32"       # the bf16 filter reads no tags
    assert R.plan(66000, 64, 9, 2048)["route"] == "flat_fused" and R.plan(66000, 64, 9, 2049)["route"] == "flat_unfused"
    # pick_nsplit: one query block -> 512 splits, two -> 256; never more splits than tiles, never fewer than one
    assert R.pick_nsplit(128, 10 ** 6) == 512 and R.pick_nsplit(129, 10 ** 6) == 256 and R.pick_nsplit(4096, 10 ** 6) == 16
    assert R.pick_nsplit(130, 16) == 16 and R.pick_nsplit(4096, 0) == 1 and R.pick_nsplit(1, 10 ** 9) == 512
    assert R.bf16_nsplit(9, 1032, 3) == 768 and R.bf16_nsplit(257, 1032, 3) == 384 and R.bf16_nsplit(4096, 516, 2) == 32
    for N, per in ((500, 1), (8212, 2), (16416, 3), (39990, 5), (65536, 8)):
        assert R.plan(N, 64, 130, 70)["scan"]["per"] == per
    s = R.plan(8212, 64, 130, 70)["scan"]
    assert (s["tiles"], s["used"], s["nsplit"], s["last_split_tiles"], s["last_tile_rows"]) == (257, 129, 256, 1, 20)
    # one query block: 512 splits
    s = R.plan(16416, 64, 128, 70)["scan"]
    assert (s["tiles"], s["per"], s["used"], s["nsplit"], s["last_split_tiles"]) == (513, 2, 257, 512, 1)
    s = R.plan(39990, 64, 128, 70)["scan"]
    assert (s["tiles"], s["per"], s["last_tile_rows"]) == (1250, 3, 22)
    assert R.plan(65536, 64, 128, 70)["scan"]["per"] == 4


def test_plan_finalize_in_lds_or_global():
    assert R.plan(16320, 64, 130, 64)["fin_lds"] and not R.plan(16321, 64, 130, 64)["fin_lds"]
    assert R.plan(16320, 64, 130, 65)["fin_lds"] is False            # the sort buffer doubles at k = 65
    assert R.plan(500, 64, 512, 64)["fin_lds"] and not R.plan(500, 64, 513, 64)["fin_lds"]
    assert R.finalize_in_lds(1, 16384, 500, 1) and not R.finalize_in_lds(1, 16385, 500, 1)      # mode 1: no sort buffer
    assert not R.finalize_in_lds(1, 0, 10, 0)


def test_plan_flat_thresholded_shapes():
    p = R.plan(66000, 64, 9, 500)
    assert (p["stride"], p["S"], p["rank"], p["cap"], p["seg_cap"], p["sample_top"], p["cap_s"]) == \
        (2, 33000, 476, 4096, 64, True, 8192)
    assert p["filter"]["per"] == 2 and p["sample"]["per"] == 2 and p["fin_thr_lds"]
    p = R.plan(66000, 64, 9, 2049)
    assert (p["route"], p["sample_top"], p["cap"], p["fin_lds"], p["fin_kth_lds"]) == ("flat_unfused", True, 16384, False, True)
    p = R.plan(66000, 64, 9, 4000)
    assert (p["route"], p["sample_top"], p["cap_s"]) == ("flat_unfused", False, 33000)
    p = R.plan(66000, 64, 257, 2000)
    assert (p["route"], p["sample_top"], p["cap"]) == ("flat_fused", False, 16384)
    assert R.plan(66000, 64, 256, 2000)["sample_top"]                # one query block keeps the streams
    p = R.plan(66000, 64, 4096, 500)
    assert (p["sample_top"], p["seg_cap"], p["filter"]["per"], p["filter"]["used"]) == (False, 128, 22, 47)
    assert R.plan(66000, 64, 4, 500)["seg_cap"] == 64
    for N, S in ((65537, 16385), (66000, 16500)):
        for k, rank in ((10, 13), (500, 174)):
            p = R.plan(N, 64, 20, k, two_precision=False)
            assert (p["route"], p["stride"], p["S"], p["rank"], p["cap"]) == ("flat_f32", 4, S, rank, 4096)
            assert p["fin_lds"] and not p["fin_thr_lds"]
    # (`cap > N` cannot happen on this route: k <= K_MAX keeps cap at 65 536 or less, and the route starts above that)
    assert R.plan(66000, 64, 20, 16384, two_precision=False)["cap"] == 65536 == R.plan(66000, 64, 20, 16384)["cap"]
    assert R.plan(2 ** 20, 128, 4096, 500)["stride"] == 32 and R.plan(2 ** 20, 128, 4096, 500, False)["stride"] == 64


LENS = [0, 1, 2, 3, 63, 64, 65, 2049, 9001, 8800, 8600, 8400, 5000, 3000, 1500, 700]


def test_plan_ivf_rules():
    g = R.ivf_geometry(LENS, 4)
    assert (g["cap_full"], g["max_tiles"], g["cap_lf"], g["cap_df"]) == (34801, 282, 9024, 36096)
    assert R.ivf_geometry(LENS, 40)["nprobe"] == 16 and R.ivf_geometry([0, 0], 1)["cap_full"] == 1
    assert R.ivf_geometry([0, 0], 1)["cap_lf"] == 32
    kw = dict(list_lens=LENS, nprobe=4)
    for nq in (1, 4, 5, 8):
        assert R.plan(47248, 64, nq, 20, **kw)["prepare"] == "small"
    assert R.plan(47248, 64, 9, 20, **kw)["prepare"] == "four"
    # the three exits to the unfiltered pass: few dense slots, a short sample, a small population
    assert R.plan(47248, 64, 232, 20, **kw)["route"] == "ivf_unfiltered"
    assert R.plan(47248, 64, 233, 20, **kw)["route"] == "ivf_thresholded"
    assert R.plan(47248, 64, 1024, 543, **kw)["route"] == "ivf_thresholded"
    assert R.plan(47248, 64, 1024, 544, **kw)["route"] == "ivf_unfiltered"        # 4 k > cap_full / 16
    assert R.plan(47248, 64, 1024, 20, list_lens=LENS, nprobe=1)["route"] == "ivf_unfiltered"   # 9 001 rows
    p = R.plan(47248, 64, 1024, 500, **kw)
    assert (p["rank"], p["cap"], p["cap_l"], p["cap_s"], p["tile_step"]) == (58, 4096, 576, 2304, 16)
    p = R.plan(47248, 64, 1024, 20, **kw)
    assert (p["rank"], p["cap"]) == (10, 4096)
    assert R.plan(47248, 64, 1024, 50, list_lens=LENS, nprobe=16)["cap"] == 4096
    # the two-level select of the unfiltered pass
    p = R.plan(47248, 64, 128, 20, **kw)
    assert p["fin_pairs_lds"] and p["fin_lds"]
    p = R.plan(47248, 64, 129, 20, **kw)
    assert not p["fin_pairs_lds"] and p["fin_lds"]
    p = R.plan(47248, 64, 3, 5000, **kw)
    assert not p["fin_pairs_lds"] and not p["fin_lds"]


def test_expected_stats_and_chunks():
    assert R.passes(4100) == [4096, 4] and R.passes(4096) == [4096] and R.passes(1) == [1]
    assert R.redo_chunks(20, False) == [8, 8, 4] and R.redo_chunks(130, True) == [64, 64, 2] and R.redo_chunks(0, True) == []
    e = R.expected_stats(66000, 64, 4100, 500)
    assert (e["flat_fused"], e["passes"], e["sample_top"], e["thr_queries"]) == (2, 2, 1, 4100)
    e = R.expected_stats(47248, 64, 4100, 20, list_lens=LENS, nprobe=4)
    assert (e["ivf_thresholded"], e["ivf_unfiltered"], e["prepare_small"], e["thr_queries"]) == (1, 1, 1, 4096)
    assert R.redo_stats([20, 2], False) == (22, 4, 0) and R.redo_stats([70], True) == (70, 2, 1)


# ---- the reference's own rules on hand-made scores ---------------------------------------------------------------------
def test_topk_order_and_padding():
    S = np.array([[5, 7, 7, -3, 7, 5], [0, 0, 0, 0, 0, 0]], dtype=np.int64)
    s, r = R.topk(S, 4)
    assert r.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]] and s.tolist() == [[7, 7, 7, 5], [0, 0, 0, 0]]
    s, r = R.topk(S, 8)
    assert r[0].tolist() == [1, 2, 4, 0, 5, 3, -1, -1] and np.isneginf(s[:, 6:]).all() and s.dtype == np.float32
    allowed = np.array([[1, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0]], dtype=bool)
    s, r = R.topk(S, 3, allowed)
    assert r.tolist() == [[2, 0, 3], [-1, -1, -1]] and np.isneginf(s[1]).all()
    Q = np.array([[1, 0], [0, 2]], dtype=np.float32)
    X = np.array([[3, 1], [3, 4], [-8, 4]], dtype=np.float32)
    s, r = R.topk_chunked(Q, X, 2, chunk=1)
    assert r.tolist() == [[0, 1], [1, 2]] and s.tolist() == [[3, 3], [8, 8]]
    with pytest.raises(AssertionError):
        R.check_exact_inputs(np.array([0.5], dtype=np.float32))
    with pytest.raises(AssertionError):
        R.check_exact_inputs(np.array([9.0], dtype=np.float32))


def test_probed_lists_tie_rule():
    C = np.array([[8, 0], [0, 8], [0, 0], [0, 0]], dtype=np.float32)
    Q = np.array([[1, 0], [0, 0], [-1, -1]], dtype=np.float32)
    assert R.probed_lists(Q, C, 3).tolist() == [[0, 1, 2], [0, 1, 2], [2, 3, 0]]
    assign = np.array([0, 1, 1, 3, 2])
    assert R.allowed_by_lists(np.array([[1, 3]]), assign, 4).tolist() == [[False, True, True, True, False]]
    assert R.pred_pass([0b01, 0b11, 0b10, 0], (0b01, 0, 0b10)).tolist() == [True, False, False, False]
    assert R.pred_pass([5, 0], (0, 0, 0)).all()


def test_threshold_interval():
    samp = np.array([9, 9, 7, 5, 5, 1])
    assert R._interval(samp, 2, 6) == (9, 7) and R._interval(samp, 1, 6) == (9, 9) and R._interval(samp, 4, 6) == (5, 5)
    assert R._interval(samp, 6, 6) == (1, R.NEG) and R._interval(samp, 7, 100) is None and R._interval(samp, 3, 2) is None


def _toy_plan(**kw):
    p = dict(N=64, k=2, cap=4, rank=2, stride=2, S=32, cap_s=32, two_precision=False, sample_top=False)
    p.update(kw)
    return p


def test_flat_verdict_rule_all_f32():
    base = np.full(64, -5, dtype=np.int64)

    def verdict(changes, **kw):
        s = base.copy()
        for rows, v in changes:
            s[list(rows)] = v
        return int(R.flat_verdicts(s[None, :], _toy_plan(**kw))[0])
    # sampled rows are the even ones.  Threshold level 3 for sure (three sampled rows tie there), 2 + 3 candidates > cap
    assert verdict([((0, 2, 4), 3), ((1, 3), 8)]) == R.REDO
    assert verdict([((0, 2, 4), 3), ((1,), 8)]) == R.KEPT                        # 4 candidates == cap
    # the k-th candidate equals the threshold: kept (>= is inclusive)
    assert verdict([((0, 2, 4), 3)]) == R.KEPT
    assert verdict([((0, 2), 3)]) == R.KEPT                    # threshold in (-5, 3]: two candidates at either end
    assert verdict([((0, 2), 3), ((1, 3, 5, 7, 9), -4)]) == R.EITHER              # ... seven just above -5: may overflow
    # deficit: one candidate only at every threshold of the interval is impossible with rank 2 -> use k = 4
    assert verdict([((0, 2, 4), 3)], k=4) == R.REDO
    # interval: threshold in (0, 3]: at 3 two candidates, just above 0 five -> the overflow is possible, not certain
    assert verdict([((0, 2), 3), ((4,), 0), ((1, 3, 5), 1)]) == R.EITHER
    assert (R.redo_bounds([R.REDO, R.KEPT, R.EITHER, R.REDO])) == (2, 3)


def test_flat_verdict_rule_two_precision():
    two = dict(two_precision=True, seg_cap=2, filter=dict(per=1, tiles=2), sample=dict(per=1), k=2, cap=8)
    s = np.full(128, -5, dtype=np.int64)
    s[[0, 2, 4]] = 3                       # threshold 3 exactly
    s[[1, 71]] = 8                         # the two results, far above: the proof holds
    p = _toy_plan(N=128, S=64, cap_s=64, **two)
    qn = np.array([1.0])
    assert R.flat_verdicts(s[None, :], p, qnorm=qn, eps=0.03)[0] == R.REDO        # rows 0, 1, 2 share segment 0: 3 > seg_cap
    p["seg_cap"] = 4
    assert R.flat_verdicts(s[None, :], p, qnorm=qn, eps=0.03)[0] == R.KEPT
    assert R.flat_verdicts(s[None, :], p, qnorm=qn, eps=6.0)[0] == R.REDO         # 8 < 3 + 6: the proof fails
    assert R.flat_verdicts(s[None, :], p, qnorm=qn, eps=5.0)[0] == R.EITHER       # inside the f32 margin
    t = s.copy()
    t[[1, 71]] = 3                         # the k-th exact score equals the threshold
    assert R.flat_verdicts(t[None, :], p, qnorm=qn, eps=0.03)[0] == R.REDO
    # the wave's survivor queue: 64 queries with the same 4 survivors in one stage bring 256 > WQE entries, 48 queries 192
    v = np.full(128, -5, dtype=np.int64)
    v[[0, 2, 4]] = 3
    v[[1, 71]] = 8                         # rows 0, 1, 2, 4 survive in stage 0
    for n, want in ((64, R.EITHER), (48, R.KEPT)):
        st = R.flat_verdicts(v[None, :], p, qnorm=qn, eps=0.03, inv=np.zeros(n, dtype=np.int64))
        assert (st == want).all() and len(st) == n
    st = R.flat_verdicts(v[None, :], p, qnorm=qn, eps=0.03, inv=np.zeros(70, dtype=np.int64))
    assert (st[:64] == R.EITHER).all() and (st[64:] == R.KEPT).all()             # the second wave holds 6 queries
    # a register top-T stream may overflow: the lower end opens and nothing below REDO is certain
    p = _toy_plan(N=128, S=64, cap_s=64, sample_top=True, **two)
    p["seg_cap"] = 64
    u = np.full(128, -5, dtype=np.int64)
    u[np.arange(0, 40, 2)] = 3
    u[[1, 71]] = 8
    p["rank"] = 12
    assert R.flat_verdicts(u[None, :], p, qnorm=qn, eps=0.03)[0] == R.REDO        # 22 candidates > cap at every threshold
    p["cap"] = 64
    assert R.flat_verdicts(u[None, :], p, qnorm=qn, eps=0.03)[0] == R.EITHER      # 20 sampled in one split > SAMPLE_T


def test_ivf_verdict_rule():
    # two lists: list 0 = rows 0 .. 39 (sampled: its first 32), list 1 = rows 40 .. 44
    assign = np.array([0] * 40 + [1] * 5)
    probes = np.array([[0], [1], [0]])
    S = np.zeros((3, 45), dtype=np.int64)
    S[0, :4] = 9                                               # rank 3: threshold 9 exactly, 4 candidates >= k
    S[2, :3] = 9
    S[2, 3] = 5                                                # threshold in (5, 9]: 3 candidates < k = 4
    p = dict(k=4, cap=8, rank=3, cap_s=32)
    assert R.ivf_sampled_positions(40).tolist() == list(range(32)) and len(R.ivf_sampled_positions(32 * 17)) == 64
    st = R.ivf_verdicts(S, p, assign, probes, 2)
    assert st.tolist() == [R.KEPT, R.KEPT, R.REDO]             # query 1: 5 sampled rows... rank 3 of them tie at 0: kept
    p = dict(k=4, cap=8, rank=6, cap_s=32)
    assert R.ivf_verdicts(S, p, assign, probes, 2)[1] == R.KEPT    # fewer sampled rows than rank: no threshold, 5 <= cap
    p = dict(k=4, cap=4, rank=6, cap_s=32)
    assert R.ivf_verdicts(S, p, assign, probes, 2)[1] == R.REDO    # ... and 5 > cap


def test_filtered_verdict_rule():
    p = dict(k=3, cap=6, rank=2)
    assert R.filtered_verdict([5, 4, 3, 2, 1, 0], [5, 4], p, 8) == R.KEPT                 # all passing rows fit: no threshold
    assert R.filtered_verdict(list(range(8)), [7], p, 8) == R.REDO                          # one sampled row < rank: 8 > cap
    assert R.filtered_verdict([9, 9, 9, 9, 1, 1, 1, 1], [9, 9, 9, 1], p, 8) == R.KEPT      # threshold 9: 4 candidates
    assert R.filtered_verdict([9, 9, 1, 1, 1, 1, 1, 1], [9, 9, 0], p, 8) == R.EITHER       # (0, 9]: 2 < k or 8 > cap
    assert R.filtered_verdict([9, 9, 8, 1, 1, 1, 1, 1], [9, 9, 8], p, 8) == R.REDO         # threshold 9: 2 < min(k, 8)


def test_top_t_kept_bounds():
    p = dict(S=256, stride=2, sample=dict(per=1))               # sample splits of 64 sampled rows = 128 corpus rows
    s = np.zeros(512, dtype=np.int64)
    s[0:40:2] = 5                                               # 20 sampled rows of split 0
    s[1:41:2] = 9                                               # unsampled
    s[[130, 300, 302]] = 5                                      # one in split 1, two in split 2
    assert R.top_t_kept(s, p, 5) == (8 + 1 + 2, 16 + 1 + 2, 20) and R.top_t_kept(s, p, 6) == (0, 0, 0)
