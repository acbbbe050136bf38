"""Host side of the evaluation-report kernel tests (TEST INFRASTRUCTURE; Python / NumPy only, no GPU, no torch, and
nothing from recommendit_amd.eval_device or recommendit_amd.metrics).

Four things.

1.  THE REFERENCE, from the definitions (recommendit_amd/metrics.py and the reference's metrics.py:20-118, 168-190).
    A user's list is the row with its -1 entries removed; membership is Python ``set`` membership; DCG is the
    left-to-right f64 sum of ``1.0 / math.log2(i + 2)`` over the hit positions i < k; IDCG the same sum over
    ``min(len(relevant_with_duplicates), k)`` terms; recall is hits / len(set(relevant)); precision hits / k (0 at
    k = 0); mrr 1 / (first hit + 1).  Users without truth score 0 and are not counted.  Diversity: the first L listed
    ids, of those the ones with a vector (id < n_rows and present), duplicates kept; the mean over the pairs i < j with
    both norms > 0 of 1 - dot / (n_i n_j), in f64; 0 with fewer than 2 listed ids or fewer than 2 vectors.

2.  EXACT INPUTS FOR DIVERSITY (``exact_table``).  Every table row is zero or has exactly 1, 4, 16 or 64 non-zero
    entries (those that fit in g) of one magnitude +-2^a, a in -2..2.  Then every squared norm is a power of four
    (2^-4 .. 2^10), so sqrtf is exact; every dot product is a multiple of 2^-4 of magnitude <= 1024, exact on the f32
    MFMA and in a sequence of fmaf in any order; n_i n_j is a power of two, so dot / (n_i n_j) is an exact multiple of
    2^-14 in [-1, 1] and 1 - c one in [0, 2]: 16 significant bits.  The f64 sum of <= 130 816 such terms is below
    2^18 on the grid 2^-14: exact in any order.  sum / count is one correctly rounded division on both sides.  The
    per-user value is therefore compared with ``==``.  The non-zero columns are drawn from the front of one shuffled
    palette per table (a row of c entries from its first 2c columns), so two rows overlap often and the pair terms
    vary: a dropped, doubled or misplaced pair moves the mean.

3.  MEANS OF THE REPORT (``check_report``): math.fsum(values) / n_scored.  The device adds, all
    in f64, at most ceil(n / 512) rows per thread group, then at most 256 partials, then 512 parts: every value passes
    through at most ceil(n/512) + 256 + 512 additions, each with relative error 2^-53 of a partial sum that is at most
    the sum of the absolute values.  So |device - fsum| <= (ceil(n/512) + 768) 2^-53 sum|v| before the division, and
    the means are held to (ceil(n/512) + 768) * 2^-53 * mean_of_abs (the division's own half ulp on both sides is
    inside the 768's slack: the three stages have 255 + 511 additions, not 768).  Where every per-user value is a
    multiple of 2^-20 and the sum of absolute values is below 2^33, every partial sum is exact in f64 in any order:
    those means are compared with ``==`` as well (``all_dyadic``).  Coverage and n_scored are always ``==``.

4.  MIRRORS OF THE LAUNCH ARITHMETIC (``rank_regions`` / ``diversity_regions`` / ``reduce_partition`` / ...): small
    restatements of the loop structure of recommendit_amd/csrc/eval.hip (same names: base0, nvalid, kmax, first, cpos,
    H, s0, rpi) that report which regions of a kernel a row reaches.  They are not independent of the kernels; they
    exist so that tests/test_eval_reference_host.py can assert on the host that the GPU cases reach what they name.

The cases of tests/test_gpu_eval_kernels.py are built at the bottom (``*_case`` functions): both test files use them.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

CHUNK = 512            # ids per base0 trip of eval_rank_kernel
RANK_WAVES = 4 * 8192  # waves of the largest eval_rank_kernel grid
DIV_BLOCKS = 65536     # blocks (one wave each) of the largest eval_diversity_kernel grid
PARTS = 512            # EVAL_PARTS
SMALL_SEG = 64         # segments up to this size are searched with shuffles


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------------------------------
def listed(row: Sequence[int]) -> List[int]:
    return [int(x) for x in row if x >= 0]


def user_ranking(row: Sequence[int], relevant: Sequence[int], ks: Sequence[int]) -> Tuple[List[Tuple[float, float, float]], float]:
    """([(ndcg, recall, precision) per k], mrr) of one user with at least one relevant item"""
    lst = listed(row)
    rel = set(int(x) for x in relevant)
    hit_pos = [i for i, x in enumerate(lst) if x in rel]
    out = []
    for k in ks:
        dcg = 0.0
        hits = 0
        for i in hit_pos:
            if i < k:
                dcg += 1.0 / math.log2(i + 2)
                hits += 1
        idcg = 0.0
        for i in range(min(len(relevant), k)):
            idcg += 1.0 / math.log2(i + 2)
        ndcg = 0.0 if idcg == 0 else dcg / idcg
        out.append((ndcg, hits / len(rel), 0.0 if k == 0 else hits / k))
    rr = 1.0 / (hit_pos[0] + 1) if hit_pos else 0.0
    return out, rr


def ranking_reference(rec: np.ndarray, truth: Sequence[Sequence[int]], ks: Sequence[int]):
    """(vals f64 [n, len(ks), 3], mrr f64 [n], scored u8 [n]); ``truth[i]`` is user i's relevant list, duplicates
    kept, empty = no truth"""
    n = rec.shape[0]
    vals = np.zeros((n, len(ks), 3), np.float64)
    rr = np.zeros(n, np.float64)
    scored = np.zeros(n, np.uint8)
    for i in range(n):
        if len(truth[i]) == 0:
            continue
        v, r = user_ranking(rec[i].tolist(), truth[i], ks)
        vals[i] = v
        rr[i] = r
        scored[i] = 1
    return vals, rr, scored


def user_diversity(row: Sequence[int], L: int, tab: np.ndarray, present: Optional[np.ndarray]) -> float:
    lst = listed(row)[:L]
    if len(lst) < 2:
        return 0.0
    n_rows = tab.shape[0]
    ids = [x for x in lst if x < n_rows and (present is None or present[x])]
    if len(ids) < 2:
        return 0.0
    X = tab[ids].astype(np.float64)
    nr = np.sqrt((X * X).sum(axis=1))
    G = X @ X.T
    iu, ju = np.triu_indices(len(ids), 1)
    ok = (nr[iu] > 0) & (nr[ju] > 0)
    if not ok.any():
        return 0.0
    iu, ju = iu[ok], ju[ok]
    terms = 1.0 - G[iu, ju] / (nr[iu] * nr[ju])
    return math.fsum(terms.tolist()) / int(ok.sum())


def user_diversity_f32(row: Sequence[int], L: int, tab: np.ndarray, present: Optional[np.ndarray]) -> float:
    """the same value with every pair term computed in float32 (norms, dot, product, quotient, 1 - c), widened and
    summed in f64: on exact inputs bit for bit user_diversity"""
    lst = listed(row)[:L]
    if len(lst) < 2:
        return 0.0
    ids = [x for x in lst if x < tab.shape[0] and (present is None or present[x])]
    if len(ids) < 2:
        return 0.0
    X = tab[ids].astype(np.float32)
    nr = np.sqrt((X * X).sum(axis=1, dtype=np.float32)).astype(np.float32)
    G = (X @ X.T).astype(np.float32)
    iu, ju = np.triu_indices(len(ids), 1)
    ok = (nr[iu] > 0) & (nr[ju] > 0)
    if not ok.any():
        return 0.0
    iu, ju = iu[ok], ju[ok]
    terms = np.float32(1.0) - G[iu, ju] / (nr[iu] * nr[ju])
    assert terms.dtype == np.float32
    return math.fsum(terms.astype(np.float64).tolist()) / int(ok.sum())


def user_diversity_pairwise(row: Sequence[int], L: int, tab: np.ndarray, present: Optional[np.ndarray]) -> float:
    """The definition pair by pair in the table's own dtype (NumPy scalar arithmetic: float32 vectors give float32
    pair terms), added into a Python float.  This is what the reference project's loop computes, rounding residue
    included (a pair of parallel float32 vectors can give -1.2e-7); for small lists only."""
    lst = listed(row)[:L]
    if len(lst) < 2:
        return 0.0
    vecs = [tab[x] for x in lst if x < tab.shape[0] and (present is None or present[x])]
    if len(vecs) < 2:
        return 0.0
    total, count = 0.0, 0
    for i in range(len(vecs)):
        for j in range(i + 1, len(vecs)):
            n1, n2 = np.linalg.norm(vecs[i]), np.linalg.norm(vecs[j])
            if n1 > 0 and n2 > 0:
                total += 1 - np.dot(vecs[i], vecs[j]) / (n1 * n2)
                count += 1
    return float(total / count) if count else 0.0


def diversity_reference(rec: np.ndarray, scored: np.ndarray, L: int, tab: np.ndarray,
                        present: Optional[np.ndarray]) -> np.ndarray:
    """f64 [n]; identical rows are computed once"""
    out = np.zeros(rec.shape[0], np.float64)
    cache: Dict[bytes, float] = {}
    for i in range(rec.shape[0]):
        if not scored[i]:
            continue
        key = rec[i].tobytes()
        if key not in cache:
            cache[key] = user_diversity(rec[i].tolist(), L, tab, present)
        out[i] = cache[key]
    return out


def coverage_reference(rec: np.ndarray, scored: np.ndarray, catalog_size: int) -> float:
    shown = set()
    for i in np.nonzero(scored)[0]:
        shown.update(listed(rec[i].tolist()))
    return len(shown) / catalog_size


# ---------------------------------------------------------------------------------------------------------------------
# 3. means of the report and the comparison helpers
# ---------------------------------------------------------------------------------------------------------------------
def mean_bound(n: int, values: np.ndarray, n_scored: int) -> float:
    if n_scored == 0:
        return 0.0
    return (-(-n // PARTS) + 768) * 2.0 ** -53 * (math.fsum(np.abs(values).tolist()) / n_scored)


def all_dyadic(values: np.ndarray) -> bool:
    """every value a multiple of 2^-20 and sum|v| < 2^33: every partial sum, in any order, is exact in f64"""
    v = np.asarray(values, np.float64) * 2.0 ** 20
    return bool(np.all(v == np.floor(v))) and math.fsum(np.abs(v).tolist()) < 2.0 ** 53


def check_equal(name: str, got: np.ndarray, exp: np.ndarray, labels: Optional[Sequence[Any]] = None) -> None:
    """array_equal with a message that names the first wrong element (user, k-index, metric) and both values"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (name, got.shape, exp.shape, got.dtype, exp.dtype)
    if not np.array_equal(got, exp):
        bad = np.argwhere(~(got == exp))
        idx = tuple(int(x) for x in bad[0])
        where = f"user {idx[0]}"
        if len(idx) == 3:
            k = labels[idx[1]] if labels is not None else idx[1]
            where += f", k-index {idx[1]} (k = {k}), metric {('ndcg', 'recall', 'precision')[idx[2]]}"
        raise AssertionError(f"{name}: {len(bad)} of {got.size} elements differ; first at {where}: "
                             f"got {got[idx]!r}, expected {exp[idx]!r}")


@dataclass
class Reference:
    """per-user expectations of one case, for the distinct k in order of first appearance"""
    ks: List[int]
    vals: np.ndarray
    mrr: np.ndarray
    scored: np.ndarray
    diversity: Optional[np.ndarray] = None
    coverage: Optional[float] = None


def distinct(ks: Sequence[int]) -> List[int]:
    return list(dict.fromkeys(int(k) for k in ks))


def case_reference(case: "Case") -> Reference:
    ks = distinct(case.ks)
    vals, rr, scored = ranking_reference(case.rec, case.truth, ks)
    ref = Reference(ks, vals, rr, scored)
    if case.tab is not None:
        ref.diversity = diversity_reference(case.rec, scored, int(case.ks[-1]), case.tab, case.present)
    if case.catalog_size:
        ref.coverage = coverage_reference(case.rec, scored, case.catalog_size)
    return ref


def check_per_user(name: str, per: Dict[str, np.ndarray], ref: Reference) -> None:
    """per: numpy copies of the device's per-user tensors; everything with =="""
    check_equal(f"{name}: scored", per["scored"], ref.scored)
    check_equal(f"{name}: vals", per["vals"], ref.vals, ref.ks)
    check_equal(f"{name}: mrr", per["mrr"], ref.mrr)
    if ref.diversity is not None:
        check_equal(f"{name}: diversity", per["diversity"], ref.diversity)
    else:
        assert "diversity" not in per


def check_report(name: str, got: Dict[str, Any], case: "Case", ref: Reference, ratios: Optional[Dict[str, float]] = None
                 ) -> None:
    """The report dict against fsum / n_scored of the reference's per-user values: key order, == where derived, the
    derived bound elsewhere.  ``ratios`` collects the worst |device - reference| / bound per metric."""
    n = case.rec.shape[0]
    nsc = int(ref.scored.sum())
    keys = ["n_users", "k_values"]
    for k in distinct(case.ks):
        keys += [f"{m}@{k}" for m in ("ndcg", "recall", "precision", "mrr", "ap")]
    keys.append("mrr")
    if case.catalog_size and nsc:
        keys.append("coverage")
    if case.tab is not None and nsc:
        keys.append("avg_diversity")
    assert list(got.keys()) == keys, (name, list(got.keys()), keys)
    assert got["n_users"] == n and got["k_values"] == list(case.ks), name
    on = ref.scored.astype(bool)

    def mean(key: str, values: np.ndarray) -> None:
        values = values[on]
        want = math.fsum(values.tolist()) / nsc if nsc else 0.0
        bound = mean_bound(n, values, nsc)
        err = abs(got[key] - want)
        print(f"{name}: {key} device {got[key]!r} reference {want!r} |diff| {err:.3e} bound {bound:.3e}")
        if ratios is not None and bound > 0:
            metric = key.split("@")[0]
            ratios[metric] = max(ratios.get(metric, 0.0), err / bound)
        assert err <= bound, (name, key, got[key], want, bound)
        if all_dyadic(values):
            assert got[key] == want, (name, key, got[key], want, "dyadic values: the sum is exact")

    for j, k in enumerate(ref.ks):
        mean(f"ndcg@{k}", ref.vals[:, j, 0])
        mean(f"recall@{k}", ref.vals[:, j, 1])
        mean(f"precision@{k}", ref.vals[:, j, 2])
        assert got[f"mrr@{k}"] == 0.0 and got[f"ap@{k}"] == 0.0
    mean("mrr", ref.mrr)
    if "coverage" in keys:
        assert got["coverage"] == ref.coverage, (name, "coverage", got["coverage"], ref.coverage)
    if "avg_diversity" in keys:
        mean("avg_diversity", ref.diversity)


# ---------------------------------------------------------------------------------------------------------------------
# 4. mirrors of the launch arithmetic of csrc/eval.hip
# ---------------------------------------------------------------------------------------------------------------------
def rank_regions(row: Sequence[int], relevant: Sequence[int], kmax: int, cov: bool) -> Dict[str, Any]:
    """which regions of eval_rank_kernel<cov> one row reaches"""
    if len(relevant) == 0:
        return dict(search="none", trips=0, early_exit=False, hit_after_first_chunk=False, compacted_differs=False,
                    first=-1, nvalid=0)
    rel = set(int(x) for x in relevant)
    K = len(row)
    nvalid, first, trips = 0, -1, 0
    early = later_hit = differs = False
    for base0 in range(0, K, CHUNK):
        trips += 1
        nvalid_at_chunk_start = nvalid
        for pos in range(base0, min(base0 + CHUNK, K)):
            x = row[pos]
            if x < 0:
                continue
            if x in rel:
                if first < 0:
                    first = nvalid
                if base0 > 0:
                    later_hit = True
                    # the position is the carried nvalid plus the in-chunk prefix: holes in an earlier chunk make
                    # it differ from the raw position
                    if nvalid_at_chunk_start != base0:
                        differs = True
            nvalid += 1
        if not cov and first >= 0 and nvalid >= kmax:
            early = base0 + CHUNK < K
            break
    return dict(search="small" if len(rel) <= SMALL_SEG else "global", trips=trips, early_exit=early,
                hit_after_first_chunk=later_hit, compacted_differs=differs, first=first, nvalid=nvalid)


def rank_grid_stride(n: int) -> bool:
    """some wave of eval_rank_kernel takes a second row"""
    return n > min(-(-n // 4), 8192) * 4


def diversity_grid_stride(n: int) -> bool:
    return n > DIV_BLOCKS


def reduce_partition(n: int) -> Dict[str, int]:
    """rows per part, parts with rows, rows of the last non-empty part"""
    per = -(-n // PARTS)
    used = -(-n // per) if per else 0
    return dict(per=per, used=used, empty=PARTS - used, last=n - (used - 1) * per if used else 0)


def reduce_rpi(n_k: int) -> int:
    return 256 // (3 * n_k)


def diversity_regions(row: Sequence[int], L: int, n_rows: int, present: Optional[np.ndarray], g: int,
                      aligned: bool = True) -> Dict[str, Any]:
    lst = listed(row)
    m = sum(1 for x in lst[:L] if x < n_rows and (present is None or present[x]))
    vec = g % 8 == 0 and aligned
    H = (g + 1) // 2
    return dict(path="vec" if vec else "scalar", m=m, nvalid=min(len(lst), L), cap_decides=len(lst) > L,
                tiles=-(-m // 32), s0_trips=-(-H // 32) if vec else 0, partial_s0_trip=vec and H % 32 != 0,
                odd_g=g % 2 == 1, computed=min(len(lst), L) >= 2 and m >= 2)


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact inputs for diversity
# ---------------------------------------------------------------------------------------------------------------------
def exact_table(seed: int, n_rows: int, g: int, p_zero: float = 0.08) -> np.ndarray:
    rng = np.random.RandomState(seed)
    H = (g + 1) // 2
    front = list(dict.fromkeys([g - 1, H - 1, H % g, 0]))          # the columns at the edges of the two halves
    rest = [c for c in rng.permutation(g) if c not in front]
    palette = np.array(front + rest, dtype=np.int64)
    counts = [c for c in (1, 4, 16, 64) if c <= g]
    tab = np.zeros((n_rows, g), np.float32)
    for r in range(n_rows):
        if rng.random_sample() < p_zero:
            continue
        c = counts[rng.randint(len(counts))]
        cols = rng.choice(palette[:min(g, max(2 * c, 4))], size=c, replace=False)
        mag = np.float32(2.0 ** rng.randint(-2, 3))
        tab[r, cols] = mag * (1 - 2 * rng.randint(0, 2, size=c)).astype(np.float32)
    return tab


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_eval_kernels.py
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    rec: np.ndarray                      # int64 [n, K]
    truth: List[List[int]]               # relevant items per user, duplicates kept; [] = no truth
    ks: List[int]                        # as passed to the wrapper (may repeat)
    catalog_size: Optional[int] = None
    n_id_space: Optional[int] = None
    tab: Optional[np.ndarray] = None     # f32 [n_rows, g]
    present: Optional[np.ndarray] = None  # u8 [n_rows]
    notes: Dict[str, Any] = field(default_factory=dict)   # row names -> row index, for the host assertions

    @property
    def kmax(self) -> int:
        return max(self.ks)

    def regions(self, cov: bool) -> List[Dict[str, Any]]:
        return [rank_regions(self.rec[i].tolist(), self.truth[i], self.kmax, cov) for i in range(self.rec.shape[0])]


def _pad(rows: List[List[int]], K: int) -> np.ndarray:
    a = np.full((len(rows), K), -1, np.int64)
    for i, r in enumerate(rows):
        assert len(r) <= K, (len(r), K)
        a[i, :len(r)] = r
    return a


SEGMENT_SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 1000)


def segment_case() -> Case:
    """40 users, K = 96: four rows per segment size.  The segment's items are spaced 2..5 apart (so an id one off a
    member is no member) and start at 10; the truth list repeats half of them (raw > cnt)."""
    rng = np.random.RandomState(41)
    K = 96
    rows, truth, notes = [], [], {}
    for cnt in SEGMENT_SIZES:
        items = (10 + np.cumsum(rng.randint(2, 6, size=cnt))).tolist()
        first, last = items[0], items[-1]
        t = items + items[:max(1, cnt // 2)]
        t = [t[j] for j in rng.permutation(len(t))]
        edge = [first - 1, 0, last + 1, last + 1000, first, last, first + 1, last - 1, first - 2, last + 2]
        mid = [items[j] for j in rng.randint(0, cnt, size=30)]
        non = [x + 1 for x in mid[:15]]
        a = edge + mid + non
        b = []
        for x in items[:45]:
            b += [x, x + 1]
        c = []
        for x in reversed(items[-45:]):
            c += [x - 1, x]
        d = [(-1 if rng.random_sample() < 0.2 else (items[rng.randint(cnt)] + rng.randint(0, 2))) for _ in range(K)]
        notes[cnt] = len(rows)
        for r in (a, b, c, d):
            rows.append(r[:K])
            truth.append(list(t))
    return Case("segments", _pad(rows, K), truth, [1, 5, 10, 96, 200], notes=notes)


ROW_LENGTHS = (1, 63, 64, 65, 511, 512, 513, 1024, 1025, 2000, 16384)
# k lists of the row-length cases.  K <= 512: one list.  K > 512: kmax <= 512 (the exit is taken after chunk one),
# kmax in chunk two (the exit waits), kmax above K (never taken), kmax = 0 (taken as soon as there is a hit).
ROW_K_LISTS = {"mixed": lambda K: [10, 1, 510, K, K + 5, 0],
               "exit1": lambda K: [10, 1, 510],
               "wait": lambda K: [600, 513, 10],
               "never": lambda K: [K + 5, 512],
               "zero": lambda K: [0]}


def row_length_case(K: int, klist: str = "mixed") -> Case:
    """Rows by name (those that fit in K).  Item ids: 7 is THE relevant item of most rows (truth [7, 7, 900000]: one
    duplicate, one item never listed), everything else listed is >= 100."""
    rng = np.random.RandomState(1000 + K)
    T = [7, 7, 900000]
    rows: List[List[int]] = []
    truth: List[List[int]] = []
    notes: Dict[str, int] = {}

    def filler(n: int) -> List[int]:
        return rng.randint(100, 5000, size=n).tolist()

    def add(name: str, row: List[int], t=T) -> None:
        assert len(row) <= K
        notes[name] = len(rows)
        rows.append(row + [-1] * (K - len(row)))
        truth.append(list(t))

    add("all_holes", [-1] * K)
    last = filler(K)
    for p in range((K - 1) // 64 * 64):
        last[p] = -1                                   # valid entries only in the last 64-wide step
    last[K - 1] = 7
    add("only_last_step", last)
    for holes in (False, True):
        r = filler(K)
        for p in (511, 512, 513, K - 1):
            if 0 <= p < K:
                r[p] = 7
        if holes:
            for p in rng.choice(K, size=max(1, K // 9), replace=False):
                if r[p] != 7:
                    r[p] = -1
        add("hits_at_chunk_edges" + ("_holes" if holes else ""), r)
    add("no_truth", filler(K), t=[])
    add("no_hit", filler(K))
    r = filler(K)
    r[0] = 7
    add("hit_first", r)
    if K >= 516:
        r = filler(K)
        for p in (3, 64, 65, 200, 300, 511):
            r[p] = -1                                  # six holes in chunk one: raw 515 -> compacted 509 (< k = 510)
        r[515] = 7
        add("raw515_compacted509", r)
        # first hit in chunk one, chunk one full (nvalid = 512 >= kmax for kmax <= 512), later hits beyond kmax
        r = filler(K)
        r[4] = 7
        for p in (512, 530, K - 1):
            r[p] = 7
        add("exit_after_chunk_one", r)
        # no hit in chunk one: no exit there although nvalid >= kmax
        r = filler(K)
        r[520] = 7
        add("first_hit_in_chunk_two", r)
        # several relevant items, hits on both sides of the boundary, holes in both chunks
        r = filler(K)
        for p in rng.choice(K, size=K // 7, replace=False):
            r[p] = -1
        t2 = [7, 8, 9, 9, 11]
        for p, x in ((2, 8), (509, 9), (514, 11), (K - 2, 7)):
            r[p] = x
        add("mixed_hits_holes", r, t=t2)
    if K >= 1024:
        r = [-1] * K
        for p in range(K - 300, K):
            r[p] = int(rng.randint(100, 5000))
        r[K - 100] = 7
        add("only_last_chunk", r)
    return Case(f"row_length_{K}_{klist}", _pad(rows, K), truth, ROW_K_LISTS[klist](K), notes=notes)


def with_coverage(case: Case) -> Case:
    """the same case through eval_rank_kernel<true>"""
    top = int(case.rec.max()) + 1
    return Case(case.name + "_cov", case.rec, case.truth, case.ks, catalog_size=max(top, 1), n_id_space=max(top, 1),
                tab=case.tab, present=case.present, notes=case.notes)


K_LIST_SIZES = (1, 29, 42, 43, 64)


def k_list(n_k: int, K: int, kmax: Optional[int] = None) -> List[int]:
    """n_k distinct values, unsorted, containing (as far as n_k allows) 1, 0, K + 7 and kmax, followed by repeats"""
    rng = np.random.RandomState(n_k)
    base = [1, 0, K + 7, K, K - 1, 2, 3][:n_k] if n_k > 1 else [5]
    if kmax is not None:
        base = list(dict.fromkeys([1, 0, kmax, K - 1, 2, 3]))[:n_k]     # nothing above kmax
    pool = [k for k in range(4, max((kmax or K) - 1, 8 + 2 * n_k)) if k not in base]
    extra = rng.choice(pool, size=n_k - len(base), replace=False).tolist() if n_k > len(base) else []
    ks = base + [int(x) for x in extra]
    ks = [ks[j] for j in rng.permutation(len(ks))]
    assert len(set(ks)) == n_k
    return ks + ks[:2]                                  # repeats: the wrapper de-duplicates


def k_list_case(n_k: int, n: int = 1100, K: int = 48, kmax: Optional[int] = None) -> Case:
    """random rows with holes and short valid counts; n = 1100 gives 3 rows per part, so rpi = 1 and 2 differ"""
    rng = np.random.RandomState(500 + n_k + K)
    rec = rng.randint(0, 400, size=(n, K)).astype(np.int64)
    rec[rng.random_sample((n, K)) < 0.1] = -1
    short = np.nonzero(rng.random_sample(n) < 0.3)[0]
    for i in short:
        rec[i, rng.randint(0, K):] = -1                 # valid counts below many of the k
    truth: List[List[int]] = []
    for i in range(n):
        if i % 9 == 4:
            truth.append([])
            continue
        m = int(rng.randint(1, 70))
        t = rng.randint(0, 400, size=m).tolist()
        row = rec[i][rec[i] >= 0]
        if row.size:
            t += rng.choice(row, size=min(6, row.size)).tolist()
        truth.append([int(x) for x in t])
    return Case(f"k_list_{n_k}_{K}", rec, truth, k_list(n_k, K, kmax))


@functools.lru_cache(maxsize=None)
def stride_case(n: int = 70000) -> Case:
    """K = 8, k in {1, 2, 4, 8}: every row's ids are distinct, the segment has 1, 2, 4 or 8 items, the first hit is at
    compacted position 0, 1, 3 or 7 (or there is none), every 5th user has no truth.  recall (hits / cnt), precision
    (hits / k) and mrr are dyadic; ndcg is not."""
    rng = np.random.RandomState(70)
    K = 8
    r0 = rng.randint(0, 997, size=n)
    rec = (r0[:, None] + 7 * np.arange(K)[None, :]) % 997          # distinct within a row (7 is a unit mod 997)
    holes = rng.random_sample((n, K)) < 0.15
    rec = np.where(holes, -1, rec).astype(np.int64)
    cnts = rng.randint(0, 4, size=n)
    fsel = rng.randint(0, 5, size=n)
    takes = rng.random_sample((n, K)) < 0.5
    truth: List[List[int]] = []
    recl = rec.tolist()
    for i in range(n):
        if i % 5 == 2:
            truth.append([])
            continue
        cnt = 1 << int(cnts[i])
        lst = [x for x in recl[i] if x >= 0]
        f = (0, 1, 3, 7, 99)[fsel[i]]
        t: List[int] = []
        if f < len(lst):
            t.append(lst[f])
            t += [x for j, x in enumerate(lst) if j > f and takes[i, j]][:cnt - 1]
        t += list(range(1000 + i % 50, 1000 + i % 50 + cnt - len(t)))   # never listed
        if i % 3 == 0:
            t = t + t[:1]                                            # a duplicate: raw > cnt
        truth.append(t)
    return Case(f"stride_{n}", rec, truth, [1, 2, 4, 8])


PARTITION_SIZES = (1, 511, 512, 513, 1025)

COVERAGE_SPACES = (1, 511, 512, 513, 100003)


def coverage_case(S: int) -> Case:
    """K = 1024, ids < S.  Rows: `ends` lists id 0 and id S - 1; `no_truth` lists ids nobody else does (they must not
    count); `second_chunk` lists an id of its own at raw position 700 only (it must count)."""
    rng = np.random.RandomState(S % 1000)
    K = 1024
    lo, hi = (1, max(2, min(S - 1, 300))) if S > 3 else (0, 1)
    reserved = [] if S <= 3 else [hi, hi + 1, hi + 2]              # ids that only the named rows list

    def filler(n: int) -> List[int]:
        return rng.randint(lo, hi, size=n).tolist() if S > 1 else [0] * n

    rows, truth, notes = [], [], {}
    r = filler(K)
    r[0], r[5] = 0, S - 1
    notes["ends"] = 0
    rows.append(r); truth.append([0, 5])
    r = filler(K)
    if reserved:
        r[3], r[900] = reserved[0], reserved[1]
    notes["no_truth"] = 1
    rows.append(r); truth.append([])
    r = filler(K)
    for p in range(0, 512, 5):
        r[p] = -1
    if reserved:
        r[700] = reserved[2]
    notes["second_chunk"] = 2
    rows.append(r); truth.append([r[1] if r[1] >= 0 else 0, 77])
    rows.append([-1] * K); truth.append([1])
    return Case(f"coverage_{S}", _pad(rows, K), truth, [10, 600], catalog_size=S + 3, n_id_space=S,
                notes=dict(notes, reserved=reserved))


# (g, L): every g of {1, 2, 3, 7, 8, 18, 72, 128, 250, 256} and every L of {0, 1, 2, 31, 32, 33, 64, 65, 100, 511, 512}
DIVERSITY_SHAPES = ((1, 2), (2, 0), (3, 1), (7, 33), (8, 31), (18, 32), (72, 65), (128, 64), (250, 100), (256, 512),
                    (18, 511), (8, 512), (3, 100), (128, 33))
DIV_ROWS = 300


def diversity_case(g: int, L: int, n_random: int = 24) -> Case:
    """K = L + 40.  Ids: table rows 0 .. 299 (about 8 % zero vectors, about 12 % absent), ids 300 .. 339 beyond the
    table.  Named rows with an exact number m of vectors among the first L listed ids, around every tile edge."""
    rng = np.random.RandomState(7000 + 13 * g + L)
    K = max(L + 40, 42)
    tab = exact_table(100 + g, DIV_ROWS, g)
    present = (rng.random_sample(DIV_ROWS) >= 0.12).astype(np.uint8)
    have = np.nonzero(present)[0]
    zero = [int(x) for x in have if not tab[x].any()]
    nonzero = [int(x) for x in have if tab[x].any()]
    absent = [int(x) for x in np.nonzero(present == 0)[0]] + list(range(DIV_ROWS, DIV_ROWS + 40))
    assert len(zero) >= 2 and len(nonzero) >= 2 and len(absent) >= 2
    rows: List[List[int]] = []
    notes: Dict[str, int] = {}

    def pick(pool: List[int], n: int) -> List[int]:
        return [pool[j] for j in rng.randint(0, len(pool), size=n)]

    def add(name: str, row: List[int]) -> None:
        notes[name] = len(rows)
        rows.append(row[:K])

    for m in (2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512):
        if m > L:
            continue
        head = pick([int(x) for x in have], m) + pick(absent, L - m)
        head = [head[j] for j in rng.permutation(L)]
        # L valid ids with exactly m vectors, a few holes in between, then vectors that the cap must keep out
        row = list(head)
        for p in sorted(rng.randint(0, L + 1, size=8).tolist(), reverse=True):
            row.insert(p, -1)
        add(f"m{m}", row + pick(nonzero, K - len(row)))
    add("one_vector", pick(nonzero, 1) + pick(absent, 9))
    add("two_zero_vectors", zero[:1] + [-1] + zero[1:2] + pick(absent, 5))
    add("duplicates", pick(nonzero, 1) * 3 + pick(nonzero, 2) * 2)
    add("dense", pick(nonzero, K))                                    # more than L valid ids: cpos < L decides
    add("all_holes", [-1] * K)
    add("one_listed", [-1, nonzero[0]])
    for _ in range(n_random):
        r = rng.randint(0, DIV_ROWS + 40, size=K)
        r[rng.random_sample(K) < 0.06] = -1
        if rng.random_sample() < 0.3:
            r[rng.randint(1, K):] = -1
        add(f"random{len(rows)}", r.tolist())
    n = len(rows)
    truth = [[] if i % 11 == 5 else [int(max(rows[i][0], 0)), 999999] for i in range(n)]
    ks = [5, L] if L != 5 else [L]
    return Case(f"diversity_g{g}_L{L}", _pad(rows, K), truth, ks, tab=tab, present=present, notes=notes)


@functools.lru_cache(maxsize=None)
def diversity_stride_case(n: int = 66000) -> Case:
    """K = 4, L = 4, g = 4 over an alphabet of 8 symbols (-1, five table rows of which one is zero and one absent, one
    id beyond the table): 4096 distinct rows, every user compared"""
    rng = np.random.RandomState(66)
    tab = exact_table(4, 6, 4, p_zero=0.0)
    tab[4] = 0.0
    present = np.array([1, 1, 1, 0, 1, 1], np.uint8)
    sym = np.array([-1, 0, 1, 2, 3, 4, 5, 6], np.int64)               # 6 >= n_rows
    rec = sym[rng.randint(0, 8, size=(n, 4))]
    truth = [[] if i % 7 == 3 else [1] for i in range(n)]
    return Case(f"diversity_stride_{n}", rec, truth, [4], tab=tab, present=present)
