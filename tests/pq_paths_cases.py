"""The cases of tests/test_gpu_pq_paths.py, built without a device: inputs, the references' expectations, and the
assertions that the inputs reach the path a case is about.  tests/test_pq_paths_host.py runs every builder on the CPU; the
GPU file runs the same builders and then the device.  Nothing here imports the package.

Everything is stated over tests/pq_reference.py, pq_residual_reference.py, sq8_reference.py, sq8_filtered_reference.py and
sq8_refine_reference.py.  With the injected quantiser (0, 1/128) and injected codebooks a row IS a codebook entry per
sub-space (plus its list's code on a residual index), so entry numbers, SQ8 codes and the decoded matrix are known by
construction and every distance of the assignment is 0 at exactly one entry."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_reference as P  # noqa: E402
import pq_residual_reference as PR  # noqa: E402
import sq8_filtered_reference as FR  # noqa: E402
import sq8_reference as S  # noqa: E402
import sq8_refine_reference as R  # noqa: E402

REDO_CHUNK = 64           # queries per re-do chunk (sq8_redo)
TRAIN_BLOCK = 2048        # physical rows per workgroup of the assignment pass (PQ_RPB)
NONE_BIT = 1 << 15        # carried by every row of one list: a predicate that excludes it passes nothing there
ID0 = 1000                # item id of row 0 wherever a case searches by item id


def unit_quantizer(du):
    """the injected quantiser (0, 1/128): the SQ8 code of x is 128 x"""
    return np.zeros(du, np.float32), np.full(du, 1.0 / 128.0, np.float32)


def list_layout(assign, nlist):
    """(pos int64 [N]: a row's position inside its list -- rows ascend inside a list; phys int64 [N]: its physical row,
    the lists in order and each padded to S.GRANULE rows; lens)"""
    assign = np.asarray(assign, dtype=np.int64)
    lens = np.bincount(assign, minlength=nlist)
    order = np.argsort(assign, kind="stable")
    start = np.cumsum(lens) - lens
    pos = np.empty(len(assign), dtype=np.int64)
    pos[order] = np.arange(len(assign)) - start[assign[order]]
    padded = (lens + S.GRANULE - 1) // S.GRANULE * S.GRANULE
    poff = np.cumsum(padded) - padded
    return pos, poff[assign] + pos, lens


def real_subspaces(du, dsub):
    return np.array([m * dsub < du for m in range(P.dpad_of(du) // dsub)])


def check_book(book, du):
    """what the gather mutants rely on: 256 pairwise distinct entries in every real sub-space, no entry (but 0) shared
    between two sub-spaces at the same number, padding columns 0"""
    M, _, dsub = book.shape
    real = np.nonzero(real_subspaces(du, dsub))[0]
    col = np.arange(M * dsub).reshape(M, 1, dsub)
    assert (book[np.broadcast_to(col >= du, book.shape)] == 0).all()
    for m in real:
        assert len({e.tobytes() for e in book[m]}) == 256, m
    for i, m in enumerate(real):
        for m2 in real[i + 1:]:
            assert (book[m, 1:] != book[m2, 1:]).any(axis=1).all(), (m, m2)


def random_book(rng, du, dsub, low=-127, low_first16=None):
    """int8 [M, 256, dsub]: entry 0 of every real sub-space is all +127 (what a padding row decodes to: it takes first
    place wherever it leaks), the others random in [low, 127] ([low_first16, 127] in columns 0 .. 15); padding columns 0"""
    dpad = P.dpad_of(du)
    M = dpad // dsub
    book = rng.integers(low, 128, (M, 256, dsub))
    col = np.arange(dpad).reshape(M, 1, dsub)
    if low_first16 is not None:
        book = np.where(col < 16, rng.integers(low_first16, 128, (M, 256, dsub)), book)
    book[:, 0] = 127
    book = np.where(col < du, book, 0).astype(np.int8)
    check_book(book, du)
    return book


def every_entry_occurs(codes, du, dsub):
    for m in np.nonzero(real_subspaces(du, dsub))[0]:
        assert (np.bincount(codes[:, m], minlength=256) > 0).all(), m


class Expect:
    """the reference of one (queries, decoded matrix) pair: the query transform and the integer scores, never changed"""

    def __init__(self, Q, dec, m, s):
        self.n, self.t, self.b = S.encode_queries(Q, m, s)
        self.Sc = S.int_scores_blas(self.n, dec)
        assert np.abs(self.Sc).max() <= PR.SCORE_BOUND
        self.Sc.setflags(write=False)

    def top(self, k, allowed=None):
        return S.topk_fast(self.Sc, k, allowed)

    def float_ref(self, sc):
        """(float32)(b + t S) evaluated in f64"""
        return (self.b[:, None] + self.t.astype(np.float64)[:, None] * sc.astype(np.float64)).astype(np.float32)


# ============================================ A. the instantiation matrix ===================================================
# r27's case c (16 lists, N 39 575, nprobe 4, nq 1 024) shrunk: the short lists stay (two empty ones, one row, 63, 64, 65),
# the long ones are a third as long, and the queries are steered onto the long lists, so the plan keeps tpi >= 3 at a
# quarter of the (query, row) pairs.  Lists 0 .. 3 hold 66 rows: what queries 0 and 1 probe.
A_LENS = [0, 1, 65, 0, 63, 64, 2049, 3001, 2777, 2203, 1999, 1131, 900, 501, 411, 277]
A_NPROBE, A_NQ, A_KS = 4, 1000, (10, 100)
A_FAIL_LIST = 8           # its rows carry NONE_BIT
A_MENU = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (4, 0, 0), (8, 0, 0), (0, 0x60, 0), (6, 0x20, 0x80)]
FMS = ("tags", "mask", "tags_mask")


def _tags(rng, n):
    """bit 0 on every row, bit 1 on half, bit 2 on a tenth, bit 3 on 3 %, bits 5 - 7 on half each"""
    t = np.zeros(n, dtype=np.uint32)
    for b, p in enumerate([1.0, 0.5, 0.1, 0.03, 0.0, 0.5, 0.5, 0.5]):
        t |= (rng.random(n) < p).astype(np.uint32) << np.uint32(b)
    return t


def matrix_plan(probes):
    """the plan of the full pass and what section A asks of it, from S.plan alone"""
    nlist = len(A_LENS)
    per_list = np.bincount(probes.ravel(), minlength=nlist)
    tpi, n_seq, splits = S.plan(A_LENS, per_list, 1)
    assert tpi >= 3, ("inputs no longer reach the path", tpi)
    probed = [l for l in range(nlist) if per_list[l] > 0]
    assert any(n_seq[l] % tpi != 0 and n_seq[l] > tpi for l in probed)          # a ragged last split behind full ones
    assert any(A_LENS[l] % S.TILE != 0 and A_LENS[l] > 0 for l in probed)       # a short last tile: n_ok
    assert any(per_list[l] % 32 != 0 for l in probed)                           # a partial last query group
    assert {0, 1, 2, 3} <= set(probed)                                          # the empty, the one-row and the 65-row list
    assert S.dense_chunk(A_LENS, A_NPROBE) >= A_NQ                              # one dense pass
    return tpi, n_seq


def matrix_case(du, dsub, res):
    """one (du, dsub, RES) fixture of section A; the three FM values share it (matrix_expect)"""
    rng = np.random.default_rng(36000 + 100 * du + 10 * dsub + int(res))
    N, nlist = sum(A_LENS), len(A_LENS)
    dpad = P.dpad_of(du)
    M = dpad // dsub
    real = real_subspaces(du, dsub)
    assert (~real).any() and du > 16                             # a fully padded sub-space
    partly = [m for m in range(M) if m * dsub < du < (m + 1) * dsub]
    assert bool(partly) == ((du, dsub) != (40, 8))               # and a partly padded one, but where 8 divides du
    m_, s_ = unit_quantizer(du)
    assign = np.concatenate([np.full(n, l, np.int32) for l, n in enumerate(A_LENS)])[rng.permutation(N)]
    pos, phys, lens = list_layout(assign, nlist)
    assert lens.tolist() == A_LENS and lens[0] == lens[3] == 0 and lens[1] == 1 and lens[2] == 65
    # centroids: -1024 on the list's own axis (columns 0 .. 15) decides the probes; beyond column 15 they are list codes
    # / 128 in [-40, 0].  On the SQ8 grid: K[l][l] = -127 (clamped), K[l][j >= 16] = Kr, else 0
    Kr = rng.integers(-40, 1, (nlist, du))
    Cc = (Kr / 128.0).astype(np.float32)
    Cc[:, :16] = 0.0
    Cc[np.arange(nlist), np.arange(nlist)] = -1024.0
    K = PR.list_codes(Cc, m_, s_, dpad)
    assert (K[np.arange(nlist), np.arange(nlist)] == -127).all() and (K[:, 16:du] == Kr[:, 16:]).all()
    assert len({k.tobytes() for k in K}) == nlist
    # residual: entries >= 0 in columns 0 .. 15 and >= -87 beyond, so list code + entry never leaves [-127, 127]: no clamp,
    # the residual of a row is its entry and the assignment finds it at D = 0
    book = random_book(rng, du, dsub, -87, 0) if res else random_book(rng, du, dsub)
    codes = rng.integers(0, 256, (N, M)).astype(np.uint8)
    codes[:, ~real] = 0
    long_rows = np.nonzero(assign == 7)[0]
    codes[long_rows[2000:2200]] = codes[long_rows[100:300]]       # ties inside a list across its splits
    every_entry_occurs(codes, du, dsub)
    if res:
        dec = PR.decode(codes, book, K, assign)
        assert dec.dtype == np.int16 and np.abs(dec).max() <= 127
        r, clamped = PR.residuals(dec.astype(np.int8), K, assign)
        assert clamped == 0
        np.testing.assert_array_equal(P.assign(r[:300], book)[0], codes[:300])        # (the restatement agrees on a sample)
    else:
        dec = P.decode(codes, book)
        np.testing.assert_array_equal(P.assign(dec[:300], book)[0], codes[:300])
    X = dec[:, :du].astype(np.float32) / np.float32(128.0)
    np.testing.assert_array_equal(S.encode(X, m_, s_), dec[:, :du])
    # queries: -1 on the axes of the four lists they probe, +1 on the other twelve
    want = np.empty((A_NQ, A_NPROBE), dtype=np.int64)
    want[0] = want[1] = [0, 1, 2, 3]
    want[2] = want[3] = [1, 2, 4, 5]
    w = np.array(A_LENS[6:], dtype=np.float64)
    prng = np.random.default_rng(36001)                          # the same probes, so the same plan, in every fixture
    for q in range(4, A_NQ):
        want[q] = 6 + prng.choice(nlist - 6, A_NPROBE, replace=False, p=w / w.sum())
    Q = (rng.integers(-16, 17, (A_NQ, du)) / 8.0).astype(np.float32)
    Q[:, :16] = 1.0
    np.put_along_axis(Q, want, -1.0, axis=1)
    Q[5, 16:] = np.abs(Q[5, 16:]) + 0.125                        # all weights beyond the axes positive: entry 0 scores best
    probes = S.probed_lists(Q, Cc, A_NPROBE)
    np.testing.assert_array_equal(np.sort(probes, axis=1), np.sort(want, axis=1))
    tpi, n_seq = matrix_plan(probes)
    probed = FR.probed_mask(assign, probes, nlist)
    assert probed[0].sum() == probed[1].sum() == 66 < max(A_KS)
    ex = Expect(Q, dec[:, :du], m_, s_)
    if res:
        np.testing.assert_array_equal(PR.split_scores(ex.n, codes, book, K, assign), ex.Sc)
        T = PR.pair_offsets(ex.n, K, probes)
        assert (np.sort(T, axis=1)[:, 1:] != np.sort(T, axis=1)[:, :-1]).all(axis=1).mean() > 0.9   # T differs by list
    # tags and per-query predicates: pass rates from 100 % down to about 3 %; list A_FAIL_LIST fails whoever excludes NONE_BIT
    tags = _tags(rng, N)
    tags[assign == A_FAIL_LIST] |= NONE_BIT
    preds = np.array([A_MENU[i] for i in rng.integers(0, len(A_MENU), A_NQ)], dtype=np.uint32)
    preds[:4] = (0, 0, 0)
    preds[np.arange(A_NQ) % 5 == 4, 2] |= NONE_BIT
    ok = FR.passes(tags, preds)
    rate = ok.mean(axis=1)
    assert rate.max() == 1.0 and rate.min() < 0.04 and (rate > 0.2).mean() > 0.4
    hit = [q for q in range(A_NQ) if (preds[q, 2] & NONE_BIT) and A_FAIL_LIST in probes[q]]
    assert hit and not (ok[hit[0]] & (assign == A_FAIL_LIST)).any() and (ok[hit[0]] & probed[hit[0]]).any()
    # seen lists: every other one of the best rows (0, 5 or 40 by query), and from query 10 on the best row and one row of
    # the last tile of a split
    top, _ = ex.top(max(A_KS), probed)
    tile = pos // S.TILE
    last_of_split = (tile % tpi == tpi - 1) | (tile == np.array(n_seq)[assign] - 1)
    counts = np.array([0] * 20 + [5] * 400 + [40] * (A_NQ - 420))
    seen = np.zeros((A_NQ, N), dtype=bool)
    for q in range(A_NQ):
        mine = top[q, 1:2 * counts[q]:2]
        seen[q, mine[mine >= 0]] = True
        if q >= 10:
            valid = top[q][top[q] >= 0]
            edge = valid[last_of_split[valid]]
            assert len(edge), q
            seen[q, [valid[0], edge[0]]] = True
    assert not seen[:10].any() and seen[10:].any(axis=1).all()
    for k in A_KS:                                               # the seen rows are among the unrestricted top k
        in_top = np.take_along_axis(seen, np.maximum(top[:, :k], 0), axis=1) & (top[:, :k] >= 0)
        assert in_top[10:].any(axis=1).all() and in_top[10:, 0].all()
    users, rows = np.nonzero(seen)
    return dict(du=du, dsub=dsub, res=res, N=N, nlist=nlist, assign=assign, pos=pos, Cc=Cc, K=K, book=book, codes=codes,
                dec=dec[:, :du], X=X, m=m_, s=s_, Q=Q, probes=probes, probed=probed, ex=ex, tags=tags, preds=preds, ok=ok,
                seen=seen, seen_pairs=(users, rows + ID0), ids=np.arange(N, dtype=np.int64) + ID0, tpi=tpi,
                last_of_split=last_of_split, top=top)


def matrix_expect(case, fm):
    """(rows, scores) of the top max(A_KS) and {k: re-do verdicts} of one filter mode, from the shared reference"""
    keep = {"tags": case["ok"], "mask": ~case["seen"], "tags_mask": case["ok"] & ~case["seen"]}[fm]
    rows, sc = case["ex"].top(max(A_KS), case["probed"] & keep)
    valid = rows[rows >= 0]
    assert case["last_of_split"][valid].any()                    # rows of the last tile of a split are among the results
    if fm != "tags":
        assert (rows[10:, 0] != case["top"][10:, 0]).all()       # the mask visibly changes every such query's result
    if fm == "tags_mask":
        only_tags = case["ex"].top(min(A_KS), case["probed"] & case["ok"])[0]
        assert (rows[:, :min(A_KS)] != only_tags).any(axis=1).mean() > 0.25
    redo = {k: FR.thresholded_redo(case["ex"].Sc, k, case["assign"], case["probes"], case["nlist"], keep) for k in A_KS}
    return rows, sc, redo


# ============================================ B1. every query re-done =======================================================
B1_SHAPES = {"pq-64-8": (64, 8, False), "pq-128-16": (128, 16, False), "res-64-16": (64, 16, True), "res-128-8": (128, 8, True)}
B1_K = 10


def redo_case(shape, nq, variant=None):
    """every row decodes to the same code x, so all probed scores of a query tie, overflow the 4 096 candidate slots and the
    query is re-done.  Plain: 6 000 rows in one list.  Residual: three lists of 3 000 rows (row i in list i mod 3) with
    pairwise different list codes K_l; entry l of every sub-space is x - K_l, so the gathered dot product and T[q, l] both
    differ by list and only their sum ties.  variant "seen": each query has seen a handful of the lowest rows; "tags":
    per-query predicates cut the rows differently"""
    d, dsub, res = B1_SHAPES[shape]
    rng = np.random.default_rng(36100 + d + dsub + nq + (0 if variant is None else len(variant)))
    M = d // dsub
    m_, s_ = unit_quantizer(d)
    book = random_book(rng, d, dsub)
    if res:
        nlist, N = 3, 9000
        assign = (np.arange(N) % nlist).astype(np.int32)
        x = rng.integers(-60, 61, d).astype(np.int16)
        Kr = rng.integers(-60, 61, (nlist, d))
        Cc = (Kr / 128.0).astype(np.float32)
        K = PR.list_codes(Cc, m_, s_, d)
        np.testing.assert_array_equal(K, Kr)
        assert all((K[a] != K[b]).mean() > 0.9 for a in range(nlist) for b in range(a))
        for l in range(nlist):
            book[:, l] = (x - Kr[l]).reshape(M, dsub)
        check_book(book, d)
        got, dist, clamped = PR.assign_with(np.tile(x.astype(np.int8), (nlist, 1)), K, np.arange(nlist), book)
        assert dist == 0 and clamped == 0 and (got == np.arange(nlist)[:, None]).all()
        codes = np.tile(assign.astype(np.uint8)[:, None], (1, M))
        dec = PR.decode(codes, book, K, assign)
        assert (dec == x[None, :]).all()                         # every decoded row equals x
        lens = [N // nlist] * nlist
    else:
        nlist, N, assign, Cc, K = 1, 6000, None, None, None
        row = rng.integers(1, 256, M).astype(np.uint8)
        codes = np.tile(row, (N, 1))
        x = P.decode(row[None, :], book)[0].astype(np.int16)
        lens = [N]
    assert np.abs(x).max() > 50
    X = np.tile(x.astype(np.float32) / np.float32(128.0), (N, 1))
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q[S.PASS_QUERIES:] = 16.0 * Q[S.PASS_QUERIES:] + 3.0         # the second pass: other t and b by an order of magnitude
    n, t, b = S.encode_queries(Q, m_, s_)
    col = S.int_scores(n, x[None, :])[:, 0]
    Sc = np.broadcast_to(col[:, None], (nq, N))
    if res:
        probes = S.probed_lists(Q, Cc, nlist)
        T = PR.pair_offsets(n, K, probes)
        assert ((T[:, 0] != T[:, 1]) & (T[:, 1] != T[:, 2]) & (T[:, 0] != T[:, 2])).mean() > 0.9
        assert len({tuple(p) for p in probes.tolist()}) > 1      # the probe order differs between queries
    else:
        assign, probes = np.zeros(N, np.int64), np.zeros((nq, 1), np.int64)
    keep = np.ones((nq, N), dtype=bool)
    tags = preds = None
    if variant == "seen":
        for q in range(nq):
            keep[q, [(5 * q + 3 * j) % 30 for j in range(2 + q % 5)]] = False
        assert len({r.tobytes() for r in keep[:, :30]}) > 25
    elif variant == "tags":
        tags = (np.uint32(1) << (np.arange(N) % 5).astype(np.uint32)).astype(np.uint32)
        preds = np.zeros((nq, 3), dtype=np.uint32)
        preds[:, 2] = np.uint32(1) << (np.arange(nq) % 5).astype(np.uint32)
        odd = np.arange(nq) % 2 == 1
        preds[odd, 2] |= np.uint32(1) << ((np.arange(nq)[odd] + 2) % 5).astype(np.uint32)
        keep = FR.passes(tags, preds)
        assert sorted(set(keep.sum(axis=1).tolist())) == [3 * N // 5, 4 * N // 5]
    # -- the path
    assert S.threshold_cap(B1_K, lens, nlist) == 4096 < keep.sum(axis=1).min()
    state = FR.thresholded_redo(Sc, B1_K, assign, probes, nlist, keep)
    assert (state == S.REDO).all(), "inputs no longer reach the path"
    assert (nq - 1) // REDO_CHUNK + 1 >= 3 and (nq > S.PASS_QUERIES or nq % REDO_CHUNK == 2)
    assert len(np.unique(col)) > 0.9 * nq and len(np.unique(t)) > 0.9 * nq
    if nq > S.PASS_QUERIES:
        assert t[S.PASS_QUERIES:].min() > 2 * t[:S.PASS_QUERIES].max()
    low = np.sort(np.argsort(~keep[:, :64], axis=1, kind="stable")[:, :B1_K], axis=1)   # the k lowest rows a query may return
    assert (np.take_along_axis(keep, low, axis=1)).all()
    ref32 = (b[:, None] + t.astype(np.float64)[:, None] * col.astype(np.float64)[:, None]).astype(np.float32)
    return dict(d=d, dsub=dsub, res=res, N=N, nlist=nlist, assign=assign, Cc=Cc, K=K, book=book, codes=codes, x=x, X=X, m=m_,
                s=s_, Q=Q, rows=low, score=col, ref32=ref32, keep=keep, tags=tags, preds=preds,
                ids=np.arange(N, dtype=np.int64) + ID0)


# ============================================ B2. deficit re-do under a real threshold ======================================
def deficit_case():
    """r27's case d on a residual index of two lists (row i in list i mod 2), <64, 8, RES>: the sampled rows' column 0 is
    far above every other row's, so fewer than k = 2 000 rows reach the 174th best sampled score and no list overflows.
    K differs by 20 on column 0: a score taken with the other list's T, or without T, moves by 20 of the 30 units between the
    two groups"""
    N, d, dsub, nq, k, nlist = 16384, 64, 8, 70, 2000, 2
    rng = np.random.default_rng(36200)
    M = d // dsub
    m_, s_ = np.zeros(d, np.float32), np.ones(d, np.float32)     # ranges (0, 1): the code of x is x
    assign = (np.arange(N) % nlist).astype(np.int32)
    pos, _, lens = list_layout(assign, nlist)
    samp = np.nonzero((pos // S.TILE) % S.SAMPLE_STEP == 0)[0]
    assert len(samp) == 1024 and S.threshold_rank(k) == 174
    Kr = rng.integers(-5, 6, (nlist, d))
    Kr[:, 0] = [-10, 10]
    Cc = Kr.astype(np.float32)
    K = PR.list_codes(Cc, m_, s_, d)
    np.testing.assert_array_equal(K, Kr)
    book = rng.integers(-3, 4, (M, 256, dsub)).astype(np.int8)
    book[0, :128, 0] = rng.integers(-20, 21, 128)
    book[0, 128:, 0] = rng.integers(70, 118, 128)
    check_book(book, d)
    codes = rng.integers(0, 256, (N, M)).astype(np.uint8)
    codes[:, 0] = rng.integers(0, 128, N)
    codes[samp, 0] = rng.integers(128, 256, len(samp))
    dec = PR.decode(codes, book, K, assign)
    assert np.abs(dec).max() <= 127
    r, clamped = PR.residuals(dec.astype(np.int8), K, assign)
    assert clamped == 0
    np.testing.assert_array_equal(P.assign(r[:300], book)[0], codes[:300])
    X = dec.astype(np.float32)
    Q = rng.uniform(-0.01, 0.01, (nq, d)).astype(np.float32)
    Q[:, 0] = rng.uniform(0.5, 2.0, nq).astype(np.float32)
    ex = Expect(Q, dec, m_, s_)
    probes = S.probed_lists(Q, Cc, nlist)
    cap = S.threshold_cap(k, lens, nlist)
    thr = -np.partition(-ex.Sc[:, samp], 173, axis=1)[:, 173]
    cnt = (ex.Sc >= thr[:, None]).sum(axis=1)
    assert (cnt >= 174).all() and (cnt < k).all() and k <= cap and (cnt <= cap).all()   # deficit, never overflow
    state = S.ivf_thresholded_redo(ex.Sc, k, assign, probes, nlist)
    assert (state == S.REDO).all(), "inputs no longer reach the path"
    T = PR.pair_offsets(ex.n, K, np.tile(np.arange(nlist), (nq, 1)))
    wrong = ex.Sc - T[:, assign] + T[:, 1 - assign]               # every row scored with the other list's T
    assert ((wrong >= thr[:, None]).sum(axis=1) != cnt).all()    # T is in the compared score
    rows, sc = ex.top(k)
    return dict(N=N, d=d, dsub=dsub, nq=nq, k=k, nlist=nlist, assign=assign, Cc=Cc, K=K, book=book, codes=codes, dec=dec, X=X,
                m=m_, s=s_, Q=Q, ex=ex, rows=rows, sc=sc)


# ============================================ B3. refined search at dpad 128, dsub 16 ========================================
C3_N, C3_D, C3_DSUB, C3_NQ, C3_NLIST, C3_NPROBE, C3_K = 6000, 128, 16, 70, 8, 3, 10
C3_KSCAN_ALL = 4096       # a k_scan beyond every query's probed rows: stage 1 returns them all and every query is certified


def refine_case(res):
    """plain: codebooks trained by the restatement (n_iter 2).  Residual: random injected residual codebooks, so list code
    + entry leaves int8.  One reference per route: plain, with per-query predicates, with seen lists"""
    rng = np.random.default_rng(36300 + int(res))
    X, Q = R.unit_rows(51 + res, C3_N, C3_D), R.unit_rows(53 + res, C3_NQ, C3_D)
    Cc, assign = R.ivf_layout(55 + res, C3_N, C3_D, C3_NLIST)
    m_, s_ = S.train_quantizer(X)
    c = P.pad_codes(S.encode(X, m_, s_), 128)
    K = book = codes = None
    if res:
        K = PR.list_codes(Cc, m_, s_, 128)
        book = rng.integers(-127, 128, (C3_D // C3_DSUB, 256, C3_DSUB)).astype(np.int8)
        r, clamped = PR.residuals(c, K, assign)
        codes, _ = P.assign_blas(r, book)
        dec = PR.decode(codes, book, K, assign)
        assert dec.dtype == np.int16 and np.abs(dec).max() > 127      # genuinely 16-bit
    else:
        book, codes, _ = P.train_blas(c, C3_DSUB, 2)
        dec = P.decode(codes, book)
    probed = R.probe_mask(Q, Cc, assign, C3_NPROBE)
    assert probed.sum(axis=1).max() < C3_KSCAN_ALL
    tags = _tags(rng, C3_N)
    preds = np.array([[(0, 0, 0), (2, 0, 0), (0, 0x20, 0), (0, 0, 0x40)][i] for i in rng.integers(0, 4, C3_NQ)], dtype=np.uint32)
    ok = FR.passes(tags, preds)
    assert ok.mean(axis=1).min() > 0.3 and (ok & probed).sum(axis=1).min() > 2 * C3_K
    ex = Expect(Q, dec, m_, s_)
    top, _ = ex.top(100, probed)
    counts = np.array([0] * 20 + [5] * 25 + [40] * (C3_NQ - 45))
    seen = np.zeros((C3_NQ, C3_N), dtype=bool)
    for q in range(C3_NQ):
        seen[q, top[q, 0:2 * counts[q]:2]] = True
    ea = R.ranges(X, dec, m_, s_)
    refine = PR.refine if res else R.refine
    allowed = {"plain": probed, "filtered": probed & ok, "excluding": probed & ~seen}
    want = {name: refine(Q, X, dec, m_, s_, C3_K, 2 * C3_K, a, ea) for name, a in allowed.items()}
    assert all((w["rows"] >= 0).all() for w in want.values())
    assert (top >= 0).all() and (want["excluding"]["rows"] != want["plain"]["rows"]).any(axis=1)[20:].mean() > 0.8
    brute = {name: R.brute_force(Q, X, C3_K, allowed[name]) for name in ("filtered", "excluding")}
    users, rows = np.nonzero(seen)
    return dict(res=res, X=X, Q=Q, Cc=Cc, assign=assign, m=m_, s=s_, K=K, book=book, codes=codes, dec=dec, tags=tags, preds=preds,
                ea=ea, want=want, brute=brute, seen_pairs=(users, rows + ID0), ids=np.arange(C3_N, dtype=np.int64) + ID0)


# ============================================ C1. the trainer across workgroups =============================================
C1_N, C1_ITER, C1_NLIST = 5 * TRAIN_BLOCK + 37, 3, 9


def train_case(du, dsub):
    """10 277 clustered rows; nine ragged lists of which 3 and 4 (consecutive) and 8 (the last) are empty.  The
    restatement's results for a plain build (flat and IVF sources: the same) and for a residual build"""
    rng = np.random.default_rng(36400 + du + dsub)
    centres = 40
    Cc0 = rng.standard_normal((centres, du)).astype(np.float32)
    X = (Cc0[rng.integers(0, centres, C1_N)] + 0.15 * rng.standard_normal((C1_N, du))).astype(np.float32)
    X[:, 2] = -0.75                                              # a constant column: its codes are 0
    assign = rng.choice([0, 1, 2, 5, 6, 7], C1_N, p=[0.35, 0.05, 0.2, 0.25, 0.1, 0.05]).astype(np.int32)
    assign[11] = 1
    lens = np.bincount(assign, minlength=C1_NLIST)
    assert lens[3] == lens[4] == 0 and lens[8] == 0 and (lens[[0, 1, 2, 5, 6, 7]] > 0).all() and (lens % 64 != 0).sum() >= 5
    Cc = (0.1 * rng.standard_normal((C1_NLIST, du))).astype(np.float32)
    for l in range(C1_NLIST):
        if lens[l]:
            Cc[l] += X[assign == l].mean(axis=0)
    dpad = P.dpad_of(du)
    m_, s_ = S.train_quantizer(X)
    c = P.pad_codes(S.encode(X, m_, s_), dpad)
    K = PR.list_codes(Cc, m_, s_, dpad)
    plain = P.train_blas(c, dsub, C1_ITER)
    r, clamped = PR.residuals(c, K, assign)
    resid = P.train_blas(r, dsub, C1_ITER)
    assert plain[2][-1] < plain[2][0] and resid[2][-1] < resid[2][0]
    # the cross-workgroup half of the Lloyd step: rows of one entry in at least 3 blocks of 2 048 physical rows, in the flat
    # and in the IVF layout, and an entry with a negative column sum in several blocks
    _, phys, _ = list_layout(assign, C1_NLIST)
    first = P.assign_blas(c, P.init_book(c, dsub))[0]
    for where in (np.arange(C1_N), phys):
        blocks = where // TRAIN_BLOCK
        spread = max(len(np.unique(blocks[first[:, 0] == e])) for e in range(256))
        assert spread >= 3, "inputs no longer reach the path"
        neg = 0
        for e in np.unique(first[:, 0])[:64]:
            mine = first[:, 0] == e
            sums = np.array([c[mine & (blocks == bl), 0].astype(np.int64).sum() for bl in np.unique(blocks[mine])])
            neg += len(sums) >= 2 and (sums < 0).all()
        assert neg >= 1
    n_phys = int(((lens + S.GRANULE - 1) // S.GRANULE * S.GRANULE).sum())
    assert (n_phys + TRAIN_BLOCK - 1) // TRAIN_BLOCK == 6 == (C1_N + TRAIN_BLOCK - 1) // TRAIN_BLOCK   # six workgroups per sub-space
    return dict(du=du, dsub=dsub, X=X, Cc=Cc, assign=assign, m=m_, s=s_, c=c, K=K, plain=plain, resid=resid, clamped=clamped,
                dec=P.decode(plain[1], plain[0])[:, :du], dec16=PR.decode(resid[1], resid[0], K, assign)[:, :du])


# ============================================ C2. the update rule's edges ===================================================
E_N, E_D = 6400, 64       # entry e is seeded from row 25 e; 6 400 rows are 3 blocks of 2 048 and one of 256


def edges_case(dsub):
    """rows with few distinct values; codes given directly (ranges (0, 1)).  Every sub-space carries the same pattern in its
    first two columns.  Row types by column 0: 0 (most rows), {42, 43}, {83, 84}, {-42, -43}, {-83, -84}, each pair in equal
    numbers, so the means after the first Lloyd step are 42.5, 83.5, -42.5, -83.5 exactly.  Entries 1 .. 4 are seeded
    from rows 25 .. 100 with the values 42, 83, -42, -83; entry 5 is seeded from a row identical to entry 1's, so every row
    of that value ties between them, goes to entry 1, and entry 5 loses all its rows; entries 6 .. 255 are seeded from
    zero rows like entry 0 and lose theirs to it.  Column 1 is +3 in even blocks of 2 048 rows and -3 in odd ones"""
    rng = np.random.default_rng(36500 + dsub)
    M = E_D // dsub
    assert (np.arange(256) * E_N // 256 == 25 * np.arange(256)).all()
    a = np.zeros(E_N, dtype=np.int64)
    free = np.setdiff1d(np.arange(E_N), 25 * np.arange(256))
    pick = rng.permutation(free)
    n_each = 300
    vals = [(42, 43), (83, 84), (-42, -43), (-83, -84)]
    for i, (lo, hi) in enumerate(vals):
        mine = pick[2 * n_each * i:2 * n_each * (i + 1)]
        a[mine[:n_each]] = lo                                    # with the seed row below: n_each + 1 of lo ...
        a[mine[n_each:]] = hi
        a[25 * (i + 1)] = lo
        a[pick[8 * n_each + i]] = hi                             # ... and n_each + 1 of hi
    a[25 * 5] = 42                                               # entry 5's seed: identical to entry 1's
    a[pick[8 * n_each + 4]] = 43                                 # keeps 42 and 43 in equal numbers
    blocks = np.arange(E_N) // TRAIN_BLOCK
    col1 = np.where(blocks % 2 == 0, 3, -3)
    col1[25 * np.arange(256)] = 3                                # seeds alike in column 1 (entry 5 == entry 1, 6 .. == 0)
    c = np.zeros((E_N, E_D), dtype=np.int8)
    c[:, 0::dsub] = a[:, None]
    c[:, 1::dsub] = col1[:, None]
    book0 = P.init_book(c, dsub)
    assert (book0[0, 5] == book0[0, 1]).all() and (book0[0, 6:] == book0[0, 0]).all()      # entries seeded from identical rows
    codes, _ = P.assign(c, book0)
    for m in range(M):
        s, cnt = P.entry_sums(c, codes, m, dsub)
        assert cnt[5] == 0 and (cnt[6:] == 0).all() and cnt[:5].sum() == E_N               # the tie went to the lower entry
        mean = s[:5, 0] / cnt[:5]
        assert mean[1:].tolist() == [42.5, 83.5, -42.5, -83.5]                             # half-way: even and odd floors, both signs
        for e in (3, 4):                                         # negative in every contributing block, and in at least 3
            mine = codes[:, m] == e
            part = [int(c[mine & (blocks == bl), m * dsub].astype(np.int64).sum()) for bl in np.unique(blocks[mine])]
            assert len(part) >= 3 and max(part) < 0
        part1 = [int(c[(codes[:, m] == 0) & (blocks == bl), m * dsub + 1].astype(np.int64).sum()) for bl in range(4)]
        assert part1[0] > 0 > part1[1] and part1[2] > 0 > part1[3]                          # both signs meet in one u64 word
    step = P.lloyd_step(c, codes, book0)
    assert step[0, 1:5, 0].tolist() == [42, 84, -42, -84]        # 42.5 -> 42, 83.5 -> 84, -42.5 -> -42, -83.5 -> -84
    assert (step[0, 5] == book0[0, 5]).all() and (step[0, 6:] == book0[0, 6:]).all()       # an entry without rows keeps its value
    return dict(dsub=dsub, c=c, X=c.astype(np.float32), m=np.zeros(E_D, np.float32), s=np.ones(E_D, np.float32),
                want=P.train_blas(c, dsub, 1), step=step)
