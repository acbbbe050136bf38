"""NumPy restatement of the inner-product index search: which path the driver takes (csrc/topk.hip: search_pass,
flat_thresholded, ivf_geom, ivf_thresholded, pick_nsplit, bf16_nsplit; launch_finalize in csrc/select.hip) and what a
search must return.  No device, nothing from recommendit_amd.

Exactness: the tests hold every input as a small integer in float32, |x| <= 8.  Every product (<= 64) and every partial
sum (<= 64 * 128) of an inner product is then an integer far below 2^24: exact in bf16 operands, in f32 accumulation and
in any summation order, so the expected scores are the integer matmul and the comparison is bitwise."""
import math

import numpy as np

# ---- the driver's constants, named once (tests/test_search_host.py compares them with the sources) ---------------------
QB = 128              # search_kernels.h: queries per workgroup of the f32 scan
QBB = 256             # ... of the bf16 scans
SAMPLE = 16384        # rows of the threshold sample (twice that for the two-precision search)
SAMPLE_T = 8          # scores a register top-T stream keeps
WQE = 192             # scan_bf16.hip: entries of a wave's survivor queue in the bf16 filter
CSTRIDE = 32
TRB = 64              # rows per stage of the bf16 scans
TRS = 32              # ip_index.h: rows per tile of the f32 scans
TR = 64               # list granule
K_MAX = 16384         # key slots of finalize's dynamic LDS
NLIST_MAX = 2048
RIHIP_NCU = 256       # common.h
IVF_SS = 16           # topk.hip: the IVF sample takes every 16th tile of a probed list
IVF_TARGET = 16 * RIHIP_NCU
PASS_QUERIES = 4096   # topk.hip CH: queries per internal pass
FLAT_REDO_CHUNK = 8   # topk.hip flat_redo FCH
IVF_REDO_CHUNK = 64   # topk.hip ivf_redo FCH
REFINE_LDS_SLOTS = 2048   # topk.hip r.lds_slots: survivors refine_kernel holds in LDS
FUSED_K_MAX = 2048    # topk.hip: the fused refine serves k <= 2048
IVF_SMALL_PREPARE = 8     # topk.hip ivf_prepare: one launch up to 8 queries
IVF_DENSE_ROWS = 16384    # search_pass: probed population that stays unfiltered
IVF_DENSE_SLOTS = 1 << 23  # search_pass: dense slots of a batch that stay unfiltered
# the slots of rihip_ip_index_search_stats, in order (recommendit_hip.h)
STATS = ("flat_dense", "flat_f32", "flat_fused", "flat_unfused", "ivf_unfiltered", "ivf_thresholded", "sample_top",
         "prepare_small", "thr_queries", "redone", "redo_chunks", "passes")


def _cdiv(a, b):
    return (a + b - 1) // b


def kernel_width(du):
    return 32 if du <= 32 else (64 if du <= 64 else 128)


def passes(nq):
    """queries of each internal pass of one search call"""
    return [min(PASS_QUERIES, nq - q0) for q0 in range(0, nq, PASS_QUERIES)]


def redo_chunks(n_fail, ivf):
    ch = IVF_REDO_CHUNK if ivf else FLAT_REDO_CHUNK
    return [min(ch, n_fail - f0) for f0 in range(0, n_fail, ch)]


def pick_nsplit(nq, n_tiles):
    qblocks = _cdiv(nq, QB)
    return min(max(1, min(_cdiv(2 * RIHIP_NCU, qblocks), n_tiles)), 65535)


def bf16_nsplit(nq, tiles, wgs_per_cu):
    qblocks = _cdiv(nq, QBB)
    return min(max(1, min(_cdiv(wgs_per_cu * RIHIP_NCU, qblocks), tiles)), 65535)


def finalize_in_lds(n_launch, cap, k, mode):
    """launch_finalize: the key list is copied to LDS for small launches whose list fits behind the sort buffer"""
    P = 0
    if mode == 0:
        P = 64
        while P < k:
            P *= 2
    return n_launch <= 2 * RIHIP_NCU and cap > 0 and P + cap <= K_MAX


def _split(n_rows, tile, nsplit):
    """(tiles, tiles per split, splits that hold rows, tiles of the last used split, rows of the last tile)"""
    tiles = _cdiv(n_rows, tile)
    per = _cdiv(tiles, nsplit)
    used = _cdiv(tiles, per)
    return dict(tiles=tiles, per=per, used=used, last_split_tiles=tiles - (used - 1) * per,
                last_tile_rows=n_rows - (tiles - 1) * tile, nsplit=nsplit)


def ivf_geometry(list_lens, nprobe):
    ll = sorted((int(x) for x in list_lens), reverse=True)
    nlist = len(ll)
    assert nlist <= NLIST_MAX
    cap_full = max(1, sum(ll[:nprobe]))
    npr = min(nprobe, nlist)
    max_tiles = max(_cdiv(l, TR) * (TR // TRS) for l in ll)
    cap_lf = max(max_tiles * TRS, TRS)
    return dict(nlist=nlist, nprobe=npr, cap_full=cap_full, max_tiles=max_tiles, cap_lf=cap_lf, cap_df=cap_lf * npr)


def plan(N, d, nq, k, two_precision=True, filtered=False, list_lens=None, nprobe=None):
    """What ONE internal pass (nq <= 4 096 queries) of a search does.  d is the kernel width (it changes no decision
    and is kept for the record).  list_lens given: an IVF index."""
    assert 1 <= nq <= PASS_QUERIES and 1 <= k <= K_MAX
    p = dict(N=N, d=d, nq=nq, k=k)
    if list_lens is not None:
        g = ivf_geometry(list_lens, nprobe)
        p.update(g)
        unf = (g["cap_full"] <= IVF_DENSE_ROWS or k * 4.0 > g["cap_full"] / IVF_SS
               or nq * g["cap_df"] <= IVF_DENSE_SLOTS)
        p["prepare"] = "small" if nq <= IVF_SMALL_PREPARE else "four"
        if unf:
            p["route"] = "ivf_unfiltered"
            p["fin_pairs_lds"] = finalize_in_lds(nq * g["nprobe"], g["cap_lf"], k, 0)
            p["fin_lds"] = finalize_in_lds(nq, g["nprobe"] * k, k, 0)
            return p
        p["route"] = "ivf_thresholded"
        m = k / IVF_SS
        rank = int(math.ceil(m + 4.0 * math.sqrt(m) + 4.0))
        cap = 4096
        while cap < 2.5 * rank * IVF_SS:
            cap *= 2
        cap = min(cap, g["cap_full"])
        cap_l = _cdiv(g["max_tiles"], IVF_SS) * TRS
        p.update(rank=rank, cap=cap, cap_l=cap_l, cap_s=cap_l * g["nprobe"], tile_step=IVF_SS)
        p["fin_thr_lds"] = finalize_in_lds(nq, p["cap_s"], k, 1)
        p["fin_lds"] = finalize_in_lds(nq, cap, k, 0)
        return p
    if N <= 4 * SAMPLE:
        p["route"] = "flat_dense"
        p["scan"] = _split(N, TRS, pick_nsplit(nq, _cdiv(N, TRS)))
        p["fin_lds"] = finalize_in_lds(nq, N, k, 0)
        return p
    two = bool(two_precision) and not filtered
    n_sample = SAMPLE * (2 if two else 1)
    stride = N // n_sample if N // n_sample > 0 else 1
    S = _cdiv(N, stride)
    m = float(k) * float(S) / float(N)
    rank = int(math.ceil((m + 4.0 * math.sqrt(m) + 4.0) * (1.5 if two else 1.0)))
    expect = float(rank) * float(N) / float(S)
    cap = 4096
    while cap < 2.5 * expect:
        cap *= 2
    cap = min(cap, N)
    tile = TRB if two else TRS
    filter_tiles, sample_tiles = _cdiv(N, tile), _cdiv(S, tile)
    seg_cap = 64
    if two:
        while seg_cap < 4.0 * expect / bf16_nsplit(nq, filter_tiles, 3):
            seg_cap *= 2
        seg_cap = min(seg_cap, cap)
    streams = 2 * bf16_nsplit(nq, sample_tiles, 2)
    sample_top = two and rank * 4 <= streams * SAMPLE_T
    cap_s = streams * SAMPLE_T if sample_top else S
    ns_sample = bf16_nsplit(nq, sample_tiles, 2) if two else pick_nsplit(nq, sample_tiles)
    ns_filter = bf16_nsplit(nq, filter_tiles, 3) if two else pick_nsplit(nq, filter_tiles)
    p.update(route="flat_f32" if not two else ("flat_fused" if k <= FUSED_K_MAX else "flat_unfused"),
             two_precision=two, fused=two and k <= FUSED_K_MAX, stride=stride, S=S, rank=rank, cap=cap, seg_cap=seg_cap,
             sample_top=sample_top, cap_s=cap_s, sample=_split(S, tile, ns_sample), filter=_split(N, tile, ns_filter))
    p["fin_thr_lds"] = finalize_in_lds(nq, cap_s, k, 1)
    if not p["fused"]:
        p["fin_lds"] = finalize_in_lds(nq, cap, k, 0)
        if two:
            p["fin_kth_lds"] = finalize_in_lds(nq, cap, k, 1)
    return p


def expected_stats(N, d, nq, k, two_precision=True, filtered=False, list_lens=None, nprobe=None):
    """the search_stats delta of one search call, without the re-dos: {name: count} of the non-zero slots"""
    out = dict.fromkeys(STATS, 0)
    for n in passes(nq):
        p = plan(N, d, n, k, two_precision, filtered, list_lens, nprobe)
        out[p["route"]] += 1
        out["passes"] += 1
        if p.get("sample_top"):
            out["sample_top"] += 1
        if p.get("prepare") == "small":
            out["prepare_small"] += 1
        if p["route"] not in ("flat_dense", "ivf_unfiltered"):
            out["thr_queries"] += n
    return out


def redo_stats(n_fail_per_pass, ivf):
    """what re-doing that many failed queries of each internal pass adds: (redone, redo_chunks, prepare_small)"""
    redone = chunks = small = 0
    for nf in n_fail_per_pass:
        redone += nf
        for c in redo_chunks(nf, ivf):
            chunks += 1
            small += int(ivf and c <= IVF_SMALL_PREPARE)
    return redone, chunks, small


# ---- exact scores, top-k ----------------------------------------------------------------------------------------------
def check_exact_inputs(*arrays):
    for a in arrays:
        a = np.asarray(a)
        assert a.dtype == np.float32 and (a == np.rint(a)).all() and np.abs(a).max() <= 8


def int_scores(Q, X):
    """int64 [nq, N]: exact inner products of small-integer inputs, through a float64 matmul"""
    out = np.asarray(Q, dtype=np.float64) @ np.asarray(X, dtype=np.float64).T
    r = np.rint(out)
    assert (r == out).all() and np.abs(r).max() < 2 ** 23
    return r.astype(np.int64)


def topk(S, k, allowed=None):
    """(scores f32 [nq, k], rows int64 [nq, k]): score descending, then row ascending; -inf / -1 behind the last row.
    allowed bool [nq, N] restricts a query to some rows"""
    nq, N = S.shape
    assert N < 2 ** 24
    kk = min(k, N)
    big = np.int64(2 ** 62)
    key = (-S) * (1 << 24) + np.arange(N, dtype=np.int64)[None, :]
    if allowed is not None:
        key = np.where(allowed, key, big)
    if kk < N:
        key = np.partition(key, kk - 1, axis=1)[:, :kk]
    key = np.sort(key, axis=1)
    ok = key < big
    r = np.where(ok, key & ((1 << 24) - 1), -1)
    s = np.where(ok, np.take_along_axis(S, np.maximum(r, 0), axis=1).astype(np.float32), np.float32(-np.inf))
    rows = np.full((nq, k), -1, dtype=np.int64)
    sc = np.full((nq, k), -np.inf, dtype=np.float32)
    rows[:, :kk], sc[:, :kk] = r, s
    return sc, rows


def topk_chunked(Q, X, k, allowed=None, chunk=256):
    """topk(int_scores(Q, X), k) without the whole score matrix; allowed: f(q0, q1) -> bool [q1 - q0, N] or None"""
    nq = Q.shape[0]
    sc = np.empty((nq, k), dtype=np.float32)
    rows = np.empty((nq, k), dtype=np.int64)
    for q0 in range(0, nq, chunk):
        q1 = min(nq, q0 + chunk)
        sc[q0:q1], rows[q0:q1] = topk(int_scores(Q[q0:q1], X), k, None if allowed is None else allowed(q0, q1))
    return sc, rows


def probed_lists(Q, C, nprobe):
    """int64 [nq, nprobe]: lists by coarse score descending, ties to the lower list id (ivf_select_kernel: `v > best ||
    (v == best && c < bi)`); the coarse scores of integer inputs are exact"""
    cs = int_scores(Q, C)
    ids = np.arange(cs.shape[1], dtype=np.int64)
    key = np.sort((-cs) * (1 << 24) + ids[None, :], axis=1)[:, :nprobe]
    return key & ((1 << 24) - 1)


def allowed_by_lists(probes, assign, nlist):
    """bool [nq, N]: the rows of the lists each query probes"""
    on = np.zeros((probes.shape[0], nlist), dtype=bool)
    np.put_along_axis(on, probes, True, axis=1)
    return on[:, np.asarray(assign)]


def pred_pass(tags, pred):
    """bool [N]: rows whose tag word passes (any_of, all_of, none_of) (search_keys.h Pred::pass)"""
    t = np.asarray(tags, dtype=np.uint32)
    a, b, c = (np.uint32(x) for x in pred)
    return ((a == 0) | ((t & a) != 0)) & ((t & b) == b) & ((t & c) == 0)


# ---- verdicts of a thresholded pass -----------------------------------------------------------------------------------
REDO, KEPT, EITHER = 1, 0, -1
NEG = -(2 ** 40)      # stands for -inf among integer scores


def _interval(samp, rank, n_slots):
    """(a, b): the threshold finalize (mode 1) hands on lies in (b, a].  samp: the real sampled scores; the list it
    selects from has n_slots >= len(samp) slots, the others hold key 0 (below every score).  a = the rank-th best
    sampled score; the select stops its radix passes as soon as exactly the keys it needs remain in the chosen bucket
    and returns the prefix, so any value down to just above the next key's score is possible -- b = the (rank+1)-th
    best score, or a itself when the two tie (the passes then run on into the row bits: the score is exact).  None: no
    threshold (fewer than rank real sampled scores: every row is a candidate)."""
    if len(samp) < rank or n_slots < rank:
        return None
    top = -np.sort(-np.asarray(samp))[:rank + 1]
    a = int(top[rank - 1])
    b = int(top[rank]) if len(top) > rank else NEG
    return a, b


def _verdict(over_hi, over_lo, under_hi, under_lo):
    """over_*: fails that get likelier as the threshold falls (overflow), at the upper / lower end of its interval;
    under_*: fails that get likelier as it rises (deficit, proof)"""
    if over_hi or under_lo:
        return REDO
    if not over_lo and not under_hi:
        return KEPT
    return EITHER


def eps_scale(X):
    """the driver's bound of the bf16 filter's error per unit of |q| (flat_thresholded), in f64"""
    max_norm = math.sqrt(float((np.asarray(X, dtype=np.float64) ** 2).sum(axis=1).max()))
    return (1.0 / 256.0 + 1.0 / 262144.0) * max_norm * 1.001


def top_t_kept(s, p, level):
    """(fewest, most) sampled scores >= level that survive a register top-T sample pass of the score row s: a stream
    (corpus split x row half) keeps its SAMPLE_T best, so of the c such scores a split holds its two streams keep
    between min(c, SAMPLE_T) and min(c, 2 SAMPLE_T), whatever the halves are; also the largest c of any split"""
    samp = np.asarray(s)[np.arange(p["S"], dtype=np.int64) * p["stride"]]
    split_of = np.arange(p["S"]) // (p["sample"]["per"] * TRB)
    c = np.bincount(split_of[samp >= level], minlength=1)
    return int(np.minimum(c, SAMPLE_T).sum()), int(np.minimum(c, 2 * SAMPLE_T).sum()), int(c.max())


def flat_verdicts(Sc, p, qnorm=None, eps=0.0, inv=None):
    """int8 [nq]: REDO / KEPT / EITHER of every query of one flat thresholded pass.  Sc int64 [u, N]: the score rows,
    query q's is Sc[inv[q]] (inv None: one row per query); p = plan(...) of the pass.  Two-precision: qnorm f64 [u],
    eps = eps_scale(X); the approximate scores equal the exact ones for the tests' inputs.
    Causes of a re-do: fewer than min(k, N) candidates, more than cap, a (query, split) segment over seg_cap, the proof
    s_k >= thr + eps |q| + 2e-6 failing -- and, in the bf16 filter, the survivor queue of a wave (64 consecutive queries
    of a 256-query block share WQE entries, emptied when a stage ends with WQE - 64 or more in any of the block's four
    queues) running over: the queries whose entries did not fit are re-done.  Which entries those are depends on the
    order inside a stage, which this reference does not restate: every query of the wave with a survivor in such a stage
    is EITHER.  The proof is evaluated in f64 with a margin of 1e-3 relative either way (the kernel evaluates it in f32):
    inside the margin the verdict is EITHER."""
    n_u, N = Sc.shape
    inv = np.arange(n_u) if inv is None else np.asarray(inv)
    nq = len(inv)
    k, cap, rank, two = p["k"], p["cap"], p["rank"], p["two_precision"]
    samp_rows = np.arange(p["S"], dtype=np.int64) * p["stride"]
    need = min(k, N)
    parts = np.zeros((n_u, 4), dtype=bool)                     # over_hi, over_lo, under_hi, under_lo
    if two:
        rows_per_split = p["filter"]["per"] * TRB
        split_of = np.arange(N) // rows_per_split
        s_split_of = np.arange(p["S"]) // (p["sample"]["per"] * TRB)
        n_stage = p["filter"]["tiles"]
        per_stage = np.zeros((n_u, n_stage), dtype=np.int64)   # survivors of every 64-row stage at the lowest threshold
    for u in range(n_u):
        s = Sc[u]
        iv = _interval(s[samp_rows], rank, p["cap_s"])
        assert iv is not None
        a, b = iv
        if p["sample_top"]:
            # a stream (split, row half) keeps its 8 best: while no SPLIT holds more than 8 sampled scores >= b the
            # union holds the sample's best rank + 1 and the interval stands; otherwise the threshold may be lower
            # (never higher) by an amount this reference does not model: the lower end opens
            if b > NEG and np.bincount(s_split_of[s[samp_rows] >= b], minlength=1).max() > SAMPLE_T:
                b = NEG

        def fails(t_cnt, t_proof):
            c = s >= t_cnt
            n = int(c.sum())
            over = n > cap
            if two and not over:
                over = bool(np.bincount(split_of[c], minlength=1).max() > p["seg_cap"])
            under_sure = under_maybe = n < need
            if two and not under_sure and not over and n >= k:
                sk = float(-np.partition(-s[c], k - 1)[k - 1])
                bound = t_proof + eps * qnorm[u] + 2e-6
                tol = 1e-3 * (1.0 + abs(bound))
                under_sure, under_maybe = sk < bound - tol, sk < bound + tol
            return over, under_sure, under_maybe
        over_hi, under_lo, under_hi = fails(a, a)
        over_lo, t_lo = over_hi, a
        if b != a:
            t_lo = b + 1
            over_lo, under_lo, _ = fails(t_lo, b)
        parts[u] = over_hi, over_lo, under_hi, under_lo
        if two:
            c = np.nonzero(s >= t_lo)[0]
            per_stage[u] = np.bincount(c // TRB, minlength=n_stage)
            if t_lo <= 0:                                      # the zero rows behind the corpus in the last stage
                per_stage[u, -1] += n_stage * TRB - N
    queue = np.zeros(nq, dtype=bool)
    if two:
        per = p["filter"]["per"]
        for q0 in range(0, nq, QBB):
            waves = [inv[w0:min(w0 + 64, nq, q0 + QBB)] for w0 in range(q0, min(q0 + QBB, nq), 64)]
            E = np.stack([per_stage[w].sum(axis=0) for w in waves])          # [waves, stages]
            carry = np.zeros(len(waves), dtype=np.int64)
            for st in range(n_stage):
                tot = carry + E[:, st]
                for wi in np.nonzero(tot > WQE)[0]:
                    w0 = q0 + 64 * wi
                    queue[w0:w0 + len(waves[wi])] |= per_stage[waves[wi], st] > 0
                last = (st + 1) % per == 0 or st + 1 == n_stage
                carry = np.zeros_like(carry) if last or tot.max() >= WQE - 64 else tot
    out = np.empty(nq, dtype=np.int8)
    for q in range(nq):
        over_hi, over_lo, under_hi, under_lo = parts[inv[q]]
        out[q] = _verdict(over_hi, over_lo or queue[q], under_hi, under_lo)
    return out


def ivf_sampled_positions(length):
    """positions inside a list of `length` rows that the threshold sample scores: every IVF_SS-th 32-row tile"""
    pos = np.arange(int(length))
    return pos[(pos // TRS) % IVF_SS == 0]


def ivf_verdicts(Sc, p, assign, probes, nlist):
    """flat_verdicts for one thresholded IVF pass: assign int [N] (rows ascend inside a list), probes int [nq, nprobe].
    A query with fewer than rank sampled rows has no threshold: every probed row is a candidate, and the query fails
    only by overflow.  Under a real threshold fewer than k candidates fail (ivf_thr in finalize)."""
    nq = Sc.shape[0]
    k, cap, rank = p["k"], p["cap"], p["rank"]
    rows_of = [np.nonzero(np.asarray(assign) == l)[0] for l in range(nlist)]
    samp_of = [r[ivf_sampled_positions(len(r))] for r in rows_of]
    out = np.empty(nq, dtype=np.int8)
    for q in range(nq):
        probed = np.concatenate([rows_of[l] for l in probes[q]])
        samp = np.concatenate([samp_of[l] for l in probes[q]])
        s = Sc[q, probed]
        iv = _interval(Sc[q, samp], rank, p["cap_s"])
        if iv is None:
            out[q] = REDO if len(s) > cap else KEPT
            continue
        a, b = iv
        n_hi = int((s >= a).sum())
        n_lo = n_hi if b == a else int((s >= b + 1).sum())
        out[q] = _verdict(n_hi > cap, n_lo > cap, n_hi < k, n_lo < k)
    return out


def filtered_verdict(scores_pass, samp_pass, p, n_slots):
    """one query of a FILTERED thresholded pass (flat all-f32 or IVF): scores_pass = the scores of the rows that pass its
    predicate (IVF: of its probed lists), samp_pass = those of them the sample visits.  All passing rows within cap, or
    fewer than rank sampled ones: no threshold.  The query fails with more than cap candidates or fewer than
    min(k, passing rows)"""
    k, cap, rank = p["k"], p["cap"], p["rank"]
    scores_pass = np.asarray(scores_pass)
    n_pass = len(scores_pass)
    need = min(n_pass, k)
    iv = None if n_pass <= cap else _interval(samp_pass, rank, n_slots)
    if iv is None:
        return REDO if n_pass > cap else KEPT
    a, b = iv
    n_hi = int((scores_pass >= a).sum())
    n_lo = n_hi if b == a else int((scores_pass >= b + 1).sum())
    return _verdict(n_hi > cap, n_lo > cap, n_hi < need, n_lo < need)


def redo_bounds(state):
    """(fewest, most) queries a thresholded pass may re-do"""
    state = np.asarray(state)
    return int((state == REDO).sum()), int((state != KEPT).sum())
