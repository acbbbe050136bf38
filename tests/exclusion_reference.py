"""NumPy restatement of seen-item exclusion inside the index scan (exclusion="scan"; csrc/search_exclude.hip).  No device,
nothing from recommendit_amd.

The contract: for query q of user u the result is the first k rows, in the index's own order, among the rows the plain
search may return (flat: all rows; IVF: the rows of the probed lists) whose item id is not in seen[u] and that pass the
query's predicate; -1 / -inf behind the last one.  The candidate sets and the order are those of the existing references
(tests/search_reference.py for the f32 index: integer inputs, score descending, lower row first on ties); this module only
takes rows out of the candidate set.

The mask the device builds: bit p & 31 of word [q, p >> 5], W = ceil(Np / 32) words per query, is set iff the row at scan
position p is excluded for query q.  A flat index scans rows in row order (p = row, Np = N); an IVF index scans the
list-major physical order: lists ascending, rows ascending inside a list, every list padded to 64 positions."""
import numpy as np

TR = 64      # ip_index.h: list granule


def seen_lists(offsets, items, user_ids, nq):
    """the seen list of every query: row user_ids[q] of the CSR (None: row q); a user outside the store has none"""
    offsets = np.asarray(offsets, dtype=np.int64)
    items = np.asarray(items)
    n_users = offsets.shape[0] - 1
    out = []
    for q in range(nq):
        u = q if user_ids is None else int(user_ids[q])
        out.append(items[offsets[u]:offsets[u + 1]] if 0 <= u < n_users else items[:0])
    return out


def excluded_rows(lists, item_ids):
    """bool [nq, N]: row r is excluded for query q iff item_ids[r] is in lists[q]; ids that are not stored change nothing"""
    item_ids = np.asarray(item_ids, dtype=np.int64)
    out = np.zeros((len(lists), item_ids.shape[0]), dtype=bool)
    for q, l in enumerate(lists):
        out[q] = np.isin(item_ids, np.asarray(l, dtype=np.int64))
    return out


def allowed_rows(excluded, candidates=None, passing=None):
    """bool [nq, N]: the rows a query may return -- candidates (bool [nq, N], None: all) minus the excluded ones, AND the
    rows that pass its predicate (bool [nq, N] or [N], None: all)"""
    ok = ~np.asarray(excluded, dtype=bool)
    if candidates is not None:
        ok &= np.asarray(candidates, dtype=bool)
    if passing is not None:
        p = np.asarray(passing, dtype=bool)
        ok &= p if p.ndim == 2 else p[None, :]
    return ok


def first_k(order_key, allowed, k):
    """int64 [nq, k]: per query the k allowed rows with the smallest order_key (int64 [nq, N], unique per query: the
    index's own order as one number), ascending; -1 behind the last allowed row"""
    order_key = np.asarray(order_key, dtype=np.int64)
    nq, N = order_key.shape
    big = np.iinfo(np.int64).max
    key = np.where(allowed, order_key, big)
    if k < N:       # the k smallest first (the keys of allowed rows are unique), then their order
        part = np.argpartition(key, k - 1, axis=1)[:, :k]
        order = np.take_along_axis(part, np.argsort(np.take_along_axis(key, part, axis=1), axis=1, kind="stable"), axis=1)
    else:
        order = np.argsort(key, axis=1, kind="stable")
    got = np.take_along_axis(key, order, axis=1) < big
    rows = np.full((nq, k), -1, dtype=np.int64)
    rows[:, :order.shape[1]] = np.where(got, order, -1)
    return rows


def f32_order_key(S):
    """the f32 index's order over integer scores S int64 [nq, N]: score descending, lower row first"""
    S = np.asarray(S, dtype=np.int64)
    assert S.shape[1] < 2 ** 24 and np.abs(S).max() < 2 ** 30
    return (-S) * (1 << 24) + np.arange(S.shape[1], dtype=np.int64)[None, :]


def topk_excluding(S, k, allowed):
    """(scores f32 [nq, k], rows int64 [nq, k]) of integer scores S under `allowed`"""
    rows = first_k(f32_order_key(S), allowed, k)
    sc = np.where(rows >= 0, np.take_along_axis(np.asarray(S), np.maximum(rows, 0), axis=1).astype(np.float32),
                  np.float32(-np.inf)).astype(np.float32)
    return sc, rows


def ivf_positions(assign, nlist):
    """(pos int64 [N], Np): the list-major physical position of every row and the padded row count"""
    assign = np.asarray(assign, dtype=np.int64)
    lens = np.bincount(assign, minlength=nlist)
    padded = (lens + TR - 1) // TR * TR
    start = np.concatenate([[0], np.cumsum(padded)])
    order = np.argsort(assign, kind="stable")
    first = np.concatenate([[0], np.cumsum(lens)])
    pos = np.empty(assign.shape[0], dtype=np.int64)
    pos[order] = start[assign[order]] + (np.arange(assign.shape[0]) - first[assign[order]])
    return pos, int(max(start[-1], TR))


def mask_words(positions_per_query, Np):
    """uint32 [nq, ceil(Np / 32)]: bit p & 31 of word p >> 5 of row q set for every p of positions_per_query[q]"""
    W = (int(Np) + 31) // 32
    out = np.zeros((len(positions_per_query), W), dtype=np.uint32)
    for q, ps in enumerate(positions_per_query):
        ps = np.asarray(ps, dtype=np.int64).reshape(-1)
        assert ps.size == 0 or (ps.min() >= 0 and ps.max() < Np)
        np.bitwise_or.at(out[q], ps >> 5, (np.uint32(1) << (ps & 31).astype(np.uint32)))
    return out
