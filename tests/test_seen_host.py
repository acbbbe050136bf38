"""CPU: the seen-item store (CSR construction) and the over-fetch plan of recommendit_amd/seen.py."""
import math
import subprocess
import sys

import numpy as np
import pytest

K_MAX = 16384


def test_module_imports_without_a_device():
    code = ("import torch; torch.cuda.is_available = lambda: False\n"
            "import recommendit_amd.seen as S\n"
            "from recommendit_amd import SeenItems\n"
            "s = SeenItems.from_pairs([1, 1, 0], [5, 3, 9])\n"
            "assert s.max_count == 2 and S.overfetch_k(500, 12, 10**6, 16384) == 512\n")
    subprocess.run([sys.executable, "-c", code], check=True)


def test_csr_duplicates_unsorted_and_empty_users():
    from recommendit_amd.seen import SeenItems
    users = [3, 1, 3, 3, 1, 6, 3]
    items = [9, 4, 2, 9, 4, 0, 7]
    s = SeenItems.from_pairs(users, items)
    assert s.n_users == 7
    assert s.counts.dtype == np.int32 and s.counts.tolist() == [0, 1, 0, 3, 0, 0, 1]
    assert s.max_count == 3
    assert s.items_of(3).tolist() == [2, 7, 9] and s.items_of(1).tolist() == [4] and s.items_of(0).tolist() == []
    assert s.items_of(6).tolist() == [0] and s.items_of(99).tolist() == []
    assert s.counts_of([3, 99, -1, 1, 0]).tolist() == [3, 0, 0, 1, 0]
    wide = SeenItems.from_pairs(users, items, n_users=10)
    assert wide.n_users == 10 and wide.counts[7:].tolist() == [0, 0, 0]
    empty = SeenItems.from_pairs([], [])
    assert empty.n_users == 0 and empty.max_count == 0 and empty.counts_of([0, 5]).tolist() == [0, 0]
    with pytest.raises(ValueError):
        SeenItems.from_pairs(users, items, n_users=3)


def test_csr_random_against_python_sets():
    from recommendit_amd.seen import SeenItems
    rng = np.random.RandomState(0)
    u = rng.randint(0, 50, 4000)
    i = rng.randint(0, 300, 4000)
    s = SeenItems.from_pairs(u, i, n_users=60)
    for user in range(60):
        assert s.items_of(user).tolist() == sorted(set(i[u == user].tolist()))
    assert s.counts.sum() == len(set(zip(u.tolist(), i.tolist())))


def test_from_dict_from_frame_and_updated():
    import pandas as pd
    from recommendit_amd.seen import SeenItems
    d = SeenItems.from_dict({2: [8, 1, 8], 0: [], 4: [3]})
    assert d.n_users == 5 and d.items_of(2).tolist() == [1, 8] and d.items_of(4).tolist() == [3]
    f = SeenItems.from_frame(pd.DataFrame({"user_id": [2, 2, 4, 2], "item_id": [8, 1, 3, 8], "rating": [5, 4, 3, 5]}))
    assert f.counts.tolist() == d.counts.tolist()
    g = SeenItems.from_frame(pd.DataFrame({"u": [1], "i": [7]}), user_col="u", item_col="i")
    assert g.items_of(1).tolist() == [7]
    up = d.updated([2, 7, 4], [5, 6, 3])
    assert up is not d and d.n_users == 5 and d.items_of(2).tolist() == [1, 8]          # the original is unchanged
    assert up.n_users == 8 and up.items_of(2).tolist() == [1, 5, 8] and up.items_of(7).tolist() == [6]
    assert up.items_of(4).tolist() == [3] and up.max_count == 3


def test_bad_ids_raise():
    from recommendit_amd.seen import SeenItems
    with pytest.raises(ValueError):
        SeenItems.from_pairs([0, -1], [1, 2])
    with pytest.raises(ValueError):
        SeenItems.from_pairs([0, 1], [1, -2])
    with pytest.raises(ValueError):
        SeenItems.from_pairs([0], [2 ** 31])
    assert SeenItems.from_pairs([0], [2 ** 31 - 1]).items_of(0).tolist() == [2 ** 31 - 1]
    with pytest.raises(ValueError):
        SeenItems.from_pairs([0, 1], [1])


def test_overfetch_k():
    from recommendit_amd.seen import overfetch_k
    big = 10 ** 6
    assert [overfetch_k(500, e, big, K_MAX) for e in (0, 12, 13, 1548, 1549)] == [500, 512, 1024, 2048, 4096]
    assert overfetch_k(500, 15884, big, K_MAX) == 16384
    assert overfetch_k(20, 0, 10, K_MAX) == 20                  # nothing excluded: k as it is
    assert overfetch_k(500, 100, 700, K_MAX) == 700             # clipped at the corpus
    assert overfetch_k(500, 100, 1024, K_MAX) == 1024
    assert overfetch_k(500, 30000, 9000, K_MAX) == 9000         # a small corpus is fetched whole, whatever the list
    assert overfetch_k(500, 15885, K_MAX, K_MAX) == K_MAX
    with pytest.raises(ValueError, match=r"15885.*16384"):
        overfetch_k(500, 15885, K_MAX + 1, K_MAX)
    for k in (1, 20, 500, 3000):
        for e in (1, 2, 63, 64, 1000, 5000):
            ke = overfetch_k(k, e, big, K_MAX)
            assert ke >= k + e and ke & (ke - 1) == 0 and ke < 2 * (k + e)


def _check_plan(plan, extra, k, ntotal):
    from recommendit_amd.seen import overfetch_k
    pos = np.concatenate([p for _, p in plan])
    assert sorted(pos.tolist()) == list(range(len(extra)))      # every query exactly once
    ks = [ke for ke, _ in plan]
    assert ks == sorted(set(ks))                                # ascending, one search per k_eff
    for ke, p in plan:
        assert p.tolist() == sorted(p.tolist())
        assert ke <= min(ntotal, K_MAX)
        for q in p:
            assert ke >= min(k + extra[q], ntotal) and ke >= overfetch_k(k, extra[q], ntotal, K_MAX)


def test_plan_overfetch_groups_and_merging():
    from recommendit_amd.seen import plan_overfetch
    big = 10 ** 6
    extra = np.array([0] * 10 + [5] * 3 + [100] * 6 + [2000])           # classes 500 x10, 512 x3, 1024 x6, 4096 x1
    plan = plan_overfetch(extra, 500, big, K_MAX, 1)
    assert [(ke, len(p)) for ke, p in plan] == [(500, 10), (512, 3), (1024, 6), (4096, 1)]
    _check_plan(plan, extra, 500, big)
    plan = plan_overfetch(extra, 500, big, K_MAX, 4)                    # 512 (3 < 4) joins 1024
    assert [(ke, len(p)) for ke, p in plan] == [(500, 10), (1024, 9), (4096, 1)]
    _check_plan(plan, extra, 500, big)
    plan = plan_overfetch(extra, 500, big, K_MAX, 11)                   # 500 + 512 -> 1024 (13 >= 11), 1024 -> 4096
    assert [(ke, len(p)) for ke, p in plan] == [(512, 13), (4096, 7)]
    _check_plan(plan, extra, 500, big)
    plan = plan_overfetch(extra, 500, big, K_MAX, math.inf)
    assert [(ke, len(p)) for ke, p in plan] == [(4096, 20)]
    plan = plan_overfetch(np.zeros(7, np.int64), 500, big, K_MAX, 64)
    assert [(ke, p.tolist()) for ke, p in plan] == [(500, list(range(7)))]
    assert plan_overfetch([], 500, big, K_MAX, 64) == []
    with pytest.raises(ValueError):
        plan_overfetch([0, 16000], 500, big, K_MAX, 1)


def test_plan_overfetch_random():
    from recommendit_amd import seen as S
    rng = np.random.RandomState(3)
    assert isinstance(S.MIN_GROUP, int) and S.MIN_GROUP >= 1
    for ntotal in (3000, 10 ** 6):
        for mg in (None, 1, 16, 300, math.inf):
            extra = np.minimum((rng.pareto(1.2, 500) * 80).astype(np.int64), 9000)
            extra[rng.rand(500) < 0.2] = 0
            plan = S.plan_overfetch(extra, 500, ntotal, K_MAX, mg)
            _check_plan(plan, extra, 500, ntotal)
            if mg is not None and mg != 1 and not math.isinf(mg):
                assert all(len(p) >= mg for _, p in plan[:-1])          # only the largest class may stay small
