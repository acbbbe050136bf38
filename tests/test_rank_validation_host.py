"""CPU: the host parts of validation-while-training (recommendit_amd/validation.py) and the self-consistency of the
NumPy reference the GPU tests compare against (tests/rank_reference.py)."""
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import rank_reference as R  # noqa: E402
from recommendit_amd.validation import leave_last_out, report_keys, select_epoch  # noqa: E402


def _frame():
    # user 1: three liked ratings, the last two share a timestamp -> input position decides (item 6 is held out)
    # user 2: one liked rating -> left whole;  user 3: liked 9 then 8 (timestamps reversed against input order)
    # user 4: liked twice, then a late rating below the threshold, which is not a candidate
    rows = [(1, 7, 5, 10), (1, 5, 5, 30), (1, 6, 4, 30), (2, 5, 5, 1), (2, 6, 2, 2), (3, 8, 5, 9), (3, 9, 4, 2),
            (4, 1, 4, 1), (4, 2, 5, 2), (4, 3, 1, 99)]
    return pd.DataFrame(rows, columns=["user_id", "item_id", "rating", "timestamp"])


def test_leave_last_out_ties_threshold_and_train_rows():
    df = _frame()
    train, truth, users, seen = leave_last_out(df)
    assert users.tolist() == [1, 3, 4]
    held = {int(u): truth.host_items[truth.host_offsets[i]:truth.host_offsets[i + 1]].tolist()
            for i, u in enumerate(users)}
    assert held == {1: [6], 3: [8], 4: [2]}
    assert truth.host_raw.tolist() == [1, 1, 1]
    # no held-out row left in train, nothing else removed, input order kept
    pairs = set(zip(train["user_id"], train["item_id"]))
    assert not pairs & {(1, 6), (3, 8), (4, 2)}
    assert len(train) == len(df) - 3 and train.index.tolist() == sorted(train.index.tolist())
    assert set(zip(df["user_id"], df["item_id"])) - pairs == {(1, 6), (3, 8), (4, 2)}
    # user 2 is whole; the seen store is the train frame
    assert seen.items_of(2).tolist() == [5, 6] and seen.items_of(1).tolist() == [5, 7]
    assert seen.items_of(4).tolist() == [1, 3]


def test_leave_last_out_n_holdout_and_max_users():
    df = _frame()
    train, truth, users, _ = leave_last_out(df, n_holdout=2)
    assert users.tolist() == [1]           # only user 1 has three liked ratings
    assert sorted(truth.host_items.tolist()) == [5, 6] and len(train) == len(df) - 2
    rng = np.random.RandomState(1)
    n = 50
    big = pd.DataFrame({"user_id": np.repeat(np.arange(1, n + 1), 4), "item_id": rng.randint(1, 30, 4 * n),
                        "rating": 5, "timestamp": rng.randint(0, 100, 4 * n)})
    _, t1, u1, _ = leave_last_out(big, max_users=10, seed=3)
    _, t2, u2, _ = leave_last_out(big, max_users=10, seed=3)
    tr3, _, u3, _ = leave_last_out(big, max_users=10, seed=4)
    assert len(u1) == 10 and u1.tolist() == u2.tolist() and u1.tolist() != u3.tolist()
    assert u1.tolist() == sorted(u1.tolist()) and t1.n == 10 and len(tr3) == len(big) - 10
    with pytest.raises(ValueError):
        leave_last_out(df, n_holdout=0)


def test_select_epoch():
    assert select_epoch([], "max", 1) == (None, None)
    assert select_epoch([0.1, 0.3, 0.2], "max") == (1, None)
    assert select_epoch([0.3, 0.1, 0.2], "min") == (1, None)
    assert select_epoch([0.2, 0.3, 0.3, 0.1], "max") == (1, None)          # a tie goes to the earlier epoch
    assert select_epoch([5, 5, 5], "min") == (0, None)
    # patience: stop at the first index that is `patience` validations past the best; later values are never read
    assert select_epoch([0.1, 0.3, 0.2, 0.25, 0.9], "max", 2) == (1, 3)
    assert select_epoch([0.1, 0.3, 0.2, 0.25, 0.9], "max", 3) == (4, None)
    assert select_epoch([0.5, 0.4, 0.3], "max", 1) == (0, 1)
    assert select_epoch([0.5, 0.5, 0.6], "max", 1) == (0, 1)               # an equal value is no improvement
    assert select_epoch([3, 2, 2, 2], "min", 2) == (1, 3)
    assert select_epoch([float("nan"), 0.2, 0.1], "max", 2) == (1, None)   # NaN never improves
    assert select_epoch([float("nan")], "max", 1) == (None, 0)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            select_epoch([1], "max", bad)
    with pytest.raises(ValueError):
        select_epoch([1], "best")
    assert "recall@50" in report_keys((10, 50)) and "mrr" in report_keys((10,))


@pytest.mark.parametrize("seed", range(6))
def test_reference_rank_metrics_equal_list_metrics(seed):
    """small random cases with plenty of exact ties: the position of every target in the full stable list is its rank,
    and the two metric routes agree bit for bit"""
    rng = np.random.RandomState(seed)
    n_items = int(rng.randint(1, 40))
    c = R.case_inputs(rng, int(rng.randint(1, 30)), n_items, 16)
    c["U"] = np.round(c["U"] * 2) / 2          # coarser values: more ties
    c["Y"] = np.round(c["Y"] * 2) / 2
    excl = (c["excl_off"], c["excl_items"]) if seed % 3 else (None, None)
    rank, tscore, err = R.ranks(c["U"], c["Y"], c["pair_off"], c["pair_item"], *excl)
    assert err == 0 and (rank >= 0).all() and (rank < n_items).all()
    lists = R.full_lists(c["U"], c["Y"], *excl)
    off = c["pair_off"]
    for u in range(len(off) - 1):
        for p in range(off[u], off[u + 1]):
            t = c["pair_item"][p]
            if excl[0] is not None and t in c["excl_items"][excl[0][u]:excl[0][u + 1]]:
                continue                          # an excluded target is not in the list; its rank ignores that entry
            assert int(np.nonzero(lists[u] == t)[0][0]) == rank[p]
    # metrics: the list cannot express "an exclusion entry equal to the target is ignored", so take the targets out
    if excl[0] is not None:
        rows, e_off = [], [0]
        for u in range(len(off) - 1):
            t = set(c["pair_item"][off[u]:off[u + 1]].tolist())
            rows += [j for j in c["excl_items"][excl[0][u]:excl[0][u + 1]].tolist() if j not in t]
            e_off.append(len(rows))
        excl = (np.asarray(e_off, np.int64), np.asarray(rows, np.int32))
        rank, _, _ = R.ranks(c["U"], c["Y"], off, c["pair_item"], *excl)
        lists = R.full_lists(c["U"], c["Y"], *excl)
    raw = np.diff(off)
    ks = [1, 3, 10]
    a = R.metrics_from_ranks(rank, off, raw, ks)
    b = R.metrics_from_lists(lists, off, c["pair_item"], raw, ks)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a[2].sum() == (raw > 0).sum() and (a[1][raw > 0] > 0).all()
