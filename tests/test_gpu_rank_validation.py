"""Validation by exact full-catalogue ranks (csrc/rank_eval.hip, recommendit_amd/validation.py) against the NumPy
restatement of its contract in tests/rank_reference.py.

* exact inputs (entries k/8, k in -8..8: every product is a multiple of 1/64 and every partial sum up to d = 256 is
  exact in f32 in any order, so the f64 reference is exact and ties are plentiful): rank and target score bit for bit;
* split independence and repeatability: identical bytes;
* random unit rows: a competitor whose row is bytewise equal to the target's must be decided by index; any other one is
  decided when its f64 score differs from the target's by more than tau = 2 d 2^-24 (twice the f32 dot-product error
  bound d 2^-24 |u| |y| on unit rows); lo <= rank <= lo + undecided;
* the list path it replaces (exact search with exclusion over the whole catalogue + evaluate_topk_device): same
  means, bitwise equal per-user arrays, each target's list position equal to its rank;
* the error word; the trainer's validation arguments."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import rank_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (33, 127), (129, 129), (300, 385)]


def run(c, excl=True, grid_splits=0):
    """-> (rank, target_score, err) as NumPy"""
    import torch
    from recommendit_amd.validation import rank_targets_device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rank, score, err = rank_targets_device(up(c["U"]), up(c["Y"]), (up(c["pair_off"]), up(c["pair_item"])),
                                           (up(c["excl_off"]), up(c["excl_items"])) if excl else None,
                                           grid_splits=grid_splits)
    return rank.cpu().numpy(), score.cpu().numpy(), int(err.item())


_CASES = {}


def exact_case(n_pairs, n_items, d):
    key = (n_pairs, n_items, d)
    if key not in _CASES:
        c = R.case_inputs(np.random.RandomState(1000 * d + n_pairs), n_pairs, n_items, d)
        c["ref"] = R.ranks(c["U"], c["Y"], c["pair_off"], c["pair_item"], c["excl_off"], c["excl_items"])
        c["ref_plain"] = R.ranks(c["U"], c["Y"], c["pair_off"], c["pair_item"])
        _CASES[key] = c
    return _CASES[key]


@pytest.mark.parametrize("d", [16, 48, 64, 128, 256])
@pytest.mark.parametrize("n_pairs,n_items", SHAPES)
def test_exact_inputs_bit_for_bit(n_pairs, n_items, d):
    c = exact_case(n_pairs, n_items, d)
    for excl, ref in ((True, c["ref"]), (False, c["ref_plain"])):
        rank, score, err = run(c, excl)
        assert err == 0 and ref[2] == 0
        assert np.array_equal(rank.astype(np.int64), ref[0]), (np.nonzero(rank != ref[0])[0][:8], rank[:8], ref[0][:8])
        assert np.array_equal(score.astype(np.float64), ref[1])
    # the exclusion rows that hold every other item give rank 0 (and the case has some)
    off, first = c["pair_off"], []
    for u in range(len(off) - 1):
        if u % 4 == 2 and off[u + 1] > off[u]:
            first.append(off[u])
    if n_pairs >= 33:
        assert first
    assert (c["ref"][0][first] == 0).all()


def test_split_independence_and_repeatability():
    c = exact_case(300, 385, 64)
    base = run(c, True, 1)
    assert np.array_equal(base[0].astype(np.int64), c["ref"][0])
    for splits in (1, 2, 3, 0, 4, 7):
        got = run(c, True, splits)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes() and got[2] == base[2]


@pytest.mark.parametrize("n_pairs,n_items,d", [(300, 385, 16), (300, 385, 64), (129, 257, 128)])
def test_random_inputs_self_consistency_and_interval(n_pairs, n_items, d):
    rng = np.random.RandomState(0)
    c = R.case_inputs(rng, n_pairs, n_items, d, exact=False)
    # 16 item rows copied onto 16 other rows, targets among both
    rows = rng.permutation(n_items)[:32]
    src, dst = rows[:16], rows[16:]
    c["Y"][dst] = c["Y"][src]
    off = c["pair_off"]
    singles = [u for u in range(len(off) - 1) if off[u + 1] - off[u] == 1][:32]
    for u, r in zip(singles, np.concatenate([src, dst])):
        c["pair_item"][off[u]] = r
    tau = 2.0 * d * 2.0 ** -24
    lo, und = R.rank_interval(c["U"], c["Y"], off, c["pair_item"], c["excl_off"], c["excl_items"], tau)
    share = float((und > 0).mean())
    print(f"d={d}: {100 * share:.1f} % of the pairs have an undecided competitor")
    assert share <= 0.10
    rank, score, err = run(c)
    assert err == 0
    bad = np.nonzero((rank < lo) | (rank > lo + und))[0]
    assert bad.size == 0, (bad[:8], rank[bad[:8]], lo[bad[:8]], und[bad[:8]])
    p_users = np.repeat(np.arange(len(off) - 1), np.diff(off))
    assert np.abs(score - R.scores64(c["U"], c["Y"])[p_users, c["pair_item"]]).max() <= tau / 2


def test_against_the_list_path():
    """exact inputs, small catalogue: the full exact list with exclusion + evaluate_topk_device"""
    import torch
    from recommendit_amd import FAISSIndex
    from recommendit_amd.eval_device import GroundTruth, evaluate_topk_device
    from recommendit_amd.seen import SeenItems
    from recommendit_amd.validation import RankValidator
    n_items, d, ks = 200, 32, [1, 5, 10, 50]
    c = R.case_inputs(np.random.RandomState(5), 90, n_items, d)
    off, n_users = c["pair_off"], len(c["pair_off"]) - 1
    # the list cannot express "an exclusion entry equal to the target is ignored": take the targets out of the rows
    e_users = np.repeat(np.arange(n_users), np.diff(c["excl_off"]))
    p_users = np.repeat(np.arange(n_users), np.diff(off))
    tset = set(zip(p_users.tolist(), c["pair_item"].tolist()))
    keep = np.array([(u, j) not in tset for u, j in zip(e_users.tolist(), c["excl_items"].tolist())], bool)
    seen = SeenItems.from_pairs(e_users[keep], c["excl_items"][keep], n_users)
    truth = GroundTruth.from_pairs(np.arange(n_users), p_users, c["pair_item"])     # item id = row
    U, Y = torch.from_numpy(c["U"]).cuda(), torch.from_numpy(c["Y"]).cuda()
    index = FAISSIndex(embed_dim=d, exact=True)
    index.build_from_device(Y, np.arange(n_items, dtype=np.int64))
    _, ids = index.batch_search_device(U, k=n_items, normalized=True, exclude=seen, user_ids=np.arange(n_users))
    assert ids.shape == (n_users, n_items)
    want = evaluate_topk_device(ids, truth, ks, per_user=True)
    val = RankValidator(None, np.arange(n_items), np.zeros((n_items, 1), np.float32), truth, np.arange(n_users), seen, ks)
    val.enqueue(U, Y)
    got = val.per_user()
    out = val.out.cpu().numpy()
    for j, k in enumerate(ks):
        assert out[3 * j] == want[f"ndcg@{k}"] and out[3 * j + 1] == want[f"recall@{k}"]
        assert out[3 * j + 2] == want[f"precision@{k}"]
    assert out[3 * len(ks)] == want["mrr"] and want["mrr"] > 0
    for name in ("vals", "mrr", "scored"):
        assert torch.equal(got[name], want["per_user"][name]), name
    assert int(got["err"].item()) == 0
    # each target's position in its list
    ids_h, rank = ids.cpu().numpy(), got["rank"].cpu().numpy()
    t_off = truth.offsets.cpu().numpy()
    t_items = truth.items.cpu().numpy()
    for u in range(n_users):
        for p in range(t_off[u], t_off[u + 1]):
            assert int(np.nonzero(ids_h[u] == t_items[p])[0][0]) == rank[p]
    # and the reference's own two routes
    ref_rank, _, _ = R.ranks(c["U"], c["Y"], t_off, t_items.astype(np.int32), seen._offsets, seen._items)
    assert np.array_equal(rank.astype(np.int64), ref_rank)
    rv = R.metrics_from_ranks(ref_rank, t_off, np.diff(t_off), ks)
    assert np.array_equal(got["vals"].cpu().numpy(), rv[0]) and np.array_equal(got["mrr"].cpu().numpy(), rv[1])


def test_error_word():
    c = dict(exact_case(129, 129, 64))
    base = run(c)
    n_items = 129
    # an exclusion entry at n_items and one at -1: bit 0, every rank unchanged (rows stay ascending)
    off, items = c["excl_off"].copy(), c["excl_items"]
    u_lo = next(u for u in range(len(off) - 1) if u % 4 == 0 and c["pair_off"][u + 1] > c["pair_off"][u])
    u_hi = next(u for u in range(len(off) - 1) if u % 4 == 1)
    new_items, new_off = [], [0]
    for u in range(len(off) - 1):
        row = items[off[u]:off[u + 1]].tolist()
        if u == u_lo:
            row = [-1] + row
        if u == u_hi:
            row = row + [n_items]
        new_items += row
        new_off.append(len(new_items))
    bad = dict(c, excl_off=np.asarray(new_off, np.int64), excl_items=np.asarray(new_items, np.int32))
    rank, score, err = run(bad)
    assert err == 1 and rank.tobytes() == base[0].tobytes() and score.tobytes() == base[1].tobytes()
    assert R.ranks(bad["U"], bad["Y"], bad["pair_off"], bad["pair_item"], bad["excl_off"], bad["excl_items"])[2] == 1
    # a target at n_items: bit 1, rank -1, score 0; the other pairs unchanged
    pi = c["pair_item"].copy()
    pi[5] = n_items
    pi[77] = -3
    rank, score, err = run(dict(c, pair_item=pi))
    assert err == 2 and rank[5] == -1 and rank[77] == -1 and score[5] == 0 and score[77] == 0
    ok = np.ones(len(pi), bool)
    ok[[5, 77]] = False
    assert np.array_equal(rank[ok], base[0][ok]) and np.array_equal(score[ok], base[1][ok])
    rank, _, err = run(dict(bad, pair_item=pi))
    assert err == 3 and np.array_equal(rank[ok], base[0][ok])


def test_argument_errors_and_empty():
    import torch
    from recommendit_amd import _lib as L
    lib = L.lib()
    assert lib.rihip_rank_targets_workspace_bytes(10, 0, 40) == -1 and lib.rihip_rank_targets_workspace_bytes(1 << 31, 0, 64) == -1
    assert lib.rihip_rank_targets_workspace_bytes(10, 5, 64) > 0
    err = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    z = torch.zeros(64, dtype=torch.float32, device="cuda")
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    args = lambda d, n_pairs, e: (z.data_ptr(), 1, z.data_ptr(), 1, d, off.data_ptr(), None, n_pairs, None, None, 0,  # noqa: E731
                                  0, None, None, e, None, 0, L.stream_ptr())
    assert lib.rihip_rank_targets(*args(64, 0, err.data_ptr())) == 0      # no pairs: err zeroed, nothing launched
    assert int(err.item()) == 0
    assert lib.rihip_rank_targets(*args(40, 0, err.data_ptr())) == 1      # bad d
    assert b"embed_dim" in lib.rihip_last_error()
    assert lib.rihip_rank_targets(*args(64, 1, err.data_ptr())) == 1      # null pointers with pairs
    assert lib.rihip_rank_targets(*args(64, 0, None)) == 1
    assert lib.rihip_rank_targets(*args(64, 1 << 31, err.data_ptr())) == 1
    torch.cuda.synchronize()


# ---- trainer -------------------------------------------------------------------------------------------------------
def _tiny_frames():
    import pandas as pd
    rng = np.random.RandomState(3)
    n_users, n_items = 64, 96
    taste = rng.randint(0, 4, n_users)
    rows = []
    for u in range(n_users):
        liked = rng.permutation(np.arange(taste[u], n_items, 4))[:10]
        other = rng.permutation(n_items)[:6]
        for t, i in enumerate(liked):
            rows.append((u + 1, int(i) + 1, 5, 100 + t))
        for t, i in enumerate(other):
            rows.append((u + 1, int(i) + 1, 2, 50 + t))
    ratings = pd.DataFrame(rows, columns=["user_id", "item_id", "rating", "timestamp"]).drop_duplicates(
        ["user_id", "item_id"]).reset_index(drop=True)
    genres = ["Action", "Comedy", "Drama", "Horror"]
    movies = pd.DataFrame({"item_id": np.arange(1, n_items + 1), "title": [f"M{i} (1990)" for i in range(n_items)],
                           "genres": [genres[i % 4] for i in range(n_items)]})
    return ratings, movies


def _trainer(tmp_path, **kw):
    from recommendit_amd.train_embeddings import EmbeddingTrainer
    return EmbeddingTrainer(model_output_path=str(tmp_path / "m.pt"), embed_dim=16, epochs=3, batch_size=128,
                            dropout=0.1, seed=1, **kw)


def test_trainer_validation_history_and_checkpoint(tmp_path):
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.train_embeddings import build_item_genre_dict
    from recommendit_amd.validation import RankValidator, leave_last_out
    ratings, movies = _tiny_frames()
    tr = _trainer(tmp_path, validation="last", val_k=(10, 50), select_by="recall@10", learning_rate=1e-2)
    tr.train(ratings, movies)
    assert len(tr.history) == 3
    for row in tr.history:
        for key in ("val_recall@10", "val_recall@50", "val_ndcg@10", "val_ndcg@50", "val_mrr", "val_seconds"):
            assert key in row, key
        assert 0.0 <= row["val_recall@10"] <= row["val_recall@50"] <= 1.0
    vals = [r["val_recall@10"] for r in tr.history]
    best = int(np.argmax(vals))           # argmax: the first of equal values
    assert [bool(r.get("val_best")) for r in tr.history][best]
    # the checkpoint on disk is the best validation's model
    _, truth, users, seen = leave_last_out(ratings)
    item_ids = sorted(movies["item_id"].tolist())
    gd = build_item_genre_dict(movies)
    gm = np.stack([gd[i] for i in item_ids])
    model = TwoTowerModel.load(str(tmp_path / "m.pt"))
    rep = RankValidator(model, item_ids, gm, truth, users, seen, (10, 50)).evaluate()
    for key in ("recall@10", "recall@50", "ndcg@10", "ndcg@50", "mrr", "median_rank"):
        assert rep[key] == tr.history[best][f"val_{key}"], key
    assert rep["n_users"] == len(users) == 64 and rep["n_scored"] == 64 and not model.training


def test_trainer_patience_stub_and_no_validator(tmp_path, monkeypatch):
    from recommendit_amd import validation as V
    from recommendit_amd.train_embeddings import EmbeddingTrainer
    ratings, movies = _tiny_frames()
    seq = [0.5, 0.4, 0.3, 0.9]
    calls = []

    def fake(self):
        calls.append(1)
        v = seq[len(calls) - 1]
        return {"recall@10": v, "ndcg@10": v, "precision@10": v, "mrr": v, "median_rank": 1.0, "n_users": 1}

    monkeypatch.setattr(V.RankValidator, "evaluate", fake)
    tr = EmbeddingTrainer(model_output_path=str(tmp_path / "p.pt"), embed_dim=16, epochs=4, batch_size=128, seed=1,
                          validation="last", val_k=(10,), select_by="recall@10", patience=1)
    tr.train(ratings, movies)
    best, stop = V.select_epoch(seq, "max", 1)
    assert (best, stop) == (0, 1) and len(tr.history) == stop + 1 and len(calls) == stop + 1
    assert tr.history[0].get("val_best") and not tr.history[1].get("val_best")
    # validation=None: nothing is constructed, no val_ keys
    monkeypatch.setattr(V.RankValidator, "__init__", lambda *a, **k: (_ for _ in ()).throw(AssertionError("constructed")))
    tr = EmbeddingTrainer(model_output_path=str(tmp_path / "n.pt"), embed_dim=16, epochs=1, batch_size=128, seed=1)
    tr.train(ratings, movies)
    assert len(tr.history) == 1 and not any(k.startswith("val_") for k in tr.history[0])
    for kw in (dict(select_by="recall@10"), dict(patience=2), dict(validation="last", select_by="recall@7"),
               dict(validation="last", patience=2), dict(validation="first")):
        with pytest.raises(ValueError):
            EmbeddingTrainer(**kw)
