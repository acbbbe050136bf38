"""Validation by exact full-catalogue ranks: what RankValidator.evaluate() costs stage by stage, what the list path it
replaces costs on the same inputs, and the per-epoch validation curve of every loss_mode (HIP events, mean of --reps
after --warmup).  Nothing here is a gate.

--launch   shapes: ML-1M (6 040 pairs x 3 706 items, d = 64) and 65 536 pairs x 1 000 000 items at d = 128, one pair per
           user, exclusion lists of ML-1M's shape (log-normal lengths, mean ~165, longest ~2 300).  Stages: the towers
           (RankValidator.embed), rihip_rank_targets without exclusion (target scores + count sweep), with exclusion
           (+ the exclusion entries' scores + the correction; the difference is reported), the metrics
           (rihip_eval_ranks + rihip_eval_reduce), and the whole evaluate().  rihip_rank_targets is one call of three
           launches: its kernels are not timed apart here.
           Beside them, same run and same inputs: the list path -- exact batch_search_device(k = 50, exclude=) +
           evaluate_topk_device (queries in --list-batch chunks) -- and rihip_inbatch_hard_select (m = 8) at the square
           shape of equal product count, with both sweeps' rates in products per second.
--quality  one ml1m_like() run per objective with validation="last": the per-epoch validation curve.

python tools/validation_bench.py [--launch] [--quality] [--reps 5] [--warmup 2] [--epochs 3] [--small-only]
"""
import argparse
import json
import os
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from recommendit_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launch", action="store_true")
ap.add_argument("--quality", action="store_true")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--small-only", action="store_true", help="--launch: the ML-1M shape only")
ap.add_argument("--list-batch", type=int, default=8192)
ap.add_argument("--arms", default="sampled,sampled4,inbatch,softmax,hard,mixed")
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
out = {}


def timed(fn, reps=None, warmup=None):
    reps, warmup = reps or args.reps, args.warmup if warmup is None else warmup
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def launch_shape(name, n_users, n_items, d, heavy):
    from recommendit_amd import FAISSIndex, TwoTowerModel
    from recommendit_amd.eval_device import GroundTruth, evaluate_topk_device
    from recommendit_amd.seen import SeenItems
    from recommendit_amd.validation import RankValidator, rank_targets_device
    rng = np.random.RandomState(0)
    reps = 2 if heavy else args.reps
    warm = 1 if heavy else args.warmup
    torch.manual_seed(0)
    model = TwoTowerModel(n_users, n_items, embed_dim=d, hidden_dim=128, dropout=0.1).to(dev)
    item_ids = np.arange(1, n_items + 1, dtype=np.int64)
    users = np.arange(1, n_users + 1, dtype=np.int64)
    gm = (rng.rand(n_items, 18) < 0.2).astype(np.float32)
    lens = np.clip(np.exp(rng.normal(4.6, 1.0, n_users)), 20, min(2314, n_items // 2)).astype(np.int64)
    su = np.repeat(users, lens)
    si = rng.randint(1, n_items + 1, su.shape[0])
    seen = SeenItems.from_pairs(su, si, n_users + 1)
    target = rng.randint(1, n_items + 1, n_users)
    truth = GroundTruth.from_pairs(users, users, target)
    val = RankValidator(model, item_ids, gm, truth, users, seen, (10, 50))
    n_excl = int(val.excl[1].shape[0])
    row = {"pairs": val.n_pairs, "items": n_items, "d": d, "excluded_entries": n_excl}
    row["towers_ms"] = timed(val.embed, reps, warm)
    U, Y = val.embed()
    pairs = (val.pair_offsets, val.pair_rows)
    row["rank_no_excl_ms"] = timed(lambda: rank_targets_device(U, Y, pairs, None), reps, warm)
    row["rank_with_excl_ms"] = timed(lambda: rank_targets_device(U, Y, pairs, val.excl), reps, warm)
    row["excl_scores_and_correction_ms"] = row["rank_with_excl_ms"] - row["rank_no_excl_ms"]
    val.enqueue(U, Y)
    lib, st, nk = L.lib(), L.stream_ptr(), len(val.uniq)

    def metrics():
        L.check(lib.rihip_eval_ranks(val.rank.data_ptr(), val.pair_offsets.data_ptr(), val.n, val.n_pairs,
                                     val.truth.raw.data_ptr(), val._karr, nk, val.disc.data_ptr(), val.idcg.data_ptr(),
                                     val.disc.shape[0], val.vals.data_ptr(), val.rr.data_ptr(), val.scored.data_ptr(), st))
        L.check(lib.rihip_eval_reduce(val.n, nk, val.vals.data_ptr(), val.rr.data_ptr(), None, val.scored.data_ptr(), None,
                                      0, 0, None, val.partials.data_ptr(), None, val.out.data_ptr(), st))
    row["metrics_ms"] = timed(metrics, reps, warm)
    row["evaluate_ms"] = timed(val.evaluate, reps, warm)
    rep = val.evaluate()
    products = float(val.n_pairs) * n_items
    row["sweep_Gproducts_per_s"] = products / (row["rank_no_excl_ms"] * 1e-3) / 1e9
    print(f"[validation] {name}: " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()),
          flush=True)

    # ---- the list path on the same inputs: exact search with exclusion at k = 50, then the list metrics
    index = FAISSIndex(embed_dim=d, exact=True)
    Yn = Y / torch.clamp(torch.linalg.norm(Y, dim=1, keepdim=True), min=1e-8)
    index.build_from_device(Yn.contiguous(), item_ids)
    Un = (U / torch.clamp(torch.linalg.norm(U, dim=1, keepdim=True), min=1e-8)).contiguous()
    lb = args.list_batch

    last = {}

    def list_path():
        res = []
        for s in range(0, n_users, lb):
            _, ids = index.batch_search_device(Un[s:s + lb], k=50, normalized=True, exclude=seen,
                                               user_ids=users[s:s + lb])
            res.append(ids)
        ids = torch.cat(res, 0) if len(res) > 1 else res[0]
        last["rep"] = evaluate_topk_device(ids, truth, (10, 50))
    try:
        row["list_path_ms"] = timed(list_path, 1 if heavy else reps, 1 if heavy else warm)
        lrep = last["rep"]
        row["list_over_rank"] = row["list_path_ms"] / (row["rank_with_excl_ms"] + row["metrics_ms"])
        row["recall@50 rank / list"] = [rep["recall@50"], lrep["recall@50"]]
    except (ValueError, RuntimeError) as e:      # e.g. k + |seen| over the search's candidate limit
        row["list_path_ms"] = f"failed: {e}"
    del index

    # ---- the parent's select sweep at the square shape of equal product count
    B = int(round(np.sqrt(products) / 128.0)) * 128
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    A = torch.randn((B, d), device=dev, generator=g)
    A = (A / A.norm(dim=1, keepdim=True)).contiguous()
    Bm = torch.randn((B, d), device=dev, generator=g)
    Bm = (Bm / Bm.norm(dim=1, keepdim=True)).contiguous()
    m = 8
    neg_idx = torch.empty((B, m), dtype=torch.int32, device=dev)
    neg_score = torch.empty((B, m), dtype=torch.float32, device=dev)
    pos_score = torch.empty((B,), dtype=torch.float32, device=dev)

    def select():
        L.check(lib.rihip_inbatch_hard_select(A.data_ptr(), B, 0, Bm.data_ptr(), B, 0, d, m, 0, None, None,
                                              neg_idx.data_ptr(), neg_score.data_ptr(), pos_score.data_ptr(), st))
    row["hard_select_B"] = B
    row["hard_select_ms"] = timed(select, reps, warm)
    row["select_Gproducts_per_s"] = float(B) * B / (row["hard_select_ms"] * 1e-3) / 1e9
    row["sweep_over_select_per_product"] = row["select_Gproducts_per_s"] / row["sweep_Gproducts_per_s"]
    out[name] = row
    print(f"[validation] {name} (all): " + json.dumps(row), flush=True)


if args.launch:
    launch_shape("ml1m 6040x3706 d=64", 6040, 3706, 64, heavy=False)
    if not args.small_only:
        launch_shape("65536x1M d=128", 65536, 1_000_000, 128, heavy=True)

if args.quality:
    from recommendit_amd import synthetic as GB
    from recommendit_amd.train_embeddings import EmbeddingTrainer
    ratings, movies, _ = GB.ml1m_like()
    arms = {"sampled": dict(loss_mode="sampled"), "sampled4": dict(loss_mode="sampled", n_negatives=4),
            "inbatch": dict(loss_mode="inbatch"), "softmax": dict(loss_mode="softmax"), "hard": dict(loss_mode="hard"),
            "mixed": dict(loss_mode="mixed")}
    res = {"epochs": args.epochs}
    for name in args.arms.split(","):
        with tempfile.TemporaryDirectory() as td:
            tr = EmbeddingTrainer(model_output_path=os.path.join(td, "m.pt"), epochs=args.epochs, seed=0,
                                  validation="last", val_k=(10, 50), **arms[name])
            tr.train(ratings, movies)
        res[name] = [{k: (round(v, 5) if isinstance(v, float) else v) for k, v in r.items()
                      if k in ("epoch", "loss", "seconds", "val_recall@10", "val_recall@50", "val_ndcg@10", "val_mrr",
                               "val_median_rank", "val_seconds")} for r in tr.history]
        for r in res[name]:
            print(f"[validation] {name}: " + ", ".join(f"{k} {v}" for k, v in r.items()), flush=True)
    out["quality"] = res
print(json.dumps(out))
