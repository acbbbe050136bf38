"""In-batch sampled softmax: what the two sweeps cost and what the loss retrieves (HIP events, mean of --reps after
--warmup).

--launch   rihip_inbatch_softmax_user_sweep / _item_sweep (logq and ids given) at B = 8192, d = 64 and at B = 65536,
           d = 128 and 144.  Beside them, same run and same shape: at d = 144 the runtime-width BPR sweeps
           (rihip_inbatch_sweep, the same two GEMMs per tile: like for like), at d = 128 the tuned two-sweep BPR (what a
           tuned softmax instantiation would buy).  Neither ratio is a gate.
--quality  hold-out recall@50 on ml1m_like() after --epochs epochs, the protocol of tools/coldstart_bench.py (80 / 20
           split of every user's liked items, top 50 of the trained row with the training items excluded, exact index):
           in-batch BPR, softmax without logQ, with logQ, with logQ and masking, and the popularity list.  One run each.

python tools/softmax_bench.py [--launch] [--quality] [--reps 20] [--warmup 3] [--epochs 3] [--users 2000]
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
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--users", type=int, default=2000)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
g = torch.Generator(device=dev)
g.manual_seed(7)
out = {}


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps


def unit(n, d):
    x = torch.randn((n, d), device=dev, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


if args.launch:
    lib, st = L.lib(), L.stream_ptr()
    f32 = dict(dtype=torch.float32, device=dev)
    for B, d in ((8192, 64), (65536, 128), (65536, 144)):
        U, Y = unit(B, d), unit(B, d)
        ids = torch.randint(1, max(2, B // 4), (B,), device=dev, generator=g)       # Zipf-free but duplicate-rich ids
        cnt = torch.bincount(ids, minlength=B).float()
        logq = torch.log(cnt[ids] / B).contiguous()
        dU, dI, lse = torch.empty((B, d), **f32), torch.empty((B, d), **f32), torch.empty((B,), **f32)
        part = torch.zeros((max(1024, lib.rihip_inbatch_workspace_doubles(B)),), dtype=torch.float64, device=dev)
        it = 20.0

        def sm_user():
            L.check(lib.rihip_inbatch_softmax_user_sweep(U.data_ptr(), B, 0, Y.data_ptr(), B, 0, d, it, logq.data_ptr(),
                                                         ids.data_ptr(), ids.data_ptr(), B, dU.data_ptr(), lse.data_ptr(),
                                                         part.data_ptr(), st))

        def sm_item():
            L.check(lib.rihip_inbatch_softmax_item_sweep(Y.data_ptr(), B, 0, U.data_ptr(), B, 0, d, it, logq.data_ptr(),
                                                         ids.data_ptr(), ids.data_ptr(), lse.data_ptr(), B, dI.data_ptr(), st))
        pos, r = torch.empty((B,), **f32), torch.empty((B,), **f32)
        ws = torch.empty((max(lib.rihip_inbatch_workspace_floats(B, B, d), 1),), **f32)
        L.check(lib.rihip_rowdot(U.data_ptr(), Y.data_ptr(), B, 0, d, pos.data_ptr(), st))

        def bpr_user():
            L.check(lib.rihip_inbatch_sweep(1, U.data_ptr(), B, 0, Y.data_ptr(), B, 0, d, pos.data_ptr(), None, B,
                                            dU.data_ptr(), r.data_ptr(), part.data_ptr(), ws.data_ptr(), 0, st))

        def bpr_item():
            L.check(lib.rihip_inbatch_sweep(0, Y.data_ptr(), B, 0, U.data_ptr(), B, 0, d, pos.data_ptr(), r.data_ptr(), B,
                                            dI.data_ptr(), None, None, ws.data_ptr(), 0, st))
        row = {"softmax_user_ms": timed(sm_user), "softmax_item_ms": timed(sm_item)}
        if B == 65536:      # d = 144: runtime-width BPR (like for like); d = 128: the tuned two-sweep BPR
            row["bpr_user_ms"], row["bpr_item_ms"] = timed(bpr_user), timed(bpr_item)
            row["bpr_kind"] = "runtime-width" if d == 144 else "tuned"
            row["ratio_user"] = row["softmax_user_ms"] / row["bpr_user_ms"]
            row["ratio_item"] = row["softmax_item_ms"] / row["bpr_item_ms"]
            row["ratio_pair"] = (row["softmax_user_ms"] + row["softmax_item_ms"]) / (row["bpr_user_ms"] + row["bpr_item_ms"])
        row["softmax_tflops_pair"] = 8.0 * B * B * d / ((row["softmax_user_ms"] + row["softmax_item_ms"]) * 1e-3) / 1e12
        out[f"launch B={B} d={d}"] = row
        print(f"[softmax] B={B} d={d}: " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}"
                                                      for k, v in row.items()), flush=True)

if args.quality:
    from recommendit_amd import FAISSIndex
    from recommendit_amd import synthetic as GB
    from recommendit_amd.coldstart import UserHistories
    from recommendit_amd.train_embeddings import EmbeddingTrainer, build_item_genre_dict
    ratings, movies, gm = GB.ml1m_like()
    rng = np.random.RandomState(1)
    liked = (ratings["rating"] >= 4).to_numpy()
    held = liked & (rng.rand(len(ratings)) < 0.2)
    train, test = ratings[~held], ratings[held]
    item_ids = np.asarray(sorted(movies["item_id"].unique().tolist()), dtype=np.int64)
    gd = build_item_genre_dict(movies)
    n_users = int(ratings["user_id"].max())
    users = rng.permutation(np.intersect1d(train["user_id"].unique(), test["user_id"].unique()))[:args.users]
    slot_of = np.full(n_users + 1, -1, np.int64)
    slot_of[users] = np.arange(users.size)
    sub = train[slot_of[train["user_id"].to_numpy()] >= 0]
    hist = UserHistories.from_pairs(slot_of[sub["user_id"].to_numpy()], sub["item_id"].to_numpy(), sub["rating"].to_numpy(),
                                    n=users.size)
    truth = [set() for _ in users]
    for u, it_ in zip(test["user_id"].to_numpy(), test["item_id"].to_numpy()):
        if slot_of[u] >= 0:
            truth[slot_of[u]].add(int(it_))

    def recall(ids):
        return float(np.mean([len(truth[s] & set(ids[s].tolist())) / len(truth[s]) for s in range(users.size)]))

    res = {"users": int(users.size), "epochs": args.epochs}
    arms = {"in-batch BPR": dict(loss_mode="inbatch"),
            "softmax, no logQ": dict(loss_mode="softmax", logq_correction=False, mask_duplicates=False),
            "softmax + logQ": dict(loss_mode="softmax", logq_correction=True, mask_duplicates=False),
            "softmax + logQ + mask": dict(loss_mode="softmax", logq_correction=True, mask_duplicates=True)}
    for name, kw in arms.items():
        with tempfile.TemporaryDirectory() as td:
            tr = EmbeddingTrainer(model_output_path=os.path.join(td, "m.pt"), epochs=args.epochs, seed=0, **kw)
            model = tr.train(train, movies)
        E = model.get_item_embeddings(item_ids.tolist(), np.stack([gd[i] for i in item_ids.tolist()]))
        index = FAISSIndex(embed_dim=E.shape[1], exact=True)
        index.build_ivf_index(E, item_ids.tolist())
        _, ids = index.batch_search_device(model.get_user_embeddings(users.tolist(), as_tensor=True), k=50, normalized=True,
                                           exclude=hist.as_seen(), user_ids=list(range(users.size)))
        res[name] = recall(ids.cpu().numpy())
        res[name + " final loss"] = tr.history[-1]["loss"]
        print(f"[softmax] {name}: recall@50 {res[name]:.4f}, final loss {tr.history[-1]['loss']:.4f}", flush=True)
    pop = train.groupby("item_id").size().sort_values(ascending=False, kind="stable").index.to_numpy()
    res["popularity"] = recall(np.stack([pop[~np.isin(pop, hist.history_of(s)[0])][:50] for s in range(users.size)]))
    out["quality"] = res
    print("[softmax] hold-out recall@50 (ml1m_like, exact index, one run each): " +
          ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in res.items()), flush=True)
print(json.dumps(out))
