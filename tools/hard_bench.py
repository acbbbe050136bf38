"""In-batch hard-negative BPR: what the select sweep, the gradient entry and the whole step cost, and what the loss
retrieves (HIP events, mean of --reps after --warmup).  Nothing here is a gate.

--launch   rihip_inbatch_hard_select and rihip_inbatch_hard_grads (ids given, m = 8) and a whole
           HipBPRTrainer(loss_mode="hard") step at B in {8192, 65536}, d in {64, 128}.  Beside them, same run and same
           shape: rihip_inbatch_softmax_user_sweep (the yardstick: the select sweep performs one of its two products and
           no exponentials) and a whole loss_mode="inbatch" step.  The mixed objective: rihip_inbatch_gmat_mine on the
           weights a user pass left (its rate = the bytes of the blocks it must read, 4 B^2, over its time),
           rihip_inbatch_mixed_apply, and a whole loss_mode="mixed" step, to be held against inbatch step + select sweep
           + gradient entry, which is what the autograd sum of the two losses costs.
--quality  hold-out recall@50 on ml1m_like() after --epochs epochs, the protocol of tools/coldstart_bench.py (80 / 20
           split of every user's liked items, top 50 of the trained row with the training items excluded, exact index):
           in-batch BPR, in-batch softmax, hard negatives, the mixed objective at hard_weight 0.1 / 0.5 / 1.0, and the
           popularity list.  One run each, unpinned.

python tools/hard_bench.py [--launch] [--quality] [--reps 20] [--warmup 3] [--epochs 3] [--users 2000] [--n-hard 8]
                          [--arms inbatch,softmax,hard,mixed0.1,mixed0.5,mixed1.0] [--hard-weight 0.1]
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
ap.add_argument("--n-hard", type=int, default=8)
ap.add_argument("--hard-weight", type=float, default=0.1, help="--launch: weight of the mixed step and of apply")
ap.add_argument("--arms", default="inbatch,softmax,hard,mixed0.1,mixed0.5,mixed1.0", help="--quality: which losses to train")
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


def step_ms(mode, B, d, n_rows=200000):
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    torch.manual_seed(1)
    model = TwoTowerModel(n_rows, n_rows, embed_dim=d, hidden_dim=128, dropout=0.1)
    model.train()
    kw = dict(n_hard=args.n_hard) if mode in ("hard", "mixed") else {}
    if mode == "mixed":
        kw["hard_weight"] = args.hard_weight
    tr = HipBPRTrainer(model, B, lr=1e-3, weight_decay=1e-5, loss_mode=mode, table_opt="sparse", seed=0, **kw)
    batches = []
    for _ in range(4):
        it = torch.randint(1, n_rows + 1, (B,), device=dev, generator=g)
        batches.append((torch.randint(1, n_rows + 1, (B,), device=dev, generator=g), it,
                        (torch.rand((B, 18), device=dev, generator=g) < 0.2).float()))
    k = [0]

    def step():
        tr.step(*batches[k[0] % 4])
        k[0] += 1
    ms = timed(step)
    tr.check_errors()
    return ms


if args.launch:
    lib, st = L.lib(), L.stream_ptr()
    f32 = dict(dtype=torch.float32, device=dev)
    m = args.n_hard
    for B in (8192, 65536):
        for d in (64, 128):
            U, Y = unit(B, d), unit(B, d)
            ids = torch.randint(1, max(2, B // 4), (B,), device=dev, generator=g)       # duplicate-rich ids
            cnt = torch.bincount(ids, minlength=B).float()
            logq = torch.log(cnt[ids] / B).contiguous()
            dU, dI, lse = torch.empty((B, d), **f32), torch.empty((B, d), **f32), torch.empty((B,), **f32)
            part = torch.zeros((max(1024, lib.rihip_inbatch_workspace_doubles(B)),), dtype=torch.float64, device=dev)
            neg_idx = torch.empty((B, m), dtype=torch.int32, device=dev)
            neg_score, pos_score = torch.empty((B, m), **f32), torch.empty((B,), **f32)
            ws = torch.empty((lib.rihip_inbatch_hard_workspace_bytes(B, B, m),), dtype=torch.uint8, device=dev)

            def select():
                L.check(lib.rihip_inbatch_hard_select(U.data_ptr(), B, 0, Y.data_ptr(), B, 0, d, m, 0, ids.data_ptr(),
                                                      ids.data_ptr(), neg_idx.data_ptr(), neg_score.data_ptr(),
                                                      pos_score.data_ptr(), st))

            def grads():
                L.check(lib.rihip_inbatch_hard_grads(U.data_ptr(), B, 0, Y.data_ptr(), B, 0, d, m, neg_idx.data_ptr(),
                                                     neg_score.data_ptr(), pos_score.data_ptr(), B, dU.data_ptr(),
                                                     dI.data_ptr(), part.data_ptr(), ws.data_ptr(), st))

            def sm_user():
                L.check(lib.rihip_inbatch_softmax_user_sweep(U.data_ptr(), B, 0, Y.data_ptr(), B, 0, d, 20.0, logq.data_ptr(),
                                                             ids.data_ptr(), ids.data_ptr(), B, dU.data_ptr(), lse.data_ptr(),
                                                             part.data_ptr(), st))
            row = {"hard_select_ms": timed(select), "hard_grads_ms": timed(grads), "softmax_user_ms": timed(sm_user)}
            row["select_over_softmax_user"] = row["hard_select_ms"] / row["softmax_user_ms"]
            row["select_tflops"] = 2.0 * B * B * d / (row["hard_select_ms"] * 1e-3) / 1e12
            # the whole steps before the 4 B^2 bytes of weights of the mine launch are allocated: measured after them, in
            # one process, the "hard" step read 6 % slower at B = 65536, d = 128 than alone (profiles/r22_mixed.md)
            row["hard_step_ms"] = step_ms("hard", B, d)
            row["inbatch_step_ms"] = step_ms("inbatch", B, d)
            row["mixed_step_ms"] = step_ms("mixed", B, d)
            # the mixed objective's two launches, on the weights of a real user pass
            pos, r = torch.empty((B,), **f32), torch.empty((B,), **f32)
            sws = torch.empty((lib.rihip_inbatch_workspace_floats(B, B, d),), **f32)
            gm = torch.empty((lib.rihip_inbatch_gmat_floats(B, B),), **f32)
            neg_w = torch.empty((B, m), **f32)
            mws = torch.empty((lib.rihip_inbatch_gmat_mine_workspace_bytes(B, B, m, 0, 0),), dtype=torch.uint8, device=dev)
            mpart = torch.zeros((lib.rihip_inbatch_mixed_loss_parts(B),), dtype=torch.float64, device=dev)
            L.check(lib.rihip_rowdot(U.data_ptr(), Y.data_ptr(), B, 0, d, pos.data_ptr(), st))
            L.check(lib.rihip_inbatch_user_pass(U.data_ptr(), B, 0, Y.data_ptr(), B, 0, d, pos.data_ptr(), B, dU.data_ptr(),
                                                r.data_ptr(), part.data_ptr(), sws.data_ptr(), gm.data_ptr(), 0, st))

            def mine():
                L.check(lib.rihip_inbatch_gmat_mine(gm.data_ptr(), B, 0, B, 0, m, 0, ids.data_ptr(), ids.data_ptr(), 0,
                                                    neg_idx.data_ptr(), neg_w.data_ptr(), mws.data_ptr(), st))

            def apply():   # boosts in place every time: the values grow from call to call, the work does not
                L.check(lib.rihip_inbatch_mixed_apply(gm.data_ptr(), U.data_ptr(), B, 0, Y.data_ptr(), B, 0, d,
                                                      pos.data_ptr(), m, neg_idx.data_ptr(), neg_w.data_ptr(),
                                                      args.hard_weight, B, dU.data_ptr(), r.data_ptr(), mpart.data_ptr(), st))
            row["mine_ms"] = timed(mine)
            row["mine_TBps"] = 4.0 * B * B / (row["mine_ms"] * 1e-3) / 1e12
            row["apply_ms"] = timed(apply)
            del U, Y, dU, dI, ws, gm, sws, mws
            row["autograd_sum_ms"] = row["inbatch_step_ms"] + row["hard_select_ms"] + row["hard_grads_ms"]
            out[f"launch B={B} d={d} m={m}"] = row
            print(f"[hard] B={B} d={d} m={m}: " + ", ".join(f"{k} {v:.3f}" for k, v in row.items()), flush=True)

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

    res = {"users": int(users.size), "epochs": args.epochs, "n_hard": args.n_hard}
    arms = {"inbatch": dict(loss_mode="inbatch"),
            "softmax": dict(loss_mode="softmax"),
            "hard": dict(loss_mode="hard", n_hard=args.n_hard)}
    for name in args.arms.split(","):       # "mixed<w>": the mixed objective at hard_weight w (the default runs three)
        if name.startswith("mixed"):
            arms[name] = dict(loss_mode="mixed", n_hard=args.n_hard, hard_weight=float(name[len("mixed"):]))
    for name, kw in arms.items():
        if name not in args.arms.split(","):
            continue
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
        print(f"[hard] {name}: recall@50 {res[name]:.4f}, final loss {tr.history[-1]['loss']:.4f}", flush=True)
    pop = train.groupby("item_id").size().sort_values(ascending=False, kind="stable").index.to_numpy()
    res["popularity"] = recall(np.stack([pop[~np.isin(pop, hist.history_of(s)[0])][:50] for s in range(users.size)]))
    out["quality"] = res
    print("[hard] hold-out recall@50 (ml1m_like, exact index, one run each): " +
          ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in res.items()), flush=True)
print(json.dumps(out))
