"""Sampled BPR with K negatives per positive: what the loss launch, the sampler and the whole step cost, and what the
objective retrieves (HIP events, mean of --reps after --warmup; min and max of the repetitions beside it).  Nothing here
is a gate.

--launch   rihip_bpr_multi_loss at B = 65536, d in {64, 128}, K in {1, 4, 8} with rihip_bpr_pair_loss at the same B, d in
           the same run: time, and time per byte against the floor of 2 (2 + K) B d 4 bytes moved.
           rihip_sample_negatives_multi at n = 65536, K in {1, 4}, uniform against alias, on an ML-1M-shaped rated set and
           on a 1 M-item catalogue.
           A whole HipBPRTrainer(loss_mode="sampled") step at K in {1, 4, 8}: B = 1024 at the ML-1M shape with the dense
           optimiser, B = 65536 at 10 M x 1 M rows, d = 128, row-sparse.
--quality  hold-out recall@50 on ml1m_like() after --epochs epochs, the protocol of tools/hard_bench.py: sampled K = 1
           alpha = 0; K = 4 alpha = 0; K = 4 alpha = 0.75; K = 8 alpha = 0.75; in-batch BPR beside them; the popularity
           list.  One run each, unpinned.

python tools/multineg_bench.py [--launch] [--quality] [--reps 20] [--warmup 3] [--epochs 3] [--users 2000] [--small]
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
ap.add_argument("--small", action="store_true", help="--launch: leave out the 10 M x 1 M step (15 GB of tables)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
g = torch.Generator(device=dev)
g.manual_seed(7)
out = {}


def timed(fn):
    """(mean, min, max) ms over --reps single launches, each between its own pair of events"""
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = [e0.elapsed_time(e1) for e0, e1 in ev]
    return float(np.mean(t)), float(min(t)), float(max(t))


def unit(*shape):
    x = torch.randn(shape, device=dev, generator=g)
    return (x / x.norm(dim=-1, keepdim=True)).contiguous()


def step_ms(K, B, d, n_users, n_items, table_opt):
    from recommendit_amd import TwoTowerModel
    from recommendit_amd.trainer import HipBPRTrainer
    torch.manual_seed(1)
    model = TwoTowerModel(n_users, n_items, embed_dim=d, hidden_dim=128, dropout=0.1)
    model.train()
    kw = dict(n_negatives=K) if K != 1 else {}          # K = 1: the trainer exactly as it was constructed before
    tr = HipBPRTrainer(model, B, lr=1e-3, weight_decay=1e-5, loss_mode="sampled", table_opt=table_opt, seed=0, **kw)
    nI = (1 + K) * B
    batches = [(torch.randint(1, n_users + 1, (B,), device=dev, generator=g),
                torch.randint(1, n_items + 1, (nI,), device=dev, generator=g),
                (torch.rand((nI, 18), device=dev, generator=g) < 0.2).float()) for _ in range(4)]
    k = [0]

    def step():
        tr.step(*batches[k[0] % 4])
        k[0] += 1
    ms = timed(step)
    tr.check_errors()
    del tr, model, batches
    torch.cuda.empty_cache()
    return ms


if args.launch:
    lib, st = L.lib(), L.stream_ptr()
    f32 = dict(dtype=torch.float32, device=dev)
    B = 65536
    for d in (64, 128):
        U, P = unit(B, d), unit(B, d)
        dU, dP = torch.empty((B, d), **f32), torch.empty((B, d), **f32)
        part = torch.zeros((1024,), dtype=torch.float64, device=dev)
        N1, dN1 = unit(1, B, d), torch.empty((1, B, d), **f32)

        def pair():
            L.check(lib.rihip_bpr_pair_loss(U.data_ptr(), P.data_ptr(), N1.data_ptr(), B, d, None, dU.data_ptr(),
                                            dP.data_ptr(), dN1.data_ptr(), part.data_ptr(), st))
        ms, lo, hi = timed(pair)
        by = 2.0 * 3 * B * d * 4
        row = {"pair_ms": ms, "pair_min_ms": lo, "pair_max_ms": hi, "pair_ps_per_byte": ms * 1e9 / by,
               "pair_spread_ps_per_byte": (hi - lo) * 1e9 / by, "pair_TBps": by / (ms * 1e-3) / 1e12}
        for K in (1, 4, 8):
            N, dN = unit(K, B, d), torch.empty((K, B, d), **f32)

            def multi():
                L.check(lib.rihip_bpr_multi_loss(U.data_ptr(), P.data_ptr(), N.data_ptr(), B, K, d, None, dU.data_ptr(),
                                                 dP.data_ptr(), dN.data_ptr(), part.data_ptr(), st))
            ms, lo, hi = timed(multi)
            by = 2.0 * (2 + K) * B * d * 4
            row.update({f"K{K}_ms": ms, f"K{K}_min_ms": lo, f"K{K}_max_ms": hi, f"K{K}_ps_per_byte": ms * 1e9 / by,
                        f"K{K}_TBps": by / (ms * 1e-3) / 1e12})
            del N, dN
        del U, P, dU, dP, N1, dN1
        # the pair loss at 2 B rows moves exactly the bytes of K = 4 at B rows: the same footprint against the 256 MiB
        # Infinity Cache, which the pair launch at B rows fits into (201 MB at d = 128) and K = 4 does not (403 MB)
        B2 = 2 * B
        U, P, N1 = unit(B2, d), unit(B2, d), unit(1, B2, d)
        dU, dP, dN1 = torch.empty((B2, d), **f32), torch.empty((B2, d), **f32), torch.empty((1, B2, d), **f32)

        def pair2():
            L.check(lib.rihip_bpr_pair_loss(U.data_ptr(), P.data_ptr(), N1.data_ptr(), B2, d, None, dU.data_ptr(),
                                            dP.data_ptr(), dN1.data_ptr(), part.data_ptr(), st))
        ms, lo, hi = timed(pair2)
        by = 2.0 * 3 * B2 * d * 4
        row.update({"pair_at_2B_ms": ms, "pair_at_2B_min_ms": lo, "pair_at_2B_max_ms": hi,
                    "pair_at_2B_ps_per_byte": ms * 1e9 / by})
        out[f"loss B={B} d={d}"] = row
        print(f"[multineg] loss B={B} d={d}: " + ", ".join(f"{k} {v:.4f}" for k, v in row.items()), flush=True)
        del U, P, dU, dP, N1, dN1

    # ---- sampler
    from recommendit_amd.negative_sampling import alias_table, popularity_weights
    rng = np.random.default_rng(3)
    n = 65536
    worlds = {"ml1m": dict(n_users=6040, n_cat=3706, n_rated=1_000_209), "1M items": dict(n_users=10_000_000, n_cat=1_000_000,
                                                                                          n_rated=10_000_000)}
    for name, w in worlds.items():
        M = w["n_cat"] + 1
        cat = np.arange(1, M, dtype=np.int64)
        zipf = 1.0 / (1.0 + rng.permutation(w["n_cat"]))
        ru = rng.integers(1, w["n_users"] + 1, size=w["n_rated"])
        ri = rng.choice(cat, size=w["n_rated"], p=zipf / zipf.sum())
        rated = torch.from_numpy(np.unique(ru * M + ri)).to(dev)
        counts = np.bincount(ri, minlength=M)[1:]
        prob, alias = alias_table(popularity_weights(counts, 0.75))
        prob_d = torch.from_numpy(prob.view(np.int32).copy()).to(dev)
        alias_d = torch.from_numpy(alias.copy()).to(dev)
        cat_d = torch.from_numpy(cat).to(dev)
        users = torch.from_numpy(ru[:n].copy()).to(dev)          # users who rated something, as in training
        row = {"rated_keys": int(rated.numel())}
        for K in (1, 4):
            neg = torch.empty((K * n,), dtype=torch.int64, device=dev)
            for kind, (pp, aa) in (("uniform", (None, None)), ("alias", (prob_d.data_ptr(), alias_d.data_ptr()))):
                def draw():
                    L.check(lib.rihip_sample_negatives_multi(users.data_ptr(), n, K, cat_d.data_ptr(), cat_d.numel(), pp, aa,
                                                             rated.data_ptr(), rated.numel(), M, 12345, 1000,
                                                             neg.data_ptr(), None, st))
                ms, lo, hi = timed(draw)
                row.update({f"K{K}_{kind}_ms": ms, f"K{K}_{kind}_min_ms": lo, f"K{K}_{kind}_max_ms": hi,
                            f"K{K}_{kind}_Mdraws_per_s": K * n / (ms * 1e-3) / 1e6})
        neg1 = torch.empty((n,), dtype=torch.int64, device=dev)

        def single():
            L.check(lib.rihip_sample_negatives(users.data_ptr(), n, cat_d.data_ptr(), cat_d.numel(), rated.data_ptr(),
                                               rated.numel(), M, 12345, 1000, neg1.data_ptr(), None, st))
        row["existing_entry_ms"] = timed(single)[0]
        out[f"sampler {name} n={n}"] = row
        print(f"[multineg] sampler {name} n={n}: " + ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}"
                                                                 for k, v in row.items()), flush=True)
        del rated, prob_d, alias_d, cat_d, users

    # ---- whole steps
    shapes = [("ml1m dense", 1024, 64, 6040, 3952, "dense")]
    if not args.small:
        shapes.append(("10M x 1M sparse", 65536, 128, 10_000_000, 1_000_000, "sparse"))
    for name, Bs, d, nu, ni, opt in shapes:
        row = {}
        for K in (1, 4, 8):
            ms, lo, hi = step_ms(K, Bs, d, nu, ni, opt)
            row.update({f"K{K}_step_ms": ms, f"K{K}_min_ms": lo, f"K{K}_max_ms": hi,
                        f"K{K}_Mpairs_per_s": Bs * K / (ms * 1e-3) / 1e6, f"K{K}_Mpositives_per_s": Bs / (ms * 1e-3) / 1e6})
        out[f"step {name} B={Bs} d={d}"] = row
        print(f"[multineg] step {name} B={Bs} d={d}: " + ", ".join(f"{k} {v:.4f}" for k, v in row.items()), flush=True)

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
    arms = {"sampled K=1 a=0": dict(), "sampled K=4 a=0": dict(n_negatives=4),
            "sampled K=4 a=0.75": dict(n_negatives=4, negative_alpha=0.75),
            "sampled K=8 a=0.75": dict(n_negatives=8, negative_alpha=0.75), "inbatch": dict(loss_mode="inbatch")}
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
        res[name + " s/epoch"] = float(np.mean([h["seconds"] for h in tr.history]))
        print(f"[multineg] {name}: recall@50 {res[name]:.4f}, final loss {tr.history[-1]['loss']:.4f}", flush=True)
    pop = train.groupby("item_id").size().sort_values(ascending=False, kind="stable").index.to_numpy()
    res["popularity"] = recall(np.stack([pop[~np.isin(pop, hist.history_of(s)[0])][:50] for s in range(users.size)]))
    out["quality"] = res
    print("[multineg] hold-out recall@50 (ml1m_like, exact index, one run each): " +
          ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in res.items()), flush=True)
print(json.dumps(out))
