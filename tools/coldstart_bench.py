"""Cold-start serving: what the fold-in and the cold chain cost, and what they retrieve (HIP events, mean of --reps
after --warmup).

--kernel   rihip_fold_in_users alone at nq in {1, 256, 4096}, d = 128, over a 1 M x 128 corpus, history lengths with the
           ml1m_like() activity distribution (the generator of tools/exclude_bench.py); printed beside the byte floor
           sum(len) * 512 B / 6.29 TB/s (every entry's vector read once at the HBM rate the README uses).
--serve    recommend_cold_batch of 256 histories against the warm recommend_batch of 256 users on the same 1 M x 128
           IVF 100/10 index, 500 candidates, a seen store attached to the warm pipeline (the yardstick, same run).
--quality  hold-out recall@50 on ml1m_like() after a short training run: every user's liked items are split 80 / 20,
           the model is trained on the 80 %, and the 20 % are looked for in the top 50 (training items excluded) of
           the user's trained row, of the fold-in of the 80 % (beta 0 / 1, both weightings) and of the popularity list.

python tools/coldstart_bench.py [--kernel] [--serve] [--quality] [--reps 20] [--warmup 3] [--epochs 3] [--users 2000]
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

from recommendit_amd import FAISSIndex, LightGBMRanker, SeenItems, TwoTowerModel  # noqa: E402
from recommendit_amd import synthetic as GB  # noqa: E402
from recommendit_amd.coldstart import UserHistories, fold_in_users_device, fold_in_users_launch  # noqa: E402
from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns  # noqa: E402

HBM = 6.29e12
ap = argparse.ArgumentParser()
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--serve", action="store_true")
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


ratings, movies, gm = GB.ml1m_like()
counts = ratings.groupby("user_id").size().to_numpy()
print(f"[cold] ml1m_like histories: {counts.size} users, mean {counts.mean():.0f}, max {counts.max()}", flush=True)
N = 1_000_000


def random_histories(rng, nq):
    """nq histories with the ml1m_like lengths over item ids 1..N, ratings with the ML-1M histogram"""
    per = [np.unique(rng.randint(1, N + 1, c)) for c in rng.choice(counts, nq)]      # (a repeated draw is dropped)
    slots = np.repeat(np.arange(nq), [p.size for p in per])
    items = np.concatenate(per)
    r = rng.choice(np.arange(1, 6), slots.size, p=[0.056, 0.108, 0.261, 0.349, 0.226])
    return UserHistories.from_pairs(slots, items, r, n=nq)


if args.kernel or args.serve:
    X = unit(N, 128)

if args.kernel:
    rng = np.random.RandomState(3)
    row_of = torch.cat([torch.full((1,), -1, dtype=torch.int32, device=dev), torch.arange(N, dtype=torch.int32, device=dev)])
    mu = X.double().mean(0)
    tab = torch.rand((N + 1, 23), device=dev, generator=g, dtype=torch.float64)
    tab[:, 5:] = (tab[:, 5:] < 0.15).double()
    for nq in (1, 256, 4096):
        h = random_histories(rng, nq)
        h.device_tensors()
        n_entries = int(h.counts.sum())
        liked = int((h.host[2] >= 4).sum())
        ms = timed(lambda: fold_in_users_launch(h, X, row_of, mu, 4, "uniform", 1.0, tab, None))
        floor_us = n_entries * 512 / HBM * 1e6
        out[f"kernel nq={nq}"] = {"ms": ms, "entries": n_entries, "liked": liked, "floor_us": floor_us,
                                  "gathered_floor_us": liked * 512 / HBM * 1e6}
        print(f"[cold] fold-in nq={nq}: {ms * 1e3:.1f} us, {n_entries} entries ({liked} rated >= 4 and gathered); floor "
              f"sum(len) * 512 B / 6.29 TB/s = {floor_us:.2f} us ({liked * 512 / HBM * 1e6:.2f} us for the gathered rows)",
              flush=True)

if args.serve:
    nu, K = 65536, 500
    torch.manual_seed(0)
    model = TwoTowerModel(nu, N, embed_dim=128, hidden_dim=128)
    model.eval()
    ivf = FAISSIndex(embed_dim=128, n_lists=100, n_probe=10)
    ivf.build_from_device(X, np.arange(1, N + 1))
    forest = GB.random_forest_model(500, 63, 50, seed=4, names=feature_columns())
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "f.lgbm")
        open(p, "w").write(GB.write_text_model(forest))
        ranker = LightGBMRanker.load(p)
    fstore = GpuFeatureStore(8, 8)
    fstore._dev = (torch.rand((nu + 1, 24), device=dev, generator=g, dtype=torch.float64),
                   torch.rand((N + 1, 23), device=dev, generator=g, dtype=torch.float64))
    fstore.item = fstore._dev[1].cpu().numpy()
    rng = np.random.RandomState(9)
    cnt = rng.choice(counts, nu)
    pu = np.repeat(np.arange(1, nu + 1), cnt)
    store = SeenItems.from_pairs(pu, rng.randint(1, N + 1, pu.size), n_users=nu + 1)
    warm = GpuRecommendationPipeline(model, ivf, ranker, fstore, top_k_candidates=K, top_k_results=20, seen=store)
    cold = GpuRecommendationPipeline(model, ivf, ranker, fstore, top_k_candidates=K, top_k_results=20)
    batches = [rng.randint(1, nu + 1, 256).tolist() for _ in range(3)]
    hists = [random_histories(rng, 256) for _ in range(3)]
    ivf.item_vectors_device()
    rows = {}
    for rep in range(3):                                    # alternated
        i = [0]

        def step_warm(i=i):
            i[0] += 1
            return warm.recommend_batch(batches[i[0] % 3])

        def step_cold(i=i):
            i[0] += 1
            return cold.recommend_cold_batch(hists[i[0] % 3])
        rows.setdefault("warm_batch256_ms", []).append(timed(step_warm))
        rows.setdefault("cold_batch256_ms", []).append(timed(step_cold))
        V, row_of, mu = ivf.item_vectors_device()
        rows.setdefault("fold_in_batch256_ms", []).append(
            timed(lambda: fold_in_users_device(hists[0], V, row_of, mu, item_table=fstore._dev[1])))
    out["serve"] = {k: float(np.median(v)) for k, v in rows.items()}
    out["serve"]["longest_history"] = int(max(h.max_count for h in hists))
    out["serve"]["longest_seen_list_of_the_warm_batches"] = int(max(store.counts_of(b).max() for b in batches))
    print("[cold] serve (IVF 100/10 over 1 M x 128, 500 candidates, median of 3 alternated means): " +
          ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in out["serve"].items()), flush=True)

if args.quality:
    from recommendit_amd.train_embeddings import EmbeddingTrainer, build_item_genre_dict
    rng = np.random.RandomState(1)
    liked = (ratings["rating"] >= 4).to_numpy()
    held = liked & (rng.rand(len(ratings)) < 0.2)
    train, test = ratings[~held], ratings[held]
    with tempfile.TemporaryDirectory() as td:
        tr = EmbeddingTrainer(model_output_path=os.path.join(td, "m.pt"), epochs=args.epochs, seed=0)
        model = tr.train(train, movies)
    item_ids = np.asarray(sorted(movies["item_id"].unique().tolist()), dtype=np.int64)
    gd = build_item_genre_dict(movies)
    E = model.get_item_embeddings(item_ids.tolist(), np.stack([gd[i] for i in item_ids.tolist()]))
    index = FAISSIndex(embed_dim=E.shape[1], exact=True)
    index.build_ivf_index(E, item_ids.tolist())
    n_users = int(ratings["user_id"].max())
    users = rng.permutation(np.intersect1d(train["user_id"].unique(), test["user_id"].unique()))[:args.users]
    slot_of = np.full(n_users + 1, -1, np.int64)
    slot_of[users] = np.arange(users.size)
    sub = train[slot_of[train["user_id"].to_numpy()] >= 0]
    hist = UserHistories.from_pairs(slot_of[sub["user_id"].to_numpy()], sub["item_id"].to_numpy(), sub["rating"].to_numpy(),
                                    n=users.size)
    truth = [set() for _ in users]
    for u, it in zip(test["user_id"].to_numpy(), test["item_id"].to_numpy()):
        if slot_of[u] >= 0:
            truth[slot_of[u]].add(int(it))

    def recall(ids):
        return float(np.mean([len(truth[s] & set(ids[s].tolist())) / len(truth[s]) for s in range(users.size)]))

    def search(q):
        _, ids = index.batch_search_device(q, k=50, normalized=True, exclude=hist.as_seen(),
                                           user_ids=list(range(users.size)))
        return ids.cpu().numpy()
    V, row_of, mu = index.item_vectors_device()
    res = {"users": int(users.size), "epochs": args.epochs, "final_loss": tr.history[-1]["loss"],
           "trained_row": recall(search(model.get_user_embeddings(users.tolist(), as_tensor=True)))}
    for beta in (1.0, 0.0):
        for w in ("uniform", "rating"):
            q, _, flags = fold_in_users_device(hist, V, row_of, mu, beta=beta, weighting=w)
            res[f"fold_in beta={beta:g} {w}"] = recall(search(q))
            res["flagged"] = int(flags.sum().item())
    pop = train.groupby("item_id").size().sort_values(ascending=False, kind="stable").index.to_numpy()
    res["popularity"] = recall(np.stack([pop[~np.isin(pop, hist.history_of(s)[0])][:50] for s in range(users.size)]))
    out["quality"] = res
    print("[cold] hold-out recall@50 (ml1m_like, exact index): " +
          ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in res.items()), flush=True)
print(json.dumps(out))
