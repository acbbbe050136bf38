"""Seen-item exclusion: what the over-fetch and the filter cost (HIP events, mean of --reps after --warmup).

Shapes: `ml1m` = the ml1m_like() catalogue (3 883 items, d 64, exact and IVF 100/10) with its own per-user lists;
`1m` = a 1 M x 128 corpus (exact) whose users have the same activity distribution (list lengths resampled from
ml1m_like(), random item ids).  Legs per query count: the plain search at k = 500, the excluded search as one group
(device ids) and as planned groups for min_group in {1, 16, 64, 256, inf} (host ids).  --serve adds the serving chain
(batch 256 and a single request, eager and hipGraph) with the store off and on.  --kernel runs only the one-group
excluded search a few times (for `rocprofv3 --kernel-trace --stats -- python tools/exclude_bench.py --kernel ...`) and
prints the byte floor of exclude_topk_kernel computed from the shapes.

python tools/exclude_bench.py [--shapes ml1m,1m] [--nq 256,4096,65536] [--reps 20] [--warmup 3] [--serve] [--kernel]
"""
import argparse
import json
import math
import os
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from recommendit_amd import FAISSIndex, LightGBMRanker, SeenItems, TwoTowerModel  # noqa: E402
from recommendit_amd import seen as S  # noqa: E402
from recommendit_amd import synthetic as GB  # noqa: E402
from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns  # noqa: E402

PEAK = 8.0e12
K = 500
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="ml1m,1m")
ap.add_argument("--nq", default="256,4096,65536")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--serve", action="store_true")
ap.add_argument("--kernel", action="store_true")
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
ml_store = SeenItems.from_frame(ratings)
c = ml_store.counts[1:]
print(f"[exclude] ml1m_like lists: {c.size} users, mean {c.mean():.0f}, median {int(np.median(c))}, max {c.max()}, "
      f"share with k_eff <= 2048 at k = 500: {100 * (c <= 1548).mean():.2f} %", flush=True)


def shapes():
    rng = np.random.RandomState(5)
    for name in filter(None, args.shapes.split(",")):
        if name == "ml1m":
            item_ids = np.sort(movies["item_id"].unique())
            X = unit(item_ids.size, 64)
            for kind in ("exact", "ivf100/10"):
                idx = FAISSIndex(embed_dim=64, exact=True) if kind == "exact" else FAISSIndex(64, 100, 10)
                idx.build_from_device(X, item_ids)
                yield f"ml1m {kind}", idx, ml_store, 64, lambda n: rng.randint(1, ml_store.n_users, n)
        elif name == "1m":
            N, nu = 1_000_000, 65536
            X = unit(N, 128)
            idx = FAISSIndex(embed_dim=128, exact=True)
            idx.build_from_device(X, np.arange(1, N + 1))
            cnt = rng.choice(c, nu)                       # the ml1m_like activity distribution
            pu = np.repeat(np.arange(nu), cnt)
            store = SeenItems.from_pairs(pu, rng.randint(1, N + 1, pu.size), n_users=nu)
            yield "1m exact", idx, store, 128, lambda n: rng.permutation(nu)[:n] if n <= nu else rng.randint(0, nu, n)
        else:
            raise SystemExit(f"unknown shape {name!r}")


def kernel_floor(idx, store, q, users):
    """bytes exclude_topk_kernel has to move for this batch: the candidates it reads (12 B each, in steps of 256, up
    to where the k-th allowed one sits or the -1 tail begins), every query's list once (4 B per id + its two
    offsets), k * 12 B written"""
    k_eff = S.overfetch_k(K, store.max_count, idx.index.ntotal, 16384)
    _, ids = idx._search_device(q, k_eff, item_ids=True)
    ids = ids.cpu().numpy()
    read = 0
    for r, u in zip(ids, users):
        keep = (r >= 0) & ~np.isin(r, store.items_of(int(u)))
        pos = np.nonzero(keep)[0]
        pad = np.nonzero(r < 0)[0]
        last = pos[K - 1] + 1 if pos.size >= K else (pad[0] + 1 if pad.size else r.size)
        read += min(r.size, 256 * math.ceil(last / 256)) * 12
    lists = int(store.counts_of(users).sum()) * 4 + 24 * len(users)
    return k_eff, read, lists, len(users) * K * 12


for name, idx, store, d, draw in shapes():
    ntotal = idx.index.ntotal
    for nq in [int(x) for x in args.nq.split(",")]:
        users = np.asarray(draw(nq), dtype=np.int64)
        ud = torch.from_numpy(users).to(dev)
        q = unit(nq, d)
        key = f"{name} nq={nq}"
        if args.kernel:
            if nq > 4096:
                continue
            k_eff, rd, ls, wr = kernel_floor(idx, store, q, users)
            for _ in range(5):
                idx.batch_search_device(q, k=K, normalized=True, exclude=store, user_ids=ud)
            torch.cuda.synchronize()
            out[key] = {"k_eff": k_eff, "candidate_bytes": rd, "list_bytes": ls, "written_bytes": wr,
                        "floor_us_at_8TBps": (rd + ls + wr) / PEAK * 1e6}
            print(f"[exclude] {key}: kernel floor {rd + ls + wr} B = {rd} candidates + {ls} lists + {wr} written "
                  f"-> {out[key]['floor_us_at_8TBps']:.2f} us at 8 TB/s (k_eff {k_eff})", flush=True)
            continue
        row = {"plain_ms": timed(lambda: idx.batch_search_device(q, k=K, normalized=True))}
        row["one_group_ms"] = timed(lambda: idx.batch_search_device(q, k=K, normalized=True, exclude=store, user_ids=ud))
        row["one_group_k_eff"] = S.overfetch_k(K, store.max_count, ntotal, 16384)
        for mg in (1, 16, 64, 256, math.inf):
            S.MIN_GROUP = mg
            plan = S.plan_overfetch(store.counts_of(users), K, ntotal, 16384)
            row[f"groups_min{mg}_ms"] = timed(
                lambda: idx.batch_search_device(q, k=K, normalized=True, exclude=store, user_ids=users))
            row[f"groups_min{mg}_plan"] = [(ke, int(p.size)) for ke, p in plan]
        assert idx.exclusion_deficit() == 0
        out[key] = row
        print(f"[exclude] {key}: plain {row['plain_ms']:.3f} ms | one group (k_eff {row['one_group_k_eff']}) "
              f"{row['one_group_ms']:.3f} ms | groups " +
              ", ".join(f"min {mg}: {row[f'groups_min{mg}_ms']:.3f} ms {row[f'groups_min{mg}_plan']}"
                        for mg in (1, 16, 64, 256, math.inf)), flush=True)

if args.serve:
    N, nu = 1_000_000, 65536
    torch.manual_seed(0)
    model = TwoTowerModel(nu, N, embed_dim=128, hidden_dim=128)
    model.eval()
    ivf = FAISSIndex(embed_dim=128, n_lists=100, n_probe=10)
    ivf.build_from_device(unit(N, 128), np.arange(1, N + 1))
    forest = GB.random_forest_model(500, 63, 50, seed=4, names=feature_columns())
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "f.lgbm")
        open(p, "w").write(GB.write_text_model(forest))
        ranker = LightGBMRanker.load(p)
    fstore = GpuFeatureStore(8, 8)
    fstore._dev = (torch.rand((nu + 1, 24), device=dev, generator=g, dtype=torch.float64),
                   torch.rand((N + 1, 23), device=dev, generator=g, dtype=torch.float64))
    rng = np.random.RandomState(9)
    cnt = rng.choice(c, nu)
    pu = np.repeat(np.arange(1, nu + 1), cnt)
    store = SeenItems.from_pairs(pu, rng.randint(1, N + 1, pu.size), n_users=nu + 1)
    off = GpuRecommendationPipeline(model, ivf, ranker, fstore, top_k_candidates=K, top_k_results=20)
    on = GpuRecommendationPipeline(model, ivf, ranker, fstore, top_k_candidates=K, top_k_results=20, seen=store)
    batches = [rng.randint(1, nu + 1, 256).tolist() for _ in range(3)]
    one = [int(np.argsort(cnt)[nu // 2]) + 1]               # a user with the median list
    rows = {}
    for rep in range(3):                                    # alternated
        for nm, pipe in (("off", off), ("on", on)):
            i = [0]

            def step(b=batches, pipe=pipe, i=i):
                i[0] += 1
                return pipe.recommend_batch(b[i[0] % 3])
            rows.setdefault(f"batch256_{nm}_ms", []).append(timed(step))
            rows.setdefault(f"single_eager_{nm}_ms", []).append(timed(lambda: pipe.recommend_batch(one)))
            rows.setdefault(f"single_graph_{nm}_ms", []).append(timed(lambda: pipe.recommend_batch(one, graph=True)))
    assert on.exclusion_deficit() == 0
    out["serve"] = {k: float(np.median(v)) for k, v in rows.items()}
    out["serve"]["single_user_list"] = int(store.counts[one[0]])
    out["serve"]["graph_k_eff"] = S.overfetch_k(K, store.max_count, N, 16384)
    print("[exclude] serve (IVF 100/10 over 1 M x 128, 500 candidates, median of 3 alternated means): " +
          ", ".join(f"{k} {v:.3f}" for k, v in out["serve"].items()), flush=True)
print(json.dumps(out))
