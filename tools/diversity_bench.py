"""Diversified top-k (csrc/rerank.hip, greedy MMR): what the stage costs and what it buys (HIP events, mean of --reps
after --warmup, as tools/exclude_bench.py).

--kernel  rihip_rank_topk_diverse against rihip_rank_topk on the same inputs at (nq, kc, k, w) = (256, 500, 20, 18),
          (1, 500, 20, 18), (256, 500, 20, 128); where the candidates' vectors fit in LDS both placements are timed
          (RIHIP_RERANK_STAGE=1: staged in LDS, =0: read from the table through L2 at every step).
--serve   recommend_batch of the serving chain (IVF 100/10 over --items x 128, 500 candidates) at batch 256 and for a
          single request, eager and hipGraph, with diversity=None and diversity=0.3: --windows alternated windows per
          leg; the median is reported and the spread of the windows (max - min) is the run-to-run noise.
--quality NDCG@10 and avg_diversity of the device evaluation report at diversity in {0, 0.1, 0.3, 0.5} on the
          ml1m_like() set: last 10 % of every user's ratings held out, the other 90 % make a genre profile; score =
          cosine(profile, item genres) + 0.05 * log(1 + popularity) over the user's unrated items, 500 candidates.
          (A content scorer, not the trained chain: the leg shows the trade the weight makes, not the chain's NDCG.)

python tools/diversity_bench.py [--kernel] [--serve] [--quality] [--reps 20] [--warmup 3] [--windows 5] [--items 1000000]
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

from recommendit_amd import FAISSIndex, LightGBMRanker, TwoTowerModel, mmr_rerank_device  # noqa: E402
from recommendit_amd import _lib as L  # noqa: E402
from recommendit_amd import synthetic as GB  # noqa: E402
from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--serve", action="store_true")
ap.add_argument("--quality", action="store_true")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--items", type=int, default=1_000_000)
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


def windows(fn):
    v = [timed(fn) for _ in range(args.windows)]
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


if args.kernel:
    lib = L.lib()
    n_items = 100_000
    for nq, kc, k, w in ((256, 500, 20, 18), (1, 500, 20, 18), (256, 500, 20, 128)):
        if w == 18:       # the serving layout: genre columns 5..22 of the item table, 0/1 with ~2 genres per item
            tab = torch.rand((n_items, 23), device=dev, generator=g, dtype=torch.float64)
            tab[:, 5:] = (torch.rand((n_items, 18), device=dev, generator=g) < 0.11).double()
            col0 = 5
        else:
            tab = torch.randn((n_items, w), device=dev, generator=g, dtype=torch.float64)
            col0 = 0
        s = torch.randn((nq, kc), device=dev, generator=g, dtype=torch.float64)
        c = torch.stack([torch.randperm(n_items, device=dev, generator=g)[:kc] for _ in range(nq)]).contiguous()
        r = torch.rand((nq, kc), device=dev, generator=g)
        ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        top = torch.empty((nq, k), dtype=torch.float64, device=dev)
        trs = torch.empty((nq, k), dtype=torch.float32, device=dev)
        st = L.stream_ptr()

        def plain():
            L.check(lib.rihip_rank_topk(s.data_ptr(), c.data_ptr(), r.data_ptr(), nq, kc, k, ids.data_ptr(), top.data_ptr(),
                                        trs.data_ptr(), st))

        def diverse(d=0.3):
            L.check(lib.rihip_rank_topk_diverse(s.data_ptr(), c.data_ptr(), r.data_ptr(), nq, kc, k, tab.data_ptr(),
                                                tab.shape[0], tab.shape[1], col0, w, d, ids.data_ptr(), top.data_ptr(),
                                                trs.data_ptr(), st))
        row = {"rank_topk": windows(plain)}
        fits = kc * w * 8 + 40 * kc < 160 * 1024
        for mode in (("1", "0") if fits else ("0",)):
            os.environ["RIHIP_RERANK_STAGE"] = mode
            row["diverse_lds" if mode == "1" else "diverse_table"] = windows(diverse)
        os.environ.pop("RIHIP_RERANK_STAGE", None)
        for name in ("diverse_lds", "diverse_table"):
            if name in row:
                row[name]["ratio_to_rank_topk"] = row[name]["median_ms"] / row["rank_topk"]["median_ms"]
        out[f"kernel nq={nq} kc={kc} k={k} w={w}"] = row
        print(f"[diversity] kernel ({nq}, {kc}, {k}, {w}): " + json.dumps(row), flush=True)

if args.serve:
    N, nu, K = args.items, 65536, 500
    torch.manual_seed(0)
    model = TwoTowerModel(nu, N, embed_dim=128, hidden_dim=128)
    model.eval()
    x = torch.randn((N, 128), device=dev, generator=g)
    ivf = FAISSIndex(embed_dim=128, n_lists=100, n_probe=10)
    ivf.build_from_device((x / x.norm(dim=1, keepdim=True)).contiguous(), np.arange(1, N + 1))
    forest = GB.random_forest_model(500, 63, 50, seed=4, names=feature_columns())
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "f.lgbm")
        open(p, "w").write(GB.write_text_model(forest))
        ranker = LightGBMRanker.load(p)
    fstore = GpuFeatureStore(8, 8)
    it = torch.rand((N + 1, 23), device=dev, generator=g, dtype=torch.float64)
    it[:, 5:] = (torch.rand((N + 1, 18), device=dev, generator=g) < 0.11).double()
    fstore._dev = (torch.rand((nu + 1, 24), device=dev, generator=g, dtype=torch.float64), it)
    pipe = GpuRecommendationPipeline(model, ivf, ranker, fstore, top_k_candidates=K, top_k_results=20)
    rng = np.random.RandomState(9)
    batches = [rng.randint(1, nu + 1, 256).tolist() for _ in range(3)]
    one = [int(rng.randint(1, nu + 1))]
    legs = {}
    for nm, users in (("batch256", None), ("single", one)):
        for graph in (False, True):
            for d in (None, 0.3):
                i = [0]

                def step(users=users, graph=graph, d=d, i=i):
                    i[0] += 1
                    return pipe.recommend_batch(users or batches[i[0] % 3], graph=graph, diversity=d)
                legs[f"{nm}_{'graph' if graph else 'eager'}_{'none' if d is None else d}"] = step
    rows = {k: [] for k in legs}
    for _ in range(args.windows):                           # alternated: every leg once per window
        for k, fn in legs.items():
            rows[k].append(timed(fn))
    serve = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
             for k, v in rows.items()}
    for nm in ("batch256_eager", "batch256_graph", "single_eager", "single_graph"):
        a, b = serve[f"{nm}_none"], serve[f"{nm}_0.3"]
        serve[f"{nm}_added_ms"] = b["median_ms"] - a["median_ms"]
        serve[f"{nm}_noise_ms"] = a["max_ms"] - a["min_ms"]
    out["serve"] = serve
    print(f"[diversity] serve (IVF 100/10 over {N} x 128, 500 candidates, {args.windows} alternated windows): "
          + json.dumps(serve), flush=True)

if args.quality:
    from recommendit_amd.eval_device import GroundTruth, TopKEvaluator
    ratings, movies, gm = GB.ml1m_like()
    ratings = ratings.sort_values(["user_id", "timestamp"], kind="stable")
    rank_in_user = ratings.groupby("user_id").cumcount().to_numpy()
    n_of_user = ratings.groupby("user_id")["item_id"].transform("size").to_numpy()
    held = rank_in_user >= np.floor(0.9 * n_of_user)
    train, test = ratings[~held], ratings[held]
    nu, ni = int(ratings["user_id"].max()) + 1, gm.shape[0]
    G64 = torch.from_numpy(gm.astype(np.float64)).to(dev)
    tu = torch.from_numpy(train["user_id"].to_numpy()).to(dev)
    ti = torch.from_numpy(train["item_id"].to_numpy()).to(dev)
    prof = torch.zeros((nu, 18), dtype=torch.float64, device=dev).index_add_(0, tu, G64[ti])
    pop = torch.zeros((ni,), dtype=torch.float64, device=dev).index_add_(0, ti, torch.ones_like(ti, dtype=torch.float64))
    gn = G64 / G64.norm(dim=1, keepdim=True).clamp_min(1e-12)
    score = (prof / prof.norm(dim=1, keepdim=True).clamp_min(1e-12)) @ gn.T + 0.05 * torch.log1p(pop)[None]
    score[tu, ti] = -float("inf")                           # rated items are not candidates
    in_catalog = torch.zeros((ni,), dtype=torch.bool, device=dev)
    in_catalog[torch.from_numpy(movies["item_id"].to_numpy()).to(dev)] = True
    score[:, ~in_catalog] = -float("inf")
    users = np.arange(1, nu)
    s, c = torch.topk(score[1:], 500, dim=1)
    c = torch.where(torch.isinf(s), torch.full_like(c, -1), c)
    truth = GroundTruth.from_pairs(users, test["user_id"].to_numpy(), test["item_id"].to_numpy())
    ev = TopKEvaluator(truth, users.size, 20, [10], item_vectors=G64.float().contiguous())
    q = {}
    for d in (0.0, 0.1, 0.3, 0.5):
        ids, _, _ = mmr_rerank_device(s.contiguous(), c.contiguous(), s.float().contiguous(), 20, d, G64)
        ev.enqueue(ids)
        res = ev.result()
        q[str(d)] = {"ndcg@10": res["ndcg@10"], "avg_diversity": res["avg_diversity"]}
    out["quality"] = q
    print("[diversity] quality (ml1m_like, content scorer, top 20 of 500): " + json.dumps(q), flush=True)

print(json.dumps(out))
