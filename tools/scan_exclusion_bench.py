"""Seen-item exclusion inside the scan against the over-fetch path and the plain search, in one run (HIP events, mean of
--reps after --warmup).  Nothing here is a pass/fail number.

1 M x 128 corpus, k = 500, users with the activity distribution of ml1m_like() (mean 166, max 2 535 items, random item
ids), the legs of tools/exclude_bench.py:
  exact   plain / over-fetch (host ids: planned groups) / scan on the exact index at 4 096 queries
  ivf     the same on IVF 100/10 at batch 256, f32 index and SQ8 index
  long    one user with a 20 000-item history at batch 256 on IVF 100/10: over-fetch raises, scan serves
  mask    the mask build + clear on their own (rihip_*_exclusion_mask writes the mask the search would build; the clear
          walks the same entries), at 256 and 4 096 queries
  serve   the serving chain at batch 256 with the store off, on with over-fetch, and on with scan

python tools/scan_exclusion_bench.py [--legs exact,ivf,long,mask,serve] [--reps 20] [--warmup 3] [--n 1000000]
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
from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns  # noqa: E402
from recommendit_amd.sq8_index import SQ8Index  # noqa: E402

K = 500
ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="exact,ivf,long,mask,serve")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n", type=int, default=1_000_000)
args = ap.parse_args()
legs = set(filter(None, args.legs.split(",")))
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


def report(key, row):
    out[key] = row
    print(f"[scan-exclusion] {key}: " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()),
          flush=True)


ratings, _, _ = GB.ml1m_like()
c = SeenItems.from_frame(ratings).counts[1:]
N, nu, d = args.n, 65536, 128
rng = np.random.RandomState(5)
cnt = rng.choice(c, nu)
pu = np.repeat(np.arange(nu), cnt)
store = SeenItems.from_pairs(pu, rng.randint(1, N + 1, pu.size), n_users=nu)
ids = np.arange(1, N + 1)
X = unit(N, d)


def three(idx, q, users, key, **kw):
    ud = torch.from_numpy(users).to(dev)
    row = {"plain_ms": timed(lambda: idx.batch_search_device(q, k=K, normalized=True, **kw))}
    row["overfetch_groups_ms"] = timed(lambda: idx.batch_search_device(q, k=K, normalized=True, exclude=store, user_ids=users, **kw))
    row["overfetch_one_group_ms"] = timed(lambda: idx.batch_search_device(q, k=K, normalized=True, exclude=store, user_ids=ud, **kw))
    x0 = idx.exclusion_stats()
    row["scan_ms"] = timed(lambda: idx.batch_search_device(q, k=K, normalized=True, exclude=store, user_ids=ud, exclusion="scan", **kw))
    x1 = idx.exclusion_stats()
    calls = args.reps + args.warmup
    row["scan_chunks_per_call"] = (x1["chunks"] - x0["chunks"]) / calls
    row["scan_redone_per_call"] = (x1["redone"] - x0["redone"]) / calls
    row["scan_over_plain"] = row["scan_ms"] / row["plain_ms"]
    row["scan_over_overfetch"] = row["scan_ms"] / min(row["overfetch_groups_ms"], row["overfetch_one_group_ms"])
    report(key, row)


if "exact" in legs:
    idx = FAISSIndex(embed_dim=d, exact=True)
    idx.build_from_device(X, ids)
    nq = 4096
    three(idx, unit(nq, d), rng.permutation(nu)[:nq].astype(np.int64), f"exact {N} x {d} nq={nq}")
    del idx

ivf = None
if legs & {"ivf", "long", "mask", "serve"}:
    ivf = FAISSIndex(embed_dim=d, n_lists=100, n_probe=10)
    ivf.build_from_device(X, ids)

if "ivf" in legs:
    nq = 256
    q, users = unit(nq, d), rng.permutation(nu)[:nq].astype(np.int64)
    three(ivf, q, users, f"ivf100/10 f32 {N} x {d} nq={nq}")
    sq = SQ8Index.from_index(ivf)
    three(sq, q, users, f"ivf100/10 sq8 {N} x {d} nq={nq}")
    del sq

if "long" in legs:
    nq = 256
    q = unit(nq, d)
    long_store = SeenItems.from_pairs(np.zeros(20000, np.int64), rng.choice(ids, 20000, replace=False), n_users=nq)
    users = np.arange(nq, dtype=np.int64)
    try:
        ivf.batch_search_device(q, k=K, normalized=True, exclude=long_store, user_ids=users)
        over = "served"
    except ValueError as e:
        over = "ValueError: " + str(e)[:60]
    ud = torch.from_numpy(users).to(dev)
    report("long history (20 000 items, one user of 256)", {
        "overfetch": over,
        "plain_ms": timed(lambda: ivf.batch_search_device(q, k=K, normalized=True)),
        "scan_ms": timed(lambda: ivf.batch_search_device(q, k=K, normalized=True, exclude=long_store, user_ids=ud, exclusion="scan"))})

if "mask" in legs:
    for nq in (256, 4096):
        users = torch.from_numpy(rng.permutation(nu)[:nq].astype(np.int64)).to(dev)
        from recommendit_amd import _lib as L
        import ctypes as C
        w = C.c_int64(0)
        L.check(L.lib().rihip_ip_index_exclusion_mask_words(ivf.index._h, C.byref(w)))
        buf = torch.empty((nq, int(w.value)), dtype=torch.int32, device=dev)
        row_of = ivf._row_of_device()

        def build():
            L.check(L.lib().rihip_ip_index_exclusion_mask(ivf.index._h, nq, users.data_ptr(), store.offsets.data_ptr(), store.n_users,
                                                          store.items.data_ptr(), row_of.data_ptr(), row_of.shape[0], buf.data_ptr(),
                                                          L.stream_ptr()))
        report(f"mask nq={nq} ({buf.numel() * 4 / 2 ** 20:.0f} MiB)", {
            "memset_plus_build_ms": timed(build), "memset_ms": timed(lambda: buf.zero_()),
            "seen_entries": int(store.counts_of(users.cpu().numpy()).sum())})

if "serve" in legs:
    torch.manual_seed(0)
    model = TwoTowerModel(nu, N, embed_dim=d, hidden_dim=128)
    model.eval()
    forest = GB.random_forest_model(500, 63, 50, seed=4, names=feature_columns())
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "f.lgbm")
        open(p, "w").write(GB.write_text_model(forest))
        ranker = LightGBMRanker.load(p)
    fstore = GpuFeatureStore(8, 8)
    fstore._dev = (torch.rand((nu + 1, 24), device=dev, generator=g, dtype=torch.float64),
                   torch.rand((N + 1, 23), device=dev, generator=g, dtype=torch.float64))
    mk = lambda **kw: GpuRecommendationPipeline(model, ivf, ranker, fstore, top_k_candidates=K, top_k_results=20, **kw)
    pipes = (("off", mk()), ("overfetch", mk(seen=store)), ("scan", mk(seen=store, exclusion="scan")))
    batches = [rng.randint(1, nu, 256).tolist() for _ in range(3)]
    rows = {}
    for rep in range(3):                                    # alternated
        for nm, pipe in pipes:
            i = [0]

            def step(b=batches, pipe=pipe, i=i):
                i[0] += 1
                return pipe.recommend_batch(b[i[0] % 3])
            rows.setdefault(f"batch256_{nm}_ms", []).append(timed(step))
    report("serve (IVF 100/10, 500 candidates, median of 3 alternated means)", {k: float(np.median(v)) for k, v in rows.items()})
print(json.dumps(out))
