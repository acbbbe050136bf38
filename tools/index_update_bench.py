"""Live-catalogue update of a built index: what one add/remove repack costs against rebuilding (HIP events, mean of
--reps after --warmup, the three legs alternated in one process).

Shape: BASELINE cfg5 (1 M x 128, IVF 100 lists).  Per churn level r/N in --churn, every repetition removes r random
stored items and adds r new ones (N stays put):
  (a) update   : FAISSIndex.remove + add as ONE repack (ids and rows already on the device), item ids copied back
  (b) rebuild  : a fresh handle from the final corpus with the centroids and the list of every row injected
                 (build_from_device(..., centroids=, assign=): set_vectors + set_ivf, no k-means)
  (c) retrain  : a fresh handle, 20 Lloyd iterations (build_from_device as build_ivf_index runs it)
--kernel runs only leg (a) a few times at the first churn level (for `rocprofv3 --kernel-trace --stats -- python
tools/index_update_bench.py --kernel`) and prints the bytes index_update_repack_kernel has to move.

python tools/index_update_bench.py [--n 1000000] [--d 128] [--lists 100] [--churn 0.001,0.01,0.1] [--reps 20] [--warmup 3]
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from recommendit_amd import FAISSIndex  # noqa: E402

COPY_RATE = 6.29e12          # float4 copy, bytes/s read + written (MI355X_MICROARCH.md)
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--lists", type=int, default=100)
ap.add_argument("--churn", default="0.001,0.01,0.1")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--retrain-reps", type=int, default=None, help="repetitions of leg (c); default: --reps")
ap.add_argument("--kernel", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
g = torch.Generator(device=dev)
g.manual_seed(7)
N, d, nlist = args.n, args.d, args.lists


def unit(n):
    x = torch.randn((n, d), device=dev, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


X = unit(N)
A = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=10)
A.build_from_device(X, np.arange(N, dtype=np.int64))
C = A.centroids()
lists = torch.from_numpy(A.list_assignment()).to(dev)          # the model of A on the device: rows, ids, lists
ids = torch.arange(N, device=dev)
next_id = N
rng = np.random.RandomState(3)
out = {"shape": {"N": N, "d": d, "lists": nlist}}
print(f"[index_update] {N} x {d}, {nlist} lists; imbalance {A.list_stats()['imbalance']:.3f}", flush=True)

for churn in [float(c) for c in args.churn.split(",")]:
    r = max(1, int(round(N * churn)))
    t = {"a": [], "b": [], "c": []}
    n_c = args.reps if args.retrain_reps is None else args.retrain_reps
    reps = 5 if args.kernel else args.warmup + args.reps
    for rep in range(reps):
        drop = ids[torch.from_numpy(rng.choice(N, r, replace=False)).to(dev)].contiguous()
        x_add = unit(r)
        add = torch.arange(next_id, next_id + r, device=dev)
        next_id += r
        a_add = A.assign_lists(x_add)
        torch.cuda.synchronize()
        ms_a, res = event_ms(lambda: A._apply_update(drop, x_add, add))
        assert res == (r, r) and A.index.ntotal == N
        keep = ~torch.isin(ids, drop)
        X = torch.cat([X[keep], x_add]).contiguous()
        ids = torch.cat([ids[keep], add])
        lists = torch.cat([lists[keep], a_add])
        assert torch.equal(A._item_ids_dev, ids)
        if args.kernel:
            continue
        ids_h, lists_h = ids.cpu().numpy(), lists.cpu().numpy()
        torch.cuda.synchronize()

        def rebuild():
            B = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=10)
            B.build_from_device(X, ids_h, centroids=C, assign=lists_h)
            return B

        def retrain():
            B = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=10)
            B.build_from_device(X, ids_h)
            return B
        ms_b, B = event_ms(rebuild)
        if rep == reps - 1:                              # the rebuilt handle answers as the updated one does
            q = unit(128)
            sa, ia = A.batch_search_device(q, k=500, normalized=True)
            sb, ib = B.batch_search_device(q, k=500, normalized=True)
            assert torch.equal(ia, ib) and torch.equal(sa, sb)
        del B
        ms_c = None
        if rep < args.warmup or rep - args.warmup < n_c:
            ms_c, B = event_ms(retrain)
            del B
        if rep >= args.warmup:
            t["a"].append(ms_a)
            t["b"].append(ms_b)
            if ms_c is not None:
                t["c"].append(ms_c)
    key = f"churn {100 * churn:g}% (r={r})"
    if args.kernel:
        sz = np.bincount(lists.cpu().numpy(), minlength=nlist)
        Np = int(((sz + 63) // 64 * 64).sum())
        rd, wr = (N * d * 4) + Np * 8 + (N + Np) * 8, Np * d * 4 + Np * 8     # rows + row ids, keep flags and scans
        out[key] = {"repack_read_bytes": rd, "repack_written_bytes": wr, "floor_ms_at_copy_rate": (rd + wr) / COPY_RATE * 1e3}
        print(f"[index_update] {key}: index_update_repack_kernel moves {rd} B read + {wr} B written = {(rd + wr) / 1e9:.3f} GB "
              f"-> {out[key]['floor_ms_at_copy_rate']:.3f} ms at {COPY_RATE / 1e12:.2f} TB/s", flush=True)
        break
    a, b, c = (float(np.mean(t[k])) for k in "abc")
    out[key] = {"update_ms": a, "rebuild_ms": b, "retrain_ms": c, "update_over_rebuild": a / b, "update_over_retrain": a / c,
                "update_min_ms": float(np.min(t["a"])), "rebuild_min_ms": float(np.min(t["b"])), "reps": len(t["a"]),
                "retrain_reps": len(t["c"]), "imbalance": A.list_stats()["imbalance"]}
    print(f"[index_update] {key}: (a) update {a:.3f} ms (min {out[key]['update_min_ms']:.3f}) | (b) injected rebuild {b:.3f} ms "
          f"| (c) k-means rebuild {c:.3f} ms | a/b {a / b:.3f}, a/c {a / c:.4f} | imbalance {out[key]['imbalance']:.3f}",
          flush=True)
print(json.dumps(out))
