"""SQ8Index against the f32 FAISSIndex on the same vectors in the same run (HIP events, mean of --reps after --warmup).

1 M x 128 unit rows.  Serve leg: IVF 100/10, batch 256, k = 500.  Flat leg: a one-list index, 4 096 queries, k = 500.
Per leg: search time of both indexes (SQ8 in its automatic mode, and with each emission forced), the SQ8 build time,
device bytes of both indexes, recall@10 and recall@500 of the SQ8 lists against the f32 lists (exact for the flat leg,
the f32 IVF result of the same probes for the serve leg) and the share of thresholded queries that were re-done.

python tools/sq8_bench.py [--legs serve,flat] [--reps 20] [--warmup 3] [--n 1000000]
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from recommendit_amd import FAISSIndex, SQ8Index  # noqa: E402

K, D = 500, 128
ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="serve,flat")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--modes", default="auto,dense,thresholded")
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


def recall(ref: torch.Tensor, got: torch.Tensor, k: int) -> float:
    """mean share of the reference's first k ids found among the first k ids returned"""
    r, x = ref[:, :k], got[:, :k]
    hit = (r.unsqueeze(2) == x.unsqueeze(1)).any(dim=2) & (r >= 0)
    return float(hit.sum().item()) / max(1, int((r >= 0).sum().item()))


def leg(name, f32, nq):
    N = f32.index.ntotal
    q = unit(nq, D)
    row = {"f32_ms": timed(lambda: f32.batch_search_device(q, k=K, normalized=True))}
    _, ref = f32.batch_search_device(q, k=K, normalized=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sq = SQ8Index.from_index(f32)
    torch.cuda.synchronize()
    row["sq8_build_ms"] = (time.perf_counter() - t0) * 1e3
    st = sq.stats()
    row["sq8_device_bytes"] = st["device_bytes"]
    row["f32_row_bytes"] = N * D * 4                          # rows only (a large flat index adds a bf16 copy: + N * D * 2)
    for mode in filter(None, args.modes.split(",")):
        n0, r0 = sq.search_stats()
        row[f"sq8_{mode}_ms"] = timed(lambda: sq.batch_search_device(q, k=K, normalized=True, mode=mode))
        n1, r1 = sq.search_stats()
        row[f"sq8_{mode}_thresholded_share"] = (n1 - n0) / max(1, nq * (args.reps + args.warmup))
        row[f"sq8_{mode}_redone_share"] = (r1 - r0) / max(1, n1 - n0)
    _, got = sq.batch_search_device(q, k=K, normalized=True)
    row["recall@10"] = recall(ref, got, 10)
    row["recall@500"] = recall(ref, got, K)
    out[name] = row
    print(f"[sq8] {name}: " + ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()),
          flush=True)


for which in filter(None, args.legs.split(",")):
    if which == "serve":
        idx = FAISSIndex(embed_dim=D, n_lists=100, n_probe=10)
        idx.build_from_device(unit(args.n, D), np.arange(1, args.n + 1))
        leg("serve ivf100/10 nq=256", idx, 256)
    elif which == "flat":
        idx = FAISSIndex(embed_dim=D, exact=True)
        idx.build_from_device(unit(args.n, D), np.arange(1, args.n + 1))
        leg("one list nq=4096", idx, 4096)
    else:
        raise SystemExit(f"unknown leg {which!r}")
    del idx
    torch.cuda.empty_cache()
print(json.dumps(out))
