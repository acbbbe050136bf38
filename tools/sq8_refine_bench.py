"""The SQ8 index's refined search against its plain search and the f32 FAISSIndex, on the same vectors in the same run
(HIP events, mean of --reps after --warmup).

1 M x 128 unit rows, k = 500.  Serve leg: IVF 100/10, batch 256.  Flat leg: a one-list index, 4 096 queries.  Per leg:
the f32 index's and the plain SQ8 search's time, then for every refine factor the refined search's time, recall@10 and
recall@500 against the f32 lists (exact for the flat leg, the f32 IVF result of the same probes for the serve leg), the
share of certified queries and the mean bound.  The plain search's recall is the row "refine none".

python tools/sq8_refine_bench.py [--legs serve,flat] [--factors 1,2,4] [--reps 20] [--warmup 3] [--n 1000000]
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
ap.add_argument("--factors", default="1,2,4")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n", type=int, default=1_000_000)
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
    hits = total = 0
    for i in range(0, ref.shape[0], 256):                      # (a [256, k, k] comparison at a time)
        r, x = ref[i:i + 256, :k], got[i:i + 256, :k]
        hits += int(((r.unsqueeze(2) == x.unsqueeze(1)).any(dim=2) & (r >= 0)).sum().item())
        total += int((r >= 0).sum().item())
    return hits / max(1, total)


def leg(name, f32, nq):
    q = unit(nq, D)
    row = {"f32_ms": timed(lambda: f32.batch_search_device(q, k=K, normalized=True))}
    _, ref = f32.batch_search_device(q, k=K, normalized=True)
    torch.cuda.synchronize()
    sq = SQ8Index.from_index(f32)
    plain_bytes = sq.stats()["device_bytes"]
    t0 = time.perf_counter()
    sq.attach_vectors(f32)
    torch.cuda.synchronize()
    row["attach_ms"] = (time.perf_counter() - t0) * 1e3
    row["sq8_device_bytes"] = plain_bytes
    row["sq8_with_vectors_device_bytes"] = sq.stats()["device_bytes"]
    row["sq8_plain_ms"] = timed(lambda: sq.batch_search_device(q, k=K, normalized=True, refine=None))
    _, got = sq.batch_search_device(q, k=K, normalized=True, refine=None)
    row["refine none recall@10"] = recall(ref, got, 10)
    row["refine none recall@500"] = recall(ref, got, K)
    for f in [float(x) for x in filter(None, args.factors.split(","))]:
        tag = f"refine {f:g}"
        row[f"{tag} ms"] = timed(lambda: sq.batch_search_device(q, k=K, normalized=True, refine=f))
        _, got, cert, bound = sq.batch_search_device(q, k=K, normalized=True, refine=f, return_cert=True)
        row[f"{tag} recall@10"] = recall(ref, got, 10)
        row[f"{tag} recall@500"] = recall(ref, got, K)
        row[f"{tag} certified"] = float(cert.float().mean().item())
        row[f"{tag} mean_bound"] = float(bound.mean().item())
    out[name] = row
    print(f"[sq8 refine] {name}: " + ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()),
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
