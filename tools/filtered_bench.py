"""Filtered retrieval: what the in-scan tag predicate costs and what it saves (HIP events, mean of --reps after --warmup).

Serve leg: 1 M x 128, IVF 100/10, k = 500, batch 256.  Flat leg: 1 M x 128 flat, 4 096 queries, timed with
set_two_precision(0) (the filtered search takes the all-f32 scan, so that is the like-for-like plain search) and the
default two-precision plain search beside it.  Each leg runs the filtered search at pass rates 100 %, 10 %, 1 % and
0.1 % (one shared predicate, and the same predicate as per-query rows) next to the plain search on the same handle, and
prints the share of filtered queries the exact fallback re-did (filtered_stats).

python tools/filtered_bench.py [--legs serve,flat] [--reps 20] [--warmup 3]
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from recommendit_amd import FAISSIndex  # noqa: E402
from recommendit_amd import _lib as L  # noqa: E402

K = 500
RATES = (("100%", 1.0), ("10%", 0.1), ("1%", 0.01), ("0.1%", 0.001))
ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="serve,flat")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
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


def rate_tags(n):
    """bit b set on a random share RATES[b] of the rows (bit 0: every row)"""
    rng = np.random.RandomState(3)
    tags = np.zeros(n, np.uint32)
    for b, (_, share) in enumerate(RATES):
        tags[rng.rand(n) < share] |= np.uint32(1 << b)
    tags |= 1
    return tags


def leg(name, idx, nq, plain_rows):
    N = idx.index.ntotal
    q = unit(nq, 128)
    tags = rate_tags(N)
    idx.set_item_tags(tags)
    row = dict(plain_rows(q))
    for b, (rate, _) in enumerate(RATES):
        pred = (0, 1 << b, 0) if b else (0, 0, 0)
        rows = torch.tensor([pred] * nq, dtype=torch.int32, device=dev)
        for kind, f in (("shared", pred), ("per_query", rows)):
            n0, r0 = idx.filtered_stats()
            row[f"filtered_{rate}_{kind}_ms"] = timed(lambda: idx.batch_search_device(q, k=K, normalized=True, item_filter=f))
            n1, r1 = idx.filtered_stats()
            row[f"filtered_{rate}_{kind}_fallback_share"] = (r1 - r0) / max(1, n1 - n0)
        row[f"pass_{rate}"] = int(((tags >> b) & 1).sum()) if b else N
    out[name] = row
    print(f"[filtered] {name}: " + ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()),
          flush=True)


for which in filter(None, args.legs.split(",")):
    if which == "serve":
        idx = FAISSIndex(embed_dim=128, n_lists=100, n_probe=10)
        idx.build_from_device(unit(1_000_000, 128), np.arange(1, 1_000_001))
        leg("serve ivf100/10 nq=256", idx, 256,
            lambda q: {"plain_ms": timed(lambda: idx.batch_search_device(q, k=K, normalized=True))})
    elif which == "flat":
        idx = FAISSIndex(embed_dim=128, exact=True)
        idx.build_from_device(unit(1_000_000, 128), np.arange(1, 1_000_001))

        def plain_rows(q, idx=idx):
            two = timed(lambda: idx.batch_search_device(q, k=K, normalized=True))
            L.check(L.lib().rihip_ip_index_set_two_precision(idx.index._h, 0), "set_two_precision")
            f32 = timed(lambda: idx.batch_search_device(q, k=K, normalized=True))
            L.check(L.lib().rihip_ip_index_set_two_precision(idx.index._h, 1), "set_two_precision")
            return {"plain_two_precision_ms": two, "plain_f32_ms": f32}
        leg("flat 1M x 128 nq=4096", idx, 4096, plain_rows)
    else:
        raise SystemExit(f"unknown leg {which!r}")
    del idx
    torch.cuda.empty_cache()
print(json.dumps(out))
