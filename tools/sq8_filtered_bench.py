"""Filtered SQ8 search: what the tag predicate inside the int8 scan costs (HIP events, mean of --reps after --warmup).

1 M x 128 unit rows, k = 500.  Serve leg: IVF 100/10, batch 256.  Flat leg: a one-list index, 4 096 queries.  Per leg and
pass rate (100 %, 10 %, 1 %, 0.1 %; one shared predicate): the filtered SQ8 search, plain and with refine = 2 (share
certified), with the share of filtered queries re-done dense, next to the plain SQ8 search (plain and refine = 2) and the
f32 FAISSIndex's filtered search of the same tags in the same run.

python tools/sq8_filtered_bench.py [--legs serve,flat] [--reps 20] [--warmup 3] [--n 1000000]
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from recommendit_amd import FAISSIndex, SQ8Index  # noqa: E402

K, D = 500, 128
RATES = (("100%", 1.0), ("10%", 0.1), ("1%", 0.01), ("0.1%", 0.001))
ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="serve,flat")
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


def rate_tags(n):
    """bit b set on a random share RATES[b] of the rows (bit 0: every row)"""
    rng = np.random.RandomState(3)
    tags = np.zeros(n, np.uint32)
    for b, (_, share) in enumerate(RATES):
        tags[rng.rand(n) < share] |= np.uint32(1 << b)
    tags |= 1
    return tags


def leg(name, f32, nq):
    q = unit(nq, D)
    f32.set_item_tags(rate_tags(f32.index.ntotal))
    sq = SQ8Index.from_index(f32, keep_vectors=True)          # (the tags come along)
    row = {"sq8_plain_ms": timed(lambda: sq.batch_search_device(q, k=K, normalized=True)),
           "sq8_plain_refine2_ms": timed(lambda: sq.batch_search_device(q, k=K, normalized=True, refine=2))}
    for b, (rate, _) in enumerate(RATES):
        pred = (0, 1 << b, 0) if b else (0, 0, 0)
        row[f"f32_filtered_{rate}_ms"] = timed(lambda: f32.batch_search_device(q, k=K, normalized=True, item_filter=pred))
        n0, r0 = sq.filtered_stats()
        ms = timed(lambda: sq.batch_search_device(q, k=K, normalized=True, item_filter=pred))
        n1, r1 = sq.filtered_stats()
        row[f"sq8_filtered_{rate}_ms"] = ms
        row[f"sq8_filtered_{rate}_vs_plain"] = ms / row["sq8_plain_ms"]
        row[f"sq8_filtered_{rate}_redone_share"] = (r1 - r0) / max(1, n1 - n0)
        ms = timed(lambda: sq.batch_search_device(q, k=K, normalized=True, item_filter=pred, refine=2))
        n2, r2 = sq.filtered_stats()
        row[f"sq8_filtered_{rate}_refine2_ms"] = ms
        row[f"sq8_filtered_{rate}_refine2_vs_plain_refine2"] = ms / row["sq8_plain_refine2_ms"]
        row[f"sq8_filtered_{rate}_refine2_redone_share"] = (r2 - r1) / max(1, n2 - n1)
        cert = sq.batch_search_device(q, k=K, normalized=True, item_filter=pred, refine=2, return_cert=True)[2]
        row[f"sq8_filtered_{rate}_refine2_certified_share"] = float(cert.float().mean().item())
    out[name] = row
    print(f"[sq8 filtered] {name}: " + ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()),
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
