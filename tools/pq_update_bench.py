"""Live-catalogue update of a PQIndex under frozen codebooks: what one remove + add repack costs against the route it
replaces (hip events around calls that synchronise themselves; a warm-up, then the median of --blocks windows of --steps
updates each; both routes in the same run).

Shape: BASELINE cfg5 (1 M x 128, IVF 100 lists, nprobe 10).  Every step removes r = churn * N random stored items and
adds r new unit rows (N stays put), ids and rows already on the device.  Three handles: bare, with tags, with tags and
attached vectors.
  (i)   update : PQIndex remove + add as ONE repack (rihip_pq_update_apply)
  (ii)  today  : an f32 FAISSIndex kept resident and updated the same way, then
                 PQIndex.from_index(ranges=old.quantizer(), codebooks=old.codebooks()) (+ set_item_tags) (+ keep_vectors=True)
  (iii) floor  : bytes the repack has to move, 2 * Np * (M + 12) (entry numbers, row ids, tag words, read and written),
                 against the 6.29 TB/s float4-copy rate; the encode kernel has no byte floor worth the name (r * dk * 4
                 bytes in): its time is the 256-entry search per (row, sub-space)
  (iv)  bytes  : what the handle holds (stats()["device_bytes"]) against the 512 MB of keeping the f32 index

--kernel LEG runs only route (i) on one handle (bare, tags or tags+vectors) four times, for
`rocprofv3 --kernel-trace --stats -- python tools/pq_update_bench.py --kernel bare`: pq_update_repack_kernel and
pq_update_encode_kernel appear by name.

python tools/pq_update_bench.py [--n 1000000] [--d 128] [--lists 100] [--dsub 8] [--residual] [--churn 0.01] [--blocks 5]
                                [--steps 3] [--kernel LEG]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from recommendit_amd import FAISSIndex, PQIndex  # noqa: E402

COPY_RATE = 6.29e12          # float4 copy, bytes/s read + written (MI355X_MICROARCH.md)
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--lists", type=int, default=100)
ap.add_argument("--dsub", type=int, default=8)
ap.add_argument("--residual", action="store_true")
ap.add_argument("--iters", type=int, default=2)
ap.add_argument("--churn", type=float, default=0.01)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--kernel", default=None, choices=["bare", "tags", "tags+vectors"])
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
g = torch.Generator(device=dev)
g.manual_seed(7)
N, d, nlist = args.n, args.d, args.lists
r = max(1, int(round(N * args.churn)))
dk = 32 if d <= 32 else (64 if d <= 64 else 128)
dpad = 64 if d <= 64 else 128
M = dpad // args.dsub
rng = np.random.RandomState(3)


def unit(n):
    x = torch.randn((n, d), device=dev, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def windows(step):
    """median and best window of the per-step time in ms"""
    for _ in range(args.warmup):
        step()
    per = [statistics.mean(step() for _ in range(args.steps)) for _ in range(args.blocks)]
    return statistics.median(per), min(per)


X = unit(N)
F = FAISSIndex(embed_dim=d, n_lists=nlist, n_probe=10)
F.build_from_device(X, np.arange(N, dtype=np.int64))
del X
tags0 = rng.randint(0, 1 << 18, N).astype(np.uint32)
out = {"shape": {"N": N, "d": d, "lists": nlist, "dsub": args.dsub, "M": M, "residual": args.residual, "churn": args.churn, "r": r,
                 "blocks": args.blocks, "steps": args.steps}}
next_id = [N]
first = PQIndex.from_index(F, dsub=args.dsub, n_iter=args.iters, by_residual=args.residual)      # the one training of the run
quant, book = first.quantizer(), first.codebooks()
n_build = first.train_stats()["distortion"]
del first


def change(ids_dev):
    """(drop ids, new rows, new ids, new tag words) of one step, on the device"""
    drop = ids_dev[torch.from_numpy(rng.choice(N, r, replace=False)).to(dev)].contiguous()
    add = torch.arange(next_id[0], next_id[0] + r, device=dev)
    next_id[0] += r
    return drop, unit(r), add, rng.randint(0, 1 << 18, r).astype(np.uint32)


def build(vectors):
    return PQIndex.from_index(F, dsub=args.dsub, ranges=quant, codebooks=book, by_residual=args.residual, keep_vectors=vectors,
                              frozen_updates=True)


for leg, tagged, vectors in (("bare", False, False), ("tags", True, False), ("tags+vectors", True, True)):
    if args.kernel not in (None, leg):
        continue
    A = build(vectors)
    if tagged:
        A.set_item_tags(tags0)

    def update():
        drop, x, add, words = change(A._item_ids_dev)
        ms, res = event_ms(lambda: A._apply_update(drop, x, add, words if tagged else None))
        assert res == (r, r) and A.index.ntotal == N
        return ms

    # the route it replaces on a copy of the f32 index's state: F itself moves along, so both routes see the same sizes
    state = {"tags": tags0.copy()}

    def today():
        drop, x, add, words = change(F._item_ids_dev)
        keep = ~np.isin(F.item_ids, drop.cpu().numpy()) if tagged else None

        def route():
            F._apply_update(drop, x, add)
            B = build(vectors)
            if tagged:
                state["tags"] = np.concatenate([state["tags"][keep], words])
                B.set_item_tags(state["tags"])
            return B
        ms, B = event_ms(route)
        assert B.index.ntotal == N
        del B
        return ms

    if args.kernel:
        print(f"[pq update] {leg}: " + ", ".join(f"{update():.3f} ms" for _ in range(4)), flush=True)
        sys.exit(0)
    up_med, up_min = windows(update)
    td_med, td_min = windows(today)
    st, us = A.stats(), A.update_stats()
    fixed = 8 * dpad + 4 * nlist * dk + 8 * (nlist + 1) + 4 * nlist + 256 * dpad + (nlist * dpad if args.residual else 0)
    Np = (st["device_bytes"] - (4 * N * dk + 16 * dk if vectors else 0) - fixed) // (M + 8 + (4 if tagged else 0))
    floor = 2 * Np * (M + 12)
    out[leg] = {"update_ms": up_med, "update_min_ms": up_min, "today_ms": td_med, "today_min_ms": td_min,
                "update_over_today": up_med / td_med, "Np": int(Np), "floor_bytes": int(floor),
                "floor_ms_at_copy_rate": floor / COPY_RATE * 1e3, "device_bytes": st["device_bytes"],
                "f32_index_bytes": int(Np * dk * 4), "clamped": us["clamped"], "residual_clamped": us["residual_clamped"],
                "distortion_per_added_row": us["distortion_added"] / max(us["added"], 1),
                "distortion_per_built_row": float(n_build[-1]) / N}
    print(f"[pq update] {leg}: (i) update {up_med:.3f} ms (best {up_min:.3f}) | (ii) today {td_med:.3f} ms (best {td_min:.3f}) | "
          f"i/ii {up_med / td_med:.4f} | (iii) floor {floor / 1e6:.1f} MB = {out[leg]['floor_ms_at_copy_rate']:.4f} ms | "
          f"(iv) held {st['device_bytes'] / 1e6:.1f} MB, f32 index {out[leg]['f32_index_bytes'] / 1e6:.1f} MB | "
          f"distortion per row: added {out[leg]['distortion_per_added_row']:.0f}, built {out[leg]['distortion_per_built_row']:.0f}",
          flush=True)
    del A
print(json.dumps(out))
