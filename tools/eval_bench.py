#!/usr/bin/env python3
"""Device evaluation report (recommendit_amd.eval_device) timings:
  * ranking metrics + coverage at 1 M users, K = 20 and K = 500, ~5 truth items per user;
  * diversity at (L 20, g 18: 0/1 genre vectors) and (L 512, g 128: an embedding table);
  * the host evaluate_model on a sample of users, for the whole-population ratio.
Prints one JSON line per leg.  Usage: python tools/eval_bench.py [n_users] [host_sample]"""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from recommendit_amd import metrics as M  # noqa: E402
from recommendit_amd.eval_device import GroundTruth, TopKEvaluator  # noqa: E402


def timed(ev, rec, reps=10):
    ev.enqueue(rec)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        ev.enqueue(rec)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    host_n = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    n_items = 1_000_000
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rng = np.random.default_rng(0)
    users = np.arange(n, dtype=np.int64)
    pu = np.repeat(users, 5)
    pi = rng.integers(0, n_items, pu.shape[0])
    truth = GroundTruth.from_pairs(users, pu, pi)
    for K in (20, 500):
        rec = torch.randint(0, n_items, (n, K), generator=g, device=dev, dtype=torch.int64)
        # a hit or two per row so the hit walk runs: position 3 holds the first truth item
        rec[:, 3] = torch.from_numpy(pi[::5].copy()).to(dev)
        for cov in (False, True):
            ev = TopKEvaluator(truth, n, K, [5, 10, 20], catalog_size=n_items if cov else None,
                               n_id_space=n_items if cov else None)
            t = timed(ev, rec)
            res = ev.result()
            print(json.dumps({"leg": f"rank_K{K}" + ("_cov" if cov else ""), "n": n, "seconds": t,
                              "id_read_TBps": n * K * 8 / t / 1e12, "users_per_s": n / t,
                              "ndcg@10": res["ndcg@10"]}), flush=True)
        if K == 20:
            rec20 = rec
        del rec
    for L, gdim, nu in ((20, 18, n), (512, 128, max(n // 100, 1000))):
        K = max(L, 20)
        rec = torch.randint(0, n_items, (nu, K), generator=g, device=dev, dtype=torch.int64)
        tr = GroundTruth.from_pairs(np.arange(nu), pu[:nu * 5], pi[:nu * 5])
        if gdim == 18:
            tab = (torch.rand((n_items, gdim), generator=g, device=dev) < 0.2).float()
        else:
            tab = torch.randn((n_items, gdim), generator=g, device=dev)
        ev = TopKEvaluator(tr, nu, K, [L], item_vectors=tab)
        t_all = timed(ev, rec, reps=3)
        ev0 = TopKEvaluator(tr, nu, K, [L])
        t_rank = timed(ev0, rec, reps=3)
        t_div = t_all - t_rank
        tiles = (L // 32) * (L // 32 + 1) // 2
        flops = nu * tiles * 32 * 32 * gdim * 2
        print(json.dumps({"leg": f"diversity_L{L}_g{gdim}", "n": nu, "seconds": t_div, "users_per_s": nu / t_div,
                          "gram_TFLOPs": flops / t_div / 1e12, "avg_diversity": ev.result()["avg_diversity"]}),
              flush=True)
        del rec, tab
    # host loop on a sample (K = 20 lists), scaled to the population
    ids = rec20[:host_n].cpu().numpy()
    recs = {int(u): [int(x) for x in row if x >= 0] for u, row in zip(range(host_n), ids)}
    tdict = {}
    for u, i in zip(pu[:host_n * 5], pi[:host_n * 5]):
        tdict.setdefault(int(u), []).append(int(i))
    t0 = time.perf_counter()
    M.evaluate_model(recs, tdict, [5, 10, 20], catalog_size=n_items)
    th = (time.perf_counter() - t0) / host_n * n
    ev = TopKEvaluator(truth, n, 20, [5, 10, 20], catalog_size=n_items, n_id_space=n_items)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.enqueue(rec20)
    ev.result()
    td = time.perf_counter() - t0
    print(json.dumps({"leg": "host_vs_device_K20", "n": n, "host_seconds_scaled": th, "device_seconds": td,
                      "ratio": th / td}), flush=True)


if __name__ == "__main__":
    main()
