"""Per-feature TreeSHAP contributions (rihip_gbdt_predict_contrib, csrc/gbdt.hip): what an explanation costs next to the
score it explains (HIP events, mean of --reps after --warmup, as tools/diversity_bench.py).

The serve-shaped forest (500 trees x 63 leaves x 50 features, counts from a routed background sample) at 20 rows (the
returned items of one request), 256 x 20 rows (those of a batch) and 256 x 500 rows (every candidate of a batch):
predict_contrib_device against predict_device on the same rows, the ratio "explain / score", and the achieved f64
FLOP/s.  FLOPs are the useful ones of the definition, counted on the host per path with D distinct features: EXTEND
updates l + 1 weights in step l at 7 FLOP each (two products of three factors, two divisions, one sum) and every one of
the D unwound sums takes D steps of 7 FLOP; idle lanes, shuffles and the go-left evaluation are not counted.  The
peak it is held against is the vector f64 rate, half the 157.3 TFLOP/s vector f32 peak (spec, not measured).

python tools/contrib_bench.py [--reps 20] [--warmup 3] [--trees 500] [--leaves 63]
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

from recommendit_amd import LightGBMRanker  # noqa: E402
from recommendit_amd import synthetic as GB  # noqa: E402

PEAK_F64_VECTOR = 157.3e12 / 2

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--trees", type=int, default=500)
ap.add_argument("--leaves", type=int, default=63)
ap.add_argument("--features", type=int, default=50)
ap.add_argument("--rows", type=int, nargs="*", default=[20, 256 * 20, 256 * 500])
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)


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


def with_counts(model, background):
    """the model text with leaf_count / internal_count: background rows per leaf (x <= threshold goes left), plus 1"""
    text = GB.write_text_model(model)
    head, *blocks = text.split("Tree=")
    out, flop = [head], 0
    for t, blk in zip(model["trees"], blocks):
        nl = t["num_leaves"]
        node = np.zeros(background.shape[0], dtype=np.int64)
        while (node >= 0).any():
            act = node >= 0
            nd = node[act]
            left = background[act, t["split_feature"][nd]] <= t["threshold"][nd]
            node[act] = np.where(left, t["left_child"][nd], t["right_child"][nd])
        lc = np.ones(nl, dtype=np.int64)
        np.add.at(lc, ~node, 1)
        ic = np.zeros(nl - 1, dtype=np.int64)
        stack = [(0, frozenset())]
        order = []
        while stack:                                    # paths: distinct features from the root to every leaf
            n, feats = stack.pop()
            if n < 0:
                D = len(feats)
                flop += 7 * (sum(l + 1 for l in range(1, D + 1)) + D * D)
                continue
            order.append(n)
            f2 = feats | {int(t["split_feature"][n])}
            stack += [(int(t["left_child"][n]), f2), (int(t["right_child"][n]), f2)]
        for n in reversed(order):                       # children before parents
            ic[n] = sum(int(ic[c]) if c >= 0 else int(lc[~c]) for c in (int(t["left_child"][n]), int(t["right_child"][n])))
        extra = ("leaf_count=" + " ".join(map(str, lc)) + "\ninternal_count=" + " ".join(map(str, ic)) + "\n")
        out.append(blk.replace("is_linear=0\n", extra + "is_linear=0\n", 1))
    return "Tree=".join(out), flop


rng = np.random.RandomState(12)
forest = GB.random_forest_model(args.trees, args.leaves, args.features, seed=4)
text, flop_per_row = with_counts(forest, rng.randn(20000, args.features))
with tempfile.TemporaryDirectory() as td:
    p = os.path.join(td, "f.lgbm")
    open(p, "w").write(text)
    ranker = LightGBMRanker.load(p)
print(f"[contrib] forest {args.trees} x {args.leaves} x {args.features}: {flop_per_row / 1e6:.2f} MFLOP (f64, useful) per row, "
      f"predict path {ranker.model.predict_path()}", flush=True)
out = {"forest": [args.trees, args.leaves, args.features], "flop_per_row": flop_per_row}
for n in args.rows:
    X = torch.from_numpy(rng.randn(n, args.features).astype(np.float32)).to(dev)
    phi = ranker.predict_contrib_device(X)              # builds the path tables / grows the scratch outside the timing
    score = ranker.predict_device(X)
    resid = float((phi.sum(1) - score).abs().max())
    t_explain = timed(lambda: ranker.predict_contrib_device(X))
    t_score = timed(lambda: ranker.predict_device(X))
    row = {"explain_ms": t_explain, "score_ms": t_score, "explain_over_score": t_explain / t_score,
           "rows_per_s": n / (t_explain * 1e-3), "f64_tflops": flop_per_row * n / (t_explain * 1e-3) / 1e12,
           "fraction_of_vector_f64_peak": flop_per_row * n / (t_explain * 1e-3) / PEAK_F64_VECTOR,
           "max_abs_sum_minus_score": resid}
    out[f"rows={n}"] = row
    print(f"[contrib] rows={n}: " + json.dumps(row), flush=True)
print(json.dumps(out))
