"""LambdaMART training-set construction on the device at the ML-1M shape (synthetic.ml1m_like(): ~1 M ratings,
n_negatives = 4): every stage of csrc/ltr_data.hip by device events (mean of 20 after 3 warm-ups), the join against
rihip_rank_features_build on the same flat rows (interleaved rounds in one process), the whole
build_ltr_dataset_device call, and RankerTrainer.run() split into data / training / holdout.
python tools/ltr_data_bench.py [n_trees=500] [n_users=6040]"""
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

from recommendit_amd import _lib as L  # noqa: E402
from recommendit_amd import synthetic  # noqa: E402
from recommendit_amd.feature_engineering import FeatureEngineer  # noqa: E402
from recommendit_amd.train_ranker import RankerTrainer  # noqa: E402

PEAK = 8.0e12
n_trees = int(sys.argv[1]) if len(sys.argv) > 1 else 500
n_users = int(sys.argv[2]) if len(sys.argv) > 2 else 6040
out = {}
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
lib = L.lib()

t0 = time.perf_counter()
kw = {} if n_users == 6040 else dict(n_users=n_users, n_ratings=int(1_000_209 * n_users / 6040))
ratings, movies, _ = synthetic.ml1m_like(**kw)
ratings["timestamp"] = pd.to_datetime(ratings["timestamp"], unit="s")
users = pd.DataFrame({"user_id": np.arange(1, n_users + 1), "gender": np.where(np.arange(n_users) % 2, "F", "M"),
                      "age": np.array([1, 18, 25, 35, 45, 50, 56])[np.arange(n_users) % 7],
                      "occupation": np.arange(n_users) % 21, "zip_code": "12345"})
print(f"[ltr] data set: {len(ratings)} ratings, {n_users} users ({time.perf_counter() - t0:.1f} s to generate)", flush=True)


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


# ---- the whole call, first from the frames (host parsing + upload included), then from device-resident ratings ----
fe = FeatureEngineer("unused")
fe.set_data(ratings, users, movies)
t0 = time.perf_counter()
ds = fe.build_ltr_dataset_device(n_negatives=4, test_ratio=0.1, seed=0)
torch.cuda.synchronize()
out["first_call_from_frames_ms"] = (time.perf_counter() - t0) * 1e3
n_rows, nf = len(ds.train) + len(ds.test), len(ds.feature_names)
out.update(n_ratings=len(ratings), n_rows=n_rows, n_queries=ds.n_queries, max_query_rows=ds.max_query_rows)


def whole():
    for k in ("user_tab", "item_tab"):
        fe._dev.pop(k, None)
    fe.build_ltr_dataset_device(n_negatives=4, test_ratio=0.1, seed=0)


whole()
torch.cuda.synchronize()
ts = []
for _ in range(10):
    t0 = time.perf_counter()
    whole()
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
out["whole_call_device_resident_ms_median"] = float(np.median(ts))
out["whole_call_device_resident_ms_min"] = float(np.min(ts))
print(f"[ltr] build_ltr_dataset_device: {n_rows} rows x {nf}; first call from DataFrames {out['first_call_from_frames_ms']:.1f} ms, "
      f"from device-resident ratings {np.median(ts):.2f} ms (min {np.min(ts):.2f})", flush=True)

# ---- per stage, through the C entry points on preallocated buffers ---------------------------------------------
d = fe._dev
nu, ni = fe._sizes
R = int(d["ru"].shape[0])
s = L.stream_ptr()
err = torch.zeros(1, dtype=torch.int32, device=dev)
scratch = torch.empty(3, dtype=torch.int64, device=dev)
ut, it = fe.build_tables_device()
i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)   # noqa: E731
i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)   # noqa: E731
p = {"bucket_off": i64(nu + 2), "bucket": i32(R), "cursor": i32(2 * (nu + 1)), "cand_index": i32(ni + 1),
     "cand_items": i64(ni + 1), "user_rows": i32(nu + 1), "query_id": i32(nu + 1), "row_start": i64(nu + 1),
     "groups": i32(nu + 1), "totals": i64(8)}
o = {"user": i64(n_rows), "item": i64(n_rows), "query": i64(n_rows), "rating": i32(n_rows),
     "label": torch.empty(n_rows, dtype=torch.float32, device=dev)}
X = torch.empty((n_rows, nf), dtype=torch.float32, device=dev)
_, cm = fe._col_map(None)
P = L.ptr


def stats():
    L.check(lib.rihip_ltr_stats(P(d["ru"]), P(d["ri"]), P(d["rv"]), P(d["rt"]), R, nu, ni, P(d["item_meta"]), P(d["in_cat"]),
                                P(d["user_acc"]), P(d["item_acc"]), P(err), 0, s))


def finalize():
    L.check(lib.rihip_ltr_finalize(P(d["user_acc"]), P(d["item_acc"]), P(d["user_meta"]), P(d["item_meta"]), nu, ni,
                                   P(scratch), P(ut), P(it), s))


def plan():
    L.check(lib.rihip_ltr_plan(P(d["ru"]), P(d["ri"]), P(d["rv"]), R, P(d["user_acc"]), P(d["item_acc"]), nu, ni, 4, 0.1, 0,
                               P(p["bucket_off"]), P(p["bucket"]), P(p["cursor"]), P(p["cand_index"]), P(p["cand_items"]),
                               P(p["user_rows"]), P(p["query_id"]), P(p["row_start"]), P(p["groups"]), P(p["totals"]), 0, s))


def emit():
    L.check(lib.rihip_ltr_emit(P(d["ri"]), P(d["rv"]), P(d["rt"]), P(d["user_acc"]), P(p["bucket_off"]), P(p["bucket"]),
                               P(p["cand_index"]), P(p["cand_items"]), P(p["user_rows"]), P(p["query_id"]),
                               P(p["row_start"]), P(p["totals"]), nu, ni, n_rows, 0, P(o["user"]), P(o["item"]),
                               P(o["label"]), P(o["rating"]), P(o["query"]), 0, s))


def join_new():
    L.check(lib.rihip_ltr_join(P(ut), ut.shape[0], P(it), it.shape[0], P(o["user"]), P(o["item"]), n_rows, P(cm), nf, P(X), P(err), 0, s))


def join_old():
    L.check(lib.rihip_rank_features_build(P(ut), ut.shape[0], P(it), it.shape[0], P(o["user"]), P(o["item"]), n_rows, 1,
                                          P(cm), nf, P(X), s))


for name, fn in (("stats", stats), ("finalize", finalize), ("plan", plan), ("emit", emit)):
    out[f"{name}_ms"] = timed(fn)
    print(f"[ltr] {name}: {out[f'{name}_ms']:.3f} ms", flush=True)
assert int(p["totals"][0].item()) == n_rows
rounds = {"new": [], "old": []}
for _ in range(5):                                   # interleaved: both kernels see the same clocks and cache state
    rounds["new"].append(timed(join_new, warm=1))
    rounds["old"].append(timed(join_old, warm=1))
traffic = n_rows * nf * 4 + n_rows * (24 + 23) * 8 + n_rows * 16
for k in ("new", "old"):
    med, best = float(np.median(rounds[k])), float(np.min(rounds[k]))
    out[f"join_{k}_ms_median"], out[f"join_{k}_ms_min"] = med, best
    out[f"join_{k}_frac_of_8TBps"] = traffic / (med * 1e-3) / PEAK
    print(f"[ltr] join ({'rihip_ltr_join' if k == 'new' else 'rihip_rank_features_build, kc=1'}): median {med:.3f} ms, "
          f"min {best:.3f} ms; {traffic / 1e9:.2f} GB (X written + one table row pair and two ids per row) = "
          f"{traffic / (med * 1e-3) / 1e12:.2f} TB/s, {100 * traffic / (med * 1e-3) / PEAK:.0f} % of 8 TB/s", flush=True)
out["device_stages_sum_ms"] = sum(out[f"{k}_ms"] for k in ("stats", "finalize", "plan", "emit")) + out["join_new_ms_median"]

# ---- RankerTrainer.run(): data / training / holdout ---------------------------------------------------------------
if n_trees > 0:
    with tempfile.TemporaryDirectory() as td:
        r = ratings.copy()
        r["timestamp"] = r["timestamp"].astype("datetime64[s]").astype(np.int64)
        synthetic.write_ml1m_files(td + "/ml", r, movies, n_users)
        t = RankerTrainer(data_dir=td + "/ml", model_output_path=td + "/ranker.lgbm", features_dir=td + "/features",
                          n_negatives=4, n_estimators=n_trees)
        t0 = time.perf_counter()
        ranker = t.run()
        out["run_total_s"] = time.perf_counter() - t0
        out["run_data_s"], out["run_train_s"], out["run_holdout_s"] = (t.timings[k] for k in ("data_s", "train_s", "holdout_s"))
        out["run_load_data_s"] = out["run_total_s"] - sum(t.timings.values())
        out["run_trees"] = ranker.model.num_trees()
        out["holdout"] = t.holdout_metrics
        out["unranked"] = t.unranked_metrics
        print(f"[ltr] RankerTrainer.run(), {n_trees} rounds asked, {out['run_trees']} trees kept: total {out['run_total_s']:.1f} s = "
              f"file parsing + save {out['run_load_data_s']:.1f} s, data stage {out['run_data_s']:.2f} s (tables to "
              f"parquet included), training {out['run_train_s']:.2f} s, holdout {out['run_holdout_s']:.2f} s", flush=True)
print(json.dumps(out))
