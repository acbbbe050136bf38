"""Training-serving skew on the device: the detector at 2.39 M + 1 M rows x 50 f32 columns (device-resident, device
events after a warm-up), the upload of an f64 DataFrame, the host detector on a subsample, and the serve chain at
batch 256 with the feature log off / on, alternated.  python tools/skew_bench.py [host_fraction]"""
import json
import os
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402
from recommendit_amd import FAISSIndex, LightGBMRanker, TwoTowerModel  # noqa: E402
from recommendit_amd import metrics as M  # noqa: E402
from recommendit_amd import skew_device as S  # noqa: E402
from recommendit_amd import synthetic as GB  # noqa: E402
from recommendit_amd.recommender import GpuFeatureStore, GpuRecommendationPipeline, feature_columns  # noqa: E402

PEAK = 8.0e12
NA, NB, NC = 2_390_000, 1_000_000, 50
frac = float(sys.argv[1]) if len(sys.argv) > 1 else 0.05
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
out = {}

g = torch.Generator(device=dev)
g.manual_seed(11)
A = torch.randn((NA, NC), generator=g, device=dev)
Bm = torch.randn((NB, NC), generator=g, device=dev) * 1.1 + 0.05
names = [f"f{i}" for i in range(NC)]

# 1. the detector's device part on device-resident f32 matrices
for _ in range(3):
    S.feature_histograms_device(A, Bm)
torch.cuda.synchronize()
reps = 20
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):
    r = S.feature_histograms_device(A, Bm)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / reps
read = 2 * (NA + NB) * NC * 4                     # range pass + histogram pass
out["detector_ms"] = ms
out["detector_bytes_read"] = read
out["detector_TBps"] = read / (ms * 1e-3) / 1e12
out["detector_frac_of_8TBps"] = read / (ms * 1e-3) / PEAK
t0 = time.perf_counter()
res = S.detect_training_serving_skew_device(A, Bm, columns=names)
torch.cuda.synchronize()
out["detect_dict_device_ms"] = (time.perf_counter() - t0) * 1e3
print(f"[skew] device histograms + KL: {ms:.3f} ms, {out['detector_TBps']:.2f} TB/s over {read / 1e9:.2f} GB "
      f"({100 * out['detector_frac_of_8TBps']:.0f} % of 8 TB/s); whole detector call {out['detect_dict_device_ms']:.2f} ms",
      flush=True)

# 2. uploading an f64 DataFrame (the DataFrame path of the detector)
An = A.cpu().numpy()
df = pd.DataFrame(An.astype(np.float64), columns=names)
S._frame_segment(df.iloc[:1000], names, dev)
torch.cuda.synchronize()
t0 = time.perf_counter()
seg = S._frame_segment(df, names, dev)
torch.cuda.synchronize()
out["upload_f64_frame_ms"] = (time.perf_counter() - t0) * 1e3
del seg
print(f"[skew] f64 DataFrame {NA} x {NC} -> device: {out['upload_f64_frame_ms']:.1f} ms", flush=True)

# 3. the host detector on a subsample, scaled by rows (np.histogram sorts: n log n, so the scaling is a lower bound)
na, nb = int(NA * frac), int(NB * frac)
tr = df.iloc[:na]
sv = pd.DataFrame(Bm[:nb].cpu().numpy().astype(np.float64), columns=names)
t0 = time.perf_counter()
host = M.detect_training_serving_skew(tr, sv)
hs = time.perf_counter() - t0
out["host_detector_s_subsample"] = hs
out["host_subsample_fraction"] = frac
out["host_detector_s_scaled"] = hs / frac
print(f"[skew] host detector on {na} + {nb} rows: {hs:.2f} s -> ~{hs / frac:.1f} s at full size (linear scaling)",
      flush=True)
del df, tr, sv, An

# 4. serve chain at batch 256, feature log off / on, alternated
N, nu = 1_000_000, 1_000_000
torch.manual_seed(0)
model = TwoTowerModel(nu, N, embed_dim=128, hidden_dim=128)
model.eval()
X = torch.randn((N, 128), device=dev, generator=g)
X = (X / X.norm(dim=1, keepdim=True)).contiguous()
ivf = FAISSIndex(embed_dim=128, n_lists=100, n_probe=10)
ivf.build_from_device(X, np.arange(1, N + 1))
forest = GB.random_forest_model(500, 63, 50, seed=4, names=feature_columns())
with tempfile.TemporaryDirectory() as td:
    p = os.path.join(td, "f.lgbm")
    open(p, "w").write(GB.write_text_model(forest))
    ranker = LightGBMRanker.load(p)
store = GpuFeatureStore(8, 8)
store._dev = (torch.rand((nu + 1, 24), device=dev, generator=g, dtype=torch.float64),
              torch.rand((N + 1, 23), device=dev, generator=g, dtype=torch.float64))
off = GpuRecommendationPipeline(model, ivf, ranker, store, top_k_candidates=500, top_k_results=20)
on = GpuRecommendationPipeline(model, ivf, ranker, store, top_k_candidates=500, top_k_results=20,
                               feature_log_rows=1_000_000)
uids = [torch.randint(1, nu + 1, (256,), device=dev, generator=g) for _ in range(3)]
rows = {"off": [], "on": []}
for rep in range(3):
    for name, pipe in (("off", off), ("on", on)):
        med, best, _ = B.timed_blocks(lambda i: pipe.recommend_batch(uids[i % 3]), 12)
        rows[name].append(med)
        print(f"[skew] serve batch 256, log {name}: {med * 1e3:.3f} ms/batch = {256 / med:,.0f} req/s", flush=True)
m_off, m_on = float(np.median(rows["off"])), float(np.median(rows["on"]))
out["serve_ms_per_batch_off"] = m_off * 1e3
out["serve_ms_per_batch_on"] = m_on * 1e3
out["serve_rps_off"] = 256 / m_off
out["serve_rps_on"] = 256 / m_on
out["log_overhead_pct"] = 100 * (m_on / m_off - 1)
print(f"[skew] feature-log overhead: {out['log_overhead_pct']:+.2f} % of the batch", flush=True)
print(json.dumps(out))
