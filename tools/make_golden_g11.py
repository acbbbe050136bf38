#!/usr/bin/env python3
"""G11: the reference's training-serving skew detector (src/evaluation/metrics.py: kl_divergence_bins :197-231,
detect_training_serving_skew :234-294) on ~25 small seeded cases -> tests/golden/g11_skew.npz.

Runs only where the reference tree is present: its metrics module (numpy + pandas only) is loaded by file path and
called unmodified; nothing of it is copied, only its outputs are recorded.  The cases cover the reference's own two
tests, int / bool / string columns, NaN holes, a column with fewer than 10 values on one side, a constant column,
+-inf, values exactly on interior edges and several copies of the max, n_bins 1 / 7 / 20 / 128, a subnormal range and
thresholds equal to a stored KL value.

Layout: ``meta`` is one JSON string (a list of cases); case i's columns are arrays ``c{i}_{side}_{j}`` (side = a for
train / p, b for serving / q; j = position in the case's column list).
Usage: python tools/make_golden_g11.py [reference_root] [out_npz]
"""
import importlib.util
import json
import sys
import warnings
from pathlib import Path

import numpy as np
import pandas as pd

ROOT = Path(__file__).resolve().parent.parent
REF = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("/root/reference")
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "tests" / "golden" / "g11_skew.npz"


def load_reference_metrics():
    spec = importlib.util.spec_from_file_location("ref_metrics", REF / "src" / "evaluation" / "metrics.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def on_edges(rng, n, n_bins):
    """integers 0..n_bins: every value sits on an edge of linspace(0, n_bins, n_bins + 1); the max repeated"""
    v = rng.integers(0, n_bins + 1, n).astype(np.float64)
    v[: 5] = n_bins
    return v


def detect_cases():
    out = []
    np.random.seed(0)
    a = np.random.normal(0, 1, 1000)
    b = np.random.normal(0, 1, 500)
    out.append({"name": "reference_no_skew", "threshold": 0.5, "a": {"x": a}, "b": {"x": b}})
    np.random.seed(0)
    a = np.random.normal(0, 1, 1000)
    b = np.random.normal(5, 1, 500)
    out.append({"name": "reference_with_skew", "threshold": 0.1, "a": {"x": a}, "b": {"x": b}})
    for s in range(10):
        rng = np.random.default_rng(100 + s)
        na, nb = int(rng.integers(40, 400)), int(rng.integers(12, 300))
        A, B = {}, {}
        A["f_norm"] = rng.normal(0, 1, na)
        B["f_norm"] = rng.normal(float(rng.choice([0.0, 0.3, 2.0])), 1, nb)
        A["f_int"] = rng.integers(0, 7, na)
        B["f_int"] = rng.integers(int(rng.integers(0, 3)), 7, nb)
        A["f_bool"] = rng.random(na) < 0.3
        B["f_bool"] = rng.random(nb) < 0.6
        A["f_str"] = np.array([f"s{int(v)}" for v in rng.integers(0, 4, na)])
        B["f_str"] = np.array([f"s{int(v)}" for v in rng.integers(0, 4, nb)])
        holes = rng.normal(1, 2, na)
        holes[rng.random(na) < 0.4] = np.nan
        A["f_holes"] = holes
        hb = rng.normal(1, 2, nb)
        hb[rng.random(nb) < 0.2] = np.nan
        B["f_holes"] = hb
        if s % 3 == 0:                                   # fewer than 10 values left on the serving side
            few = np.full(nb, np.nan)
            few[:9] = rng.normal(0, 1, 9)
            A["f_few"] = rng.normal(0, 1, na)
            B["f_few"] = few
        if s % 3 == 1:
            A["f_const"] = np.full(na, 2.5)
            B["f_const"] = np.full(nb, 2.5)
        if s % 4 == 2:                                   # an infinite value on one side
            v = rng.normal(0, 1, nb)
            v[3] = np.inf if s % 8 == 2 else -np.inf
            A["f_inf"] = rng.normal(0, 1, na)
            B["f_inf"] = v
        A["f_edges"] = on_edges(rng, na, 20)
        B["f_edges"] = on_edges(rng, nb, 20)
        A["f_f32"] = rng.standard_normal(na).astype(np.float32)
        B["f_f32"] = (rng.standard_normal(nb) * 1.5).astype(np.float32)
        if s % 2:
            B["only_serving"] = rng.normal(0, 1, nb)
            A["only_train"] = rng.normal(0, 1, na)
        case = {"name": f"mixed_{s}", "threshold": [0.1, 0.0, 0.5, 1e-6][s % 4], "a": A, "b": B}
        if s == 5:
            case["numeric_cols"] = ["f_holes", "f_norm", "f_bool"]
        out.append(case)
    return out


def kl_cases():
    out = []
    for i, nb in enumerate((1, 7, 20, 128)):
        rng = np.random.default_rng(200 + i)
        p = rng.normal(0, 1, 300)
        q = rng.normal(0.5, 1.3, 200)
        out.append({"name": f"bins_{nb}", "n_bins": nb, "epsilon": 1e-10, "p": p, "q": q})
    rng = np.random.default_rng(210)
    out.append({"name": "edges_and_max", "n_bins": 20, "epsilon": 1e-10, "p": on_edges(rng, 200, 20),
                "q": on_edges(rng, 150, 20)})
    out.append({"name": "edges_7", "n_bins": 7, "epsilon": 1e-8, "p": on_edges(rng, 100, 7) * 0.5,
                "q": on_edges(rng, 90, 7) * 0.5})
    p = rng.normal(0, 1, 50)
    p[7] = np.nan
    out.append({"name": "nan_propagates", "n_bins": 20, "epsilon": 1e-10, "p": p, "q": rng.normal(0, 1, 40)})
    q = rng.normal(0, 1, 40)
    q[0] = np.inf
    out.append({"name": "inf", "n_bins": 20, "epsilon": 1e-10, "p": rng.normal(0, 1, 50), "q": q})
    out.append({"name": "constant", "n_bins": 20, "epsilon": 1e-10, "p": np.full(30, -1.25), "q": np.full(12, -1.25)})
    tiny = np.array([0.0, 5e-324])
    out.append({"name": "subnormal_delta", "n_bins": 20, "epsilon": 1e-10, "p": np.tile(tiny, 8),
                "q": np.zeros(5)})
    out.append({"name": "subnormal_range", "n_bins": 7, "epsilon": 1e-10,
                "p": np.array([0.0, 1e-310, 3e-310, 2e-310]), "q": np.array([1e-311, 3e-310])})
    out.append({"name": "f32_values", "n_bins": 128, "epsilon": 1e-10,
                "p": rng.standard_normal(400).astype(np.float32).astype(np.float64),
                "q": rng.standard_normal(300).astype(np.float32).astype(np.float64)})
    return out


def main():
    M = load_reference_metrics()
    arrays, meta = {}, []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in detect_cases():
            i = len(meta)
            ta, tb = pd.DataFrame(c["a"]), pd.DataFrame(c["b"])
            res = M.detect_training_serving_skew(ta, tb, threshold=c["threshold"], numeric_cols=c.get("numeric_cols"))
            if c["name"] == "mixed_0" and res["feature_kl"]:       # a threshold equal to a stored value
                c["threshold"] = sorted(res["feature_kl"].values())[len(res["feature_kl"]) // 2]
                res = M.detect_training_serving_skew(ta, tb, threshold=c["threshold"])
            raw = {}
            for col in res["feature_kl"]:                           # the unrounded values behind the rounded ones
                raw[col] = M.kl_divergence_bins(ta[col].dropna().values.astype(float),
                                                tb[col].dropna().values.astype(float))
            for side, cols in (("a", c["a"]), ("b", c["b"])):
                for j, (name, v) in enumerate(cols.items()):
                    arrays[f"c{i}_{side}_{j}"] = np.asarray(v)
            meta.append({"kind": "detect", "name": c["name"], "threshold": c["threshold"],
                         "numeric_cols": c.get("numeric_cols"), "a_cols": list(c["a"]), "b_cols": list(c["b"]),
                         "result": [[k, v] for k, v in res.items()], "raw_kl": [[k, v] for k, v in raw.items()]})
        for c in kl_cases():
            i = len(meta)
            kl = M.kl_divergence_bins(c["p"], c["q"], n_bins=c["n_bins"], epsilon=c["epsilon"])
            arrays[f"c{i}_a_0"] = np.asarray(c["p"])
            arrays[f"c{i}_b_0"] = np.asarray(c["q"])
            meta.append({"kind": "kl", "name": c["name"], "n_bins": c["n_bins"], "epsilon": c["epsilon"],
                         "kl": None if np.isnan(kl) else kl})
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **arrays)
    print(f"{len(meta)} cases -> {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
