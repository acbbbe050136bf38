"""Writes tests/golden/g13_contrib.npz: the TreeSHAP contribution cases whose reference is too slow for test time.

Per case: the model text (with leaf_count / internal_count), the rows X, phi = the recursive Algorithm 2 of
tests/shap_reference.py evaluated in x87 long double and rounded to f64, dev_ref = max |phi_f64 - phi_longdouble| (the
f64 recursion's own error: the scale of the tolerance of tests/test_gpu_contrib.py) and resid = max |phi.sum(1) -
oracle predict_raw| of the stored values.

  large  40 random 63-leaf trees over 50 features, decision types 0/2/6/8/10 mixed, 8 rows with NaN and 0.0
  chain   4 chain-shaped 63-leaf trees whose longest path has 50 distinct features, 6 rows: the unwind divides by
          products of small cover fractions and cancels, which is where f32 arithmetic fails by 1e-3 and worse

    python tools/make_golden_g13.py            (about a minute)
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import shap_reference as S  # noqa: E402
from oracle import gbdt_np as G  # noqa: E402


def case(model, X, background):
    S.add_counts(model, background)
    text = S.write_text_model_with_counts(model)
    parsed = S.parse_model(text)
    ld = S.tree_shap(parsed, X, np.longdouble)
    f64 = S.tree_shap(parsed, X, np.float64)
    phi = ld.astype(np.float64)
    dev_ref = float(np.abs(f64.astype(np.longdouble) - ld).max())
    resid = float(np.abs(phi.sum(1) - G.predict_raw(parsed, X)).max())
    return text, phi, dev_ref, resid


def main():
    assert np.finfo(np.longdouble).nmant >= 63, "needs an extended-precision long double"
    rng = np.random.RandomState(13)
    out = {}
    X = rng.randn(8, 50).astype(np.float32)
    X[0, ::7] = np.nan
    X[1, ::5] = 0.0
    X[2, 3] = np.nan
    out["large"] = (S.mixed_forest(40, 63, 50, seed=31), X, rng.randn(4000, 50))
    Xc = rng.randn(6, 50).astype(np.float32)
    Xc[0, ::9] = np.nan
    out["chain"] = (S.chain_forest(4, 63, 50, seed=32), Xc, rng.randn(4000, 50))
    arrays = {}
    for name, (model, X, bg) in out.items():
        text, phi, dev_ref, resid = case(model, X, bg)
        print(f"{name}: max|phi| {np.abs(phi).max():.4g}  dev_ref {dev_ref:.3g}  resid {resid:.3g}  text {len(text)} B")
        arrays[f"text_{name}"] = np.frombuffer(text.encode(), dtype=np.uint8)
        arrays[f"X_{name}"] = X
        arrays[f"phi_{name}"] = phi
        arrays[f"dev_ref_{name}"] = np.float64(dev_ref)
        arrays[f"resid_{name}"] = np.float64(resid)
    path = ROOT / "tests" / "golden" / "g13_contrib.npz"
    np.savez_compressed(path, **arrays)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
