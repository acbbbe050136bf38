"""CPU: the host skew detector (recommendit_amd.metrics.kl_divergence_bins / detect_training_serving_skew) against the
G11 outputs of the reference's own functions (tools/make_golden_g11.py): KL to 1e-14 relative, result dicts equal in
keys, key order, flagged features, skew_detected and n_features_checked; plus the reference's two tests restated."""
import json
import math
import warnings

import numpy as np
import pandas as pd

from recommendit_amd import metrics as M


def load_g11(golden_dir):
    """-> list of cases; detect cases carry DataFrames "train" / "serving", kl cases arrays "p" / "q" """
    z = np.load(golden_dir / "g11_skew.npz")
    cases = json.loads(str(z["meta"]))
    for i, c in enumerate(cases):
        if c["kind"] == "detect":
            c["train"] = pd.DataFrame({n: z[f"c{i}_a_{j}"] for j, n in enumerate(c["a_cols"])})
            c["serving"] = pd.DataFrame({n: z[f"c{i}_b_{j}"] for j, n in enumerate(c["b_cols"])})
        else:
            c["p"], c["q"] = z[f"c{i}_a_0"], z[f"c{i}_b_0"]
    return cases


def close(got, want, rel):
    if want is None or (isinstance(want, float) and math.isnan(want)):
        return isinstance(got, float) and math.isnan(got)
    return abs(got - want) <= rel * max(abs(want), 1e-300)


def assert_skew_dict(got, ref, rounded_tol=0.0, raw=None):
    """ref: list of (key, value) pairs from the fixture"""
    ref = dict(ref)
    assert list(got) == ["feature_kl", "flagged_features", "max_kl", "skew_detected", "threshold", "n_features_checked"]
    assert list(got["feature_kl"]) == list(ref["feature_kl"])
    for col, want in ref["feature_kl"].items():
        v = got["feature_kl"][col]
        if isinstance(want, float) and math.isnan(want):
            assert math.isnan(v), col
        elif v != want:
            # a rounded value may move by one unit of 1e-6 only where the unrounded value sits on a rounding boundary
            assert rounded_tol and abs(v - want) <= rounded_tol * 1.0000001, (col, v, want)
            r = raw[col]
            assert abs(r * 1e6 - math.floor(r * 1e6) - 0.5) < 1e-6, (col, r)
    assert got["flagged_features"] == ref["flagged_features"]
    assert got["skew_detected"] == ref["skew_detected"]
    assert got["n_features_checked"] == ref["n_features_checked"]
    assert got["threshold"] == ref["threshold"]
    mk, wk = got["max_kl"], ref["max_kl"]
    assert (isinstance(wk, float) and math.isnan(wk) and math.isnan(mk)) or abs(mk - wk) <= rounded_tol * 1.0000001


def test_g11_fixture_shape(golden_dir):
    cases = load_g11(golden_dir)
    assert len(cases) >= 20
    kinds = {c["kind"] for c in cases}
    assert kinds == {"detect", "kl"}
    assert {c["n_bins"] for c in cases if c["kind"] == "kl"} >= {1, 7, 20, 128}


def test_g11_host_matches_reference(golden_dir):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in load_g11(golden_dir):
            if c["kind"] == "kl":
                got = M.kl_divergence_bins(c["p"], c["q"], n_bins=c["n_bins"], epsilon=c["epsilon"])
                assert close(got, c["kl"], 1e-14), (c["name"], got, c["kl"])
                continue
            raw = dict(c["raw_kl"])
            for col, want in raw.items():
                got = M.kl_divergence_bins(c["train"][col].dropna().values.astype(float),
                                           c["serving"][col].dropna().values.astype(float))
                assert close(got, want, 1e-14), (c["name"], col, got, want)
            res = M.detect_training_serving_skew(c["train"], c["serving"], threshold=c["threshold"],
                                                 numeric_cols=c["numeric_cols"])
            assert_skew_dict(res, c["result"])


def test_column_choice_skips_bool_and_text_keeps_int():
    tr = pd.DataFrame({"b": [True, False] * 10, "i": np.arange(20), "s": ["x"] * 20, "f": np.linspace(0, 1, 20),
                       "only_train": np.zeros(20)})
    sv = pd.DataFrame({"f": np.linspace(0, 2, 15), "i": np.arange(15), "b": [True] * 15, "s": ["y"] * 15})
    assert M.skew_columns(tr.select_dtypes(include=[np.number]).columns, sv.columns) == ["i", "f"]
    res = M.detect_training_serving_skew(tr, sv)
    assert list(res["feature_kl"]) == ["i", "f"]


def test_skew_detection_no_skew():
    np.random.seed(0)
    train = pd.DataFrame({"x": np.random.normal(0, 1, 1000)})
    serving = pd.DataFrame({"x": np.random.normal(0, 1, 500)})
    result = M.detect_training_serving_skew(train, serving, threshold=0.5)
    assert not result["skew_detected"]


def test_skew_detection_with_skew():
    np.random.seed(0)
    train = pd.DataFrame({"x": np.random.normal(0, 1, 1000)})
    serving = pd.DataFrame({"x": np.random.normal(5, 1, 500)})
    result = M.detect_training_serving_skew(train, serving, threshold=0.1)
    assert result["skew_detected"]
    assert "x" in result["flagged_features"]
