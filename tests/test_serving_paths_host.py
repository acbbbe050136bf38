"""CPU: the forests of tests/test_gpu_serving_kernels.py take the kernels their tests assert, by a host restatement
(oracle.gbdt_np.predict_plan) of the chunk and record arithmetic of csrc/gbdt.hip -- so a shape that no longer reaches
its kernel is noticed without a GPU -- and the restatement's constants are the library's."""
import re
from pathlib import Path

import numpy as np

from oracle import gbdt_np as G

ROOT = Path(__file__).resolve().parent.parent


def test_plan_constants_are_the_librarys():
    src = (ROOT / "recommendit_amd" / "csrc" / "gbdt.hip").read_text()
    for name in ("N8_CAP", "L8_CAP", "T8_CAP", "R_CAP", "NODE_CAP", "LEAF_CAP"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == getattr(G, name), name
    assert f"ct >= {G.T_CAP})" in src


def test_forest_cases_take_the_kernels_they_name():
    from tests.test_gpu_serving_kernels import FOREST_CASES, expected_paths
    cases = expected_paths()
    assert list(cases) == FOREST_CASES
    plans = {}
    for name, (model, path) in cases.items():
        plans[name] = G.predict_plan(model)
        assert plans[name]["path"] == path, (name, plans[name])
    assert {p for _, p in cases.values()} == {0, 1, 2, 3}
    # the shapes the cases were chosen for
    for name in ("simple8_32x65", "simple8_40x65"):                      # one chunk over the record cap is enough
        assert plans[name]["records"][0] == 32 * 130 == G.R_CAP + 64 and plans[name]["chunks"][1] == 32
    assert plans["walk_record_cap"]["records"] == [G.R_CAP, G.R_CAP]
    assert plans["global_memory"]["chunks"] == [0, 1, 2, 12] and plans["global_memory_reversed"]["chunks"] == [0, 10, 11, 12]
    sizes = [t["num_leaves"] for t in cases["global_memory"][0]["trees"]]
    assert sizes == [1300, 1600] + [31] * 10 and sizes[0] - 1 > G.NODE_CAP and sizes[1] > G.LEAF_CAP
    assert len(plans["missing8_striding"]["chunks"]) - 1 == 13
    for name in ("one_leaf_path_0", "one_leaf_path_1", "one_leaf_path_3"):
        leaves = [t["num_leaves"] for t in cases[name][0]["trees"]]
        assert leaves[0] == leaves[-1] == 1 and leaves.count(1) == 3 and 1 < leaves.index(1, 1) < len(leaves) - 2
    cat = cases["categorical"][0]["trees"]
    assert [t["num_cat"] for t in cat] == [3, 0, 0] * 3
    assert all(np.diff(t["cat_boundaries"]).tolist() == [1, 2, 5] for t in cat[::3])
    assert set(cat[3]["decision_type"].tolist()) == {1, 4, 6, 8, 10}
    assert cases["average_path_0"][0]["average_output"] and cases["average_path_3"][0]["average_output"]


def test_average_output_header_round_trips():
    model = G.random_forest_model(3, 4, 2, seed=1)
    assert "average_output" not in G.write_text_model(model)
    text = G.write_text_model(model, average_output=True)
    assert "\naverage_output\n" in text and G.parse_text_model(text)["average_output"]
    X = np.array([[0.1, -0.2], [2.0, 0.5]], np.float32)
    np.testing.assert_array_equal(G.predict_raw(G.parse_text_model(text), X), G.predict_raw(model, X) / 3)
    s, a = G.predict_raw(model, X, return_abs=True)
    assert (a >= np.abs(s)).all()
