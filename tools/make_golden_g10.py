#!/usr/bin/env python3
"""G10: the reference's full evaluation report (src/evaluation/metrics.py: evaluate_model :301-384 and the component
functions it calls) on ~30 small seeded cases -> tests/golden/g10_evaluate_model.json.

Runs only where the reference tree is present: its metrics module (numpy + pandas only) is loaded by file path and
called unmodified; nothing of it is copied, only its outputs are recorded.  The cases cover duplicates in the
recommendations and in the ground truth, empty and missing ground truth, k beyond the list, unsorted k_values,
catalog_size None / 0, items without a vector and zero vectors.
Usage: python tools/make_golden_g10.py [reference_root] [out_json]
"""
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
REF = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("/root/reference")
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "tests" / "golden" / "g10_evaluate_model.json"


def load_reference_metrics():
    spec = importlib.util.spec_from_file_location("ref_metrics", REF / "src" / "evaluation" / "metrics.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(seed: int):
    rng = np.random.default_rng(seed)
    n_items = int(rng.integers(5, 40))
    n_users = int(rng.integers(1, 9))
    recs, truth = {}, {}
    for u in range(n_users):
        uid = int(rng.integers(0, 1000))
        if uid in recs:
            continue
        ln = int(rng.integers(0, 25))
        recs[uid] = [int(x) for x in rng.integers(0, n_items, ln)]          # duplicates happen
        t = int(rng.integers(0, 5))
        if t == 0:
            continue                                                         # no ground truth at all
        if t == 1:
            truth[uid] = []                                                  # empty ground truth
        else:
            truth[uid] = [int(x) for x in rng.integers(0, n_items, int(rng.integers(1, 8)))]
    truth[5000 + seed] = [1, 2]                                              # a truth-only user: ignored
    ks = [int(x) for x in rng.choice([0, 1, 2, 3, 5, 7, 10, 20, 30], size=int(rng.integers(1, 5)), replace=False)]
    catalog = [None, 0, n_items, 3 * n_items][seed % 4]
    vecs, vec_dtype = None, "float32"
    if seed % 3 != 2:
        g = int(rng.choice([3, 18, 5]))
        vecs = {}
        for i in range(n_items):
            r = rng.random()
            if r < 0.2:
                continue                                                     # no vector for this item
            if r < 0.3:
                vecs[i] = [0.0] * g                                          # zero vector
            else:
                vecs[i] = [float(x) for x in (rng.random(g) < 0.4).astype(np.float32)] if seed % 2 \
                    else [float(np.float32(x)) for x in rng.standard_normal(g)]
        if seed % 5 == 4:
            vec_dtype = "float64"
    return {"seed": seed, "recs": [[u, r] for u, r in recs.items()], "truth": [[u, t] for u, t in truth.items()],
            "k_values": ks, "catalog_size": catalog, "vectors": None if vecs is None else [[i, v] for i, v in vecs.items()],
            "vec_dtype": vec_dtype}


def run(M, case):
    recs = {u: r for u, r in case["recs"]}
    truth = {u: t for u, t in case["truth"]}
    vecs = None
    if case["vectors"] is not None:
        vecs = {i: np.asarray(v, dtype=case["vec_dtype"]) for i, v in case["vectors"]}
    report = M.evaluate_model(recs, truth, case["k_values"], catalog_size=case["catalog_size"], item_genre_vectors=vecs)
    rng = np.random.default_rng(case["seed"] + 100)
    comps = []
    for u, r in case["recs"]:
        rel = truth.get(u, [])
        grades = {int(i): float(rng.integers(0, 4)) for i in set(rel)}
        row = {"user": u, "per_k": [], "mrr": M.mrr(r, rel), "ap": M.average_precision(r, rel),
               "grades": [[i, s] for i, s in grades.items()]}
        for k in case["k_values"]:
            row["per_k"].append({"k": k, "ndcg": M.ndcg_at_k(r, rel, k), "recall": M.recall_at_k(r, rel, k),
                                 "precision": M.precision_at_k(r, rel, k),
                                 "ndcg_graded": M.ndcg_at_k(r, rel, k, relevance_scores=grades)})
        if vecs is not None:
            row["ild"] = float(M.intra_list_diversity(r[:case["k_values"][-1]], vecs))
        comps.append(row)
    cov = M.coverage([r for _, r in case["recs"]], case["catalog_size"]) if case["catalog_size"] is not None else None
    return {"report": [[k, v] for k, v in report.items()], "components": comps, "coverage_all": cov}


def main():
    M = load_reference_metrics()
    cases = []
    # the worked example: float64 / list vectors, an empty-truth user, catalog 10
    ex = {"seed": -1, "recs": [[1, [1, 2, 3]], [2, [9, 8, 7]], [3, [5]]], "truth": [[1, [1]], [2, [7]], [3, []]],
          "k_values": [1, 3], "catalog_size": 10, "vectors": [[1, [1.0, 1.0, 1.0]], [2, [1.0, 0.0, 0.0]]],
          "vec_dtype": "float64"}
    cases.append(ex)
    # duplicates on both sides, k beyond the list, unsorted k, last k smaller than the others
    cases.append({"seed": -2, "recs": [[7, [4, 4, 2, 9, 4, 1]], [8, [3, 3, 3]], [9, []]],
                  "truth": [[7, [4, 4, 1, 1, 6]], [8, [3]], [9, [2]]], "k_values": [10, 2, 4], "catalog_size": 12,
                  "vectors": [[4, [1.0, 0.0]], [2, [0.0, 0.0]], [9, [0.5, 0.5]], [1, [2.0, 1.0]], [3, [1.0, 1.0]]],
                  "vec_dtype": "float32"})
    cases.append({"seed": -3, "recs": [], "truth": [[1, [1]]], "k_values": [5], "catalog_size": 3, "vectors": None,
                  "vec_dtype": "float32"})
    for s in range(28):
        cases.append(make_case(s))
    out = []
    for c in cases:
        c = dict(c)
        c.update(run(M, c))
        out.append(c)
    OUT.write_text(json.dumps(out, separators=(",", ":")))
    print(f"{len(out)} cases -> {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
