"""CPU: the ranking-feature oracle against the outputs of the reference's own _build_ranking_features (G8)."""
import json

import numpy as np

from oracle import ranking_features_np as RF


def load_g8(golden_dir):
    g = np.load(golden_dir / "g8_ranking_features.npz")
    meta = json.loads((golden_dir / "g8_inputs.json").read_text())
    return g, meta


def test_g8_columns_and_values(golden_dir):
    g, meta = load_g8(golden_dir)
    for m in meta:
        s = m["seed"]
        items = {int(k): v for k, v in m["items"].items()}
        cols = RF.build_ranking_features(m["user"], items, m["cand"])
        ref_cols = [str(c) for c in g[f"s{s}_columns"]]
        assert list(cols.keys()) == ref_cols
        got = np.stack([cols[c] for c in ref_cols], axis=1)
        np.testing.assert_array_equal(got, g[f"s{s}_values"])   # Python-float arithmetic: bit-exact
    assert set(RF.feature_columns()) == set(ref_cols) - {"item_id"} and len(RF.feature_columns()) == 50


def test_vectorised_table_oracle_equals_the_per_row_restatement_bitwise():
    """RF.table_feature_matrix (the reference of the device kernels) against build_ranking_features / feature_matrix
    row by row, on 3 users x 120 candidates with general float64 table values (products and sums that round), absent
    entities, padding, and a ranker column order with unknown and repeated names."""
    rng = np.random.default_rng(8)
    n_u, n_i, kc = 7, 40, 120
    ut = rng.standard_normal((n_u, RF.USER_WIDTH)) * 3
    it = rng.standard_normal((n_i, RF.ITEM_WIDTH)) * 3
    ut[0, :6] = [d for _, d in RF.USER_SCALARS]; ut[0, 6:] = 0.0
    it[0, :5] = [d for _, d in RF.ITEM_SCALARS]; it[0, 5:] = 0.0
    it[5, 1] = 0.0                                      # popularity ratio divides by the bare 1e-8
    canon = RF.feature_columns()
    names = ["nope_a"] + list(rng.permutation(canon)) + ["nope_b", canon[13], canon[12]]
    names.insert(20, "nope_c")
    col_map = np.array([canon.index(c) if c in canon else -1 for c in names])
    user_ids = np.array([3, 0, 99])                     # 99: not in the store -> defaults
    cand = rng.integers(1, n_i + 6, size=(3, kc))       # ids >= n_i: not in the store -> defaults
    cand[:, 5] = 5
    got = RF.table_feature_matrix(ut, it, user_ids, cand, col_map)
    assert got.dtype == np.float32 and got.shape == (3 * kc, len(names))

    def user_dict(u):
        if not 0 <= u < n_u:
            return {}
        d = {name: ut[u, j] for j, (name, _) in enumerate(RF.USER_SCALARS)}
        d["genre_pref"] = list(ut[u, 6:])
        return d

    def item_dict(i):
        if i >= n_i:
            return None
        d = {name: it[i, j] for j, (name, _) in enumerate(RF.ITEM_SCALARS)}
        d["genre_vector"] = list(it[i, 5:])
        return d

    for q, u in enumerate(user_ids):
        ids = [int(i) for i in cand[q]]
        cols = RF.build_ranking_features(user_dict(int(u)), {i: item_dict(i) for i in ids}, ids)
        ref = RF.feature_matrix(cols, names)
        np.testing.assert_array_equal(got[q * kc:(q + 1) * kc].view(np.uint32), ref.view(np.uint32))
    # padding: a row of zeros whatever the user
    cand[1, 7] = -1
    assert not RF.table_feature_matrix(ut, it, user_ids, cand, col_map)[kc + 7].any()
