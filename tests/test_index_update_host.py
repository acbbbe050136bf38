"""CPU: the host-side parts of the live-catalogue update of FAISSIndex -- list_stats arithmetic, the lazily rebuilt
{item id: row} dict, the binding of the two new exports."""
import numpy as np
import pytest


def test_list_stats_arithmetic():
    from recommendit_amd.faiss_index import _list_stats
    st = _list_stats(np.array([4, 0, 2, 2]))
    assert st == {"n_lists": 4, "min": 0, "max": 4, "mean": 2.0, "empty": 1, "imbalance": 4 * 24 / 64}
    even = _list_stats(np.full(100, 10000))
    assert even["imbalance"] == 1.0 and even["empty"] == 0 and even["mean"] == 10000.0
    one = _list_stats(np.array([0, 0, 0, 9]))                      # everything in one of four lists: faiss gives nlist
    assert one["imbalance"] == 4.0 and one["empty"] == 3 and (one["min"], one["max"]) == (0, 9)
    big = _list_stats(np.array([3_000_000_000, 3_000_000_000]))   # squares beyond int64 stay exact
    assert big["imbalance"] == 1.0
    assert _list_stats(np.zeros(3, dtype=np.int64))["imbalance"] == 0.0


def test_id_to_row_dict_is_a_plain_dict_until_an_update_marks_it_stale():
    from recommendit_amd import FAISSIndex
    idx = FAISSIndex(embed_dim=8)
    assert idx._item_id_to_faiss_idx == {} and not idx._id_map_stale
    d = {5: 0, 9: 1}
    idx._item_id_to_faiss_idx = d
    assert idx._item_id_to_faiss_idx is d                          # after a build or load: the very dict that was set
    idx.item_ids = np.array([9, 7, 5], dtype=np.int64)             # what an update leaves: new ids, stale dict
    idx._id_map_stale = True
    assert idx._id_map is d                                        # nothing was rebuilt yet
    got = idx._item_id_to_faiss_idx                                # first read rebuilds from item_ids
    assert got == {9: 0, 7: 1, 5: 2} and not idx._id_map_stale
    assert all(type(k) is int and type(v) is int for k, v in got.items())
    assert idx._item_id_to_faiss_idx is got                        # and only once
    idx._id_map_stale = True
    idx._item_id_to_faiss_idx = {1: 0}                             # the setter clears the mark
    assert not idx._id_map_stale and idx._item_id_to_faiss_idx == {1: 0}


def test_stats_keeps_its_keys_and_updates_need_a_built_index():
    from recommendit_amd import FAISSIndex
    idx = FAISSIndex(embed_dim=8)
    assert idx.stats() == {"status": "not built"}
    x = np.zeros((1, 8), dtype=np.float32)
    for call in (lambda: idx.add_items(x, [1]), lambda: idx.remove_items([1]), lambda: idx.update_items(x, [1]),
                 lambda: idx.list_stats()):
        with pytest.raises(RuntimeError, match="Index not built."):
            call()


def test_update_entry_points_are_bound():
    from recommendit_amd import _lib
    l = _lib.lib()
    assert l.rihip_ip_index_update.argtypes == _lib.SIGNATURES["rihip_ip_index_update"][1]
    assert len(_lib.SIGNATURES["rihip_ip_index_update"][1]) == 13
    assert l.rihip_ip_index_list_sizes.restype is _lib.C.c_int
    assert l.rihip_abi_version() == 1
