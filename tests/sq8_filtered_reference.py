"""NumPy restatement of the SQ8 index's filtered search, written from the specification (recommendit_hip.h at
rihip_sq8_filter_*), not from the kernels.  The integer search is sq8_reference's, restricted to the rows that pass; the
thresholded pass's re-do rule is sq8_reference._redo_state applied to the passing rows and the passing sampled rows only,
because a failing row enters neither the sample nor the survivors."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sq8_reference as S  # noqa: E402


def words(preds, nq):
    """a 3-tuple shared by the batch, or [nq, 3] -> uint32 [nq, 3]"""
    a = np.asarray(preds, dtype=np.int64) & 0xFFFFFFFF
    if a.shape == (3,):
        a = np.tile(a, (nq, 1))
    assert a.shape == (nq, 3)
    return a.astype(np.uint32)


def passes(tags, preds):
    """bool [nq, N]: (any_of == 0 or tag & any_of) and tag & all_of == all_of and tag & none_of == 0"""
    t = np.asarray(tags, dtype=np.uint32)[None, :]
    p = np.asarray(preds, dtype=np.uint32)
    any_of, all_of, none_of = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    return ((any_of == 0) | ((t & any_of) != 0)) & ((t & all_of) == all_of) & ((t & none_of) == 0)


def probed_mask(assign, probes, nlist):
    """bool [nq, N]: the rows of each query's probed lists"""
    on = np.zeros((probes.shape[0], nlist), dtype=bool)
    np.put_along_axis(on, probes, True, axis=1)
    return on[:, np.asarray(assign)]


def thresholded_redo(Sc, k, assign, probes, nlist, ok):
    """int8 [nq] of S.REDO / S.KEPT / S.EITHER for a filtered thresholded pass.  assign int [N] (a flat index: zeros,
    nlist = 1, probes = zeros [nq, 1]); ok bool [nq, N]: the rows that pass.  Rank and cap are the plain search's (they
    depend on k and the list lengths, not on tags); the sample is every 16th tile of each probed list BY POSITION in the
    list, of which only the passing rows count"""
    nq, N = Sc.shape
    assign = np.asarray(assign)
    list_lens = np.bincount(assign, minlength=nlist)
    rank, cap = S.threshold_rank(k), S.threshold_cap(k, list_lens, probes.shape[1])
    rows_of = [np.nonzero(assign == l)[0] for l in range(nlist)]
    samp_of = [r[(np.arange(len(r)) // S.TILE) % S.SAMPLE_STEP == 0] for r in rows_of]
    out = np.empty(nq, dtype=np.int8)
    for q in range(nq):
        probed = np.concatenate([rows_of[l] for l in probes[q]])
        samp = np.concatenate([samp_of[l] for l in probes[q]])
        probed, samp = probed[ok[q, probed]], samp[ok[q, samp]]
        out[q] = S._redo_state(Sc[q, probed], Sc[q, samp], rank, cap, k)
    return out
