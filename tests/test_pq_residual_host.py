"""Host: the residual product quantiser's NumPy restatement (tests/pq_residual_reference.py) alone -- the properties the
specification states -- plus the argument checks of PQIndex.from_index(by_residual=) that need no device and the C ABI's
declarations."""
import os
import re
import sys
import types
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_reference as P  # noqa: E402
import pq_residual_reference as PR  # noqa: E402
import sq8_reference as S  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
ABI = ["from_ip_index_residual", "is_residual", "get_list_codes", "get_decoded16", "residual_clamped", "load_residual"]


def _fixture(du=64, nlist=8, n=2000, seed=5):
    X, C, assign = PR.clustered(seed, n, du, nlist)
    m, s = S.train_quantizer(X)
    dpad = P.dpad_of(du)
    return dict(X=X, C=C, assign=assign, m=m, s=s, c=P.pad_codes(S.encode(X, m, s), dpad), K=PR.list_codes(C, m, s, dpad))


@pytest.fixture(scope="module")
def clustered_case():
    return _fixture()


def test_argument_checks_and_the_flat_source_refusal_need_no_device(monkeypatch):
    import inspect
    from recommendit_amd import FAISSIndex, PQIndex
    assert inspect.signature(PQIndex.from_index).parameters["by_residual"].default is False
    with pytest.raises(ValueError):
        PQIndex.from_index("not an index", by_residual=True)
    with pytest.raises(RuntimeError):
        PQIndex.from_index(FAISSIndex(embed_dim=32, exact=True), by_residual=True)
    # a source that looks built (no device call is reached before the checks below)
    src = FAISSIndex(embed_dim=32, exact=True)
    src.index = types.SimpleNamespace(is_ivf=False, _h=None)
    monkeypatch.setattr(src, "search_pending", lambda: False)
    with pytest.raises(ValueError, match="by_residual"):
        PQIndex.from_index(src, by_residual=1)
    with pytest.raises(ValueError, match="IVF"):
        PQIndex.from_index(src, by_residual=True)
    idx = PQIndex(embed_dim=32)
    assert idx.by_residual is False and idx.stats() == {"status": "not built"}
    with pytest.raises(RuntimeError):
        idx.list_codes()
    for call in (lambda: idx.add_items(np.zeros((1, 32), np.float32), [1]), lambda: idx.remove_items([1])):
        with pytest.raises(NotImplementedError, match="rebuild"):
            call()


@pytest.mark.parametrize("dsub", [8, 16])
def test_all_zero_list_codes_give_the_plain_quantiser_bit_for_bit(clustered_case, dsub):
    c, assign = clustered_case["c"], clustered_case["assign"]
    K0 = np.zeros_like(clustered_case["K"])
    r, clamped = PR.residuals(c, K0, assign)
    assert clamped == 0 and r.tobytes() == c.tobytes()
    book, codes, trace, clamped = PR.train(c, K0, assign, dsub, 3)
    pb, pc, pt = P.train(c, dsub, 3)
    assert book.tobytes() == pb.tobytes() and codes.tobytes() == pc.tobytes() and trace.tobytes() == pt.tobytes()
    dec = PR.decode(codes, book, K0, assign)
    assert dec.dtype == np.int16
    np.testing.assert_array_equal(dec, P.decode(pc, pb).astype(np.int16))


@pytest.mark.parametrize("dsub", [8, 16])
def test_residual_distortion_is_below_the_plain_one_and_the_decoded_code_leaves_int8(clustered_case, dsub):
    cs = clustered_case
    c, K, assign = cs["c"], cs["K"], cs["assign"]
    assert np.abs(K.astype(np.int32)).max() <= 127 and (K[:, 64:] == 0).all()
    book, codes, trace, clamped = PR.train(c, K, assign, dsub, 5)
    _, _, plain = P.train(c, dsub, 5)
    print("dsub", dsub, "final distortion plain", int(plain[-1]), "residual", int(trace[-1]), "clamped", clamped)
    assert trace[-1] < plain[-1]
    dec = PR.decode(codes, book, K, assign)
    assert dec.dtype == np.int16 and np.abs(dec.astype(np.int32)).max() > 127      # genuinely 16-bit
    assert np.abs(dec.astype(np.int32)).max() <= PR.CODE_BOUND
    # the trace is the squared error against the RESIDUALS, and (no clamp) against the codes through the decoded matrix
    r, _ = PR.residuals(c, K, assign)
    assert trace[-1] == int(((r.astype(np.int64) - P.decode(codes, book).astype(np.int64)) ** 2).sum())
    if clamped == 0:
        assert trace[-1] == int(((c.astype(np.int64) - dec.astype(np.int64)) ** 2).sum())
    # the score splits as the scan forms it
    n, _, _ = S.encode_queries(cs["X"][:9], cs["m"], cs["s"])
    np.testing.assert_array_equal(PR.int_scores(n, dec), PR.split_scores(n, codes, book, K, assign))
    probes = np.array([[0, 3], [7, 7]] * 4 + [[1, 2]])
    T = PR.pair_offsets(n, K, probes)
    assert T.shape == (9, 2) and T[1, 0] == int(n[1].astype(np.int64) @ K[7, :64].astype(np.int64))


def test_the_residual_clamp_is_counted_and_clamps():
    c = np.zeros((3, 64), dtype=np.int8)
    c[0, :4] = [127, -127, 100, -5]
    c[1, :4] = [127, -127, 100, -5]
    K = np.zeros((2, 64), dtype=np.int8)
    K[1, :4] = [-127, 127, -28, 5]
    r, clamped = PR.residuals(c, K, np.array([0, 1, 1]))
    assert clamped == 3 and r.dtype == np.int8
    assert r[0, :4].tolist() == [127, -127, 100, -5] and r[1, :4].tolist() == [127, -127, 127, -10]
    assert r[2, :4].tolist() == [127, -127, 28, -5]


@pytest.mark.parametrize("dpad", [64, 128])
def test_the_score_extremes_do_not_wrap(dpad):
    K = np.full((1, dpad), 127, dtype=np.int8)
    book = np.zeros((dpad // 8, 256, 8), dtype=np.int8)
    book[:, 0], book[:, 1] = 127, -127
    codes = np.zeros((2, dpad // 8), dtype=np.uint8)
    dec = PR.decode(codes, book, K, np.zeros(2, dtype=np.int64))
    assert (dec == 254).all()
    dec[1] = PR.decode(codes + 1, book, -K, np.zeros(2, dtype=np.int64))[1]
    assert (dec[1] == -254).all()
    n = np.full((2, dpad), 32512, dtype=np.int32)
    n[1] = -32512
    Sc = PR.int_scores(n, dec)
    top = 32512 * 254 * dpad
    assert Sc.dtype == np.int64 and Sc.tolist() == [[top, -top], [-top, top]]
    assert PR.SCORE_BOUND == 1057030144 and PR.SCORE_BOUND < 2 ** 30 and (dpad < 128 or top == PR.SCORE_BOUND)
    # the candidate key's high word orders these as signed integers: (uint32)S ^ 0x80000000
    words = [(v & 0xFFFFFFFF) ^ 0x80000000 for v in (-top, 0, top)]
    assert words == sorted(words) and all(w != 0 for w in words)


def test_the_header_declares_the_residual_abi_and_the_loader_binds_it():
    hdr = (ROOT / "include" / "recommendit_hip.h").read_text()
    lib = (ROOT / "recommendit_amd" / "_lib.py").read_text()
    src = (ROOT / "recommendit_amd" / "csrc" / "pq.hip").read_text()
    for name in ABI:
        fn = f"rihip_pq_index_{name}"
        assert re.search(rf"\bint {fn}\(", hdr), fn
        assert f'"{fn}"' in lib, fn
        assert re.search(rf'extern "C" int {fn}\(', src), fn
