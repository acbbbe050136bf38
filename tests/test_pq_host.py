"""Host: the product quantiser's NumPy restatement (tests/pq_reference.py) alone, on a fixed clustered fixture -- the
properties the specification states -- plus the argument checks of PQIndex that need no device and the C ABI's
declarations."""
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pq_reference as P  # noqa: E402
import sq8_reference as S  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
ABI = ["from_ip_index", "dims", "get_codes", "get_codebooks", "train_stats", "save", "load"]


def clustered_codes(n=2000, du=40, centres=40, seed=11):
    """SQ8 codes [n, dpad] of n rows drawn around `centres` centres, original row order"""
    rng = np.random.default_rng(seed)
    Cc = rng.standard_normal((centres, du)).astype(np.float32)
    X = (Cc[rng.integers(0, centres, n)] + 0.15 * rng.standard_normal((n, du))).astype(np.float32)
    m, s = S.train_quantizer(X)
    return P.pad_codes(S.encode(X, m, s), P.dpad_of(du))


@pytest.fixture(scope="module")
def fixture_codes():
    return clustered_codes()


@pytest.mark.parametrize("dsub", [8, 16])
def test_training_lowers_the_distortion_and_decodes_in_range(fixture_codes, dsub):
    c = fixture_codes
    book, codes, trace = P.train(c, dsub, 5)
    assert trace.shape == (6,) and trace.dtype == np.int64
    assert trace[-1] < trace[0], trace
    assert (np.diff(trace) <= 0).sum() >= 4          # Lloyd steps with rounded means: all but at most one step go down
    dec = P.decode(codes, book)
    assert dec.dtype == np.int8 and dec.shape == c.shape
    assert dec.min() >= -127 and dec.max() <= 127 and book.min() >= -127
    # a sub-space wholly in the padding columns (du = 40, dpad = 64): its codes are all 0 and every row takes entry 0
    pad_m = [m for m in range(c.shape[1] // dsub) if m * dsub >= 40]
    assert pad_m and all((codes[:, m] == 0).all() and (book[m] == 0).all() for m in pad_m)
    # the stored distortion is the decoded matrix's squared error
    assert trace[-1] == int(((c.astype(np.int64) - dec.astype(np.int64)) ** 2).sum())


def test_ties_go_to_the_lowest_entry():
    dsub = 8
    c = np.zeros((3, 64), dtype=np.int8)
    c[0, :8] = 5
    c[1, :8] = [1, 0, 0, 0, 0, 0, 0, 0]
    c[2, :8] = 100
    book = np.full((8, 256, dsub), 90, dtype=np.int8)
    book[0, 9] = 5; book[0, 4] = 5; book[0, 200] = 5             # three copies of row 0's sub-vector
    book[0, 17] = [2, 0, 0, 0, 0, 0, 0, 0]; book[0, 12] = 0      # row 1 is at distance 1 from both
    codes, dist = P.assign(c, book)
    assert codes[0, 0] == 4 and codes[1, 0] == 12 and codes[2, 0] == 0
    # every other sub-space: all entries equal, so entry 0
    assert (codes[:, 1:] == 0).all()
    D = sum(int(((c[i, m * 8:(m + 1) * 8].astype(np.int64) - book[m, codes[i, m]].astype(np.int64)) ** 2).sum())
            for i in range(3) for m in range(8))
    assert dist == D


def test_an_entry_without_rows_keeps_its_value_and_100_rows_build():
    c = clustered_codes(n=100, du=64, centres=7, seed=3)
    assert c.shape == (100, 64)
    for dsub in (8, 16):
        book0 = P.init_book(c, dsub)
        rows = (np.arange(256) * 100) // 256
        assert len(set(rows.tolist())) == 100                     # every row seeds an entry, 156 entries are repeats
        codes, _ = P.assign(c, book0)
        first = np.array([np.nonzero(rows == r)[0][0] for r in range(100)])
        # a row is its own entry at distance 0 (or an earlier identical one): never a later repeat
        assert (codes <= first[:, None]).all()
        book1 = P.lloyd_step(c, codes, book0)
        for m in range(book0.shape[0]):
            empty = np.bincount(codes[:, m], minlength=256) == 0
            assert empty.sum() >= 156
            np.testing.assert_array_equal(book1[m][empty], book0[m][empty])
        book, codes, trace = P.train(c, dsub, 3)
        assert trace.shape == (4,) and trace[-1] <= trace[0]
        assert np.abs(P.decode(codes, book).astype(np.int32)).max() <= 127


def test_lloyd_mean_rounds_half_to_even_and_clamps():
    c = np.zeros((4, 64), dtype=np.int8)
    c[:, 0] = [1, 2, -127, -127]          # entry 0: rows 0, 1 -> 1.5 -> 2; entry 1: rows 2, 3 -> -127
    c[:, 1] = [0, 1, 3, 4]                # 0.5 -> 0; 3.5 -> 4
    codes = np.zeros((4, 8), dtype=np.uint8)
    codes[2:, 0] = 1
    book = np.full((8, 256, 8), 7, dtype=np.int8)
    new = P.lloyd_step(c, codes, book)
    assert new[0, 0, 0] == 2 and new[0, 0, 1] == 0 and new[0, 1, 0] == -127 and new[0, 1, 1] == 4
    assert (new[0, 2:] == 7).all()


def test_argument_checks_need_no_device():
    from recommendit_amd import FAISSIndex, PQIndex, SQ8Index
    assert issubclass(PQIndex, SQ8Index)
    with pytest.raises(ValueError):
        PQIndex.from_index("not an index")
    with pytest.raises(RuntimeError):
        PQIndex.from_index(FAISSIndex(embed_dim=32, exact=True))
    idx = PQIndex(embed_dim=32)
    for call in (lambda: idx.add_items(np.zeros((1, 32), np.float32), [1]), lambda: idx.remove_items([1]),
                 lambda: idx.update_items(np.zeros((1, 32), np.float32), [1])):
        with pytest.raises(NotImplementedError, match="rebuild"):
            call()
    assert idx.stats() == {"status": "not built"}


def test_the_header_declares_the_pq_abi_and_the_loader_binds_it():
    hdr = (ROOT / "include" / "recommendit_hip.h").read_text()
    lib = (ROOT / "recommendit_amd" / "_lib.py").read_text()
    src = (ROOT / "recommendit_amd" / "csrc" / "pq.hip").read_text()
    for name in ABI:
        fn = f"rihip_pq_index_{name}"
        assert re.search(rf"\bint {fn}\(", hdr), fn
        assert f'"{fn}"' in lib, fn
        assert re.search(rf'extern "C" int {fn}\(', src), fn
    assert "pq.hip" in (ROOT / "recommendit_amd" / "csrc" / "Makefile").read_text()
