"""NumPy restatement of the product quantiser: train, assign, decode and the distortion trace, written from the
specification (recommendit_hip.h at rihip_pq_index_*), not from the kernels.  Everything after the SQ8 code is integer
arithmetic (int64 here), the one division is a float64 division of two exactly representable integers and np.rint rounds
half to even, so every function is bit for bit what the specification asks for.

The input is the rows' SQ8 codes c int8 [N, dpad] in ORIGINAL row order, padding columns 0 (tests/sq8_reference.py's
encode() padded by pad_codes()).  Search expectations are not restated here: they are tests/sq8_reference.py's, applied
to decode()'s matrix."""
import numpy as np

ENTRIES = 256


def pad_codes(c, dpad):
    """int8 [N, du] -> int8 [N, dpad], padding columns 0"""
    out = np.zeros((c.shape[0], dpad), dtype=np.int8)
    out[:, :c.shape[1]] = c
    return out


def dpad_of(du):
    return 64 if du <= 64 else 128


def init_book(c, dsub):
    """book int8 [M, 256, dsub]: entry e of every sub-space is the sub-vector of original row (e N) // 256"""
    N, dpad = c.shape
    M = dpad // dsub
    rows = (np.arange(ENTRIES, dtype=np.int64) * np.int64(N)) // ENTRIES
    return np.ascontiguousarray(c[rows].reshape(ENTRIES, M, dsub).transpose(1, 0, 2))


def distances(c, book, m, chunk=1024):
    """yields (row slice, D int64 [rows, 256]) of sub-space m: D = sum_j (c - book)^2"""
    dsub = book.shape[2]
    sub = c[:, m * dsub:(m + 1) * dsub].astype(np.int64)
    b = book[m].astype(np.int64)
    for r0 in range(0, c.shape[0], chunk):
        diff = sub[r0:r0 + chunk, None, :] - b[None, :, :]
        yield slice(r0, r0 + chunk), (diff * diff).sum(axis=2)


def assign(c, book):
    """(codes uint8 [N, M], distortion int): the entry of the smallest D, the lowest entry on a tie"""
    N = c.shape[0]
    M = book.shape[0]
    codes = np.empty((N, M), dtype=np.uint8)
    total = 0
    for m in range(M):
        for rows, D in distances(c, book, m):
            e = np.argmin(D, axis=1)                 # the first of equal minima
            codes[rows, m] = e
            total += int(D[np.arange(D.shape[0]), e].sum())
    return codes, total


def lloyd_step(c, codes, book):
    """the codebooks after one step: clamp(rint(sum / cnt), +-127) per entry, an entry without rows as it was"""
    M, _, dsub = book.shape
    new = book.copy()
    for m in range(M):
        s = np.zeros((ENTRIES, dsub), dtype=np.int64)
        np.add.at(s, codes[:, m].astype(np.int64), c[:, m * dsub:(m + 1) * dsub].astype(np.int64))
        cnt = np.bincount(codes[:, m], minlength=ENTRIES).astype(np.int64)
        has = cnt > 0
        mean = np.rint(s[has].astype(np.float64) / cnt[has].astype(np.float64)[:, None])
        new[m][has] = np.clip(mean, -127, 127).astype(np.int8)
    return new


def train(c, dsub, n_iter):
    """(book int8 [M, 256, dsub], codes uint8 [N, M], trace int64 [n_iter + 1])"""
    book = init_book(c, dsub)
    trace = []
    for _ in range(n_iter):
        codes, dist = assign(c, book)
        trace.append(dist)
        book = lloyd_step(c, codes, book)
    codes, dist = assign(c, book)
    trace.append(dist)
    return book, codes, np.array(trace, dtype=np.int64)


def decode(codes, book):
    """int8 [N, dpad]: column m dsub + j of row i is book[m][codes[i][m]][j]"""
    M, _, dsub = book.shape
    out = np.empty((codes.shape[0], M * dsub), dtype=np.int8)
    for m in range(M):
        out[:, m * dsub:(m + 1) * dsub] = book[m][codes[:, m]]
    return out


# ---- additions for tests/test_gpu_pq_paths.py: a faster exact trainer and the Lloyd step's sums ---------------------------
def assign_blas(c, book):
    """assign() through float64 matmuls: D = |c|^2 + |b|^2 - 2 <c, b>, every term an integer below 2^22, so each D is the
    same integer in any summation order; the first of equal minima, as assign()"""
    N = c.shape[0]
    M, _, dsub = book.shape
    codes = np.empty((N, M), dtype=np.uint8)
    total = 0
    rows = np.arange(N)
    for m in range(M):
        sub = c[:, m * dsub:(m + 1) * dsub].astype(np.float64)
        b = book[m].astype(np.float64)
        D = (sub * sub).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] - 2.0 * (sub @ b.T)
        assert (D == np.rint(D)).all() and D.min() >= 0
        e = np.argmin(D, axis=1)
        codes[:, m] = e
        total += int(D[rows, e].astype(np.int64).sum())
    return codes, total


def train_blas(c, dsub, n_iter):
    """train() with assign_blas in place of assign: the same three results"""
    book = init_book(c, dsub)
    trace = []
    for _ in range(n_iter):
        codes, dist = assign_blas(c, book)
        trace.append(dist)
        book = lloyd_step(c, codes, book)
    codes, dist = assign_blas(c, book)
    trace.append(dist)
    return book, codes, np.array(trace, dtype=np.int64)


def entry_sums(c, codes, m, dsub):
    """(sum int64 [256, dsub], cnt int64 [256]) of sub-space m over the rows given: what lloyd_step divides (all rows), or
    the partial sums of one block of rows"""
    s = np.zeros((ENTRIES, dsub), dtype=np.int64)
    np.add.at(s, codes[:, m].astype(np.int64), c[:, m * dsub:(m + 1) * dsub].astype(np.int64))
    return s, np.bincount(codes[:, m], minlength=ENTRIES).astype(np.int64)
