"""Simulated doublets restated from the definition alone: the draw of the parents on the NumPy Philox of
_thin_reference, the sum of a pair as a dict merge per row, Scrublet's score in NumPy.  The host restatement of the library
(schpf_debug_doublet_rows) and, through it, the kernels are held to this bit for bit.  Also what both doublet test files
share: the kernel matrix with its pairs, and the calls of the library."""
import ctypes

import numpy as np
from scipy.sparse import csr_matrix

from schpf_amd import _lib
from _thin_reference import KINDS, philox

PIECE = 64                      # entries of a parent a wavefront handles per pass (doublets.hip DOUBLET_PIECE)
LONG, LONGER = 300, 257         # the long rows: more than twice PIECE, and not a multiple of it
NGENES = 700
MESSAGES = {
    "indptr": "doublets: indptr must be 0 at row 0, must be non-decreasing and must end at nnz; offending row %d",
    "index": "doublets: column index out of range at entry %d",
    "order": "doublets: columns must be strictly ascending within a row; offending row %d",
    "value": "doublets: values must be integer counts in [0, 2^24]; offending entry %d",
    "parent": "doublets: parents must be in [0, ncells); offending pair %d",
}


def draw_parents(first, n_sim, ncells, seed):
    """(n_sim, 2) int32: the parents of the simulated rows first .. first + n_sim - 1 among ncells cells."""
    s = [first + t for t in range(n_sim)]
    lo = np.array([v & 0xFFFFFFFF for v in s], dtype=np.uint64)
    hi = np.array([v >> 32 for v in s], dtype=np.uint64)
    w = philox(lo, hi, np.zeros_like(lo), np.ones_like(lo), seed & 0xFFFFFFFF, seed >> 32)
    N = np.uint64(ncells)           # words < 2^32 and N < 2^31: the products stay below 2^63
    return np.stack([(w[0] * N) >> np.uint64(32), (w[1] * N) >> np.uint64(32)], axis=1).astype(np.int32)


def pair_sums(X, parents):
    """(indptr int64, indices int32, values int32) of the rows X[a] + X[b]: one entry per column stored in either parent,
    stored zeros included, columns ascending."""
    indptr, indices, values = [0], [], []
    for a, b in np.asarray(parents).reshape(-1, 2):
        row = {}
        for r in (int(a), int(b)):
            for e in range(X.indptr[r], X.indptr[r + 1]):
                row[int(X.indices[e])] = row.get(int(X.indices[e]), 0) + int(X.data[e])
        for c in sorted(row):
            indices.append(c)
            values.append(row[c])
        indptr.append(len(indices))
    return np.array(indptr, np.int64), np.array(indices, np.int32), np.array(values, np.int32)


def scrublet(k_sim, k_adj, r, rho=0.06, se_rho=0.02):
    k_sim = np.asarray(k_sim, dtype=np.float64)
    q = (k_sim + 1) / (k_adj + 2)
    d = 1 - rho - q * (1 - rho - rho / r)
    score = q * rho / r / d
    se_q = np.sqrt(q * (1 - q) / (k_adj + 3))
    return score, score / d * np.sqrt((se_q / q * (1 - rho)) ** 2 + (se_rho / rho * (1 - q)) ** 2)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma(a, b, c):
    """round(a * b + c) with ONE rounding, elementwise on float64 arrays, as std::fma gives it: the product as an unevaluated
    sum p + e (Dekker), then Boldo and Melquiond's emulation (2008) -- the two small terms are added with rounding to odd,
    the last addition rounds to nearest.  No overflow or underflow care: cell scores are of moderate size."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    p = a * b
    split = lambda x: (lambda t: (t - (t - x), x - (t - (t - x))))(x * 134217729.0)  # noqa: E731
    (ah, al), (bh, bl) = split(a), split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl          # a * b == p + e exactly
    s, t = _two_sum(p, c)                                      # p + c == s + t exactly
    u, v = _two_sum(t, e)                                      # t + e == u + v exactly; u to odd:
    bits = u.copy().view(np.int64)
    fix = (v != 0) & ((bits & 1) == 0)
    bits[fix] += np.where((v[fix] > 0) == (u[fix] > 0), 1, -1)
    return s + bits.view(np.float64)


def knn_counts(x, k, n_obs):
    """k_sim of every row of x by brute force under the key of DESIGN.md 16: d2 by subtraction and fma in factor order, the
    k smallest (d2, r) with the row itself left out, and how many of them are rows >= n_obs."""
    x = np.asarray(x, np.float64)
    d2 = np.zeros((x.shape[0], x.shape[0]))
    for f in range(x.shape[1]):
        d = x[:, None, f] - x[None, :, f]
        d2 = fma(d, d, d2)
    np.fill_diagonal(d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]       # stable: equal d2 by the smaller row
    return (order >= n_obs).sum(axis=1), order, np.take_along_axis(d2, order, axis=1)


def _row(rng, n, lo=0, hi=NGENES):
    return np.sort(rng.choice(np.arange(lo, hi), n, replace=False))


def kernel_matrix():
    """(X, parents): the smallest matrix on which the merge can go wrong, 80 x 700 canonical CSR with int32 counts, and 83
    pairs of its rows.  Rows: 0, 1 empty; 2, 3, 4, 5 of 1, 63, 64, 65 entries; 6 all even and 7 all odd columns (350 each);
    8, 9 the same 100 columns, one of them holding 2^24 in both; 10 below column 50 and 11 from column 600 on; 12 with stored
    zeros; 13 of LONG = 300 and 14 of LONGER = 257 entries -- a wavefront takes PIECE = 64 entries of a parent per pass, so
    both need more than four; 15 .. 79 random, 0 .. 120 entries."""
    rng = np.random.RandomState(20)
    shared = _row(rng, 100)
    cols = [np.zeros(0, np.int64), np.zeros(0, np.int64), _row(rng, 1), _row(rng, 63), _row(rng, 64), _row(rng, 65),
            np.arange(0, NGENES, 2), np.arange(1, NGENES, 2), shared, shared.copy(), _row(rng, 30, 0, 50),
            _row(rng, 70, 600, NGENES), _row(rng, 40), _row(rng, LONG), _row(rng, LONGER)]
    cols += [_row(rng, n) for n in rng.randint(0, 121, 80 - len(cols))]
    vals = [rng.randint(1, 41, len(c)).astype(np.int32) for c in cols]
    vals[8][17] = vals[9][17] = 2 ** 24             # the largest sum: 2^25
    vals[12][::3] = 0
    vals[13][5] = 0
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    X = csr_matrix((np.concatenate(vals), np.concatenate(cols).astype(np.int32), indptr), shape=(80, NGENES))
    fixed = [(0, 1), (13, 14), (0, 0), (0, 13), (13, 0), (13, 13), (5, 5), (6, 7), (7, 6), (8, 9), (14, 13), (3, 5), (5, 3),
             (10, 11), (11, 10), (12, 12), (12, 4), (2, 2), (2, 3), (6, 13),
             (3, 6), (6, 3), (2, 7)]         # 63 columns spread over a parent of 350: a window past the in-register search
    parents = np.concatenate([np.array(fixed), rng.randint(0, 80, (60, 2))]).astype(np.int32)
    return X, parents


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)


def call_rows(entry, X, parents, fill=True, short=0, device=None, val_dtype=None):
    """schpf_debug_doublet_rows (device=None) or schpf_doublet_rows on the arrays of the CSR X as they are: the sizing call,
    then (fill) the filling call with capacity = the total - short.  Returns (out_indptr, out_indices, out_values); the last
    two None without fill.  The output arrays start as -7."""
    lib = _lib.load()
    indptr = np.ascontiguousarray(X.indptr, np.int64)
    indices = np.ascontiguousarray(X.indices, np.int32)
    val = np.ascontiguousarray(X.data if val_dtype is None else X.data.astype(val_dtype))
    parents = np.ascontiguousarray(parents, np.int32).reshape(-1, 2)
    n_pairs = parents.shape[0]
    head = () if device is None else (device,)
    fn = getattr(lib, entry)
    args = head + (X.shape[0], X.shape[1], len(val), _p(indptr), _p(indices), _p(val), KINDS[val.dtype], n_pairs, _p(parents))
    out_indptr = np.full(n_pairs + 1, -7, np.int64)
    _lib.check(fn(*(args + (_p(out_indptr), None, None, 0))))
    if not fill:
        return out_indptr, None, None
    total = int(out_indptr[-1])
    again = np.full(n_pairs + 1, -7, np.int64)
    out_indices, out_values = np.full(max(total, 1), -7, np.int32), np.full(max(total, 1), -7, np.int32)
    _lib.check(fn(*(args + (_p(again), _p(out_indices), _p(out_values), total - short))))
    assert (again == out_indptr).all()
    return out_indptr, out_indices[:total], out_values[:total]


def debug_rows(X, parents, **kw):
    return call_rows("schpf_debug_doublet_rows", X, parents, **kw)


def host_parents(first, n_sim, ncells, seed):
    out = np.full((n_sim, 2), -7, np.int32)
    _lib.check(_lib.load().schpf_doublet_parents(first, n_sim, ncells, ctypes.c_uint64(seed), _p(out)))
    return out


def spoiled(kind):
    """(X, parents, message): the kernel matrix with two offenders of `kind`, the smaller one placed behind the larger
    one in memory order of the launch (a later wavefront finds the smaller one), and the message that names the smaller."""
    X, parents = kernel_matrix()
    X, parents = X.copy(), parents.copy()
    if kind == "indptr":
        X.indptr = X.indptr.astype(np.int64)
        X.indptr[70], X.indptr[30] = X.indptr[69] - 1, X.indptr[29] - 1       # rows 69 and 29 end before they start
        return X, parents, MESSAGES[kind] % 29
    if kind == "indptr_end":
        X.indptr = X.indptr.astype(np.int64)
        X.indptr[80] += 1
        return X, parents, MESSAGES["indptr"] % 80
    if kind == "index":
        late, early = int(X.indptr[60]), int(X.indptr[13]) + 100
        X.indices[late], X.indices[early] = NGENES, -1
        return X, parents, MESSAGES[kind] % early
    if kind == "order":
        for r in (50, 13):
            e = int(X.indptr[r]) + 2
            assert e < X.indptr[r + 1]
            X.indices[e] = X.indices[e - 1]                                    # a duplicate: not strictly ascending
        return X, parents, MESSAGES[kind] % 13
    if kind == "value":
        X.data[int(X.indptr[40])] = -1
        X.data[int(X.indptr[6]) + 300] = 2 ** 24 + 1
        return X, parents, MESSAGES[kind] % (int(X.indptr[6]) + 300)
    assert kind == "parent"
    parents[77, 1], parents[3, 0] = -1, 80
    return X, parents, MESSAGES[kind] % 3
