"""NumPy / SciPy yardstick and graph makers of the Louvain tests, and the ctypes calls of the three entry
points.  The yardstick is written from the definition in include/schpf_hip.h in another shape than the library's serial
restatement: per round ONE sparse product of the level's matrix with the community indicator gives every K(i, d) at once,
and one lexsort picks every vertex's best candidate.

The fused multiply-add.  NumPy has none.  For a resolution that is a power of two the product -gamma * t is exact, so
fma(-gamma, t, K) is the one rounding of the sum and equals the plain double expression; for any other resolution the
yardstick takes the correctly rounded value of the exact rational."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
from scipy.sparse import csr_matrix

from _graph_reference import JACCARD, debug_graph


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------------- the yardstick
def _fma_neg(gamma, t, among):
    """fma(-gamma, t, among), elementwise."""
    mantissa, _ = np.frexp(gamma)
    if mantissa == 0.5:                       # a power of two: -gamma * t is exact
        return -gamma * t + among.astype(np.float64)
    g = Fraction(-gamma)
    return np.array([float(g * Fraction(float(x)) + int(y)) for x, y in zip(t, among)], np.float64)


def _scores(k, base, w2, among, gamma):
    p = k.astype(np.float64) * base.astype(np.float64)
    t = p / np.float64(w2)
    return _fma_neg(gamma, t, among)


def eligible(n, r):
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(2654435761)) >> np.uint64(16)) & np.uint64(1) == np.uint64(r & 1)


def numpy_louvain(indptr, indices, data, gamma=1.0):
    """(labels int32, stats int64[4]) of the definition."""
    indptr, indices, data = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(data, np.float64)
    n = len(indptr) - 1
    labels = np.arange(n, dtype=np.int32)
    wmax = data.max() if len(data) else 0.0
    if n == 0 or len(data) == 0 or wmax == 0:
        return labels, np.array([n, 0, 0, 0], np.int64)
    q = np.rint(np.ldexp(data / wmax, 30)).astype(np.int64)            # rint: to nearest, ties to even
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = indices
    nl, levels, rounds, w2_first = n, 0, 0, None
    for level in range(32):
        k = np.zeros(nl, np.int64)
        np.add.at(k, rows, q)
        w2 = int(k.sum())
        w2_first = w2 if level == 0 else w2_first
        off = rows != cols
        weights = csr_matrix((q[off], (rows[off], cols[off])), shape=(nl, nl))
        pattern = csr_matrix((np.ones(int(off.sum()), np.int64), (rows[off], cols[off])), shape=(nl, nl))
        c = np.arange(nl, dtype=np.int64)
        tot = k.copy()
        level_moved = False
        for r in range(32):
            rounds += 1
            member = csr_matrix((np.ones(nl, np.int64), (np.arange(nl), c)), shape=(nl, nl))
            seen = (pattern @ member).tocoo()        # counts: > 0 wherever row i has an entry in community d
            i, d = seen.row.astype(np.int64), seen.col.astype(np.int64)
            among = np.asarray((weights @ member)[i, d]).ravel().astype(np.int64) if len(i) else np.zeros(0, np.int64)
            may = (eligible(nl, r) & (k > 0))[i]
            i, d, among = i[may], d[may], among[may]
            own = d == c[i]
            own_among = np.zeros(nl, np.int64)
            own_among[i[own]] = among[own]
            i, d, among = i[~own], d[~own], among[~own]
            s = _scores(k[i], tot[d], w2, among, gamma)
            order = np.lexsort((d, -s, i))            # by vertex, then the key (score descending, d ascending)
            i, d, s = i[order], d[order], s[order]
            first = np.ones(len(i), bool)
            first[1:] = i[1:] != i[:-1]
            i, d, s = i[first], d[first], s[first]
            stay = _scores(k[i], tot[c[i]] - k[i], w2, own_among[i], gamma)
            go = s > stay
            if not go.any():
                break
            level_moved = True
            c = c.copy()
            c[i[go]] = d[go]
            tot = np.zeros(nl, np.int64)
            np.add.at(tot, c, k)
        if not level_moved:
            break
        levels += 1
        present = np.zeros(nl, np.int64)
        present[c] = 1
        renum = np.cumsum(present) - present
        n_next = int(present.sum())
        key = renum[c[rows]] * n_next + renum[c[cols]]
        uniq, inverse = np.unique(key, return_inverse=True)
        summed = np.zeros(len(uniq), np.int64)
        np.add.at(summed, inverse, q)
        rows, cols, q = uniq // n_next, uniq % n_next, summed
        labels = renum[c[labels]].astype(np.int32)
        nl = n_next
    return labels, np.array([nl, levels, rounds, w2_first], np.int64)


# ------------------------------------------------------------------------------------------------------------ the inputs
def as_arrays(G):
    """(indptr int64, indices int32, data float64) of a SciPy matrix, columns ascending."""
    G = csr_matrix(G)
    G.sort_indices()
    return G.indptr.astype(np.int64), G.indices.astype(np.int32), G.data.astype(np.float64)


def as_csr(graph):
    indptr, indices, data = graph
    n = len(indptr) - 1
    return csr_matrix((data, indices, indptr), shape=(n, n))


def list_graph(idx, dist, method):
    """The section-17 graph of neighbour lists, by the library's host restatement."""
    indptr, indices, data = debug_graph(idx, dist, method)[:3]
    return indptr.copy(), indices.copy(), data.copy()


def knn_jaccard(x, k=15):
    """The Jaccard graph of the exact k-NN self graph of the rows of x (both by the library's host restatements)."""
    from _knn_reference import debug_knn
    idx, _ = debug_knn(x, x, k, 0)
    return list_graph(idx, None, JACCARD)


def blob_scores(n=2000, centres=10, K=20, seed=0):
    """Ten well-separated blobs: unit normal clouds round centres about 20 apart."""
    rng = np.random.RandomState(seed)
    mu = rng.normal(0.0, 10.0, (centres, K))
    return mu[rng.randint(0, centres, n)] + rng.normal(0.0, 1.0, (n, K))


def clique_ring(cliques=12, size=8, bridge=1e-3):
    """Cliques of `size` with unit weights, joined in a ring: the last vertex of one to the first of the next."""
    n = cliques * size
    A = np.kron(np.eye(cliques), np.ones((size, size)) - np.eye(size))
    for b in range(cliques):
        u, v = b * size + size - 1, ((b + 1) % cliques) * size
        A[u, v] = A[v, u] = bridge
    assert n == A.shape[0]
    return as_arrays(A)


def ring_lattice(n=200, reach=2):
    """Every vertex joined to its `reach` neighbours on either side by weight 1: every score of a round ties."""
    i = np.arange(n)
    A = np.zeros((n, n))
    for s in range(1, reach + 1):
        A[i, (i + s) % n] = A[(i + s) % n, i] = 1.0
    return as_arrays(A)


def hub(n=5000, seed=0):
    """A hub of degree n - 1 (vertex 0) over a sparse random graph."""
    from scipy.sparse import coo_matrix
    rng = np.random.RandomState(seed)
    u, v = rng.randint(1, n, 3 * n), rng.randint(1, n, 3 * n)
    keep = u != v
    u, v = u[keep], v[keep]
    w = rng.gamma(2.0, 0.5, len(u))
    spokes = np.arange(1, n)
    sw = rng.gamma(2.0, 0.1, n - 1)
    rows = np.concatenate([np.minimum(u, v), np.zeros(n - 1, np.int64)])
    cols = np.concatenate([np.maximum(u, v), spokes])
    upper = coo_matrix((np.concatenate([w, sw]), (rows, cols)), shape=(n, n)).tocsr()     # a pair drawn twice adds up
    G = upper + upper.T
    return as_arrays(G)


def two_components(n=60, seed=0):
    """Two random graphs side by side, no edge between vertices below n / 2 and the others."""
    rng = np.random.RandomState(seed)
    A = np.zeros((n, n))
    h = n // 2
    for lo in (0, h):
        B = np.triu((rng.rand(h, h) < 0.2) * rng.gamma(2.0, 0.5, (h, h)), 1)
        A[lo:lo + h, lo:lo + h] = B + B.T
    for lo in (0, h):                                  # a path through each half keeps it in one piece
        for v in range(lo, lo + h - 1):
            A[v, v + 1] = A[v + 1, v] = max(A[v, v + 1], 0.5)
    return as_arrays(A)


def with_empty_rows(graph, rows):
    """The graph with these vertices cut off: their rows and columns removed."""
    G = as_csr(graph).tolil()
    for v in rows:
        G[v, :] = 0
        G[:, v] = 0
    G = G.tocsr()
    G.eliminate_zeros()
    return as_arrays(G)


def with_zero_rows(graph, rows):
    """The same structure, the entries of these rows and columns 0.0: stored, of no weight."""
    indptr, indices, data = graph
    data = data.copy()
    row_of = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    data[np.isin(row_of, rows) | np.isin(indices, rows)] = 0.0
    return indptr, indices, data


def with_tiny_weights(graph, seed=0):
    """One pair in five scaled to below 2^-31 of the largest weight: q = 0, the entry still a candidate."""
    G = as_csr(graph).tocoo()
    lo, hi = np.minimum(G.row, G.col).astype(np.int64), np.maximum(G.row, G.col).astype(np.int64)
    tiny = (lo * 7919 + hi * 104729 + seed) % 5 == 0                              # the same for (i, j) and (j, i)
    data = np.where(tiny, G.data * 2.0 ** -40, G.data)
    return as_arrays(csr_matrix((data, (G.row, G.col)), shape=G.shape))


def with_diagonal(graph, seed=0):
    G = as_csr(graph).tolil()
    rng = np.random.RandomState(seed)
    for v in range(0, G.shape[0], 3):
        G[v, v] = rng.gamma(2.0, 0.5)
    return as_arrays(G.tocsr())


@functools.lru_cache(maxsize=None)
def score_graph(n, k, method, seed):
    from _graph_reference import score_lists
    idx, dist = score_lists(n, k, seed=seed)
    return list_graph(idx, dist, method)


# ------------------------------------------------------------------------------------------------------ the entry points
def _call(fn, graph, gamma, fill=-7):
    from schpf_amd import _lib
    indptr, indices, data = graph
    indptr = np.ascontiguousarray(indptr, np.int64)
    indices = np.ascontiguousarray(indices, np.int32)
    data = np.ascontiguousarray(data, np.float64)
    n = len(indptr) - 1
    labels = np.full(n, fill, np.int32)
    stats = np.full(4, fill, np.int64)
    _lib.check(fn(n, _p(indptr), _p(indices), _p(data), float(gamma), _p(labels),
                  stats.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    return labels, stats


def debug_louvain(graph, gamma=1.0):
    """schpf_debug_louvain: the library's serial restatement on the host -> (labels, stats)."""
    from schpf_amd import _lib
    return _call(_lib.load().schpf_debug_louvain, graph, gamma)


def host_louvain(graph, gamma=1.0):
    """schpf_louvain: host pointers, staged through the device."""
    from schpf_amd import _lib
    lib = _lib.load()
    return _call(lambda *a: lib.schpf_louvain(0, *a), graph, gamma)

