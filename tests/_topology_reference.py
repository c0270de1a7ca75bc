"""Yardsticks, inputs and ctypes calls of the topology tests: connected components against SciPy's
`connected_components(directed=True, connection="weak")` canonicalised by first member, the cluster graph against
`np.add.at`, and `absorb_small` / `paga` against loops written from their definitions."""
import ctypes
import functools

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components as scipy_components

from _louvain_reference import hub, two_components, with_empty_rows

I64P = ctypes.POINTER(ctypes.c_int64)


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)


def rows_of(indptr):
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))


# ------------------------------------------------------------------------------------------------------ the yardsticks
def by_first_member(labels):
    """Any labelling renumbered 0 .. C - 1 in ascending order of each label's first member."""
    labels = np.asarray(labels)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inverse].astype(np.int32)


def numpy_components(structure, within=None):
    """(comp int32, stats[0..3]) of the definition, by SciPy."""
    indptr, indices = np.asarray(structure[0], np.int64), np.asarray(structure[1], np.int64)
    n = len(indptr) - 1
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(4, np.int64)
    rows = rows_of(indptr)
    edge = rows != indices
    if within is not None:
        within = np.asarray(within)
        edge &= (within[rows] == within[indices]) & (within[rows] >= 0)
    A = csr_matrix((np.ones(int(edge.sum()), np.int8), (rows[edge], indices[edge])), shape=(n, n))
    C, labels = scipy_components(A, directed=True, connection="weak")
    comp = by_first_member(labels)
    size = np.bincount(comp, minlength=C)
    return comp, np.array([C, size.max(), (size == 1).sum(), edge.sum()], np.int64)


def numpy_cluster_graph(graph, labels, G, weights=True):
    """(n_cells, count, weight or None, wmax) of the definition: one np.add.at per table."""
    indptr, indices, data = graph
    indices = np.asarray(indices, np.int64)
    labels = np.asarray(labels, np.int64)
    rows = rows_of(np.asarray(indptr, np.int64))
    a, b = labels[rows], labels[indices]
    take = (rows != indices) & (a >= 0) & (b >= 0)
    cells = np.bincount(labels[labels >= 0], minlength=G).astype(np.int64)
    count = np.zeros((G, G), np.int64)
    np.add.at(count, (a[take], b[take]), 1)
    if not weights:
        return cells, count, None, None
    if data is None:
        q, wmax = np.full(len(indices), 1 << 30, np.int64), (1.0 if len(indices) else 0.0)
    else:
        data = np.asarray(data, np.float64)
        wmax = float(data.max()) if len(data) else 0.0
        q = np.rint(np.ldexp(data / wmax, 30)).astype(np.int64) if wmax > 0 else np.full(len(data), 1 << 30, np.int64)
    weight = np.zeros((G, G), np.int64)
    np.add.at(weight, (a[take], b[take]), q[take])
    return cells, count, weight, wmax


def loop_absorb_small(labels, table, sizes, min_size):
    """absorb_small of the definition, one Python loop per sentence."""
    table = [[int(x) for x in row] for row in np.asarray(table)]
    sizes = [int(s) for s in sizes]
    G = len(sizes)
    alive = [True] * G
    into = list(range(G))
    while True:
        pick = None
        for a in range(G):
            if not alive[a] or sizes[a] >= min_size:
                continue
            ties = [table[a][b] + table[b][a] if alive[b] and b != a else 0 for b in range(G)]
            if max(ties, default=0) <= 0:
                continue
            if pick is None or sizes[a] < sizes[pick[0]]:
                pick = (a, ties.index(max(ties)))
        if pick is None:
            break
        a, b = pick
        for c in range(G):
            table[b][c] += table[a][c]
        for c in range(G):
            table[c][b] += table[c][a]
        for c in range(G):
            table[a][c] = table[c][a] = 0
        sizes[b] += sizes[a]
        sizes[a] = 0
        alive[a] = False
        into = [b if t == a else t for t in into]
    keep = [g for g in range(G) if alive[g]]
    new = {g: r for r, g in enumerate(keep)}
    out = np.array([new[into[int(v)]] if v >= 0 else -1 for v in labels], np.int64)
    return out, np.array([[table[x][y] for y in keep] for x in keep], np.int64).reshape(len(keep), len(keep)), \
        np.array([sizes[g] for g in keep], np.int64)


def loop_paga(count, ns):
    """(connectivities, expected) of the definition, pair by pair."""
    count = np.asarray(count, np.int64)
    G = len(ns)
    N = int(np.sum(ns))
    inter = [[int(count[a, b]) if a != b else 0 for b in range(G)] for a in range(G)]
    es = [int(count[a, a]) + sum(inter[a]) for a in range(G)]
    conn, expected = np.zeros((G, G)), np.zeros((G, G))
    for a in range(G):
        for b in range(G):
            sym = inter[a][b] + inter[b][a]
            if sym > 0:
                expected[a, b] = (es[a] * int(ns[b]) + es[b] * int(ns[a])) / (N - 1)
                conn[a, b] = min(1.0, sym / expected[a, b]) if expected[a, b] != 0 else 1.0
    return conn, expected


# ------------------------------------------------------------------------------------------------------------ the inputs
def structure_of(G):
    """(indptr int64, indices int32, data float64) of a SciPy matrix as it is stored."""
    G = csr_matrix(G)
    return G.indptr.astype(np.int64), G.indices.astype(np.int32), G.data.astype(np.float64)


def from_pairs(n, u, v, symmetric=True):
    """The CSR of the entries (u, v) -- and (v, u) -- in the order they come: columns not ascending, repeats kept."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    if symmetric:
        u, v = np.concatenate([u, v]), np.concatenate([v, u])
    order = np.argsort(u, kind="stable")
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(u, minlength=n), out=indptr[1:])
    data = 0.25 + ((u[order] * 7 + v[order] * 13) % 11) / 8.0
    return indptr, v[order].astype(np.int32), data.astype(np.float64)


def path(n, shuffled, seed=0):
    """A path over n vertices: stored in order, or with its vertices numbered at random."""
    name = np.random.RandomState(seed).permutation(n) if shuffled else np.arange(n)
    return from_pairs(n, name[:-1], name[1:])


def random_pairs(n=20000, pairs=11000, seed=3):
    rng = np.random.RandomState(seed)
    return from_pairs(n, rng.randint(0, n, pairs), rng.randint(0, n, pairs))


@functools.lru_cache(maxsize=None)
def plane_points(n=20000, seed=7):
    return np.random.RandomState(seed).rand(n, 2)


@functools.lru_cache(maxsize=None)
def plane_knn(n=20000, k=3, seed=7):
    """The directed k-NN lists of n uniform points in the plane, unsymmetrised."""
    from scipy.spatial import cKDTree
    x = plane_points(n, seed)
    idx = cKDTree(x).query(x, k + 1)[1][:, 1:]
    indptr = np.arange(0, n * k + 1, k, dtype=np.int64)
    out = (indptr, idx.astype(np.int32).ravel(), np.ones(n * k))
    for a in out:
        a.setflags(write=False)
    return out


def chessboard(n=20000, seed=7, squares=8):
    """within: the square of a chessboard each plane point lies on, every 50th vertex -1."""
    x = plane_points(n, seed)
    w = (np.floor(x[:, 0] * squares) * squares + np.floor(x[:, 1] * squares)).astype(np.int32)
    w[::50] = -1
    return w


def two_cliques_through_a_stranger(size=6):
    """Community 0: two cliques of `size` joined only through vertex 2 * size, which belongs to community 1 (with one
    more vertex).  -> (graph, within)"""
    n = 2 * size + 2
    A = np.zeros((n, n))
    for lo in (0, size):
        A[lo:lo + size, lo:lo + size] = 1.0 - np.eye(size)
    s = 2 * size
    for v in (size - 1, size, s + 1):
        A[v, s] = A[s, v] = 1.0
    within = np.zeros(n, np.int32)
    within[s:] = 1
    return structure_of(A), within


def diagonal_only(n=9):
    return np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.ones(n)


def empty(n):
    return np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0)


def cases():
    """name -> (graph, within or None): every input the host and the GPU tests share."""
    cliques, cliques_within = two_cliques_through_a_stranger()
    small = two_components()
    return {
        "n0": (empty(0), None),
        "n1": (empty(1), None),
        "no_entries": (empty(37), None),
        "diagonal_only": (diagonal_only(), None),
        "path_4097_shuffled": (path(4097, True), None),
        "path_4097_in_order": (path(4097, False), None),
        "hub_5000": (hub(5000), None),
        "two_components": (small, None),
        "empty_rows": (with_empty_rows(small, [0, 7, 31, 59]), None),
        "random_pairs": (random_pairs(), None),
        "plane_3nn_directed": (plane_knn(), None),
        "plane_3nn_chessboard": (plane_knn(), chessboard()),
        "two_cliques_through_a_stranger": (cliques, cliques_within),
    }


# ------------------------------------------------------------------------------------------------------ the entry points
def _components(fn, structure, within, fill=-7):
    indptr = np.ascontiguousarray(structure[0], np.int64)
    indices = np.ascontiguousarray(structure[1], np.int32)
    within = None if within is None else np.ascontiguousarray(within, np.int32)
    n = len(indptr) - 1
    comp = np.full(n, fill, np.int32)
    stats = np.full(6, fill, np.int64)
    status = fn(n, _p(indptr), _p(indices), None if within is None else within.ctypes.data_as(ctypes.c_void_p), _p(comp),
                stats.ctypes.data_as(I64P))
    return status, comp, stats


def debug_components(structure, within=None):
    """schpf_debug_components: the serial restatement on the host -> (comp, stats)."""
    from schpf_amd import _lib
    status, comp, stats = _components(_lib.load().schpf_debug_components, structure, within)
    _lib.check(status)
    return comp, stats


def host_components(structure, within=None):
    """schpf_components: host pointers, staged through the device."""
    from schpf_amd import _lib
    lib = _lib.load()
    status, comp, stats = _components(lambda *a: lib.schpf_components(0, *a), structure, within)
    _lib.check(status)
    return comp, stats


def _cluster_graph(fn, graph, labels, G, weights=True, fill=-7):
    indptr = np.ascontiguousarray(graph[0], np.int64)
    indices = np.ascontiguousarray(graph[1], np.int32)
    data = None if graph[2] is None else np.ascontiguousarray(graph[2], np.float64)
    labels = np.ascontiguousarray(labels, np.int32)
    n = len(indptr) - 1
    cells = np.full(G, fill, np.int64)
    count = np.full((G, G), fill, np.int64)
    weight = np.full((G, G), fill, np.int64) if weights else None
    wmax = ctypes.c_double(float(fill))
    status = fn(n, _p(indptr), _p(indices), _p(data), _p(labels), G, cells.ctypes.data_as(ctypes.c_void_p),
                count.ctypes.data_as(ctypes.c_void_p), None if weight is None else weight.ctypes.data_as(ctypes.c_void_p),
                ctypes.byref(wmax))
    return status, cells, count, weight, wmax.value


def debug_cluster_graph(graph, labels, G, weights=True):
    from schpf_amd import _lib
    out = _cluster_graph(_lib.load().schpf_debug_cluster_graph, graph, labels, G, weights)
    _lib.check(out[0])
    return out[1:]


def host_cluster_graph(graph, labels, G, weights=True):
    from schpf_amd import _lib
    lib = _lib.load()
    out = _cluster_graph(lambda *a: lib.schpf_cluster_graph(0, *a), graph, labels, G, weights)
    _lib.check(out[0])
    return out[1:]
