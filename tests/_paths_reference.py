"""Yardstick, inputs and ctypes calls of the shortest-path tests: `scipy.sparse.csgraph.dijkstra` compared by
the int64 view of the doubles, a set of many roots being the elementwise minimum over its members' rows, and loops written
from the definitions of `farthest_landmarks` and `landmark_isomap`."""
import functools

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra

from _louvain_reference import hub, two_components
from _topology_reference import I64P, _p, diagonal_only, empty, from_pairs, plane_knn, plane_points, rows_of

ROOT_TILE = 8      # schpf_amd.paths.ROOT_TILE, asserted equal in test_paths_host.py


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------------- the yardstick
def as_stored(graph):
    """The SciPy CSR of (indptr, indices, data) exactly as stored: zeros and repeats survive."""
    indptr, indices, data = graph
    n = len(indptr) - 1
    data = np.ones(len(indices)) if data is None else data
    return csr_matrix((np.asarray(data, np.float64), np.asarray(indices, np.int32), np.asarray(indptr, np.int64)), shape=(n, n))


def scipy_geodesic(graph, directed, sets):
    """float64[len(sets), n] by SciPy's Dijkstra; an empty set is a row of inf."""
    n = len(graph[0]) - 1
    out = np.full((len(sets), n), np.inf)
    if n == 0:
        return out
    G = as_stored(graph)
    for r, members in enumerate(sets):
        members = np.asarray(members, np.int64)
        if len(members) == 0:
            continue
        if len(members) > 16:
            out[r] = dijkstra(G, directed=directed, indices=members, min_only=True)
        else:
            out[r] = dijkstra(G, directed=directed, indices=members).reshape(len(members), n).min(axis=0)
    return out


def loop_farthest_landmarks(D, L, first=0):
    """Maxmin sampling on a full distance matrix D[n, n] (D[l] = the distances from l), from the definition."""
    chosen = [first]
    while len(chosen) < L:
        best, best_value = None, None
        for v in range(D.shape[1]):
            value = min(D[l, v] for l in chosen)
            if best is None or value > best_value:          # strictly: ties stay with the lowest index
                best, best_value = v, value
        chosen.append(best)
    return np.array(chosen, np.int32)


def loop_landmark_isomap(dist, landmarks, n_components):
    """landmark_isomap from its docstring, entry by entry where a loop says it plainly."""
    L, n = dist.shape
    S = np.zeros((L, L))
    for a in range(L):
        for b in range(L):
            S[a, b] = (dist[a, landmarks[b]] ** 2 + dist[b, landmarks[a]] ** 2) / 2
    row_mean = np.array([sum(S[a]) / L for a in range(L)])
    total = sum(row_mean) / L
    B = np.zeros((L, L))
    for a in range(L):
        for b in range(L):
            B[a, b] = -0.5 * (S[a, b] - row_mean[a] - row_mean[b] + total)
    lam, U = np.linalg.eigh(B)
    order = np.argsort(lam, kind="stable")[::-1][:n_components]
    X = np.zeros((n, n_components))
    for c, a in enumerate(order):
        if lam[a] <= 0:
            continue
        for v in range(n):
            X[v, c] = -0.5 * sum(U[l, a] / np.sqrt(lam[a]) * (dist[l, v] ** 2 - row_mean[l]) for l in range(L))
        at = X[landmarks, c]
        if at[np.argmax(np.abs(at))] < 0:
            X[:, c] = -X[:, c]
    return X


# ------------------------------------------------------------------------------------------------------------ the inputs
def weighted_path(n, shuffled, seed=0):
    """A path over n vertices with a random length per pair, the same in both directions -> (graph, one end of it)."""
    name = np.random.RandomState(seed).permutation(n) if shuffled else np.arange(n)
    indptr, indices, _ = from_pairs(n, name[:-1], name[1:])
    rows = rows_of(indptr)
    lo, hi = np.minimum(rows, indices), np.maximum(rows, indices)
    return (indptr, indices, 0.125 + ((lo * 31 + hi * 17) % 97) / 16.0), int(name[0])


@functools.lru_cache(maxsize=None)
def plane_lengths():
    """The directed 3-NN lists of 20 000 uniform points with their Euclidean lengths."""
    indptr, indices, _ = plane_knn()
    x = plane_points()
    rows = rows_of(indptr)
    out = (indptr, indices, np.sqrt(((x[rows] - x[indices]) ** 2).sum(axis=1)))
    out[2].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def plane_special():
    """The same with 200 lengths 0, 200 of 1e-300, 200 of 1e300, and 500 entries stored twice with different lengths:
    columns no longer ascend and a row holds a repeat.  (1e300 does not overflow here: see plane_huge.)"""
    indptr, indices, data = plane_lengths()
    rng = np.random.RandomState(21)
    data = data.copy()
    pick = rng.permutation(len(data))
    data[pick[:200]] = 0.0
    data[pick[200:400]] = 1e-300
    data[pick[400:600]] = 1e300
    twice = np.sort(pick[600:1100])
    rows = rows_of(indptr)
    order = np.argsort(np.concatenate([rows, rows[twice]]), kind="stable")
    cols = np.concatenate([indices, indices[twice]])[order].astype(np.int32)
    vals = np.concatenate([data, data[twice] * rng.choice([0.5, 3.0], len(twice))])[order]
    new_ptr = np.zeros(len(indptr), np.int64)
    np.cumsum(np.bincount(np.concatenate([rows, rows[twice]]), minlength=len(indptr) - 1), out=new_ptr[1:])
    return new_ptr, cols, vals


@functools.lru_cache(maxsize=None)
def plane_huge():
    """One length in four at 1.2e308: 1e300 needs 1e8 edges to overflow, two of these do.  A vertex behind two of them is at
    +inf although a path leads there."""
    indptr, indices, data = plane_lengths()
    data = data.copy()
    data[np.random.RandomState(22).rand(len(data)) < 0.25] = 1.2e308
    return indptr, indices, data


def grid(side=30):
    """side x side vertices with unit edges between 4-neighbours: the distance is the Manhattan distance."""
    v = np.arange(side * side).reshape(side, side)
    u = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    w = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    indptr, indices, _ = from_pairs(side * side, u, w)
    return indptr, indices, np.ones(len(indices))


def plane_root_sets(n=20000):
    rng = np.random.RandomState(4)
    singles = [[int(v)] for v in rng.choice(n, ROOT_TILE + 1, replace=False)]
    return {
        "one_root": singles[:1],
        "a_tile_of_roots": singles[:ROOT_TILE],
        "a_tile_and_one": singles,
        "empty_between": [[11], [], [19999]],
        "repeated_in_a_set": [[5, 5, 77, 5], [77]],
        "a_thousand_members": [np.sort(rng.choice(n, 1000, replace=False)).tolist()],
    }


def cases():
    """name -> (graph, directed, root sets): every input the host and the GPU tests share."""
    out = {
        "n0": (empty(0), False, [[]]),
        "n1": (empty(1), False, [[0], []]),
        "no_entries": (empty(37), False, [[3], [], [5, 5, 36]]),
        "diagonal_only": (diagonal_only(), True, [[0], [8]]),
        "hub_5000": (hub(5000), False, [[v] for v in range(0, 5000, 5000 // ROOT_TILE)][:ROOT_TILE]),
        "two_components": (two_components(), False, [[0], [45], [3, 50]]),
        "two_components_directed": (two_components(), True, [[0], [45], [3, 50]]),
        "grid_30": (grid(), False, [[0], [899], [0, 899]]),
    }
    for shuffled in (True, False):
        graph, end = weighted_path(4097, shuffled)
        out["path_4097_" + ("shuffled" if shuffled else "in_order")] = (graph, False, [[end]])
    for name, sets in plane_root_sets().items():
        for directed in (True, False):
            out["plane_3nn_%s_%s" % ("directed" if directed else "undirected", name)] = (plane_lengths(), directed, sets)
    for directed in (True, False):
        tail = "directed" if directed else "undirected"
        out["plane_special_" + tail] = (plane_special(), directed, plane_root_sets()["empty_between"])
        out["plane_huge_" + tail] = (plane_huge(), directed, plane_root_sets()["empty_between"])
        out["plane_hops_" + tail] =(plane_lengths()[:2] + (None,), directed, plane_root_sets()["repeated_in_a_set"])
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """SciPy's answer for a case, computed once and shared; read-only."""
    graph, directed, sets = cases()[name]
    want = scipy_geodesic(graph, directed, sets)
    want.setflags(write=False)
    return want


# ------------------------------------------------------------------------------------------------------ the entry points
def pack_sets(sets):
    set_ptr = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([len(s) for s in sets], out=set_ptr[1:])
    roots = np.concatenate([np.asarray(s, np.int32) for s in sets]).astype(np.int32) if sets else np.zeros(0, np.int32)
    return set_ptr, np.ascontiguousarray(roots)


def _geodesic(fn, graph, directed, set_ptr, roots, fill=-7):
    indptr = np.ascontiguousarray(graph[0], np.int64)
    indices = np.ascontiguousarray(graph[1], np.int32)
    data = None if graph[2] is None else np.ascontiguousarray(graph[2], np.float64)
    n, nsets = len(indptr) - 1, len(set_ptr) - 1
    dist = np.full((nsets, n), float(fill))
    stats = np.full(3, fill, np.int64)
    status = fn(n, _p(indptr), _p(indices), _p(data), int(directed), nsets, _p(set_ptr), _p(roots), _p(dist), stats.ctypes.data_as(I64P))
    return status, dist, stats


def debug_geodesic(graph, directed, sets):
    """schpf_debug_geodesic: the serial Dijkstra on the host -> (dist, stats)."""
    from schpf_amd import _lib
    status, dist, stats = _geodesic(_lib.load().schpf_debug_geodesic, graph, directed, *pack_sets(sets))
    _lib.check(status)
    return dist, stats


def host_geodesic(graph, directed, sets):
    """schpf_geodesic: host pointers, staged through the device."""
    from schpf_amd import _lib
    lib = _lib.load()
    status, dist, stats = _geodesic(lambda *a: lib.schpf_geodesic(0, *a), graph, directed, *pack_sets(sets))
    _lib.check(status)
    return dist, stats
