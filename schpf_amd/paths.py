"""Distances along the neighbour graph on the GPU: exact shortest paths, pseudotime and landmark Isomap.

`geodesic_distances` walks the graph from root cells or root clusters; the distance is defined as the greatest solution of
d[root] = 0, d[v] = min over edges (u, v) of fl(d[u] + w_uv), one set of doubles that the library reaches bit for bit however
the work was scheduled -- SciPy's `dijkstra` gives the same bits.  `pseudotime` scales one such row to [0, 1],
`farthest_landmarks` picks landmarks by maxmin sampling on the exact distances, and `landmark_isomap` is classical MDS on
the landmarks with de Silva and Tenenbaum's triangulation of every other cell: an L x L eigendecomposition in NumPy, whose
floats are outside the bit contract.
"""
import numpy as np

from . import _lib
from ._call import array_ptr as _p, device_of, library, stats_ptr, stream_of, tensor_ptr as ptr
from .device_input import from_torch, from_torch_on_gpu, gpu_graph, host_graph

__all__ = ["geodesic_distances", "pseudotime", "farthest_landmarks", "landmark_isomap"]

ROOT_TILE = 8     # csrc/geodesic.hip ROOT_TILE: the root sets the device relaxes together
GEODESIC_STATS = ("finite", "rounds", "lowering_writes")


def _as_numpy(a):
    return a.cpu().numpy() if from_torch(a) else np.asarray(a)


def _one_set(root, n):
    """The members of ONE root set: a cell index, an index array or a boolean mask over the cells -> int32 array."""
    root = _as_numpy(root)
    if root.dtype == np.bool_:
        if root.shape != (n,):
            raise ValueError("a root mask must hold one boolean per row of the graph")
        return np.flatnonzero(root).astype(np.int32)
    if root.size and not np.issubdtype(root.dtype, np.integer):
        raise ValueError("roots must be integers or a boolean mask")
    root = np.atleast_1d(root).astype(np.int64)
    if root.ndim != 1:
        raise ValueError("a root set must be a cell index, a 1-D index array or a boolean mask")
    if root.size and (root.min() < 0 or root.max() >= n):
        raise ValueError("roots must be in [0, n)")
    return root.astype(np.int32)


def _root_sets(roots, n):
    """(set_ptr int64[nsets + 1], roots int32) of what `geodesic_distances` takes."""
    nested = isinstance(roots, (list, tuple)) and any(np.ndim(_as_numpy(r)) > 0 for r in roots)
    if nested:
        sets = [_one_set(r, n) for r in roots]
    else:
        flat = _as_numpy(roots)
        if flat.dtype == np.bool_ or flat.ndim == 0:
            sets = [_one_set(flat, n)]
        else:
            sets = [m.reshape(1) for m in _one_set(flat, n)]       # one row each
    set_ptr = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([len(s) for s in sets], out=set_ptr[1:])
    members = np.concatenate(sets).astype(np.int32) if sets else np.zeros(0, np.int32)
    return set_ptr, np.ascontiguousarray(members)


def geodesic_distances(graph, roots, directed=False, device=None, return_stats=False):
    """float64[nsets, n]: the exact shortest-path distance of every row of the graph from every root set, +inf where a row
    cannot be reached.

    graph is what `connected_components` takes -- a SciPy sparse matrix, a dense array, or a torch.sparse_csr_tensor on a
    GPU, which stays there, runs on torch's current stream and gives a tensor.  A stored entry (i, j, w) is an edge i -> j
    of length w >= 0 (a stored zero is an edge of length 0); with directed=False it is also an edge j -> i, as SciPy's
    `dijkstra(directed=False)` reads it.  roots: an int (one row), a 1-D int array (one row each), a list of arrays (one
    row per set: the distance to the nearest member) or a boolean mask over the cells (one set).

    Every distance is a sum of IEEE additions along one path and the same bits on every run; return_stats=True: also
    {"finite", "rounds", "lowering_writes"}, of which the last two depend on how the GPU scheduled the work."""
    lib = library()
    stats = np.zeros(3, np.int64)
    if from_torch_on_gpu(graph):
        import torch
        dev, n, indptr, cols, data = gpu_graph(graph, device, values=True)
        set_ptr, members = _root_sets(roots, n)
        nsets = len(set_ptr) - 1
        with torch.cuda.device(dev):
            d_set_ptr = torch.from_numpy(set_ptr).to(dev)
            d_members = torch.from_numpy(members).to(dev)
            dist = torch.empty((nsets, n), dtype=torch.float64, device=dev)
            _lib.check(lib.schpf_geodesic_device(dev.index, stream_of(dev), n, ptr(indptr), ptr(cols), ptr(data),
                                                 int(bool(directed)), nsets, ptr(d_set_ptr), ptr(d_members), ptr(dist),
                                                 stats_ptr(stats)))
    else:
        back_to_torch = from_torch(graph)
        n, indptr, indices, data = host_graph(graph)
        set_ptr, members = _root_sets(roots, n)
        nsets = len(set_ptr) - 1
        dist = np.empty((nsets, n), np.float64)
        _lib.check(lib.schpf_geodesic(device_of(device), n, _p(indptr), _p(indices), _p(data), int(bool(directed)), nsets,
                                      _p(set_ptr), _p(members), _p(dist), stats_ptr(stats)))
        if back_to_torch:
            import torch
            dist = torch.from_numpy(dist)
    return (dist, dict(zip(GEODESIC_STATS, stats.tolist()))) if return_stats else dist


def _n_rows(graph):
    return int(graph.shape[0]) if hasattr(graph, "shape") else len(graph)


def pseudotime(graph, root, directed=False, device=None):
    """float64[n]: the distance of every row from the root set, divided by the largest finite one.  root: a cell index, an
    index array or a boolean mask -- one set, the distance to its nearest member.  Rows that cannot be reached stay inf;
    where the largest finite distance is 0, every reachable row is 0.  The scaling is plain NumPy or torch on the exact
    distances of `geodesic_distances`."""
    dist = geodesic_distances(graph, [_one_set(root, _n_rows(graph))], directed=directed, device=device)[0]
    if from_torch(dist):
        import torch
        finite = torch.isfinite(dist)
        top = dist[finite].max() if bool(finite.any()) else dist.new_zeros(())
        return torch.where(finite, dist / top if float(top) > 0 else torch.zeros_like(dist), dist)
    finite = np.isfinite(dist)
    top = dist[finite].max() if finite.any() else 0.0
    out = dist.copy()
    out[finite] = dist[finite] / top if top > 0 else 0.0
    return out


def farthest_landmarks(graph, n_landmarks, first=0, directed=False, device=None):
    """(landmarks int32[L], dist float64[L, n]) by maxmin sampling: landmark 0 is `first`, landmark l + 1 the row with the
    largest distance to the nearest of landmarks 0 .. l, ties to the lowest index.  A row at inf -- in another component --
    counts as largest, so every component gets a landmark before any gets a second one at a finite distance.  Each step is
    one single-root call of `geodesic_distances` and one running minimum; the integers and the distances are exact."""
    n = _n_rows(graph)
    L = int(n_landmarks)
    if not 1 <= L <= n:
        raise ValueError("n_landmarks must be in [1, n], got %d" % L)
    if not 0 <= int(first) < n:
        raise ValueError("first must be in [0, n)")
    landmarks, rows, nearest = [int(first)], [], None
    for step in range(L):
        d = geodesic_distances(graph, landmarks[-1], directed=directed, device=device)[0]
        rows.append(d)
        nearest = d if nearest is None else (nearest.minimum(d) if from_torch(d) else np.minimum(nearest, d))
        if step + 1 < L:
            at_top = nearest == nearest.max()         # inf == inf: the rows no landmark reaches come first
            landmarks.append(int(at_top.nonzero()[0][0]) if from_torch(d) else int(np.flatnonzero(at_top)[0]))
    if from_torch(rows[0]):
        import torch
        return torch.tensor(landmarks, dtype=torch.int32, device=rows[0].device), torch.stack(rows)
    return np.array(landmarks, np.int32), np.stack(rows)


def landmark_isomap(dist, landmarks, n_components=2):
    """float64[n, n_components]: landmark Isomap of the distances `farthest_landmarks` returned.  NumPy only.

    With D = dist[:, landmarks] (L x L), S = (D * D + (D * D).T) / 2 and J = I - 1/L: B = -1/2 J S J, `np.linalg.eigh(B)`,
    the n_components largest eigenvalues lam_a with their vectors u_a.  Every row v is then placed by de Silva and
    Tenenbaum's triangulation, x_v[a] = -1/2 u_a / sqrt(lam_a) . (dist[:, v]^2 - S.mean(axis=1)) -- an axis whose eigenvalue
    is not positive is 0 -- which puts the landmarks where classical MDS puts them.  The sign of every axis is fixed so that
    its landmark coordinate of largest magnitude (the first of equals) is positive.

    Raises ValueError if any distance is infinite: the graph is in pieces, see `connected_components`.  These floats depend
    on LAPACK and are OUTSIDE the bit contract of the distances."""
    dist = np.asarray(_as_numpy(dist), np.float64)
    landmarks = np.asarray(_as_numpy(landmarks), np.int64)
    if dist.ndim != 2 or landmarks.shape != (dist.shape[0],):
        raise ValueError("dist must be L x n with one row per landmark")
    L = dist.shape[0]
    if not 1 <= int(n_components) <= L:
        raise ValueError("n_components must be in [1, L]")
    if not np.isfinite(dist).all():
        raise ValueError("landmark_isomap needs finite distances: the graph is in pieces (see connected_components); "
                         "lay out one component at a time")
    sq = dist * dist
    S = sq[:, landmarks]
    S = (S + S.T) / 2
    J = np.eye(L) - 1.0 / L
    lam, U = np.linalg.eigh(-0.5 * J @ S @ J)
    top = np.argsort(lam, kind="stable")[::-1][:int(n_components)]
    lam, U = lam[top], U[:, top]
    scale = np.zeros_like(lam)
    scale[lam > 0] = 1.0 / np.sqrt(lam[lam > 0])
    X = -0.5 * (sq - S.mean(axis=1)[:, None]).T @ (U * scale)
    at_landmarks = X[landmarks]
    lead = at_landmarks[np.argmax(np.abs(at_landmarks), axis=0), np.arange(X.shape[1])]
    return X * np.where(lead < 0, -1.0, 1.0)
