"""The shape of the neighbour graph on the GPU: connected components, connected clusters and the cluster graph.

`connected_components` tells which cells can reach each other -- over the whole graph, or `within` the groups of a
labelling, which is how `louvain(connected=True)` splits a community that fell into pieces.  `cluster_graph` counts the
entries and adds up Louvain's integer weights between every pair of clusters; `paga` turns the counts into the
connectivities of a PAGA plot and `absorb_small` merges splinters into the cluster they hang on.  Everything the library
computes here is an integer, equal bit for bit however the work was scheduled; the floats of `paga` are plain NumPy.
"""
import ctypes

import numpy as np

from . import _lib
from ._call import array_ptr as _p, device_of, library, stats_ptr, stream_of, tensor_ptr as ptr
from .device_input import from_torch, from_torch_on_gpu, gpu_graph, host_graph, int32_labels

__all__ = ["connected_components", "cluster_graph", "absorb_small", "paga"]

COMPONENT_STATS = ("components", "largest", "singletons", "edges", "hook_rounds", "shortcut_passes")


def _row_labels(labels, n, name):
    """One integer per row of the graph, from NumPy or a tensor, as int32 in host memory."""
    if from_torch(labels):
        labels = labels.cpu().numpy()
    labels = np.asarray(labels)
    if labels.shape != (n,):
        raise ValueError("%s must hold one integer per row of the graph" % name)
    if not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("%s must be integers" % name)
    return int32_labels(labels)


def connected_components(graph, within=None, device=None, return_stats=False):
    """The connected components of a graph as int32 labels 0 .. C - 1, one per row, numbered in ascending order of their
    first member -- SciPy's `connected_components(graph, directed=True, connection="weak")` numbers them the same way.

    Every stored entry (i, j) with j != i is an undirected edge: the matrix need not be symmetric, so the directed lists of
    `knn_graph` give the weakly connected components.  Values are not read.  within: one integer per row; an entry is then
    an edge only between two rows of the same group, and a row of group -1 has no edges -- the pieces of every group.

    Accepts what `louvain` accepts: a SciPy sparse matrix gives a NumPy array; a torch.sparse_csr_tensor on a GPU stays
    there, runs on torch's current stream and gives a tensor.  return_stats=True: also {"components", "largest",
    "singletons", "edges", "hook_rounds", "shortcut_passes"}; the last two depend on how the GPU scheduled the work, the
    labels and the other four do not."""
    lib = library()
    stats = np.zeros(6, np.int64)
    if from_torch_on_gpu(graph):
        import torch
        dev, n, indptr, cols, _ = gpu_graph(graph, device, values=False)
        with torch.cuda.device(dev):
            w = None
            if within is not None:
                w = torch.as_tensor(within if from_torch(within) else _row_labels(within, n, "within"))
                if tuple(w.shape) != (n,) or w.is_floating_point():
                    raise ValueError("within must hold one integer per row of the graph")
                w = w.to(device=dev, dtype=torch.int32).contiguous()
            comp = torch.empty(n, dtype=torch.int32, device=dev)
            _lib.check(lib.schpf_components_device(dev.index, stream_of(dev), n, ptr(indptr), ptr(cols), ptr(w), ptr(comp),
                                                   stats_ptr(stats)))
    else:
        back_to_torch = from_torch(graph)
        n, indptr, indices, _ = host_graph(graph)
        w = None if within is None else _row_labels(within, n, "within")
        comp = np.empty(n, np.int32)
        _lib.check(lib.schpf_components(device_of(device), n, _p(indptr), _p(indices), _p(w), _p(comp), stats_ptr(stats)))
        if back_to_torch:
            import torch
            comp = torch.from_numpy(comp)
    return (comp, dict(zip(COMPONENT_STATS, stats.tolist()))) if return_stats else comp


def cluster_graph(graph, labels, ngroups=None, weights=True, device=None):
    """The graph of the clusters: {"n_cells": int64[G], "count": int64[G, G], "weight": int64[G, G] or None, "wmax"}.

    count[a, b] is the number of stored entries (i, j), j != i, from a row of cluster a to a column of cluster b (stored
    zeros count); weight[a, b] is the sum over the same entries of Louvain's integers llrint(ldexp(value / wmax, 30)), wmax
    the largest stored value.  labels: one integer per row in [-1, G), -1 for a row in no cluster; ngroups=None: G =
    max(labels) + 1.  The graph may be directed: count is then not symmetric.  A torch.sparse_csr_tensor on a GPU gives
    tensors on that GPU."""
    lib = library()
    wmax = ctypes.c_double(0.0)
    if from_torch_on_gpu(graph):
        import torch
        dev, n, indptr, cols, data = gpu_graph(graph, device, values=bool(weights))
        with torch.cuda.device(dev):
            lab = torch.as_tensor(labels if from_torch(labels) else _row_labels(labels, n, "labels"))
            if tuple(lab.shape) != (n,) or lab.is_floating_point():
                raise ValueError("labels must hold one integer per row of the graph")
            lab = lab.to(device=dev, dtype=torch.int32).contiguous()
            G = _ngroups(ngroups, int(lab.max()) if n else -1)
            cells = torch.empty(G, dtype=torch.int64, device=dev)
            count = torch.empty((G, G), dtype=torch.int64, device=dev)
            weight = torch.empty((G, G), dtype=torch.int64, device=dev) if weights else None
            _lib.check(lib.schpf_cluster_graph_device(dev.index, stream_of(dev), n, ptr(indptr), ptr(cols), ptr(data), ptr(lab), G,
                                                      ptr(cells), ptr(count), ptr(weight), ctypes.byref(wmax)))
    else:
        n, indptr, indices, data = host_graph(graph)
        lab = _row_labels(labels, n, "labels")
        G = _ngroups(ngroups, int(lab.max()) if n else -1)
        cells = np.empty(G, np.int64)
        count = np.empty((G, G), np.int64)
        weight = np.empty((G, G), np.int64) if weights else None
        _lib.check(lib.schpf_cluster_graph(device_of(device), n, _p(indptr), _p(indices), _p(data) if weights else None, _p(lab),
                                           G, _p(cells), _p(count), _p(weight), ctypes.byref(wmax)))
    return {"n_cells": cells, "count": count, "weight": weight, "wmax": wmax.value}


def _ngroups(ngroups, largest):
    G = max(largest + 1, 1) if ngroups is None else int(ngroups)
    if G < 1 or G * G >= 2 ** 31:
        raise ValueError("ngroups must be at least 1 with ngroups^2 below 2^31, got %d" % G)
    return G


def absorb_small(labels, table, sizes, min_size):
    """Merge every group of fewer than `min_size` members into the group it is tied to most: (labels, table, sizes) after
    the merges, plain NumPy on integers.

    table[G, G] is a cluster graph (`cluster_graph`'s count or weight) and sizes[G] its groups' members.  Repeatedly: of the
    groups below min_size that have a positive symmetrised entry table[a, b] + table[b, a] with another group b, take the
    smallest (ties: the lowest id) and merge it into the b with the largest such entry (ties: the lowest id), adding its
    rows, columns and size -- until no group qualifies.  A group with no outside weight stays as it is, however small.
    The survivors are renumbered in ascending old id; labels of -1 stay -1."""
    labels = np.asarray(labels)
    table = np.array(table, dtype=np.int64)
    sizes = np.array(sizes, dtype=np.int64)
    G = len(sizes)
    if table.shape != (G, G):
        raise ValueError("table must be G x G for the G groups of sizes")
    if len(labels) and (labels.min() < -1 or labels.max() >= G):
        raise ValueError("labels must be in [-1, G)")
    alive = np.ones(G, bool)
    target = np.arange(G)
    while True:
        sym = table + table.T
        np.fill_diagonal(sym, 0)
        ok = alive & (sizes < min_size) & (sym.max(axis=1, initial=0) > 0)
        if not ok.any():
            break
        a = int(np.flatnonzero(ok)[np.argmin(sizes[ok])])   # argmin and argmax keep the first of equals: the lowest id
        b = int(np.argmax(sym[a]))
        table[b, :] += table[a, :]
        table[:, b] += table[:, a]
        table[a, :] = 0
        table[:, a] = 0
        sizes[b] += sizes[a]
        sizes[a] = 0
        alive[a] = False
        target[target == a] = b
    keep = np.flatnonzero(alive)
    renum = np.full(G + 1, -1, np.int64)     # the last slot: labels of -1
    renum[keep] = np.arange(len(keep))
    merged = renum[np.where(labels >= 0, target[np.maximum(labels, 0)], G)].astype(labels.dtype if len(labels) else np.int32)
    return merged, table[np.ix_(keep, keep)], sizes[keep]


def paga(graph, labels, ngroups=None, device=None):
    """The PAGA graph of a clustering: {"connectivities", "expected", "count", "n_cells"} over the G clusters.

    graph is the DIRECTED k-NN graph, `knn_graph(indices, distances)`; the counts come from `cluster_graph` on the GPU.
    With ns = n_cells, N = ns.sum(), inner[a] = count[a, a], inter = count without its diagonal, es[a] = inner[a] +
    inter[a, :].sum() and sym = inter + inter.T: where sym[a, b] > 0,
        expected[a, b] = (es[a] * ns[b] + es[b] * ns[a]) / (N - 1)
        connectivities[a, b] = min(1, sym[a, b] / expected[a, b]), or 1 where expected is 0;
    elsewhere both are 0.  The integers are exact; the two float tables are NumPy's."""
    found = cluster_graph(graph, labels, ngroups=ngroups, weights=False, device=device)
    count, ns = found["count"], found["n_cells"]
    if from_torch(count):
        count, ns = count.cpu().numpy(), ns.cpu().numpy()
    connectivities, expected = paga_tables(count, ns)
    return {"connectivities": connectivities, "expected": expected, "count": count, "n_cells": ns}


def paga_tables(count, n_cells):
    """(connectivities, expected) of `paga` from the integer tables."""
    count = np.asarray(count, dtype=np.int64)
    ns = np.asarray(n_cells, dtype=np.int64)
    inter = count.copy()
    np.fill_diagonal(inter, 0)
    es = np.diagonal(count) + inter.sum(axis=1)
    sym = inter + inter.T
    linked = sym > 0
    total = int(ns.sum())
    expected = np.zeros(count.shape, np.float64)
    np.divide((es[:, None] * ns[None, :] + es[None, :] * ns[:, None]).astype(np.float64), float(total - 1), out=expected,
              where=linked)
    connectivities = np.zeros(count.shape, np.float64)
    positive = linked & (expected > 0)
    np.divide(sym.astype(np.float64), expected, out=connectivities, where=positive)
    np.minimum(connectivities, 1.0, out=connectivities)
    connectivities[linked & ~positive] = 1.0
    return connectivities, expected
