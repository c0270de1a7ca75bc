"""Nearest neighbours of cells in factor space on the GPU: the exact k-NN graph of cell scores.

The cell-score matrix of a fitted model goes straight into a k-nearest-neighbour graph (UMAP, Phenograph, Leiden), and,
with `scHPF.project`, into label transfer: every projected cell's nearest cells of the atlas.  The search runs in the
library (schpf_knn[_device]): every pair is looked at, nothing of size n_query x n_ref ever exists, and the result is
defined bit for bit -- squared distances by one subtraction and one fused multiply-add per factor in double, ties by the
smaller index.  Here are the argument plumbing, the two metrics and the assembly of the sparse graph.
"""
import ctypes

import numpy as np

from . import _lib
from ._call import array_ptr as _p, device_of, library, same_device, stats_ptr, stream_of, tensor_ptr as ptr
from .device_input import from_torch, from_torch_on_gpu, gpu_graph, host_graph, host_graph_matrix

__all__ = ["knn", "knn_graph", "knn_connectivities", "louvain", "modularity"]

METRICS = ("euclidean", "cosine")
GRAPH_METHODS = {"umap": _lib.GRAPH_UMAP, "jaccard": _lib.GRAPH_JACCARD}
_DTYPES = {np.dtype(np.float32): _lib.F32, np.dtype(np.float64): _lib.F64}


def _unit_rows(x, name):
    """Rows scaled to unit length (cosine: |a - b|^2 / 2 = 1 - cos for unit a, b); plumbing, in NumPy or torch."""
    if from_torch(x):
        import torch
        norm = torch.linalg.vector_norm(x, dim=1, keepdim=True)
        zero = bool((norm == 0).any())
    else:
        norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
        zero = bool((norm == 0).any())
    if zero:
        raise ValueError("metric='cosine' needs nonzero rows; %s has a zero row" % name)
    return x / norm


def _check(metric, k):
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (", ".join(METRICS), metric))
    k = int(k)
    if not 1 <= k <= 128:
        raise ValueError("k must be in [1, 128], got %d" % k)
    return k


def _search_host(query, ref, k, self_first, device):
    """schpf_knn on two C-contiguous NumPy matrices of one dtype (float32 / float64) -> (idx, d2)."""
    lib = library()
    idx = np.empty((query.shape[0], k), np.int32)
    d2 = np.empty((query.shape[0], k), np.float64)
    _lib.check(lib.schpf_knn(device_of(device), _DTYPES[query.dtype], query.shape[0], ref.shape[0], query.shape[1], _p(query),
                             _p(ref), k, ctypes.c_int64(self_first), _p(idx), _p(d2)))
    return idx, d2


def knn(query, ref=None, k=15, metric="euclidean", exclude_self=None, device=None):
    """(indices, distances) of the k nearest rows of `ref` for every row of `query`: int32 and float64, n_query x k,
    ascending in distance, equal distances by the smaller index.

    query, ref: n x K arrays of cell scores, float32 or float64 (anything else is converted to float64), NumPy or torch.
    A torch tensor in GPU memory stays there and two torch tensors on the same GPU come back, the call running on
    torch's current stream; NumPy in gives NumPy out.  ref=None is the self graph: query against itself.

    exclude_self: leave row q of the reference out of query row q's neighbours -- a cell as its own neighbour; by index,
    so duplicated cells at distance 0 stay neighbours.  Default: True for the self graph, False with a `ref`.

    metric: "euclidean" returns the distance sqrt(d2); "cosine" normalises the rows to unit length first and returns
    d2 / 2 = 1 - cos (a zero row raises ValueError).  Non-finite values raise ValueError naming the smallest offending
    row.  `device`: HIP device ordinal, default the tensor's GPU, else $SCHPF_DEVICE or 0.
    """
    k = _check(metric, k)
    self_graph = ref is None
    if exclude_self is None:
        exclude_self = self_graph
    tensors = from_torch(query)
    if not self_graph and from_torch(ref) != tensors:
        raise ValueError("query and ref must both be NumPy arrays or both be torch tensors")
    if tensors and not query.is_cuda:      # a tensor in host memory: as NumPy, and back
        import torch
        idx, dist = knn(query.numpy(), None if self_graph else ref.cpu().numpy(), k, metric, exclude_self, device)
        return torch.from_numpy(idx), torch.from_numpy(dist)
    self_first = 0 if exclude_self else -1

    if not tensors:
        query = np.asarray(query)
        dtype = query.dtype if query.dtype in _DTYPES else np.dtype(np.float64)
        query = np.ascontiguousarray(query, dtype=dtype)
        ref = query if self_graph else np.ascontiguousarray(ref, dtype=dtype)
        if query.ndim != 2 or ref.ndim != 2 or query.shape[1] != ref.shape[1]:
            raise ValueError("query and ref must be matrices with the same number of columns")
        if metric == "cosine":
            query = np.ascontiguousarray(_unit_rows(query, "query"))
            ref = query if self_graph else np.ascontiguousarray(_unit_rows(ref, "ref"))
        idx, d2 = _search_host(query, ref, k, self_first, device)
        return idx, (np.sqrt(d2) if metric == "euclidean" else d2 / 2)

    import torch
    lib = library()
    _TORCH = {torch.float32: _lib.F32, torch.float64: _lib.F64}
    dev = query.device
    same_device(dev.index, device, "query")
    if not self_graph and ref.device != dev:
        raise ValueError("query is on %s, ref on %s" % (dev, ref.device))
    dtype = query.dtype if query.dtype in _TORCH else torch.float64
    query = query.detach().to(dtype).contiguous()
    ref = query if self_graph else ref.detach().to(dtype).contiguous()
    if query.dim() != 2 or ref.dim() != 2 or query.shape[1] != ref.shape[1]:
        raise ValueError("query and ref must be matrices with the same number of columns")
    with torch.cuda.device(dev):
        if metric == "cosine":
            query = _unit_rows(query, "query").contiguous()
            ref = query if self_graph else _unit_rows(ref, "ref").contiguous()
        idx = torch.empty((query.shape[0], k), dtype=torch.int32, device=dev)
        d2 = torch.empty((query.shape[0], k), dtype=torch.float64, device=dev)
        # on torch's current stream: ordered after whatever produced the scores and before whatever reads the result
        _lib.check(lib.schpf_knn_device(dev.index, stream_of(dev), _TORCH[dtype], query.shape[0], ref.shape[0], query.shape[1],
                                        ptr(query), ptr(ref), k, ctypes.c_int64(self_first), ptr(idx), ptr(d2)))
        return idx, (torch.sqrt(d2) if metric == "euclidean" else d2 / 2)


def knn_graph(indices, distances, n_ref):
    """The neighbour lists as a SciPy CSR matrix n_query x n_ref that holds the distances: row q has the entries
    (indices[q, j], distances[q, j]) -- the layout of scanpy's obsp["distances"] and of UMAP's precomputed input.
    A neighbour at distance 0 (a duplicated cell) is stored explicitly."""
    from scipy.sparse import csr_matrix
    if from_torch(indices):
        indices, distances = indices.cpu().numpy(), distances.cpu().numpy()
    indices, distances = np.asarray(indices), np.asarray(distances)
    if indices.ndim != 2 or indices.shape != distances.shape:
        raise ValueError("indices and distances must be matrices of one shape")
    n_query, k = indices.shape
    if indices.size and (indices.min() < 0 or indices.max() >= n_ref):
        raise ValueError("indices must be in [0, n_ref)")
    indptr = np.arange(n_query + 1, dtype=np.int64) * k
    return csr_matrix((distances.ravel(), indices.ravel(), indptr), shape=(n_query, int(n_ref)))


def _graph_host(method, idx, dist, device):
    """schpf_knn_graph on C-contiguous NumPy lists (dist None: jaccard) -> (indptr, indices, data) of the CSR matrix, cut
    to nnz."""
    lib = library()
    n, k = idx.shape
    indptr = np.zeros(n + 1, np.int64)
    indices = np.empty(2 * n * k, np.int32)
    data = np.empty(2 * n * k, np.float64)
    _lib.check(lib.schpf_knn_graph(device_of(device), method, n, k, _p(idx), _p(dist), _p(indptr), _p(indices), _p(data), None,
                                   None))
    nnz = int(indptr[n])
    return indptr, indices[:nnz], data[:nnz]


def knn_connectivities(indices, distances=None, method="umap", device=None):
    """The weighted, symmetric neighbour graph of the k-NN lists `knn(x, k=k)` returned (the self graph, no cell its own
    neighbour): n x n CSR, every pair stored in both rows with the same bits, no diagonal.

    method="umap": UMAP's fuzzy simplicial set (local_connectivity 1, set_op_mix_ratio 1) -- scanpy's
    obsp["connectivities"], the input of sc.tl.umap / leiden / louvain.  UMAP's n_neighbors counts the cell itself:
    knn(k=14) and this is scanpy's n_neighbors=15.  Needs the distances.
    method="jaccard": the shared-neighbour graph of Phenograph / Seurat, |N(i) & N(j)| / |N(i) | N(j)| with a cell in its
    own neighbourhood; the distances are not read.

    NumPy in gives a SciPy CSR matrix out (umap: without explicit zeros).  Two torch tensors on a GPU give a
    torch.sparse_csr_tensor on that GPU, computed on torch's current stream; nothing but two integers crosses to the
    host.  Lists that name a row outside [0, n), the row itself or a row twice, and distances that are negative or not
    finite, raise ValueError naming the smallest offending row."""
    if method not in GRAPH_METHODS:
        raise ValueError("method must be one of %s, got %r" % (", ".join(GRAPH_METHODS), method))
    if method == "umap" and distances is None:
        raise ValueError("method='umap' needs the distances of the neighbour lists")
    code = GRAPH_METHODS[method]
    if from_torch_on_gpu(indices):
        import torch
        lib = library()
        dev = indices.device
        same_device(dev.index, device, "indices", "are")
        if method == "umap" and (not from_torch(distances) or distances.device != dev):
            raise ValueError("indices and distances must be on the same GPU")
        if indices.dim() != 2 or (method == "umap" and distances.shape != indices.shape):
            raise ValueError("indices and distances must be matrices of one shape")
        n, k = indices.shape
        with torch.cuda.device(dev):
            idx = indices.detach().to(torch.int32).contiguous()
            dist = distances.detach().to(torch.float64).contiguous() if method == "umap" else None
            indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            cols = torch.empty(2 * n * k, dtype=torch.int32, device=dev)
            data = torch.empty(2 * n * k, dtype=torch.float64, device=dev)
            _lib.check(lib.schpf_knn_graph_device(dev.index, stream_of(dev), code, n, k, ptr(idx), ptr(dist), ptr(indptr),
                                                  ptr(cols), ptr(data), None, None))
            nnz = int(indptr[n]) if n else 0
            # one index type for both, as torch's kernels expect: int32 where it holds nnz
            indptr, cols = (indptr.to(torch.int32), cols[:nnz]) if nnz < 2 ** 31 else (indptr, cols[:nnz].to(torch.int64))
            import warnings
            with warnings.catch_warnings():          # torch announces that its CSR tensors are in beta, once per process
                warnings.filterwarnings("ignore", message="Sparse CSR tensor support is in beta")
                return torch.sparse_csr_tensor(indptr, cols, data[:nnz], size=(n, n))

    from scipy.sparse import csr_matrix
    if from_torch(indices):
        indices = indices.cpu().numpy()
    if distances is not None and from_torch(distances):
        distances = distances.cpu().numpy()
    idx = np.ascontiguousarray(indices, dtype=np.int32)
    dist = np.ascontiguousarray(distances, dtype=np.float64) if method == "umap" else None
    if idx.ndim != 2 or (dist is not None and dist.shape != idx.shape):
        raise ValueError("indices and distances must be matrices of one shape")
    n = idx.shape[0]
    indptr, cols, data = _graph_host(code, idx, dist, device)
    if len(cols) < 2 ** 31:
        indptr = indptr.astype(np.int32)
    G = csr_matrix((data, cols, indptr), shape=(n, n))
    if method == "umap":
        G.eliminate_zeros()
    return G


def _louvain_host(indptr, indices, data, gamma, device):
    """schpf_louvain on the three C-contiguous arrays of a CSR matrix (int64, int32, float64) -> (labels, stats)."""
    lib = library()
    n = len(indptr) - 1
    labels = np.empty(n, np.int32)
    stats = np.zeros(4, np.int64)
    _lib.check(lib.schpf_louvain(device_of(device), n, _p(indptr), _p(indices), _p(data), float(gamma), _p(labels),
                                 stats_ptr(stats)))
    return labels, stats


def _resolution(resolution):
    gamma = float(resolution)
    if not (gamma > 0 and np.isfinite(gamma)):
        raise ValueError("resolution must be finite and > 0, got %r" % (resolution,))
    return gamma


def _connected(graph, labels, stats, device, return_stats):
    """louvain(connected=True): the connected pieces of every community, and the community each piece came from."""
    from .topology import connected_components
    pieces, found = connected_components(graph, within=labels, device=device, return_stats=True)
    if not return_stats:
        return pieces
    if from_torch(pieces):
        import torch
        parent = torch.empty(found["components"], dtype=labels.dtype, device=pieces.device)
        parent[pieces.long()] = labels.to(pieces.device)   # every member of a piece writes the same community
    else:
        parent = np.empty(found["components"], np.int32)
        parent[pieces] = labels
    return pieces, dict(stats, clusters=found["components"], parent=parent)


def louvain(graph, resolution=1.0, device=None, return_stats=False, connected=False):
    """Louvain clusters of a weighted symmetric graph -- `knn_connectivities(...)`, or any n x n CSR matrix with finite
    entries >= 0 that equals its transpose -- as int32 labels 0 .. C - 1, one per row.

    The weights are quantised once to integers (30 bits below the largest), every sum of the algorithm is then an integer
    sum, and the moves of a round are applied together: the same graph gives the same labels bit for bit, on any GPU and
    however the work was scheduled.  `resolution` multiplies the null model's term: larger values give more, smaller
    clusters.  Symmetry is the caller's contract and is not checked.

    A SciPy sparse matrix in gives a NumPy array out.  A torch.sparse_csr_tensor on a GPU gives a tensor on that GPU,
    computed on torch's current stream; nothing but four integers crosses to the host.  return_stats=True: also
    {"communities", "levels", "rounds", "total_weight"} (the levels that moved a vertex, the rounds of all levels, the sum
    of the quantised weights).  A matrix the library refuses -- columns out of range, negative or non-finite values --
    raises ValueError naming the smallest offending row.

    connected=True: Louvain can return a community that is not connected; every community is then split into its connected
    pieces (schpf_amd.connected_components `within` the labels) and that labelling is returned, numbered in ascending order
    of first member.  return_stats then also holds "clusters", their number, and "parent", the Louvain label each came from."""
    gamma = _resolution(resolution)
    names = ("communities", "levels", "rounds", "total_weight")
    if from_torch_on_gpu(graph):
        import torch
        dev, n, indptr, cols, data = gpu_graph(graph, device, values=True)
        lib = library()
        with torch.cuda.device(dev):
            labels = torch.empty(n, dtype=torch.int32, device=dev)
            stats = np.zeros(4, np.int64)
            _lib.check(lib.schpf_louvain_device(dev.index, stream_of(dev), n, ptr(indptr), ptr(cols), ptr(data), gamma,
                                                ptr(labels), stats_ptr(stats)))
        if connected:
            return _connected(graph, labels, dict(zip(names, stats.tolist())), device, return_stats)
        return (labels, dict(zip(names, stats.tolist()))) if return_stats else labels

    back_to_torch = from_torch(graph)
    if back_to_torch:
        import torch
    G = host_graph_matrix(graph)
    if not G.has_canonical_format:          # columns ascending, no entry twice: on a copy
        G = G.copy()
        G.sum_duplicates()
    labels, stats = _louvain_host(*(host_graph(G)[1:] + (gamma, device)))
    if connected:
        pieces = _connected(G, labels, dict(zip(names, np.asarray(stats).tolist())), device, return_stats)
        if back_to_torch:
            pieces = (torch.from_numpy(pieces[0]), pieces[1]) if return_stats else torch.from_numpy(pieces)
        return pieces
    if back_to_torch:
        labels = torch.from_numpy(labels)
    return (labels, dict(zip(names, np.asarray(stats).tolist()))) if return_stats else labels


def modularity(graph, labels, resolution=1.0):
    """Newman's modularity of a labelling of a weighted symmetric graph, in plain double arithmetic on the host:
    sum over the communities of  in_c / W - resolution * (tot_c / W)^2,  W the sum of all entries, in_c the sum of the
    entries with both ends in c, tot_c the sum of the rows of c.  0 for a graph without weight."""
    from scipy.sparse import coo_matrix, issparse
    gamma = _resolution(resolution)
    if from_torch(graph):
        graph = graph.cpu().to_dense().numpy()
    if from_torch(labels):
        labels = labels.cpu().numpy()
    A = graph.tocoo() if issparse(graph) else coo_matrix(np.asarray(graph))
    labels = np.asarray(labels).astype(np.int64).ravel()
    if A.shape[0] != A.shape[1] or len(labels) != A.shape[0]:
        raise ValueError("graph must be square, with one label per row")
    if len(labels) and labels.min() < 0:
        raise ValueError("labels must be >= 0")
    data = A.data.astype(np.float64)
    total = data.sum()
    if not total > 0:
        return 0.0
    inside = data[labels[A.row] == labels[A.col]].sum()
    tot = np.bincount(labels[A.row], weights=data)
    return float(inside / total - gamma * (tot * tot).sum() / (total * total))
