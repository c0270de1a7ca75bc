"""What the library is handed, normalised: the count matrices, graphs and labels that `DeviceCAVI.upload` and the
stateless operators accept, brought into the forms the entry points take.

`classify(X, shape)` needs no GPU and does not touch one: it looks at the argument's type, layout, dtypes and shape and
returns a `MatrixInput` that says which entry point of the library takes it -- the host upload (SciPy matrices and CPU
tensors, the latter converted to a SciPy COO) or the device uploads of DESIGN.md 13 (tensors in GPU memory, handed over
by pointer).  An uncoalesced COO tensor keeps its duplicates as separate observations, like a SciPy COO.

Below it, one function per form an operator asks for: of a matrix in GPU memory `gpu_csr`, `gpu_coo` and
`gpu_csc`; of a matrix anywhere else `host_csr` with `host_csr_arrays`, and `host_csc`; of a square graph `gpu_graph`, and
`host_graph_matrix` with `host_graph`; of labels `int32_labels`.  The conversions are plumbing, done with torch where the
tensor lives or with SciPy; the pointers, the device and the stream of the call itself are in `_call`.
"""
import numpy as np

from . import _lib
from ._call import same_device

ACCEPTED = ("a SciPy sparse matrix, a 2-d torch sparse COO tensor (torch.sparse_coo_tensor) or a 2-d torch sparse CSR "
            "tensor (torch.sparse_csr_tensor) with int32, int64, float32 or float64 values")

_VALUE_KINDS = {"torch.int32": _lib.VAL_I32, "torch.int64": _lib.VAL_I64, "torch.float32": _lib.VAL_F32,
                "torch.float64": _lib.VAL_F64}
_INDEX_KINDS = {"torch.int32": _lib.IDX_I32, "torch.int64": _lib.IDX_I64}
# the value kinds of NumPy arrays; values of another dtype go to the library as float64
NUMPY_VALUE_KINDS = {np.dtype(np.int32): _lib.VAL_I32, np.dtype(np.int64): _lib.VAL_I64,
                     np.dtype(np.float32): _lib.VAL_F32, np.dtype(np.float64): _lib.VAL_F64}


class MatrixInput(object):
    """kind: 'host' (`.matrix`, a SciPy COO), 'coo' or 'csr' (GPU tensors: `.major` = row indices / crow_indices,
    `.minor` = col indices, `.values`, contiguous 1-d; `.major_kind`, `.minor_kind`, `.value_kind` the library's codes;
    `.device` the tensors' GPU ordinal).  `.nnz` and `.shape` in every case."""

    def __init__(self, kind, shape, nnz, matrix=None, major=None, minor=None, values=None, major_kind=None,
                 minor_kind=None, value_kind=None, device=None):
        self.kind, self.shape, self.nnz, self.matrix = kind, tuple(shape), int(nnz), matrix
        self.major, self.minor, self.values = major, minor, values
        self.major_kind, self.minor_kind, self.value_kind, self.device = major_kind, minor_kind, value_kind, device


def is_torch_tensor(X):
    return type(X).__module__.split(".")[0] == "torch" and hasattr(X, "layout")


def on_gpu(X):
    """True for a torch tensor in GPU memory (the inputs that take the device uploads)."""
    return is_torch_tensor(X) and X.device.type == "cuda"


def from_torch(x):
    """Anything of torch's, with a `.layout` or without: the looser question that the neighbour, graph and path operators
    have always asked of their arguments.  `is_torch_tensor` is the one for count matrices."""
    return type(x).__module__.split(".")[0] == "torch"


def from_torch_on_gpu(x):
    return from_torch(x) and x.is_cuda


def to_numpy(a):
    """A tensor fetched to the host, anything else through np.asarray."""
    return a.detach().cpu().numpy() if is_torch_tensor(a) else np.asarray(a)


def shape_of(X):
    return tuple(int(n) for n in X.shape)


def _kind(table, t, what):
    try:
        return table[str(t.dtype)]
    except KeyError:
        raise TypeError("%s of dtype %s are not supported; X must be %s" % (what, t.dtype, ACCEPTED))


def classify(X, shape=None):
    """X -> MatrixInput.  `shape`: the (ncells, ngenes) X must have, or None.  TypeError for an input of another kind
    (a dense tensor, another layout, unsupported dtypes), ValueError for a wrong shape or number of dimensions."""
    if is_torch_tensor(X):
        import torch
        layouts = {torch.sparse_coo: "coo", torch.sparse_csr: "csr"}
        if X.layout not in layouts:
            raise TypeError("a torch tensor of layout %s is not supported; X must be %s" % (X.layout, ACCEPTED))
        if X.dim() != 2 or (X.layout == torch.sparse_coo and X.dense_dim() != 0):
            raise ValueError("X must be a 2-d cell x gene matrix, got a tensor of shape %s; X must be %s"
                             % (shape_of(X), ACCEPTED))
        _check_shape(X, shape)
        if X.layout == torch.sparse_coo:
            ind, values = X._indices(), X._values()
            major, minor = ind[0], ind[1]
        else:
            major, minor, values = X.crow_indices(), X.col_indices(), X.values()
        vk = _kind(_VALUE_KINDS, values, "values")
        mk, nk = _kind(_INDEX_KINDS, major, "indices"), _kind(_INDEX_KINDS, minor, "indices")
        nnz = int(values.shape[0])
        if X.device.type != "cuda":
            return MatrixInput("host", X.shape, nnz, matrix=_to_scipy(layouts[X.layout], X.shape, major, minor, values))
        return MatrixInput(layouts[X.layout], X.shape, nnz, major=major.contiguous(), minor=minor.contiguous(),
                           values=values.contiguous(), major_kind=mk, minor_kind=nk, value_kind=vk,
                           device=X.device.index if X.device.index is not None else torch.cuda.current_device())
    if not (hasattr(X, "tocoo") or (hasattr(X, "row") and hasattr(X, "col") and hasattr(X, "data"))):
        raise TypeError("cannot upload a %s; X must be %s" % (type(X).__name__, ACCEPTED))
    _check_shape(X, shape)
    if not hasattr(X, "row"):
        X = X.tocoo()
    return MatrixInput("host", X.shape, np.shape(X.data)[0], matrix=X)


def as_matrix(X):
    """X as the loss functions and scHPF._fit pass it on: a torch tensor as it is (classify() sorts it out at the upload),
    anything else as a COO."""
    return X if is_torch_tensor(X) or hasattr(X, "row") else X.tocoo()


def _check_shape(X, shape):
    if shape is not None and shape_of(X) != tuple(shape):
        raise ValueError("X has shape %s, engine was created for %s" % (shape_of(X), tuple(shape)))


def _to_scipy(layout, shape, major, minor, values):
    """A CPU tensor's arrays as a SciPy COO with the same entries in the same order."""
    from scipy.sparse import coo_matrix
    minor, values = minor.numpy(), values.numpy()
    if layout == "coo":
        row = major.numpy()
    else:
        row = np.repeat(np.arange(shape[0], dtype=np.int64), np.diff(major.numpy()))
    return coo_matrix((values, (row, minor)), shape=tuple(shape))


# ---- a count matrix in GPU memory ----

def gpu_csr(X, device=None):
    """A sparse CSR / COO tensor on a GPU -> (its MatrixInput as a CSR, its torch device).  A COO is brought to canonical
    CSR with torch on that GPU, as plumbing: coalesce() sums the duplicates and orders the entries by row, then column.
    `device`: the ordinal the caller asked for, refused if it names another GPU."""
    import torch
    with torch.cuda.device(X.device):
        inp = classify(X)
        if inp.kind != "csr":
            C = X.detach().coalesce()
            rows, cols = C.indices()[0], C.indices()[1]
            crow = torch.zeros(inp.shape[0] + 1, dtype=torch.int64, device=X.device)
            if inp.shape[0]:
                crow[1:] = torch.cumsum(torch.bincount(rows, minlength=inp.shape[0]), 0)
            inp = classify(torch.sparse_csr_tensor(crow, cols.contiguous(), C.values().contiguous(), size=inp.shape))
    same_device(inp.device, device, "X")
    return inp, torch.device("cuda", inp.device)


def gpu_coo(X):
    """A sparse COO / CSR tensor on a GPU -> (rows, cols, values) of its coalesced COO form: duplicates summed, row-major."""
    import torch
    if X.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise TypeError("a matrix on the GPU must be a torch sparse COO or CSR tensor, got layout %s" % X.layout)
    if X.dim() != 2:
        raise ValueError("X must be a 2-d cell x gene matrix, got a tensor of shape %s" % (tuple(X.shape),))
    X = X.detach()
    if X.layout == torch.sparse_csr:
        crow = X.crow_indices().to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(X.shape[0], device=X.device), crow[1:] - crow[:-1])
        X = torch.sparse_coo_tensor(torch.stack([rows, X.col_indices().to(torch.int64)]), X.values(), size=tuple(X.shape))
    X = X.coalesce()
    return X.indices()[0], X.indices()[1], X.values()


def gpu_csc(X):
    """A sparse COO / CSR tensor on a GPU -> (indptr int64, cell ids int32, values float32) of its CSC form, duplicates
    summed: what `gene_major(X)` holds.  A CSR tensor with canonical rows goes through the library's exact transpose
     and meets no sort; anything else is coalesced with torch on that GPU first."""
    from .gene_major import gene_major
    return gene_major(X).float32()


# ---- a count matrix anywhere else ----

def _host_matrix(X):
    return classify(X).matrix if is_torch_tensor(X) else X          # a tensor in host memory: as SciPy


def host_csr(X, canonical):
    """Anything that is not a GPU tensor as a SciPy CSR that is the caller's no longer; canonical: duplicates summed."""
    from scipy.sparse import csr_matrix, issparse
    X = _host_matrix(X)
    C = X.tocsr() if issparse(X) else csr_matrix(X)
    if canonical:
        if C is X:
            C = C.copy()
        C.sum_duplicates()                               # also sorts the columns of every row
    return C


def host_csr_arrays(C):
    """(indptr int64, indices int32, values of a kind in NUMPY_VALUE_KINDS) of a SciPy CSR, C-contiguous."""
    data = np.ascontiguousarray(C.data)
    vals = data if data.dtype in NUMPY_VALUE_KINDS else data.astype(np.float64)
    return np.ascontiguousarray(C.indptr, dtype=np.int64), np.ascontiguousarray(C.indices, dtype=np.int32), vals


def host_csc(X):
    """Anything that is not a GPU tensor -> (N, J, the C-contiguous arrays of the canonical CSC form: int64, int32, float32)."""
    from scipy.sparse import csc_matrix, issparse
    X = _host_matrix(X)
    C = csc_matrix(X) if not issparse(X) else X.tocsc()
    if C is X:
        C = C.copy()
    C.sum_duplicates()                    # also sorts the cells of every gene
    N, J = C.shape
    return (N, J, np.ascontiguousarray(C.indptr, dtype=np.int64), np.ascontiguousarray(C.indices, dtype=np.int32),
            np.ascontiguousarray(C.data, dtype=np.float32))


# ---- a square graph ----

def gpu_graph(graph, device, values):
    """(torch device, n, indptr int64, cols int32, data float64 or None) of a torch.sparse_csr_tensor on a GPU."""
    import torch
    if graph.layout != torch.sparse_csr:
        raise ValueError("a graph on the GPU must be a torch.sparse_csr_tensor")
    if graph.dim() != 2 or graph.shape[0] != graph.shape[1]:
        raise ValueError("graph must be a square matrix")
    dev = graph.device
    same_device(dev.index, device, "graph")
    with torch.cuda.device(dev):
        indptr = graph.crow_indices().detach().to(torch.int64).contiguous()
        cols = graph.col_indices().detach().to(torch.int32).contiguous()
        data = graph.values().detach().to(torch.float64).contiguous() if values else None
    return dev, graph.shape[0], indptr, cols, data


def host_graph_matrix(graph):
    """A SciPy matrix, a dense array or a torch tensor on the host as a square SciPy CSR, its entries as they are stored."""
    from scipy.sparse import csr_matrix, issparse
    if from_torch(graph):
        graph = graph.to_sparse_csr()
        graph = csr_matrix((graph.values().numpy(), graph.col_indices().numpy(), graph.crow_indices().numpy()),
                           shape=tuple(graph.shape))
    G = graph.tocsr() if issparse(graph) else csr_matrix(np.asarray(graph))
    if G.shape[0] != G.shape[1]:
        raise ValueError("graph must be a square matrix")
    return G


def host_graph(graph):
    """(n, indptr int64, indices int32, data float64) of what `host_graph_matrix` takes.  The entries stay as they are
    stored: columns need not ascend and repeats are harmless; a caller that wants them summed does so on the matrix first."""
    G = host_graph_matrix(graph)
    return (G.shape[0], np.ascontiguousarray(G.indptr, dtype=np.int64), np.ascontiguousarray(G.indices, dtype=np.int32),
            np.ascontiguousarray(G.data, dtype=np.float64))


# ---- labels ----

def int32_labels(labels, lowest=None, refusal=None):
    """Integer labels in host memory as a C-contiguous int32 array.  lowest: a label below it or above int32's largest
    cannot be meant and is refused with `refusal` before the cast could hide it; a %d in `refusal` takes the first
    offending position."""
    labels = np.asarray(labels)
    if lowest is not None:
        bad = (labels < lowest) | (labels > np.iinfo(np.int32).max)
        if bad.any():
            raise ValueError(refusal % int(np.flatnonzero(bad)[0]) if "%d" in refusal else refusal)
    return np.ascontiguousarray(labels, dtype=np.int32)
