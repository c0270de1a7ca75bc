"""The count matrix gene-major, converted once.

The operators that work on genes -- `rank_sums`, `pair_rank_sums`, `residual_variance` -- take the matrix as CSC arrays: an
int64 `indptr` over the genes, int32 cell ids ascending within a gene, float32 values.  Everything upstream produces it
cell-major.  For a CSR tensor in GPU memory the library's exact transpose (schpf_transpose_device) goes from one to the
other without a sort: the rows already hold their columns in order.  `gene_major` returns the result as a `GeneMajor`,
which the three operators accept in place of X, so that a caller who runs several of them on one matrix converts once:

    G = gene_major(X)
    found = residual_variance(G)
    sums = rank_sums(G, labels)
"""
import numpy as np

from . import _lib
from ._call import library, same_device, stream_of, tensor_ptr as ptr
from .device_input import _VALUE_KINDS, classify, gpu_coo, host_csc, is_torch_tensor, on_gpu

__all__ = ["GeneMajor", "gene_major"]

NOT_ASCENDING = "transpose: columns must be strictly ascending within a row"


class GeneMajor(object):
    """The CSC arrays of a cells x genes matrix: `indptr` (int64, J + 1), `cells` (int32, ascending within a gene) and
    `values`, all three torch tensors on one GPU or all three NumPy arrays; `shape` = (N, J) of the matrix they came from,
    and `nnz`."""

    def __init__(self, indptr, cells, values, shape):
        self.indptr, self.cells, self.values = indptr, cells, values
        self.shape = (int(shape[0]), int(shape[1]))
        self.nnz = int(values.shape[0])

    @property
    def on_gpu(self):
        return on_gpu(self.indptr)

    @property
    def device(self):
        """The tensors' torch device; None for NumPy arrays."""
        return self.indptr.device if is_torch_tensor(self.indptr) else None

    def float32(self):
        """(indptr, cells, values as float32): what the gene-side entry points of the library take."""
        if is_torch_tensor(self.values):
            import torch
            return self.indptr, self.cells, self.values.to(torch.float32).contiguous()
        return self.indptr, self.cells, np.ascontiguousarray(self.values, dtype=np.float32)

    def tensor(self):
        """The transpose as a matrix, genes x cells: a torch.sparse_csr_tensor on the arrays' GPU, or a SciPy CSR."""
        J_by_N = (self.shape[1], self.shape[0])
        if is_torch_tensor(self.indptr):
            import torch
            return torch.sparse_csr_tensor(self.indptr, self.cells, self.values, size=J_by_N)
        from scipy.sparse import csr_matrix
        return csr_matrix((self.values, self.cells, self.indptr), shape=J_by_N)


def refuse_gene_major(X, who):
    """The TypeError of a function that also needs the cell-major matrix."""
    if isinstance(X, GeneMajor):
        raise TypeError("%s needs the cell-major count matrix X as well, not only its GeneMajor form: hand it X" % who)


def held_on_gpu(X):
    """True for a matrix or a GeneMajor in GPU memory."""
    return X.on_gpu if isinstance(X, GeneMajor) else on_gpu(X)


def gpu_arrays(X):
    """(indptr int64, cells int32, values float32) of a GeneMajor or a sparse tensor on a GPU."""
    return X.float32() if isinstance(X, GeneMajor) else gene_major(X).float32()


def host_arrays(X):
    """(N, J, indptr int64, cells int32, values float32) of a GeneMajor or a matrix in host memory, C-contiguous."""
    if isinstance(X, GeneMajor):
        return (X.shape[0], X.shape[1]) + tuple(np.ascontiguousarray(a) for a in X.float32())
    return host_csc(X)


def _transpose(lib, inp, dev, same):
    """schpf_transpose_device on a MatrixInput of kind 'csr' on torch's current stream -> GeneMajor of tensors on that GPU."""
    import torch
    N, J = inp.shape
    out_kind = inp.value_kind if same else _lib.VAL_F32
    indptr = torch.empty(J + 1, dtype=torch.int64, device=dev)
    cells = torch.empty(inp.nnz, dtype=torch.int32, device=dev)
    values = torch.empty(inp.nnz, dtype=inp.values.dtype if same else torch.float32, device=dev)
    _lib.check(lib.schpf_transpose_device(inp.device, stream_of(dev), N, J, inp.nnz, ptr(inp.major), inp.major_kind, ptr(inp.minor),
                                          inp.minor_kind, ptr(inp.values), inp.value_kind, out_kind, ptr(indptr), ptr(cells),
                                          ptr(values), None))
    return GeneMajor(indptr, cells, values, (N, J))


def _as_csr(X, rows, cols, values):
    """The arrays of a coalesced COO as a CSR tensor: the row pointer by bincount and cumsum."""
    import torch
    N = int(X.shape[0])
    crow = torch.zeros(N + 1, dtype=torch.int64, device=X.device)
    if N:
        crow[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    return torch.sparse_csr_tensor(crow, cols.contiguous(), values.contiguous(), size=tuple(X.shape))


def _supported(X, same):
    """A CSR tensor whose values are of a kind the library reads; values of another dtype go over as float32, which is what
    they become in the end."""
    import torch
    if str(X.values().dtype) in _VALUE_KINDS:
        return X
    if same:
        raise TypeError('values="same" needs int32, int64, float32 or float64 values, got %s' % X.values().dtype)
    return torch.sparse_csr_tensor(X.crow_indices(), X.col_indices(), X.values().to(torch.float32), size=tuple(X.shape))


def gene_major(X, values="float32", device=None):
    """The cells x genes matrix X gene-major: a `GeneMajor`.

    A torch sparse CSR tensor on a GPU goes to the library's exact transpose on torch's current stream, and tensors on that
    GPU come back; no sort.  Only if the library refuses its rows as not strictly ascending is the matrix coalesced first
    (duplicates summed, columns sorted) and transposed after that.  A sparse COO tensor on a GPU is coalesced and then
    transposed.  Anything in host memory goes through SciPy (`tocsc()` on a copy, duplicates summed), and NumPy comes back.
    values: "float32" -- what the operators on genes take, exact for counts up to 2^24 -- or "same", the values' own kind
    with the bytes of every value unchanged.  device: refused if it names another GPU than the one X lives on."""
    if values not in ("float32", "same"):
        raise ValueError('values must be "float32" or "same", got %r' % (values,))
    same = values == "same"
    if isinstance(X, GeneMajor):
        return X
    if not on_gpu(X):
        if same:
            from scipy.sparse import csc_matrix, issparse
            M = classify(X).matrix if is_torch_tensor(X) else X
            C = M.tocsc() if issparse(M) else csc_matrix(M)
            if C is M:
                C = C.copy()
            C.sum_duplicates()
            return GeneMajor(np.ascontiguousarray(C.indptr, dtype=np.int64), np.ascontiguousarray(C.indices, dtype=np.int32),
                             np.ascontiguousarray(C.data), C.shape)
        N, J, indptr, indices, data = host_csc(X)
        return GeneMajor(indptr, indices, data, (N, J))
    import torch
    same_device(X.device.index if X.device.index is not None else torch.cuda.current_device(), device, "X")
    with torch.cuda.device(X.device):
        if X.layout == torch.sparse_csr and X.dim() == 2:
            lib = library()
            inp = classify(_supported(X.detach(), same))
            try:
                return _transpose(lib, inp, X.device, same)
            except ValueError as refusal:
                if not str(refusal).startswith(NOT_ASCENDING):
                    raise
        rows, cols, vals = gpu_coo(X)                 # refuses other layouts; duplicates summed, row-major
        lib = library()
        return _transpose(lib, classify(_supported(_as_csr(X, rows, cols, vals), same)), X.device, same)
