"""What DeviceCAVI.upload accepts, normalised: a SciPy sparse matrix, or a torch sparse COO / CSR tensor.

`classify(X, shape)` needs no GPU and does not touch one: it looks at the argument's type, layout, dtypes and shape and
returns a `MatrixInput` that says which entry point of the library takes it -- the host upload (SciPy matrices and CPU
tensors, the latter converted to a SciPy COO) or the device uploads of DESIGN.md 13 (tensors in GPU memory, handed over
by pointer).  An uncoalesced COO tensor keeps its duplicates as separate observations, like a SciPy COO.
"""
import numpy as np

from . import _lib

ACCEPTED = ("a SciPy sparse matrix, a 2-d torch sparse COO tensor (torch.sparse_coo_tensor) or a 2-d torch sparse CSR "
            "tensor (torch.sparse_csr_tensor) with int32, int64, float32 or float64 values")

_VALUE_KINDS = {"torch.int32": _lib.VAL_I32, "torch.int64": _lib.VAL_I64, "torch.float32": _lib.VAL_F32,
                "torch.float64": _lib.VAL_F64}
_INDEX_KINDS = {"torch.int32": _lib.IDX_I32, "torch.int64": _lib.IDX_I64}


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
