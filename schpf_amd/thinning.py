"""Count thinning (count splitting) on the GPU: split a count matrix into train and test counts.

Every stored count x is split into x_test ~ Binomial(x, frac) and x_train = x - x_test.  If x ~ Poisson(l) the parts are
independent Poisson((1 - frac) l) and Poisson(frac l): a model fitted to X_train by the usual engine is scored on X_test
by the usual loss with the rate scaled by frac / (1 - frac) (`loss.thinned_mean_negative_pois_llh`), on counts the fit
has not seen and without giving up whole cells.  The split runs in the library (schpf_thin_counts[_device]); here are
the argument plumbing and the assembly of the two matrices.
"""
import ctypes

import numpy as np

from . import _lib
from ._call import array_ptr as _p, device_of, library, same_device, stream_of, tensor_ptr as ptr
from .device_input import NUMPY_VALUE_KINDS, classify

__all__ = ["thin_counts"]


def _seed(seed):
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2^64), got %d" % seed)
    return ctypes.c_uint64(seed)


def thin_counts(X, frac, seed=0, device=None):
    """X -> (X_train, X_test) with X_train + X_test == X exactly.

    X: a SciPy sparse matrix, or a torch sparse COO / CSR tensor (whatever DeviceCAVI.upload accepts).  A tensor in GPU
    memory stays there -- nothing of it crosses PCIe -- and the result is two torch sparse COO tensors on the same GPU;
    anything else gives two scipy coo_matrix.  Values keep the input's dtype.

    X_test holds EVERY stored entry of X, in X's order, with its test count, explicit zeros included: the held-out loss
    then averages over the same support as the loss on X.  X_train holds the entries with a positive train count, in X's
    order.

    The split of an entry depends only on (seed, frac, row, col, x): not on the entry's position, the storage format,
    the index or value dtype, or on where the matrix lives.  Entries that share a coordinate (an uncoalesced COO) share
    their random stream and are therefore not split independently: sum duplicates first (X.sum_duplicates(),
    X.coalesce()).

    0 < frac < 1 (and frac >= 2^-32); the values must be non-negative integers <= 2^24 (ValueError names the smallest
    offending entry).  `device`: HIP device ordinal, default the tensor's GPU, else $SCHPF_DEVICE or 0.  A model fitted
    to X_train has seen (1 - frac) of the counts: the scale of its theta is reduced by that factor.
    """
    lib = library()
    inp = classify(X)
    frac, seed = float(frac), _seed(seed)
    stats = (ctypes.c_int64 * 4)()
    if inp.kind == "host":
        from scipy.sparse import coo_matrix
        M = inp.matrix
        data = np.ascontiguousarray(M.data)
        vals = data if data.dtype in NUMPY_VALUE_KINDS else data.astype(np.float64)
        row = np.ascontiguousarray(M.row, dtype=np.int32)
        col = np.ascontiguousarray(M.col, dtype=np.int32)
        train, test = np.empty(inp.nnz, np.int32), np.empty(inp.nnz, np.int32)
        _lib.check(lib.schpf_thin_counts(device_of(device), inp.nnz, _p(row), _p(col), _p(vals),
                                         NUMPY_VALUE_KINDS[vals.dtype], frac, seed, _p(train), _p(test), stats))
        keep = train > 0
        return (coo_matrix((train[keep].astype(data.dtype), (row[keep], col[keep])), shape=inp.shape),
                coo_matrix((test.astype(data.dtype), (row, col)), shape=inp.shape))

    import torch
    same_device(inp.device, device, "X")
    dev = torch.device("cuda", inp.device)
    col = inp.minor
    if inp.kind == "coo":
        row = inp.major
    else:      # a CSR's row of every entry, from its row pointers: plumbing, with torch
        crow = inp.major
        row = torch.repeat_interleave(torch.arange(inp.shape[0], device=dev, dtype=col.dtype),
                                      (crow[1:] - crow[:-1]).to(torch.int64), output_size=inp.nnz)
    with torch.cuda.device(dev):
        train = torch.empty(inp.nnz, dtype=torch.int32, device=dev)
        test = torch.empty(inp.nnz, dtype=torch.int32, device=dev)
        # on torch's current stream: ordered after whatever produced X and before whatever reads the result
        _lib.check(lib.schpf_thin_counts_device(inp.device, stream_of(dev), inp.nnz, ptr(row), ptr(col),
                                                inp.minor_kind, ptr(inp.values), inp.value_kind, frac, seed, ptr(train),
                                                ptr(test), stats))
        index = torch.stack([row, col]).to(torch.int64)
        keep = train > 0
        dtype = inp.values.dtype
        return (torch.sparse_coo_tensor(index[:, keep], train[keep].to(dtype), inp.shape),
                torch.sparse_coo_tensor(index, test.to(dtype), inp.shape))
