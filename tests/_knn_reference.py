"""NumPy yardstick and input makers of the nearest-neighbour tests, and the ctypes calls of the three
entry points."""
import ctypes

import numpy as np

DTYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}   # SCHPF_F32, SCHPF_F64


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def integer_scores(n, K, dtype, seed):
    """Values in {0, .., 3}: every difference, square and sum is exact in double, and most pairs tie."""
    return np.random.RandomState(seed).randint(0, 4, (n, K)).astype(dtype)


def gamma_scores(n, K, dtype=np.float64, seed=0):
    """Cell scores as a fit leaves them: Gamma-distributed, a few factors large, most small."""
    return np.random.RandomState(seed).gamma(0.3, 2.0, (n, K)).astype(dtype)


def numpy_d2(query, ref):
    """All squared distances in double, by NumPy's own summation."""
    a, b = np.asarray(query, np.float64), np.asarray(ref, np.float64)
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def numpy_knn(query, ref, k, self_first=-1):
    """The k smallest keys (d2, r) per row by a stable lexsort; exact only where numpy_d2 is (integer_scores)."""
    d2 = numpy_d2(query, ref)
    n_ref = d2.shape[1]
    idx = np.empty((d2.shape[0], k), np.int32)
    out = np.empty((d2.shape[0], k), np.float64)
    for q in range(d2.shape[0]):
        r = np.arange(n_ref)
        if self_first >= 0:
            r = r[r != self_first + q]
        order = r[np.lexsort((r, d2[q, r]))][:k]
        idx[q], out[q] = order, d2[q, order]
    return idx, out


def debug_knn(query, ref, k, self_first=-1):
    """schpf_debug_knn: the library's serial restatement on the host."""
    from schpf_amd import _lib
    query = np.ascontiguousarray(query)
    ref = query if ref is query else np.ascontiguousarray(ref)
    assert query.dtype == ref.dtype
    idx = np.full((query.shape[0], k), -7, np.int32)
    d2 = np.full((query.shape[0], k), -7.0, np.float64)
    _lib.check(_lib.load().schpf_debug_knn(DTYPES[query.dtype], query.shape[0], ref.shape[0], query.shape[1], _p(query),
                                           _p(ref), k, ctypes.c_int64(self_first), _p(idx), _p(d2)))
    return idx, d2


def host_knn(query, ref, k, self_first=-1):
    """schpf_knn: host pointers, staged through the device."""
    from schpf_amd import _lib
    query = np.ascontiguousarray(query)
    ref = query if ref is query else np.ascontiguousarray(ref)
    idx = np.full((query.shape[0], k), -7, np.int32)
    d2 = np.full((query.shape[0], k), -7.0, np.float64)
    _lib.check(_lib.load().schpf_knn(0, DTYPES[query.dtype], query.shape[0], ref.shape[0], query.shape[1], _p(query),
                                     _p(ref), k, ctypes.c_int64(self_first), _p(idx), _p(d2)))
    return idx, d2


def bits(d2):
    return np.ascontiguousarray(d2, np.float64).view(np.uint64)
