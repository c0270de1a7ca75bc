"""The yardstick of the exact sparse transpose, the cases both test modules run, and the calls into the library.

Yardstick: `scipy.sparse.csr_matrix.tocsc()` on a CSR with sorted indices -- a stable counting transpose, whose `indptr`,
`indices` and the bytes of `data` are the definition of include/schpf_hip.h: entry (i, j) at out_indptr[j] + the stored
(i', j) with i' < i.  `out_source` is the same transpose of the stored positions 0 .. nnz - 1.  `restated` gives the
definition a second shape in NumPy (a stable argsort of the columns), so that the yardstick is not SciPy alone.  Every
comparison against it is bit for bit: the result is integers and moved bytes, there is no tolerance to choose.

The sizes of the cases follow the constants of csrc/transpose.hip, named here: W columns per window, S rows per slab, and
groups of 64 M rows."""
import ctypes
import functools

import numpy as np

W, S, M = 3072, 2048, 1       # TR_BINS, TR_SLAB, TR_GROUP / 64 of csrc/transpose.hip
FILL = -7                     # what the outputs hold before a call
DEBUG, HOST, DEVICE = "schpf_debug_transpose", "schpf_transpose", "schpf_transpose_device"

VAL_DTYPES = (np.int32, np.int64, np.float32, np.float64)      # SCHPF_VAL_I32 .. SCHPF_VAL_F64
VAL_F32 = 2

BAD_INDPTR = "transpose: indptr must be 0 at row 0, must be non-decreasing and must end at nnz; offending row %d"
BAD_INDEX = "transpose: column index out of range at entry %d"
BAD_ORDER = "transpose: columns must be strictly ascending within a row; offending row %d"


def kind_of(dtype):
    return [np.dtype(d) for d in VAL_DTYPES].index(np.dtype(dtype))


def from_mask(mask, seed, dtype=np.float32, odd_bits=True):
    """(N, J, indptr int64, indices int32, data) of the CSR with an entry wherever `mask` is set.  The values are small
    integers with stored zeros among them; with odd_bits the first entries hold a -0.0 and a NaN with a payload (floats) or
    the extremes (integers), which a move must carry across unchanged."""
    rng = np.random.default_rng(seed)
    N, J = mask.shape
    rows, cols = np.nonzero(mask)                                    # row-major, the columns ascending within a row
    indptr = np.zeros(N + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=N))
    data = rng.integers(0, 5, size=len(cols)).astype(dtype)
    if odd_bits and len(data) >= 3:
        if np.dtype(dtype).kind == "f":
            bits = data.view(np.uint32 if np.dtype(dtype).itemsize == 4 else np.uint64)
            bits[1] = 0x80000000 if bits.dtype == np.uint32 else 0x8000000000000000       # -0.0
            bits[2] = 0x7FC12345 if bits.dtype == np.uint32 else 0x7FF8000000012345       # a NaN with a payload
        else:
            data[1], data[2] = np.iinfo(dtype).min, np.iinfo(dtype).max
    return N, J, indptr, cols.astype(np.int32), data


def random_mask(N, J, density, seed):
    return np.random.default_rng(seed).random((N, J)) < density


def _edges():
    """(S + 1) x (2 W + 1) at 1 %: an empty row, an empty column, a column stored in every row, and the first and the last
    column of every window populated."""
    N, J = S + 1, 2 * W + 1
    mask = random_mask(N, J, 0.01, 5)
    mask[7] = False                       # an empty row
    mask[:, 100] = False                  # an empty column
    mask[:, 200] = True                   # a column in every row ...
    mask[7, 200] = False                  # ... but the empty one
    for c in (0, W - 1, W, 2 * W - 1, 2 * W):
        mask[c % 5::97, c] = True
    mask[7] = False
    return mask


CASES = {
    "1x1": lambda: np.ones((1, 1), bool),
    "1x(W+1)": lambda: np.ones((1, W + 1), bool),                    # one row across two windows
    "64x3 dense": lambda: np.ones((64, 3), bool),                    # every mask bit set: t = 0 and t = 63
    "65x3 dense": lambda: np.ones((65, 3), bool),                    # the cursor is handed to a second group
    "(64M+1)x5": lambda: random_mask(64 * M + 1, 5, 0.3, 1) | (np.arange(64 * M + 1)[:, None] == 64 * M),   # one row past a group
    "(S+1)x(2W+1)": _edges,
    "70001x67": lambda: random_mask(70001, 67, 0.2, 2),              # many slabs, long columns
    "130x9300": lambda: random_mask(130, 9300, 0.05, 3),             # several windows, a short slab
}
MIDDLE = "257x129"                                                   # the case every kind is run on
CASES[MIDDLE] = lambda: random_mask(257, 129, 0.1, 4)
CASE_NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def case(name, dtype=np.float32, odd_bits=True):
    matrix = from_mask(CASES[name](), seed=len(name), dtype=dtype, odd_bits=odd_bits)
    for a in matrix[2:]:
        a.setflags(write=False)
    return matrix


def yardstick(matrix):
    """(out_indptr int64, out_cells int32, out_values of the input's kind, out_source int64) by SciPy's tocsc()."""
    from scipy.sparse import csr_matrix
    N, J, indptr, indices, data = matrix
    C = csr_matrix((data, indices, indptr), shape=(N, J))
    assert C.has_sorted_indices
    T = C.tocsc()
    P = csr_matrix((np.arange(len(data), dtype=np.int64), indices, indptr), shape=(N, J)).tocsc()
    return T.indptr.astype(np.int64), T.indices.astype(np.int32), T.data, P.data.astype(np.int64)


@functools.lru_cache(maxsize=None)
def expected(name, dtype=np.float32, odd_bits=True):
    out = yardstick(case(name, dtype, odd_bits))
    for a in out:
        a.setflags(write=False)
    return out


def restated(matrix):
    """The definition once more, in NumPy: a stable sort of the stored positions by column."""
    N, J, indptr, indices, data = matrix
    order = np.argsort(indices, kind="stable")
    rows = np.repeat(np.arange(N, dtype=np.int32), np.diff(indptr))
    out_indptr = np.zeros(J + 1, np.int64)
    out_indptr[1:] = np.cumsum(np.bincount(indices, minlength=J))
    return out_indptr, rows[order], data[order], order.astype(np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(got, want, what=""):
    for name, g, w in zip(("out_indptr", "out_cells", "out_values", "out_source"), got, want):
        assert same_bits(g, w), "%s %s differs" % (what, name)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def outputs(J, nnz, out_dtype, source=True):
    return [np.full(J + 1, FILL, np.int64), np.full(nnz, FILL, np.int32), np.full(nnz, FILL, out_dtype),
            np.full(nnz, FILL, np.int64) if source else None]


def call(entry, matrix, out_dtype=None, source=True, **change):
    """One call of a host-pointer entry (DEBUG or HOST) -> (status, the library's message, the four outputs, which held FILL).
    change: arguments to replace -- ncells, ngenes, nnz, val_kind, out_val_kind -- or the name of a pointer to pass as NULL
    (`indptr=None`, `out_cells=None`, ...)."""
    from schpf_amd import _lib
    lib = _lib.load()
    N, J, indptr, indices, data = matrix
    out_dtype = np.dtype(out_dtype or data.dtype)
    nnz = len(data)
    out = outputs(J, nnz, out_dtype, source)
    args = {"ncells": N, "ngenes": J, "nnz": nnz, "indptr": _p(indptr), "indices": _p(indices), "val": _p(data),
            "val_kind": kind_of(data.dtype), "out_val_kind": kind_of(out_dtype), "out_indptr": _p(out[0]), "out_cells": _p(out[1]),
            "out_values": _p(out[2]), "out_source": _p(out[3])}
    args.update(change)
    lead = (0,) if entry == HOST else ()
    status = getattr(lib, entry)(*(lead + tuple(args.values())))
    return status, lib.schpf_last_error().decode() if status else "", out


def untouched(out):
    return all(a is None or (a == FILL).all() for a in out)


def spoiled(matrix, indptr=None, indices=None):
    """The matrix with entries of its indptr / indices replaced: {position: value}."""
    N, J, ptr, idx, data = matrix
    ptr, idx = ptr.copy(), idx.copy()
    for at, v in (indptr or {}).items():
        ptr[at] = v
    for at, v in (indices or {}).items():
        idx[at] = v
    return N, J, ptr, idx, data


def argument_refusals():
    """(message, change): what is refused before anything is read, in the order it is asked."""
    return [("ncells must be in [0, 2^31)", {"ncells": -1}), ("ncells must be in [0, 2^31)", {"ncells": 1 << 31}),
            ("ngenes must be in [0, 2^31)", {"ngenes": 1 << 31}), ("nnz must be in [0, 2^31)", {"nnz": -1}),
            ("nnz must be in [0, 2^31)", {"nnz": 1 << 31}), ("unknown index or value kind", {"val_kind": 4}),
            ("unknown index or value kind", {"val_kind": -1, "out_val_kind": -1}),
            ("out_val_kind must be val_kind or SCHPF_VAL_F32", {"out_val_kind": 0}),
            ("out_val_kind must be val_kind or SCHPF_VAL_F32", {"out_val_kind": 3}),
            ("out_indptr must not be NULL", {"out_indptr": None}),
            ("indptr, indices and val must not be NULL", {"indptr": None}),
            ("indptr, indices and val must not be NULL", {"val": None, "out_cells": None}),
            ("out_cells and out_values must not be NULL", {"out_cells": None}),
            ("out_cells and out_values must not be NULL", {"out_values": None})]


def matrix_refusals(matrix):
    """(message, spoiled matrix) on the middle case, in the order of precedence: what stands earlier wins where two are
    planted, and of two offenders of a kind the smaller is named."""
    N, J, indptr, indices, data = matrix
    nnz = len(data)
    long_rows = [r for r in range(N) if indptr[r + 1] - indptr[r] >= 2]
    a, b = long_rows[3], long_rows[40]
    ea, eb = int(indptr[a]), int(indptr[b])
    return [(BAD_INDPTR % 0, spoiled(matrix, indptr={0: 1})),
            (BAD_INDPTR % 9, spoiled(matrix, indptr={10: int(indptr[9]) - 1, 30: 0})),
            (BAD_INDPTR % N, spoiled(matrix, indptr={N: nnz - 1})),
            (BAD_INDPTR % 0, spoiled(matrix, indptr={0: 1}, indices={ea: J, eb + 1: int(indices[eb])})),     # before the entries
            (BAD_INDEX % ea, spoiled(matrix, indices={ea: J, eb: -1})),
            (BAD_INDEX % eb, spoiled(matrix, indices={eb: -1, ea + 1: int(indices[ea])})),                    # before the order
            (BAD_ORDER % a, spoiled(matrix, indices={ea + 1: int(indices[ea]), eb + 1: int(indices[eb])})),    # equal columns
            (BAD_ORDER % b, spoiled(matrix, indices={eb: int(indices[eb + 1]), eb + 1: int(indices[eb])}))]    # descending
