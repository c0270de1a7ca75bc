"""Cell and gene filtering restated from the definitions alone, as plain loops over one entry at a time: the
axis statistics and the submatrix.  The host restatements of the library (schpf_debug_axis_stats, schpf_debug_submatrix)
and, through them, the kernels are held to these bit for bit; SciPy is a second witness, not the definition.  Also what
both qc test files share: the kernel matrix, the calls of the library and the spoiled matrices of the refusals."""
import ctypes

import numpy as np
from scipy.sparse import csr_matrix

from schpf_amd import _lib
from _thin_reference import KINDS

PIECE = 64                      # entries of a row a wavefront handles per pass
BINS = 3072                     # columns per window of the gene side's LDS bins (qc.hip QC_BINS)
NGENES = BINS + 229             # more than one window, the second one short
NROWS = 140
EVERY, EMPTY = 7, 11            # the column stored in every row that stores anything, and the column no row stores
LONG = 300                      # the long row: more than four pieces of a wavefront
NARROW_BELOW = 32               # entries of a row per window below which 16 lanes share a row, not 64 (qc.hip QC_NARROW_BELOW)
assert NGENES > BINS + 1 and LONG > 4 * PIECE
FILL = -7                       # what the outputs hold before a call
IDX = {np.dtype(np.int32): _lib.IDX_I32, np.dtype(np.int64): _lib.IDX_I64}
MESSAGES = {
    "indptr": "qc: indptr must be 0 at row 0, must be non-decreasing and must end at nnz; offending row %d",
    "index": "qc: column index out of range at entry %d",
    "order": "qc: columns must be strictly ascending within a row; offending row %d",
    "value": "qc: values must be integer counts in [0, 2^24]; offending entry %d",
    "rows": "qc: rows must be in [0, ncells); offending position %d",
    "overflow": "qc: sum of squares may overflow: largest value %d over %d cells",
    "capacity": "capacity must be at least the %d entries of the result, got %d",
}


def loop_stats(X, flags=None, n_sets=0):
    """(cell_n, cell_total, cell_set_total[n_sets, N], gene_n, gene_total, gene_sumsq), int64, one entry after the other."""
    N, J = X.shape
    cell_n, cell_total, cell_set = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros((n_sets, N), np.int64)
    gene_n, gene_total, gene_sumsq = np.zeros(J, np.int64), np.zeros(J, np.int64), np.zeros(J, np.int64)
    for i in range(N):
        for e in range(X.indptr[i], X.indptr[i + 1]):
            j, v = int(X.indices[e]), int(X.data[e])
            if v <= 0:
                continue
            cell_n[i] += 1
            cell_total[i] += v
            for s in range(n_sets):
                if (int(flags[j]) >> s) & 1:
                    cell_set[s, i] += v
            gene_n[j] += 1
            gene_total[j] += v
            gene_sumsq[j] += v * v
    return cell_n, cell_total, cell_set, gene_n, gene_total, gene_sumsq


def loop_submatrix(X, rows=None, keep=None):
    """(out_ngenes, out_indptr int64, out_indices int32, out_values of X's dtype) of X[rows][:, keep]: the kept entries of
    every listed row in their stored order, the values as they are."""
    N, J = X.shape
    rows = range(N) if rows is None else [int(r) for r in rows]
    new, kept = [], 0
    for j in range(J):
        new.append(kept)
        kept += 1 if keep is None or keep[j] else 0
    indptr, where = [0], []
    for r in rows:
        for e in range(X.indptr[r], X.indptr[r + 1]):
            if keep is None or keep[int(X.indices[e])]:
                where.append(e)
        indptr.append(len(where))
    where = np.array(where, np.int64)
    indices = np.array([new[int(X.indices[e])] for e in where], np.int32)
    return kept, np.array(indptr, np.int64), indices, X.data[where]


def kernel_matrix():
    """(X, flags): the smallest matrix on which the kernels can go wrong, 140 x 3301 canonical CSR with int32 counts, and a
    random 32-bit flag word per gene.  Rows 0 .. 5 hold exactly 0, 1, 63, 64, 65 and LONG = 300 entries, the others 2 ..
    120.  Column EVERY is stored in every row but the empty one, column EMPTY in none; the long row stores the first and
    the last column and both sides of the window boundary BINS; a few stored zeros; one value of 2^24."""
    rng = np.random.RandomState(21)
    lengths = [0, 1, 63, 64, 65, LONG] + list(rng.randint(2, 121, NROWS - 6))
    free = np.setdiff1d(np.arange(NGENES), [EVERY, EMPTY])
    cols = []
    for r, n in enumerate(lengths):
        if n == 0:
            cols.append(np.zeros(0, np.int64))
            continue
        must = [EVERY] + ([0, BINS - 1, BINS, NGENES - 1] if r == 5 else [])
        rest = rng.choice(np.setdiff1d(free, must), n - len(must), replace=False)
        cols.append(np.sort(np.concatenate([must, rest])))
    vals = [rng.randint(1, 41, len(c)).astype(np.int32) for c in cols]
    vals[5][::7] = 0
    vals[9][1] = 0
    vals[20][0] = 2 ** 24
    vals[5][-1] = 2 ** 24 - 1                        # the last column, in the second window
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    X = csr_matrix((np.concatenate(vals), np.concatenate(cols).astype(np.int32), indptr), shape=(NROWS, NGENES))
    flags = rng.randint(0, 2 ** 32, NGENES, dtype=np.uint64).astype(np.uint32)
    return X, flags


def lanes_per_row(X):
    """The lanes of the gene side that share a row of X: the mean share of a window in a row decides."""
    return 16 if X.nnz // X.shape[0] // -(-X.shape[1] // BINS) < NARROW_BELOW else 64


def wide_matrix():
    """(X, flags): 24 rows of 100 .. 260 entries over the columns of the kernel matrix: the gene side gives every row a whole
    wavefront here, and 16 lanes on the kernel matrix.  Every row stores both sides of the window boundary."""
    rng = np.random.RandomState(22)
    cols = [np.sort(np.concatenate([[BINS - 1, BINS], rng.choice(np.setdiff1d(np.arange(NGENES), [BINS - 1, BINS]), n - 2, replace=False)]))
            for n in rng.randint(100, 261, 24)]
    vals = [rng.randint(0, 9, len(c)).astype(np.int32) for c in cols]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    X = csr_matrix((np.concatenate(vals), np.concatenate(cols).astype(np.int32), indptr), shape=(24, NGENES))
    assert lanes_per_row(X) == 64 and lanes_per_row(kernel_matrix()[0]) == 16
    return X, rng.randint(0, 2 ** 32, NGENES, dtype=np.uint64).astype(np.uint32)


VALUE_KINDS = (np.int32, np.int64, np.float32, np.float64)


def row_lists():
    """What both test files take out of the kernel matrix: (name, rows, keep)."""
    rng = np.random.RandomState(3)
    every_other = np.arange(NGENES) % 2 == 0
    return [("one row", [5], None), ("65 rows", list(range(3, 68)), every_other), ("all rows reversed", list(range(NROWS))[::-1], None),
            ("repeats", [5, 5, 0, 139, 5, 2, 2] + list(rng.randint(0, NROWS, 40)), every_other),
            ("every other gene", None, every_other), ("no gene", None, np.zeros(NGENES, bool)), ("no mask", None, None),
            ("the second window alone", [5, 20, 9], np.arange(NGENES) >= BINS)]


def odd_values(dtype):
    """Values a copy must not touch, as bits: stored zeros, 2^24, and for floats -0.0, a NaN with a payload, infinity."""
    if np.dtype(dtype).kind == "f":
        wide = np.dtype(dtype).itemsize == 8
        nan = np.array([0x7FF0DEADBEEF0001 if wide else 0x7FA0BEEF], np.uint64 if wide else np.uint32).view(dtype)[0]
        return np.array([0.0, -0.0, nan, 2.0 ** 24, -1.5, np.inf, 1e-40, 3.0], dtype)
    return np.array([0, -1, 2 ** 24, np.iinfo(dtype).max, np.iinfo(dtype).min, 7, 0, 3], dtype)


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)


def _arrays(X, val_dtype=None):
    val = np.ascontiguousarray(X.data if val_dtype is None else X.data.astype(val_dtype))
    return np.ascontiguousarray(X.indptr, np.int64), np.ascontiguousarray(X.indices, np.int32), val


def stats_out(N, J, n_sets):
    return [np.full(N, FILL, np.int64), np.full(N, FILL, np.int64), np.full((n_sets, N), FILL, np.int64),
            np.full(J, FILL, np.int64), np.full(J, FILL, np.int64), np.full(J, FILL, np.int64)]


def call_stats(entry, X, flags=None, n_sets=0, device=None, val_dtype=None, out=None, shape=None):
    """schpf_debug_axis_stats (device=None) or schpf_axis_stats on the arrays of the CSR X as they are.  Returns the six
    outputs, which start as FILL; `out`: the caller's arrays, to look at after a refusal; `shape`: claimed in X.shape's place."""
    indptr, indices, val = _arrays(X, val_dtype)
    N, J = X.shape if shape is None else shape
    out = stats_out(N, J, n_sets) if out is None else out
    head = () if device is None else (device,)
    _lib.check(getattr(_lib.load(), entry)(*(head + (N, J, len(val), _p(indptr), _p(indices), _p(val), KINDS[val.dtype], n_sets,
                                                      _p(flags)) + tuple(_p(a) for a in out))))
    return out


def debug_stats(X, flags=None, n_sets=0, **kw):
    return call_stats("schpf_debug_axis_stats", X, flags, n_sets, **kw)


def call_submatrix(entry, X, rows=None, keep=None, device=None, val_dtype=None, fill=True, short=0, n_rows=None, out=None):
    """schpf_debug_submatrix (device=None) or schpf_submatrix on the arrays of the CSR X as they are: the sizing call, then
    (fill) the filling call with capacity = the total - short.  Returns (out_ngenes, out_indptr, out_indices, out_values);
    the last two None without fill.  The outputs start as FILL; `out` = [ngenes (c_int64), indptr]: the caller's, to look at
    after a refusal."""
    indptr, indices, val = _arrays(X, val_dtype)
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    keep = None if keep is None else np.ascontiguousarray(keep).astype(np.uint8)
    n_rows = (X.shape[0] if rows is None else len(rows)) if n_rows is None else n_rows
    # an empty list or mask is still one: NULL would ask for all rows, or keep all genes
    ptr = lambda a: None if a is None else (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    kept, out_indptr = (ctypes.c_int64(FILL), np.full(n_rows + 1, FILL, np.int64)) if out is None else out
    head = () if device is None else (device,)
    fn = getattr(_lib.load(), entry)
    args = head + (X.shape[0], X.shape[1], len(val), _p(indptr), _p(indices), _p(val), KINDS[val.dtype], n_rows,
                   ptr(rows), ptr(keep))
    _lib.check(fn(*(args + (ctypes.byref(kept), _p(out_indptr), None, None, 0))))
    if not fill:
        return int(kept.value), out_indptr, None, None
    total = int(out_indptr[-1])
    again_kept, again = ctypes.c_int64(FILL), np.full(n_rows + 1, FILL, np.int64)
    out_indices = np.full(max(total, 1), FILL, np.int32)
    out_values = np.full(max(total, 1) * val.dtype.itemsize, 0xF9, np.uint8).view(val.dtype)
    _lib.check(fn(*(args + (ctypes.byref(again_kept), _p(again), _p(out_indices), _p(out_values), total - short))))
    assert (again == out_indptr).all() and again_kept.value == kept.value
    return int(kept.value), out_indptr, out_indices[:total], out_values[:total]


def debug_submatrix(X, rows=None, keep=None, **kw):
    return call_submatrix("schpf_debug_submatrix", X, rows, keep, **kw)


def bits(a):
    """The bytes of an array as unsigned integers of its width: what "bit for bit" compares (NaN payloads, -0.0)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want):
    """Equal dtypes and equal bits, array by array."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
            assert (bits(g) == bits(w)).all()
        else:
            assert g == w


# ---- the _device entry points: the arrays as torch tensors on the GPU, any index and value dtype, a caller's stream ----

def _device_args(X, device, indptr_dtype, idx_dtype, val_dtype):
    import torch
    dev = torch.device("cuda", device)
    indptr = torch.from_numpy(np.ascontiguousarray(X.indptr, indptr_dtype)).to(dev)
    indices = torch.from_numpy(np.ascontiguousarray(X.indices, idx_dtype)).to(dev)
    val = torch.from_numpy(np.ascontiguousarray(X.data if val_dtype is None else X.data.astype(val_dtype))).to(dev)
    keepalive = (indptr, indices, val)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)  # noqa: E731
    args = (X.shape[0], X.shape[1], int(val.numel()), ptr(indptr), IDX[np.dtype(indptr_dtype)], ptr(indices), IDX[np.dtype(idx_dtype)],
            ptr(val), KINDS[np.dtype(val.cpu().numpy().dtype)])
    return dev, args, ptr, keepalive


def _stream_arg(stream):
    return ctypes.c_void_p(_lib.STREAM_DEFAULT if stream is None else int(stream.cuda_stream))


def device_stats(X, flags=None, n_sets=0, device=0, indptr_dtype=np.int64, idx_dtype=np.int32, val_dtype=None, stream=None):
    """schpf_axis_stats_device on tensors of the given dtypes, on `stream` (a torch stream; None: the null stream).  Returns
    the six outputs as NumPy arrays; they start as FILL, and come back also where the call was refused (as the second item
    of the ValueError's args)."""
    import torch
    dev, args, ptr, keepalive = _device_args(X, device, indptr_dtype, idx_dtype, val_dtype)
    N, J = X.shape
    d_flags = None if flags is None else torch.from_numpy(flags.view(np.int32)).to(dev)
    out = [torch.full(s, FILL, dtype=torch.int64, device=dev) for s in ((N,), (N,), (n_sets, N), (J,), (J,), (J,))]
    torch.cuda.synchronize(dev)
    status = _lib.load().schpf_axis_stats_device(device, _stream_arg(stream), *(args + (n_sets, ptr(d_flags)) + tuple(ptr(a) for a in out)))
    result = [a.cpu().numpy() for a in out]
    if status:
        raise ValueError(_lib.load().schpf_last_error().decode(), result)
    return result


def device_submatrix(X, rows=None, keep=None, device=0, indptr_dtype=np.int64, idx_dtype=np.int32, val_dtype=None, stream=None,
                     fill=True, short=0):
    """schpf_submatrix_device likewise: the sizing call, then (fill) the filling call with capacity = the total - short.
    A refusal raises ValueError(message, outputs as they are then)."""
    import torch
    dev, args, ptr, keepalive = _device_args(X, device, indptr_dtype, idx_dtype, val_dtype)
    val = keepalive[2]
    d_rows = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(dev)
    d_keep = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep).astype(np.uint8)).to(dev)
    n_rows = X.shape[0] if rows is None else len(rows)
    if d_rows is not None and n_rows == 0:
        d_rows = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = _lib.load()
    kept, out_indptr = ctypes.c_int64(FILL), torch.full((n_rows + 1,), FILL, dtype=torch.int64, device=dev)
    args = (device, _stream_arg(stream)) + args + (n_rows, ptr(d_rows), ptr(d_keep))
    torch.cuda.synchronize(dev)
    if lib.schpf_submatrix_device(*(args + (ctypes.byref(kept), ptr(out_indptr), None, None, 0))):
        raise ValueError(lib.schpf_last_error().decode(), [kept.value, out_indptr.cpu().numpy()])
    first = out_indptr.cpu().numpy()
    if not fill:
        return int(kept.value), first, None, None
    total = int(first[-1])
    again_kept, again = ctypes.c_int64(FILL), torch.full((n_rows + 1,), FILL, dtype=torch.int64, device=dev)
    out_indices = torch.full((max(total, 1),), FILL, dtype=torch.int32, device=dev)
    out_values = torch.full((max(total, 1),), FILL, dtype=val.dtype, device=dev)
    if lib.schpf_submatrix_device(*(args + (ctypes.byref(again_kept), ptr(again), ptr(out_indices), ptr(out_values), total - short))):
        raise ValueError(lib.schpf_last_error().decode(), [again_kept.value, again.cpu().numpy(), out_indices.cpu().numpy(),
                                                           out_values.cpu().numpy()])
    assert (again.cpu().numpy() == first).all() and again_kept.value == kept.value
    return int(kept.value), first, out_indices[:total].cpu().numpy(), out_values[:total].cpu().numpy()


def spoiled(kind):
    """(X, message): the kernel matrix with two offenders of `kind`, the smaller one placed behind the larger one in memory
    order of the launch, and the message that names the smaller."""
    X, _ = kernel_matrix()
    X = X.copy()
    if kind == "indptr":
        X.indptr = X.indptr.astype(np.int64)
        X.indptr[100], X.indptr[30] = X.indptr[99] - 1, X.indptr[29] - 1       # rows 99 and 29 end before they start
        return X, MESSAGES[kind] % 29
    if kind == "indptr_end":
        X.indptr = X.indptr.astype(np.int64)
        X.indptr[NROWS] += 1
        return X, MESSAGES["indptr"] % NROWS
    if kind == "index":
        late, early = int(X.indptr[90]), int(X.indptr[5]) + 100
        X.indices[late], X.indices[early] = NGENES, -1
        return X, MESSAGES[kind] % early
    if kind == "order":
        for r in (90, 5):
            e = int(X.indptr[r]) + 2
            assert e < X.indptr[r + 1]
            X.indices[e] = X.indices[e - 1]                                    # a duplicate: not strictly ascending
        return X, MESSAGES[kind] % 5
    assert kind == "value"
    X.data[int(X.indptr[90])] = -1
    X.data[int(X.indptr[5]) + 200] = 2 ** 24 + 1
    return X, MESSAGES[kind] % (int(X.indptr[5]) + 200)
