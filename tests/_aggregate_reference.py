"""Pseudobulk restated from the definition alone in NumPy: every stored entry added into int64 tables with
np.add.at.  The host restatement of the library (schpf_debug_group_stats) and, through it, the kernels are held to this bit
for bit.  Also what both group_stats test files share: the matrices, the label sets, the calls of the three entry points
and the spoiled inputs of the refusals."""
import numpy as np
from scipy.sparse import csr_matrix, vstack

from schpf_amd import _lib
from _qc_reference import BINS as QC_BINS, FILL, IDX, LONG, NGENES, NROWS, VALUE_KINDS, _arrays, _device_args, _p, _stream_arg, kernel_matrix, spoiled as qc_spoiled, wide_matrix  # noqa: F401,E501
from _thin_reference import KINDS

BINS = 2048                     # columns per window of the LDS bins (group_stats.hip GS_BINS)
SLAB = 2048                     # positions of the ordered cells per slab (group_stats.hip GS_SLAB)
NARROW_BELOW = 32               # entries of a row per window below which 16 lanes share a row, not 64 (GS_NARROW_BELOW)
COPIES, WIDE_COPIES = 56, 100   # row-permuted copies of the kernel matrix (140 rows) and of the wide matrix (24 rows)
N = COPIES * NROWS              # 7840 cells
FIRST, SECOND = SLAB, 2 * SLAB + 100   # "three groups": a full slab, whose end is a slab's end; three slabs, the last short
SMALL_COLUMNS = 400             # the columns of the G = N case
assert NGENES > BINS + 1 and N - -(-N // 7) > FIRST + SECOND
MESSAGES = {
    "indptr": "group_stats: indptr must be 0 at row 0, must be non-decreasing and must end at nnz; offending row %d",
    "index": "group_stats: column index out of range at entry %d",
    "order": "group_stats: columns must be strictly ascending within a row; offending row %d",
    "value": "group_stats: values must be integer counts in [0, 2^24]; offending entry %d",
    "labels": "group_stats: labels must be in [-1, ngroups); offending cell %d",
    "overflow": "group_stats: sum of squares may overflow: largest value %d over %d cells",
    "product": "ngroups * ngenes must be below 2^31",
}


def numpy_stats(X, labels, ngroups):
    """(n[G], nexpr[G, J], total[G, J], sumsq[G, J]), int64: every stored entry > 0 of a cell with a label >= 0, added where
    it belongs."""
    J = X.shape[1]
    labels = np.asarray(labels, np.int64)
    n = np.zeros(ngroups, np.int64)
    np.add.at(n, labels[labels >= 0], 1)
    group = np.repeat(labels, np.diff(X.indptr))
    v = X.data.astype(np.int64)
    take = (group >= 0) & (v > 0)
    at = group[take] * J + X.indices[take].astype(np.int64)
    nexpr, total, sumsq = (np.zeros(ngroups * J, np.int64) for _ in range(3))
    np.add.at(nexpr, at, 1)
    np.add.at(total, at, v[take])
    np.add.at(sumsq, at, v[take] * v[take])
    return n, nexpr.reshape(ngroups, J), total.reshape(ngroups, J), sumsq.reshape(ngroups, J)


def lanes_per_row(X):
    """The lanes that share a row of X in gs_sum_kernel: the mean share of a window in a row decides."""
    return 16 if X.nnz // X.shape[0] // -(-X.shape[1] // BINS) < NARROW_BELOW else 64


def _stacked(X, copies, seed):
    rng = np.random.RandomState(seed)
    S = vstack([X] + [X[rng.permutation(X.shape[0])] for _ in range(copies - 1)]).tocsr()
    S.sort_indices()
    return S


def stacked_matrix():
    """COPIES row-permuted copies of the kernel matrix of _qc_reference, the first one as it is (row 5 is the 300-entry row):
    7840 x 3301 canonical CSR with int32 counts, two windows of columns, 16 lanes per row."""
    X = _stacked(kernel_matrix()[0], COPIES, 31)
    assert X.shape == (N, NGENES) and X.indptr[6] - X.indptr[5] == LONG and lanes_per_row(X) == 16
    return X


def stacked_wide_matrix():
    """WIDE_COPIES row-permuted copies of the wide matrix: 2400 rows of 100 .. 260 entries, 64 lanes per row, two slabs."""
    X = _stacked(wide_matrix()[0], WIDE_COPIES, 32)
    assert lanes_per_row(X) == 64 and X.shape[0] > SLAB
    return X


def small_matrix():
    """The kernel matrix cut to its first SMALL_COLUMNS columns: every cell its own group keeps G * J small."""
    return kernel_matrix()[0][:, :SMALL_COLUMNS].tocsr()


def slabs_of(labels, ngroups):
    """The slab lengths of every group, as gs_starts_kernel cuts them."""
    n = np.bincount(np.asarray(labels)[np.asarray(labels) >= 0], minlength=ngroups)
    return [[min(SLAB, c - s) for s in range(0, c, SLAB)] for c in n]


def label_sets(ncells, long_row=5):
    """(name, labels int32[ncells], ngroups) for a matrix of ncells rows; the groups are interleaved, not contiguous."""
    rng = np.random.RandomState(5)
    sets = [("one group", np.zeros(ncells, np.int32), 1)]
    # three groups of uneven size among the cells that are not every seventh one
    three = np.full(ncells, -1, np.int32)
    inside = rng.permutation(np.flatnonzero(np.arange(ncells) % 7 != 0))
    if ncells == N:
        sizes = [FIRST, SECOND, len(inside) - FIRST - SECOND]
    else:
        sizes = [len(inside) // 6, len(inside) // 2, len(inside) - len(inside) // 6 - len(inside) // 2]
    three[inside[:sizes[0]]], three[inside[sizes[0]:sizes[0] + sizes[1]]], three[inside[sizes[0] + sizes[1]:]] = 0, 1, 2
    sets.append(("three groups", three, 3))
    gaps = rng.randint(0, 4, ncells).astype(np.int32)
    gaps[gaps >= 2] += 1                                   # groups 0, 1, 3, 4 of 0 .. 5: 2 in the middle and 5 at the end are empty
    sets.append(("empty groups", gaps, 6))
    single = rng.randint(0, 2, ncells).astype(np.int32)
    single[long_row] = 2
    sets.append(("one cell", single, 3))
    return sets


def check_the_cases():
    """The cases the kernels can go wrong on exist in what the tests run, by the constants mirrored from group_stats.hip."""
    three = dict((name, (lab, G)) for name, lab, G in label_sets(N))["three groups"]
    cut = slabs_of(*three)
    assert (three[0][::7] == -1).all()
    assert len(cut[1]) >= 3 and cut[1][-1] < SLAB                       # one group spans three slabs, the last one short
    assert cut[0] == [SLAB]                                             # a group boundary falls on a slab boundary
    assert lanes_per_row(stacked_matrix()) == 16 and lanes_per_row(stacked_wide_matrix()) == 64
    assert len(slabs_of(np.zeros(N, np.int32), 1)[0]) == -(-N // SLAB) > 3


def labels_out(ngroups, J, sumsq=True):
    return [np.full(ngroups, FILL, np.int64), np.full((ngroups, J), FILL, np.int64), np.full((ngroups, J), FILL, np.int64),
            np.full((ngroups, J), FILL, np.int64) if sumsq else None]


def call_group_stats(entry, X, labels, ngroups, device=None, val_dtype=None, out=None, sumsq=True, shape=None):
    """schpf_debug_group_stats (device=None) or schpf_group_stats on the arrays of the CSR X as they are.  Returns [n, nexpr,
    total, sumsq or None], which start as FILL; `out`: the caller's arrays, to look at after a refusal."""
    indptr, indices, val = _arrays(X, val_dtype)
    ncells, J = X.shape if shape is None else shape
    labels = np.ascontiguousarray(labels, np.int32)
    out = labels_out(ngroups, J, sumsq) if out is None else out
    head = () if device is None else (device,)
    _lib.check(getattr(_lib.load(), entry)(*(head + (ncells, J, len(val), _p(indptr), _p(indices), _p(val), KINDS[val.dtype], _p(labels),
                                                      ngroups) + tuple(_p(a) for a in out))))
    return out


def debug_group_stats(X, labels, ngroups, **kw):
    return call_group_stats("schpf_debug_group_stats", X, labels, ngroups, **kw)


def device_group_stats(X, labels, ngroups, device=0, indptr_dtype=np.int64, idx_dtype=np.int32, val_dtype=None, stream=None, sumsq=True):
    """schpf_group_stats_device on tensors of the given dtypes, on `stream` (a torch stream; None: the null stream).  Returns
    the outputs as NumPy arrays; they start as FILL, and come back also where the call was refused (as the second item of
    the ValueError's args)."""
    import torch
    dev, args, ptr, keepalive = _device_args(X, device, indptr_dtype, idx_dtype, val_dtype)
    J = X.shape[1]
    d_labels = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(dev)
    out = [torch.full(s, FILL, dtype=torch.int64, device=dev) for s in ((ngroups,), (ngroups, J), (ngroups, J))]
    out.append(torch.full((ngroups, J), FILL, dtype=torch.int64, device=dev) if sumsq else None)
    torch.cuda.synchronize(dev)
    status = _lib.load().schpf_group_stats_device(device, _stream_arg(stream), *(args + (ptr(d_labels), ngroups) + tuple(ptr(a) for a in out)))
    result = [None if a is None else a.cpu().numpy() for a in out]
    if status:
        raise ValueError(_lib.load().schpf_last_error().decode(), result)
    return result


def equal(got, want):
    """Equal int64 arrays, one after the other; None stays None."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w is None:
            assert g is None
        else:
            assert g.dtype == np.int64 and g.shape == w.shape, (g.dtype, g.shape, w.shape)
            np.testing.assert_array_equal(g, w)


def untouched(out):
    return all(a is None or (a == FILL).all() for a in out)


def spoiled(kind):
    """(X, labels, ngroups, message): an input with two offenders of `kind`, and the message that names the smaller."""
    labels = (np.arange(NROWS) % 3).astype(np.int32)
    if kind in ("below", "above"):
        X = kernel_matrix()[0]
        labels[[100, 31]] = -2 if kind == "below" else 3
        return X, labels, 3, MESSAGES["labels"] % 31
    X, message = qc_spoiled(kind)
    assert message.startswith("qc: ")
    return X, labels, 3, "group_stats: " + message[len("qc: "):]


def overflowing():
    """(X, labels, ngroups, message): 2^24 squared over 32768 cells is 2^63."""
    ncells = 32768
    X = csr_matrix((np.full(1, 2 ** 24, np.int32), np.zeros(1, np.int32), np.concatenate([[0], np.ones(ncells, np.int64)])),
                   shape=(ncells, 1))
    return X, np.zeros(ncells, np.int32), 1, MESSAGES["overflow"] % (2 ** 24, ncells)
