"""The yardstick of the Pearson residual variance per gene: the definition of include/schpf_hip.h on a dense
matrix in NumPy float64, the split into distinct cell totals plus a correction of the stored entries that the kernels use,
the batch rule of highly_variable_genes, a generator of count matrices with the special cases planted, the bound every
restatement is held to, and the library's refusals with their words.  Shared by tests/test_residual_var_host.py and
tests/test_residual_var_gpu.py; everything cached is read-only."""
import ctypes
import functools

import numpy as np

EPS = 2.0 ** -53
NAMES = ("sum", "sumsq", "cell_total", "gene_total")

SIZES = "hvg: ncells, ngenes and nnz must be in [0, 2^31)"
INV_THETA = "hvg: inv_theta must be finite and >= 0"
CLIP = "hvg: clip must be > 0"
NULL_SUMS = "hvg: sum and sumsq must not be NULL"
NULL_INDPTR = "hvg: indptr must not be NULL"
NULL_ENTRIES = "hvg: indices and data must not be NULL"
BAD_INDPTR = "hvg: indptr must be 0 at gene 0, must be non-decreasing and must end at nnz; offending gene %d"
BAD_CELLS = "hvg: cell ids must be in [0, ncells) and strictly ascending within a gene; offending gene %d"
BAD_VALUES = "hvg: values must be integer counts in [0, 2^24]; offending gene %d"


def tolerance(N):
    """A sum of n doubles in any order is within (n - 1) eps sum|terms| of exact; every term carries a few ulps of rcp and
    sqrt; the yardstick rounds as well: 4 N eps, and never below 1e-12."""
    return max(1e-12, 4 * N * EPS)


def inverse(theta):
    return 0.0 if np.isinf(theta) else 1.0 / theta


def dense_reference(X, theta=100.0, clip=None):
    """The definition: (S1, S2, sum |r|, the variance with ddof = 0, the genes ordered by (-variance, gene index))."""
    X = np.asarray(X, dtype=np.float64)
    N, J = X.shape
    clip = np.sqrt(N) if clip is None else clip
    n, s = X.sum(axis=1), X.sum(axis=0)
    T = s.sum()
    q = s / T if T > 0 else np.zeros(J)
    mu = n[:, None] * q[None, :]
    with np.errstate(all="ignore"):
        r = (X - mu) / np.sqrt(mu * (1.0 + mu * inverse(theta)))
    r[mu == 0] = 0.0
    r = np.clip(r, -clip, clip)
    S1, S2 = r.sum(axis=0), (r * r).sum(axis=0)
    var = S2 / N - (S1 / N) ** 2 if N else np.zeros(J)
    return S1, S2, np.abs(r).sum(axis=0), var, np.argsort(-var, kind="stable")


def split_reference(X, theta=100.0, clip=None):
    """(S1, S2, U) the way the kernels sum them: the zero residual at every distinct cell total times its multiplicity, plus
    r - z and r^2 - z^2 at the entries with x > 0."""
    X = np.asarray(X)
    N, J = X.shape
    clip = np.sqrt(N) if clip is None else clip
    inv = inverse(theta)
    n, s = X.sum(axis=1).astype(np.int64), X.sum(axis=0).astype(np.float64)
    q = s / s.sum()
    u, m = np.unique(n, return_counts=True)
    mu = u[:, None].astype(np.float64) * q[None, :]
    z = np.maximum(-np.sqrt(mu / (1.0 + mu * inv)), -clip)
    S1, S2 = (m[:, None] * z).sum(axis=0), (m[:, None] * z * z).sum(axis=0)
    i, j = np.nonzero(X)
    x, mu = X[i, j].astype(np.float64), n[i] * q[j]
    z = np.maximum(-np.sqrt(mu / (1.0 + mu * inv)), -clip)
    r = np.clip((x - mu) / np.sqrt(mu * (1.0 + mu * inv)), -clip, clip)
    np.add.at(S1, j, r - z)
    np.add.at(S2, j, r * r - z * z)
    return S1, S2, len(u)


def cut_gap(var, order, n_top):
    """The relative gap of the variance between the last selected gene and the first one left out."""
    return (var[order[n_top - 1]] - var[order[n_top]]) / var[order[n_top - 1]]


def batch_reference(X, batch, n_top, theta=100.0):
    """The batch rule: (the genes in their final order, n_batches, the median rank, the mean variance)."""
    X = np.asarray(X)
    J = X.shape[1]
    labels = np.unique(batch)
    ranks, var = np.empty((len(labels), J)), np.zeros(J)
    for b, label in enumerate(labels):
        _, _, _, var_b, order = dense_reference(X[batch == label], theta)
        ranks[b, order] = np.arange(J)
        var += var_b
    ranks[ranks >= n_top] = np.nan
    n_batches = (~np.isnan(ranks)).sum(axis=0)
    median = np.array([np.median(ranks[~np.isnan(ranks[:, g]), g]) if n_batches[g] else np.inf for g in range(J)])
    order = sorted(range(J), key=lambda g: (-n_batches[g], median[g], g))
    return np.array(order), n_batches, median, var / len(labels)


# ------------------------------------------------------------------------------------------------------------- matrices
def counts(N, J, seed):
    """Negative-binomial-like counts with a planted block of co-varying genes, dense int64.  From 8 x 8 up: gene 0 without
    counts, cell 3 without counts, gene 1 expressed in every other cell, and one entry of a sparse gene so large that its
    residual exceeds sqrt(N)."""
    rng = np.random.default_rng(seed)
    lam = rng.gamma(0.3, 2.0, size=J) * (1 + 5 * (rng.random(J) < 0.1))
    size = rng.lognormal(0, 0.6, size=N)
    program = np.ones((N, J))
    program[: N // 5, : J // 6] = 6.0
    X = rng.poisson(size[:, None] * lam[None, :] * program * rng.gamma(2.0, 0.5, size=(N, J))).astype(np.int64)
    if N >= 8 and J >= 8:
        X[:, 1] += 1
        X[N - 1, J - 1] = 5000
        X[:, 0] = 0
        X[3, :] = 0
    elif not X.any():
        X[0, 0] = 3
    return X


def equal_totals(N, J, seed, total=40):
    """Every cell has the same total: one distinct total."""
    rng = np.random.default_rng(seed)
    return rng.multinomial(total, rng.dirichlet(np.full(J, 0.3)), size=N).astype(np.int64)


def distinct_totals(N, J, seed):
    """Cell c has the total c + 1: as many distinct totals as cells."""
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.full(J, 0.3))
    return np.stack([rng.multinomial(c + 1, p) for c in range(N)]).astype(np.int64)


def gene_major(X, stored_zeros=0, seed=0):
    """(N, J, indptr int64, cell ids int32, data float32) of the dense X, gene-major; `stored_zeros` of the zero entries are
    stored as well (gene 1, where the generator planted it, gets its missing cells: a segment of length N)."""
    X = np.asarray(X)
    N, J = X.shape
    stored = X > 0
    if stored_zeros:
        rng = np.random.default_rng(seed)
        zeros = np.flatnonzero(~stored.ravel())
        stored.ravel()[rng.choice(zeros, size=min(stored_zeros, len(zeros)), replace=False)] = True
        if J > 1:
            stored[:, 1] = True
    cols, rows = np.nonzero(stored.T)
    indptr = np.zeros(J + 1, np.int64)
    np.cumsum(stored.sum(axis=0), out=indptr[1:])
    return N, J, indptr, rows.astype(np.int32), X[rows, cols].astype(np.float32)


def _frozen(matrix):
    for a in matrix[2:]:
        a.setflags(write=False)
    return matrix


SHAPES = {"1x1": (1, 1), "63x65": (63, 65), "130x70": (130, 70), "257x129": (257, 129), "70001x67": (70001, 67)}
CASE_NAMES = tuple(SHAPES) + ("equal_totals", "distinct_totals")


@functools.lru_cache(maxsize=None)
def case(name):
    """(dense X, the gene-major matrix with stored zeros); read-only."""
    if name == "equal_totals":
        X = equal_totals(2000, 70, 11)
    elif name == "distinct_totals":
        X = distinct_totals(2000, 70, 12)
    else:
        N, J = SHAPES[name]
        X = counts(N, J, 100 + N)
    X.setflags(write=False)
    return X, _frozen(gene_major(X, stored_zeros=min(X.size // 20, 500), seed=5))


THETAS = (100.0, np.inf)
CLIPS = (None, 2.0)


@functools.lru_cache(maxsize=None)
def expected(name, theta, clip):
    """dense_reference of a case, computed once."""
    out = dense_reference(case(name)[0], theta, clip)
    for a in out:
        a.setflags(write=False)
    return out


def errors(got_sum, got_sumsq, want):
    """(the error of S1 relative to sum |r|, the error of S2 relative to S2), the largest over the genes."""
    S1, S2, absr = want[:3]
    e1 = np.abs(got_sum - S1) / np.maximum(absr, 1e-300)
    e2 = np.abs(got_sumsq - S2) / np.maximum(S2, 1e-300)
    return float(e1.max()), float(e2.max())


# ---------------------------------------------------------------------------------------------------------------- calls
def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)


def outputs(N, J, fill=-7):
    return [np.full(J, fill, np.float64), np.full(J, fill, np.float64), np.full(N, fill, np.int64), np.full(J, fill, np.int64)]


def clip_of(clip, N):
    return float(np.sqrt(N)) if clip is None else float(clip)


def call(entry, matrix, theta=100.0, clip=None, device=None, fill=-7):
    """`entry` (schpf_debug_residual_var, or schpf_residual_var with device=0) on NumPy arrays -> the four arrays."""
    from schpf_amd import _lib
    N, J, indptr, indices, data = matrix
    out = outputs(N, J, fill)
    head = () if device is None else (device,)
    _lib.check(getattr(_lib.load(), entry)(*head, N, J, len(data), indptr.ctypes.data_as(ctypes.c_void_p), _p(indices), _p(data),
                                           inverse(theta), clip_of(clip, N), *[_p(a) for a in out]))
    return out


def good_call():
    """A small valid call: 20 cells, 6 genes, every gene with at least three entries."""
    X = counts(20, 6, 3) + (np.arange(120).reshape(20, 6) % 5 == 0)
    N, J, indptr, indices, data = gene_major(X)
    assert (np.diff(indptr) >= 3).all()
    return N, J, indptr, indices, data


def refusals():
    """(message, dict of the arguments that differ from good_call()): every refusal, the smallest offender and the order."""
    N, J, indptr, indices, data = good_call()
    nnz = len(data)

    def changed(a, at, value):
        b = a.copy()
        b[at] = value
        return b

    def swapped(a, i, j):
        b = a.copy()
        b[i], b[j] = a[j], a[i]
        return b

    e = lambda g, k=0: int(indptr[g]) + k  # noqa: E731
    yield SIZES, {"ncells": -1}
    yield SIZES, {"ngenes": 2 ** 31}
    yield SIZES, {"nnz": 2 ** 31}
    yield SIZES, {"nnz": -1, "inv_theta": -1.0}                                   # the sizes go first
    for bad in (-1e-3, np.nan, np.inf):
        yield INV_THETA, {"inv_theta": bad}
    yield INV_THETA, {"inv_theta": -1.0, "clip": 0.0}
    for bad in (0.0, -2.0, np.nan):
        yield CLIP, {"clip": bad}
    yield CLIP, {"clip": 0.0, "sum": None}
    yield NULL_SUMS, {"sum": None}
    yield NULL_SUMS, {"sumsq": None, "indptr": None}
    yield NULL_INDPTR, {"indptr": None, "indices": None}
    yield NULL_ENTRIES, {"indices": None}
    yield NULL_ENTRIES, {"data": None}
    yield BAD_INDPTR % 0, {"indptr": changed(indptr, 0, 1)}
    yield BAD_INDPTR % 2, {"indptr": changed(indptr, 3, indptr[2] - 1)}
    yield BAD_INDPTR % 1, {"indptr": changed(changed(indptr, 4, indptr[3] - 1), 2, indptr[1] - 1)}     # the smaller gene
    yield BAD_INDPTR % (J - 1), {"nnz": nnz - 1}
    yield BAD_INDPTR % (J - 1), {"nnz": nnz + 1}
    yield BAD_INDPTR % 2, {"indptr": changed(indptr, 3, indptr[2] - 1), "indices": changed(indices, e(0), N)}   # indptr first
    yield BAD_CELLS % 1, {"indices": changed(indices, e(1, 1), N)}
    yield BAD_CELLS % 4, {"indices": changed(indices, e(4), -1)}
    yield BAD_CELLS % 3, {"indices": swapped(indices, e(3), e(3, 1))}
    yield BAD_CELLS % 2, {"indices": changed(indices, e(2, 1), indices[e(2)])}                            # a repeated cell
    yield BAD_CELLS % 2, {"indices": changed(changed(indices, e(5), N), e(2), -3)}                       # the smaller gene
    yield BAD_CELLS % 3, {"indices": changed(indices, e(3), N), "data": changed(data, e(1), 0.5)}         # cells before values
    for bad in (1.5, -1.0, np.nan, np.inf, 2.0 ** 24 + 2, 1e-45, 0.25):
        yield BAD_VALUES % 2, {"data": changed(data, e(2, 1), np.float32(bad))}
    yield BAD_VALUES % 1, {"data": changed(changed(data, e(4), -2.0), e(1, 2), 2.5)}                     # the smaller gene


def refused(entry, change, device=None):
    """The status, the message and the outputs (which held -7) of a call of `entry` with `change` applied to good_call()."""
    from schpf_amd import _lib
    N, J, indptr, indices, data = good_call()
    out = dict(zip(NAMES, outputs(N, J)))
    args = {"ncells": N, "ngenes": J, "nnz": len(data), "indptr": indptr, "indices": indices, "data": data, "inv_theta": 0.01,
            "clip": float(np.sqrt(N))}
    args.update(out)
    args.update(change)
    head = () if device is None else (device,)
    lib = _lib.load()
    status = getattr(lib, entry)(*head, args["ncells"], args["ngenes"], args["nnz"], *[_p(args[k]) for k in ("indptr", "indices", "data")],
                                 args["inv_theta"], args["clip"], *[_p(args[k]) for k in NAMES])
    return status, lib.schpf_last_error().decode(), list(out.values())
