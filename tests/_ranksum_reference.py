"""The yardstick of the rank-sum tests, the matrix makers and the callers of the library's three entry points.

The yardstick is written in another shape than the library's host restatement (one std::sort per gene and a walk over the
runs): the columns are densified, scipy.stats.rankdata(method="average") ranks them along axis 0, twice the ranks are summed
per group, and the ties come from np.unique's counts.  Everything is an integer, so "equal" means equal.

A matrix is the tuple (N, J, indptr, indices, data) of a CSC matrix of cells x genes, so that a test can hand over arrays
no SciPy matrix would hold.  A case is (matrix, labels, G)."""
import ctypes

import numpy as np
from scipy.sparse import coo_matrix, csc_matrix
from scipy.stats import rankdata

NAMES = ("n", "zeros", "ties", "nexpr", "rank2")


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------------- the yardstick
def dense_of(matrix):
    N, J, indptr, indices, data = matrix
    return np.asarray(csc_matrix((data, indices, indptr), shape=(N, J)).todense(), dtype=np.float32).reshape(N, J)


def reference_rank_sums(matrix, labels, G):
    """(n, zeros, ties, nexpr, rank2) by rankdata on the densified columns."""
    D = dense_of(matrix)
    N, J = D.shape
    labels = np.asarray(labels)
    twice = np.rint(2.0 * rankdata(D, method="average", axis=0)).astype(np.int64) if N and J else np.zeros((N, J), np.int64)
    n = np.bincount(labels[labels >= 0], minlength=G).astype(np.int64)
    zeros = (D == 0).sum(axis=0).astype(np.int64)
    ties = np.zeros(J, np.int64)
    for j in range(J):
        t = np.unique(D[:, j], return_counts=True)[1].astype(np.int64)
        ties[j] = (t ** 3 - t).sum()
    nexpr, rank2 = np.zeros((G, J), np.int64), np.zeros((G, J), np.int64)
    for g in range(G):
        inside = labels == g
        nexpr[g] = (D[inside] > 0).sum(axis=0)
        rank2[g] = twice[inside].sum(axis=0)
    return n, zeros, ties, nexpr, rank2


# ----------------------------------------------------------------------------------------------------------- the makers
def as_matrix(X):
    """A SciPy matrix of cells x genes -> the tuple, in canonical CSC form (stored zeros stay)."""
    C = csc_matrix(X, dtype=np.float32)
    C.sum_duplicates()
    return (C.shape[0], C.shape[1], np.ascontiguousarray(C.indptr, np.int64), np.ascontiguousarray(C.indices, np.int32),
            np.ascontiguousarray(C.data, np.float32))


def as_csc(matrix):
    N, J, indptr, indices, data = matrix
    return csc_matrix((data, indices, indptr), shape=(N, J))


def poisson_counts(N, J, seed=0, rate=0.7):
    """Dense Poisson counts with gene-wise rates round `rate`: many ties, many zeros."""
    rng = np.random.RandomState(seed)
    return as_matrix(csc_matrix(rng.poisson(rate * rng.gamma(2.0, 0.5, (1, J)), (N, J)).astype(np.float32)))


def sparse_entries(N, J, per_cell, seed=0):
    """(cells, genes, counts) of N * per_cell draws, never dense: the genes drawn with a skewed popularity, counts 1 + Poisson;
    a pair drawn twice adds up.  The maker of the timing tool's shapes."""
    rng = np.random.RandomState(seed)
    m = int(N) * int(per_cell)
    cells = rng.randint(0, N, m).astype(np.int32)
    genes = np.minimum((J * rng.random_sample(m) ** 2).astype(np.int32), J - 1)
    return cells, genes, (1 + rng.poisson(0.5, m)).astype(np.float32)


def sparse_counts(N, J, per_cell, seed=0):
    cells, genes, values = sparse_entries(N, J, per_cell, seed)
    return as_matrix(coo_matrix((values, (cells, genes)), shape=(N, J)))


def random_labels(N, G, seed=0, outside=0.0):
    """Labels in [0, G), a fraction `outside` of them -1."""
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, G, N).astype(np.int32)
    labels[rng.random_sample(N) < outside] = -1
    return labels


def one_dense_gene(N, value=3.0):
    """One gene expressed in every cell at a single value: one run of N equal keys."""
    return (N, 1, np.array([0, N], np.int64), np.arange(N, dtype=np.int32), np.full(N, value, np.float32))


def all_distinct_gene(N, seed=0):
    rng = np.random.RandomState(seed)
    return (N, 1, np.array([0, N], np.int64), np.arange(N, dtype=np.int32), (rng.permutation(N) + 1).astype(np.float32))


def short_genes(N=500, J=300, seed=0):
    """Genes of 0 to 3 entries each."""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(0, 4, J)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(N, k, replace=False)) for k in lengths] + [np.zeros(0, int)]).astype(np.int32)
    return (N, J, indptr, indices, rng.randint(1, 3, len(indices)).astype(np.float32))


def with_values(matrix, values, seed=0):
    """The same structure, the entries drawn from `values`."""
    N, J, indptr, indices, data = matrix
    rng = np.random.RandomState(seed)
    return (N, J, indptr, indices, np.asarray(values, np.float32)[rng.randint(0, len(values), len(data))])


def scaled(matrix, target_sum):
    from schpf_amd.markers import _scaled
    return as_matrix(_scaled(as_csc(matrix), target_sum))


EMPTY_65 = (65, 7, np.zeros(8, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
ONE = (1, 1, np.array([0, 1], np.int64), np.zeros(1, np.int32), np.array([2.0], np.float32))
SUBNORMAL = [0.0, -0.0, 1e-45, 3e-45, 1e-39, 1.1754944e-38, 0.1, 0.3, 1.5, 2.0]
HUGE = [3e38, 3.4028235e38, 2.9999999e38, 1.0, 3e38]


def some_labels(case):
    """-1 labels and an empty group (group 1 of 4)."""
    labels = random_labels(case[0], 4, seed=5, outside=0.2)
    labels[labels == 1] = 3
    return labels


# the shapes both test files walk; every one fits densified.  The large ones are made once (functools.lru_cache by the callers)
CASES = {
    "one_cell_one_gene": lambda: (ONE, np.zeros(1, np.int32), 1),
    "no_entries": lambda: (EMPTY_65, random_labels(65, 3, 1), 3),
    "poisson_65": lambda: (poisson_counts(65, 7, 1), random_labels(65, 3, 1), 3),
    "poisson_130": lambda: (poisson_counts(130, 7, 2), random_labels(130, 3, 2), 3),
    "all_distinct_3000": lambda: (all_distinct_gene(3000), random_labels(3000, 5, 3), 5),
    "short_genes_300": lambda: (short_genes(), random_labels(500, 7, 4), 7),
    "one_group": lambda: (poisson_counts(130, 7, 2), np.zeros(130, np.int32), 1),
    "groups_300_cells_5000": lambda: (poisson_counts(5000, 5, 6, rate=3.0), random_labels(5000, 300, 6), 300),
    "empty_group_and_outside": lambda: (poisson_counts(301, 40, 7), some_labels((301,)), 4),
    "all_outside": lambda: (poisson_counts(130, 7, 2), np.full(130, -1, np.int32), 3),
    "stored_zeros_and_subnormals": lambda: (with_values(poisson_counts(301, 40, 7, rate=3.0), SUBNORMAL, 8), some_labels((301,)), 4),
    "near_float_max": lambda: (with_values(poisson_counts(301, 40, 7, rate=3.0), HUGE, 9), some_labels((301,)), 4),
    "scaled_to_target_sum": lambda: (scaled(poisson_counts(301, 40, 7), 1e4), some_labels((301,)), 4),
    "scaled_to_median": lambda: (scaled(poisson_counts(301, 40, 7), "median"), some_labels((301,)), 4),
}


def dense_gene_case():
    """70 001 cells, one gene expressed everywhere at a single value -- one run across many workgroups -- and beside it a
    Poisson gene and an all-distinct one."""
    N = 70001
    a, b, c = one_dense_gene(N), poisson_counts(N, 1, 11, rate=2.0), all_distinct_gene(N, 12)
    indptr = np.concatenate([[0], np.cumsum([m[2][1] for m in (a, b, c)])]).astype(np.int64)
    matrix = (N, 3, indptr, np.concatenate([m[3] for m in (a, b, c)]), np.concatenate([m[4] for m in (a, b, c)]))
    return matrix, random_labels(N, 20, 13, outside=0.05), 20


# ----------------------------------------------------------------------------------------------------- refused calls
MESSAGES = {
    "indptr": "indptr must be 0 at gene 0 and must be non-decreasing; offending gene %d",
    "cells": "cell ids must be in [0, ncells) and strictly ascending within a gene; offending gene %d",
    "values": "values must be finite and >= 0; offending gene %d",
    "labels": "labels must be in [-1, ngroups); offending cell %d",
}


def refusals(N, J, indptr, indices, data, labels, G):
    """(message, arguments) of calls the library refuses, from a good matrix with at least 2 entries in the genes used."""
    at = lambda gene, k=0: int(indptr[gene]) + k  # noqa: E731
    out = []

    def add(message, indptr=indptr, indices=indices, data=data, labels=labels, N=N, J=J, G=G):
        out.append((message, (N, J, indptr, indices, data), labels, G))

    bad = indptr.copy()
    bad[0] = 1
    add(MESSAGES["indptr"] % 0, indptr=bad)
    bad = indptr.copy()
    bad[J - 3], bad[J - 1] = bad[J - 4] - 1, bad[J - 2] - 1
    add(MESSAGES["indptr"] % (J - 4), indptr=bad)
    for wrong in (-1, N):
        bad = indices.copy()
        bad[at(J - 1)], bad[at(2, 1)] = N, wrong
        add(MESSAGES["cells"] % 2, indices=bad)
    bad = indices.copy()
    bad[at(3, 1)] = bad[at(3, 0)]                                # twice: not strictly ascending
    add(MESSAGES["cells"] % 3, indices=bad)
    bad = indices.copy()
    bad[at(4, 0)], bad[at(4, 1)] = bad[at(4, 1)], bad[at(4, 0)]
    add(MESSAGES["cells"] % 4, indices=bad)
    for value in (-1e-45, -1.0, np.inf, np.nan):
        bad = data.copy()
        bad[at(3, 1)], bad[at(J - 1)] = value, np.nan
        add(MESSAGES["values"] % 3, data=bad)
    for wrong in (-2, G):
        bad = labels.copy()
        bad[N - 1], bad[7] = G, wrong
        add(MESSAGES["labels"] % 7, labels=bad)
    bad_cells, bad_data, bad_labels = indices.copy(), data.copy(), labels.copy()        # structure before values before labels
    bad_cells[at(5, 1)] = bad_cells[at(5, 0)]
    bad_data[at(1)] = -1.0
    bad_labels[0] = G
    add(MESSAGES["values"] % 1, data=bad_data, labels=bad_labels)
    add(MESSAGES["cells"] % 5, indices=bad_cells, data=bad_data, labels=bad_labels)
    bad_ptr = indptr.copy()                                      # indptr before the cell ids
    bad_ptr[J - 1] = bad_ptr[J - 2] - 1
    add(MESSAGES["indptr"] % (J - 2), indptr=bad_ptr, indices=bad_cells, data=bad_data, labels=bad_labels)
    add("ncells must be in [0, 2^21)", N=1 << 21)                # before anything is read
    add("ncells must be in [0, 2^21)", N=-1)
    add("ngroups must be at least 1", G=0)
    add("ngroups * ngenes must be below 2^31", G=(1 << 31) // J + 1)
    return out


def good_call():
    N, J, indptr, indices, data = poisson_counts(130, 9, 31, rate=2.0)
    assert np.diff(indptr).min() >= 3
    return N, J, indptr, indices, data, random_labels(130, 3, 31, outside=0.1), 3


# ---------------------------------------------------------------------------------------------- the library's entry points
def _call(fn, matrix, labels, G, fill=0):
    from schpf_amd import _lib
    N, J, indptr, indices, data = matrix
    indptr, indices = np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32)
    data, labels = np.ascontiguousarray(data, np.float32), np.ascontiguousarray(labels, np.int32)
    out = (np.full(G, fill, np.int64), np.full(J, fill, np.int64), np.full(J, fill, np.int64), np.full((G, J), fill, np.int64),
           np.full((G, J), fill, np.int64))
    _lib.check(fn(N, J, _p(indptr), _p(indices), _p(data), _p(labels), G, *[_p(a) for a in out]))
    return out


def debug_rank_sums(matrix, labels, G):
    """schpf_debug_rank_sums: the library's serial restatement on the host -> (n, zeros, ties, nexpr, rank2)."""
    from schpf_amd import _lib
    return _call(_lib.load().schpf_debug_rank_sums, matrix, labels, G)


def host_rank_sums(matrix, labels, G):
    """schpf_rank_sums: host pointers, staged through the device."""
    from schpf_amd import _lib
    lib = _lib.load()
    return _call(lambda *a: lib.schpf_rank_sums(0, *a), matrix, labels, G)
