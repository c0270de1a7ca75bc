"""The yardstick of the pairwise rank-sum tests and the callers of the library's three entry points.

The yardstick is written in another shape than the library's host restatement (one std::sort per gene and a merge of two
value lists per pair): for every pair the rows of the cells of a and b are cut out of the densified matrix,
scipy.stats.rankdata(method="average") ranks them along axis 0, twice the ranks of a are summed, and the ties come from
np.unique's counts.  Everything is an integer, so "equal" means equal.

The matrix makers are those of _ranksum_reference.py; a case is (matrix, labels, G, pairs)."""
import numpy as np
from scipy.stats import rankdata

from _ranksum_reference import (CASES, MESSAGES, _p, dense_gene_case, dense_of, good_call, poisson_counts, random_labels,  # noqa: F401
                                refusals)

NAMES = ("n", "nexpr", "u2", "ties")
BAD_PAIRS = "pairs must name two different groups in [0, ngroups); offending pair %d"


def all_pairs(G):
    a, b = np.triu_indices(G, 1)
    return np.ascontiguousarray(np.stack([a, b], axis=1), np.int32).reshape(-1, 2)


def mixed_pairs(G):
    """Every a < b, then a repeat, a reversed pair and -- for G > 2 -- nothing that names the last group twice over."""
    pairs = all_pairs(G)
    return np.concatenate([pairs, pairs[:1], pairs[:2, ::-1]]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------- the yardstick
def reference_pair_rank_sums(matrix, labels, G, pairs):
    """(n, nexpr, u2, ties) by rankdata on the rows of a ∪ b of the densified matrix."""
    D = dense_of(matrix)
    N, J = D.shape
    labels, pairs = np.asarray(labels), np.asarray(pairs).reshape(-1, 2)
    n = np.bincount(labels[labels >= 0], minlength=G).astype(np.int64)
    nexpr = np.zeros((G, J), np.int64)
    for g in range(G):
        nexpr[g] = (D[labels == g] > 0).sum(axis=0)
    u2, ties = np.zeros((len(pairs), J), np.int64), np.zeros((len(pairs), J), np.int64)
    for p, (a, b) in enumerate(pairs):
        sub = np.concatenate([D[labels == a], D[labels == b]])
        if sub.shape[0] == 0 or J == 0:
            continue
        twice = np.rint(2.0 * rankdata(sub, method="average", axis=0)).astype(np.int64)
        u2[p] = twice[:n[a]].sum(axis=0) - n[a] * (n[a] + 1)
        for j in range(J):
            t = np.unique(sub[:, j], return_counts=True)[1].astype(np.int64)
            ties[p, j] = (t ** 3 - t).sum()
    return n, nexpr, u2, ties


# ---------------------------------------------------------------------------------------------- the library's entry points
def _call(fn, matrix, labels, G, pairs, fill=0):
    from schpf_amd import _lib
    N, J, indptr, indices, data = matrix
    indptr, indices = np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32)
    data, labels = np.ascontiguousarray(data, np.float32), np.ascontiguousarray(labels, np.int32)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    P = len(pairs)
    out = (np.full(G, fill, np.int64), np.full((G, J), fill, np.int64), np.full((P, J), fill, np.int64), np.full((P, J), fill, np.int64))
    _lib.check(fn(N, J, _p(indptr), _p(indices), _p(data), _p(labels), G, _p(pairs), P, *[_p(a) for a in out]))
    return out


def debug_pair_rank_sums(matrix, labels, G, pairs, fill=0):
    """schpf_debug_pair_rank_sums: the library's serial restatement on the host -> (n, nexpr, u2, ties)."""
    from schpf_amd import _lib
    return _call(_lib.load().schpf_debug_pair_rank_sums, matrix, labels, G, pairs, fill)


def host_pair_rank_sums(matrix, labels, G, pairs, fill=0):
    """schpf_pair_rank_sums: host pointers, staged through the device."""
    from schpf_amd import _lib
    lib = _lib.load()
    return _call(lambda *a: lib.schpf_pair_rank_sums(0, *a), matrix, labels, G, pairs, fill)


# ----------------------------------------------------------------------------------------------------- refused calls
def pair_refusals():
    """(message, matrix, labels, G, pairs) of calls the library refuses, in the stated precedence: those of the rank sums
    with a bad pair added to each -- the pair is asked last -- then the pairs' own."""
    N, J, indptr, indices, data, labels, G = good_call()
    good, bad = all_pairs(G), np.array([[0, 1], [1, 1], [0, G]], np.int32)
    out = [(message, matrix, lab, groups, bad if groups == G else good) for message, matrix, lab, groups in refusals(N, J, indptr, indices, data, labels, G)]
    matrix = (N, J, indptr, indices, data)
    for wrong, row in (([[0, 1], [2, 2], [0, 1]], 1), ([[0, 1], [1, 2], [-1, 0]], 2), ([[G, 0]], 0), ([[1, 0], [0, G]], 1)):
        out.append((BAD_PAIRS % row, matrix, labels, G, np.array(wrong, np.int32)))
    out.append(("npairs * ngenes must be below 2^31", matrix, labels, G, ((1 << 31) // J + 1,)))     # a count, no array of that size
    out.append(("npairs must be >= 0", matrix, labels, G, (-1,)))
    return out
