"""Pseudobulk on the GPU: exact sums per group of cells and gene.

After the clusters, every question is asked per group of cells: the counts of each gene summed over a cluster, the same per
sample x cluster -- the pseudobulk table that DESeq2- or edgeR-style differential expression between conditions takes --
and per-group mean, variance and fraction of expressing cells for dot plots and annotation.  `group_stats` hands the count
matrix and one label per cell to the library (schpf_group_stats[_device]) and gets exact int64 sums back, the same bits
wherever the matrix lives and however the work was scheduled; `group_codes` turns one or several per-cell keys (a sample
id, a cluster) into those labels; `pseudobulk` puts the two together.

    labels = model.clusters()
    bulk = pseudobulk(X, (sample_ids, labels), min_cells=10)
    bulk["counts"]          # groups x genes, int64: what DESeq2 takes
    bulk["groups"]          # one (sample, cluster) per row
"""
import numpy as np

from . import _lib
from ._call import array_ptr as _p, device_of, library, stream_of, tensor_ptr as ptr
from .device_input import (NUMPY_VALUE_KINDS, gpu_csr, host_csr, host_csr_arrays, int32_labels, is_torch_tensor, on_gpu,
                           to_numpy as _host)

__all__ = ["group_stats", "pseudobulk", "group_codes"]

NAMES = ("n", "nexpr", "total", "sumsq")


def _group_stats_host(ncells, ngenes, indptr, indices, vals, labels, ngroups, sumsq, device):
    """schpf_group_stats on NumPy arrays: [n[G], nexpr[G, J], total[G, J], sumsq[G, J] or None]."""
    lib = library()
    out = [np.zeros(ngroups, np.int64), np.zeros((ngroups, ngenes), np.int64), np.zeros((ngroups, ngenes), np.int64),
           np.zeros((ngroups, ngenes), np.int64) if sumsq else None]
    _lib.check(lib.schpf_group_stats(device, ncells, ngenes, len(vals), _p(indptr), _p(indices), _p(vals),
                                     NUMPY_VALUE_KINDS[vals.dtype], _p(labels), ngroups, *[_p(a) for a in out]))
    return out


def _sizes(labels, ngroups, ncells, ngenes, nnz=0):
    """G = ngroups or the largest label + 1, at least 1; what the library refuses before it reads anything is said here,
    before anything is converted, in the library's words."""
    if len(labels.shape) != 1 or labels.shape[0] != ncells:
        raise ValueError("labels must hold one label per cell: %d, got shape %s" % (ncells, tuple(labels.shape)))
    if ngroups is None:
        ngroups = max(1, int(labels.max()) + 1) if ncells else 1
    ngroups = int(ngroups)
    for name, size in (("ncells", ncells), ("ngenes", ngenes), ("nnz", nnz)):
        if size >= 2 ** 31:
            raise ValueError("%s must be in [0, 2^31)" % name)
    if ngroups < 1 or ngroups >= 2 ** 31:
        raise ValueError("ngroups must be in [1, 2^31)")
    if ngroups * ngenes >= 2 ** 31:
        raise ValueError("ngroups * ngenes must be below 2^31")
    return ngroups


def _labels_int32(labels):
    """Labels outside int32 cannot be in [-1, ngroups): the first one is named before the cast could hide it."""
    return int32_labels(labels, -1, "group_stats: labels must be in [-1, ngroups); offending cell %d")


def group_stats(X, labels, ngroups=None, sumsq=True, device=None):
    """Per group of cells and gene, the exact sums of a cells x genes count matrix X: a dict of int64 arrays n[G] (the cells
    per group), nexpr[G, J] (the cells of the group with a count > 0), total[G, J] (the sum of their counts) and, with
    `sumsq`, sumsq[G, J] (the sum of the squares).

    X: non-negative integer counts <= 2^24.  A torch sparse CSR or COO tensor on a GPU stays there -- a COO is brought to
    canonical CSR with torch on that GPU, duplicates summed -- the sums run on torch's current stream and tensors on that
    GPU come back.  Anything else, a torch tensor in host memory included, goes through SciPy (`tocsr()` and
    `sum_duplicates()` on a copy) and the GPU `device` ($SCHPF_DEVICE or 0), and NumPy arrays come back.

    labels: one integer per cell in [-1, G), NumPy or a tensor; -1 puts the cell in no group.  ngroups: G, default the
    largest label + 1, at least 1.  G * J < 2^31.  What the library refuses raises ValueError naming the smallest offending
    row, entry or cell."""
    if on_gpu(X):
        import torch
        lib = library()
        lab = (labels if is_torch_tensor(labels) else torch.as_tensor(np.asarray(labels))).detach()
        N, J = int(X.shape[0]), int(X.shape[1])
        G = _sizes(lab, ngroups, N, J)
        if lab.numel() and (int(lab.min()) < -1 or int(lab.max()) > np.iinfo(np.int32).max):
            _labels_int32(lab.cpu().numpy())
        inp, dev = gpu_csr(X, device)
        with torch.cuda.device(dev):
            stream = stream_of(dev)
            lab = lab.to(device=dev, dtype=torch.int32).contiguous()
            n = torch.zeros(max(G, 1), dtype=torch.int64, device=dev)
            out = [torch.zeros((G, J), dtype=torch.int64, device=dev) for _ in range(3 if sumsq else 2)] + ([] if sumsq else [None])
            _lib.check(lib.schpf_group_stats_device(inp.device, stream, N, J, inp.nnz, ptr(inp.major), inp.major_kind, ptr(inp.minor),
                                                    inp.minor_kind, ptr(inp.values), inp.value_kind, ptr(lab), G, ptr(n),
                                                    *[ptr(t) for t in out]))
        found = [n] + out
    else:
        lab = _host(labels)
        G = _sizes(lab, ngroups, int(X.shape[0]), int(X.shape[1]))
        lab = _labels_int32(lab)
        C = host_csr(X, canonical=True)
        N, J = C.shape
        found = _group_stats_host(N, J, *(host_csr_arrays(C) + (lab, G, bool(sumsq), device_of(device))))
    return {name: a for name, a in zip(NAMES, found) if a is not None}


def _key(values):
    """One per-cell key as (codes, levels): codes[i] the rank of cell i's value among the distinct ones, -1 for a no-group
    value (the integer -1; None or the empty string)."""
    values = _host(values)
    if values.ndim != 1:
        raise ValueError("a key must hold one value per cell, got shape %s" % (values.shape,))
    if values.dtype.kind in "iub":
        none = values == -1 if values.dtype.kind == "i" else np.zeros(len(values), bool)
    elif values.dtype.kind in "OUS":
        none = np.array([v is None or (isinstance(v, (str, bytes)) and len(v) == 0) for v in values], bool)
        values = np.array(["" if v is None else (v.decode() if isinstance(v, bytes) else str(v)) for v in values], dtype=str)
    else:
        raise ValueError("a key must hold integers or strings, got dtype %s" % values.dtype)
    levels, inverse = np.unique(values[~none], return_inverse=True)
    codes = np.full(len(values), -1, np.int64)
    codes[~none] = inverse
    return codes, levels


def group_codes(*keys):
    """(codes int32[N], table): the group of every cell from one or several per-cell keys -- integers or strings, say a
    sample id and a cluster.  `table` holds one row per distinct combination that occurs, in lexicographic order (integers
    by value, strings as strings; the first key is the most significant), as a list of tuples; codes[i] is the row of cell
    i.  A cell with -1 (integers) or None / "" (strings) in any key is in no group: code -1.  Plain NumPy on the host."""
    if not keys:
        raise ValueError("group_codes needs at least one key")
    coded = [_key(k) for k in keys]
    N = len(coded[0][0])
    if any(len(c) != N for c, _ in coded):
        raise ValueError("all keys must hold one value per cell: got lengths %s" % ([len(c) for c, _ in coded],))
    inside = np.ones(N, bool)
    combined = np.zeros(N, np.int64)          # mixed radix over the levels: the order of the ranks is the lexicographic one
    for c, levels in coded:
        inside &= c >= 0
        if float(combined.max(initial=0) + 1) * max(len(levels), 1) >= 2.0 ** 62:
            raise ValueError("too many key combinations")
        combined = combined * max(len(levels), 1) + np.maximum(c, 0)
    seen, inverse = np.unique(combined[inside], return_inverse=True)
    if len(seen) >= 2 ** 31:
        raise ValueError("ngroups must be in [1, 2^31)")
    codes = np.full(N, -1, np.int32)
    codes[inside] = inverse
    table, rest = [], seen.copy()
    for c, levels in reversed(coded):
        size = max(len(levels), 1)
        table.append(levels[rest % size] if len(levels) else np.zeros(0, levels.dtype))
        rest //= size
    table = table[::-1]
    return codes, [tuple(col[g].item() for col in table) for g in range(len(seen))]


def pseudobulk(X, by, min_cells=1, device=None):
    """The pseudobulk table of a cells x genes count matrix X: a dict.

    by: one label array or a tuple of them (a sample id and a cluster), turned into groups by `group_codes`; one call of
    `group_stats`.  Keys: `groups` (the table of key combinations, one tuple per group), `n_cells`, `counts` (G x J int64:
    the sums of the counts, the pseudobulk matrix), `pct` (the fraction of the group's cells with a count > 0), `mean` and
    `var` (over the cells of the group, zeros included, ddof = 1; a one-cell group gets var 0).  Groups with fewer than
    `min_cells` cells are dropped from every array.  `counts` and `n_cells` are exact (tensors on the GPU of X where X is a
    tensor there, else NumPy); `pct`, `mean` and `var` are float64 NumPy worked out from the integers on the host, as
    qc_metrics works out gene_mean and gene_var."""
    keys = by if isinstance(by, (tuple, list)) else (by,)
    codes, table = group_codes(*keys)
    if len(codes) != int(X.shape[0]):
        raise ValueError("the keys must hold one value per cell: %d, got %d" % (int(X.shape[0]), len(codes)))
    found = group_stats(X, codes, ngroups=max(len(table), 1), sumsq=True, device=device)
    n = _host(found["n"])
    keep = np.flatnonzero((n >= min_cells) & (np.arange(len(n)) < len(table)))
    pick = (lambda a: a[_like(keep, a)])
    n_cells, counts = pick(found["n"]), pick(found["total"])
    nf = n[keep].astype(np.float64)[:, None]
    total, sumsq = _host(counts).astype(np.float64), _host(pick(found["sumsq"])).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):   # the formulas of qc._moments, per group
        mean = np.where(nf > 0, total / nf, 0.0)
        var = np.where(nf > 1, (sumsq - total * total / nf) / (nf - 1), 0.0)
        pct = np.where(nf > 0, _host(pick(found["nexpr"])).astype(np.float64) / nf, 0.0)
    return {"groups": [table[g] for g in keep], "n_cells": n_cells, "counts": counts, "pct": pct, "mean": mean, "var": var}


def _like(index, a):
    """A NumPy index array as one that `a` takes: a tensor on a's device for a tensor."""
    if is_torch_tensor(a):
        import torch
        return torch.from_numpy(index).to(a.device)
    return index
