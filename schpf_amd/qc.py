"""Cell and gene filtering on the GPU: QC sums per cell and per gene, and a sparse submatrix.

Two steps of a single-cell workflow that would otherwise take a count matrix in GPU memory back to the host: the statistics
a quality filter looks at before the fit (genes per cell, counts per cell, the share of mitochondrial counts, cells per
gene), and taking cells and genes out of the matrix -- the filter itself, the called doublets after `doublet_scores`, a
subsample, a bootstrap, a validation split.  Both run in the library (schpf_axis_stats[_device],
schpf_submatrix[_device]) and are integer work: every array they return holds the same bits wherever the matrix lives and
however the work was scheduled.

Removing called doublets and refitting:

    found = model.doublets(X, threshold=0.25)
    X_clean = submatrix(X, cells=~found["calls"])
    model = scHPF(K).fit(X_clean)
"""
import ctypes

import numpy as np

from . import _lib
from ._call import array_ptr as _p, device_of, library, stream_of, tensor_ptr as ptr
from .device_input import (NUMPY_VALUE_KINDS, gpu_csr, host_csr, host_csr_arrays, is_torch_tensor, on_gpu,
                           to_numpy as _host)

__all__ = ["qc_metrics", "submatrix", "filter_counts"]

MAX_SETS = 32      # one bit of a gene's flag word per gene set (qc.h QC_MAX_SETS)


def _mask(sel, n, what, ascending=False):
    """A boolean mask of length n or an integer index array -> the boolean mask, in NumPy."""
    sel = _host(sel)
    if sel.dtype == np.bool_:
        if sel.shape != (n,):
            raise ValueError("a boolean %s mask must have shape (%d,), got %s" % (what, n, sel.shape))
        return sel
    if sel.ndim != 1 or (sel.size and not np.issubdtype(sel.dtype, np.integer)):
        raise ValueError("%s must be a boolean mask or a 1-d integer index array" % what)
    if sel.size and (sel.min() < 0 or sel.max() >= n):
        raise ValueError("%s indices must be in [0, %d)" % (what, n))
    if ascending and sel.size > 1 and (np.diff(sel) <= 0).any():
        raise ValueError("%s indices must be strictly ascending: the kept genes keep their order" % what)
    mask = np.zeros(n, np.bool_)
    mask[sel.astype(np.int64)] = True
    return mask


def _flags(gene_sets, ngenes):
    """gene_sets (name -> mask or indices over genes) -> (names, uint32[ngenes] with bit s set for the genes of set s)."""
    names = list(gene_sets or ())
    if len(names) > MAX_SETS:
        raise ValueError("at most %d gene sets, got %d" % (MAX_SETS, len(names)))
    flags = np.zeros(ngenes, np.uint32)
    for s, name in enumerate(names):
        flags[_mask(gene_sets[name], ngenes, "gene set %r" % (name,))] |= np.uint32(1 << s)
    return names, flags


def _rows(cells, ncells):
    """cells (a boolean mask, or row numbers in any order, repeats allowed) -> int32 row numbers in NumPy; None: all."""
    if cells is None:
        return None
    cells = _host(cells)
    if cells.dtype == np.bool_:
        return np.flatnonzero(_mask(cells, ncells, "cell")).astype(np.int32)
    if cells.ndim != 1 or (cells.size and not np.issubdtype(cells.dtype, np.integer)):
        raise ValueError("cells must be a boolean mask or a 1-d integer array of rows")
    bad = (cells < 0) | (cells >= ncells)                # before the cast to int32 could hide it
    if bad.any():
        raise ValueError("qc: rows must be in [0, ncells); offending position %d" % int(np.flatnonzero(bad)[0]))
    return np.ascontiguousarray(cells, dtype=np.int32)


def _axis_stats_host(ncells, ngenes, indptr, indices, vals, n_sets, flags, device):
    """schpf_axis_stats on NumPy arrays: (cell_n, cell_total, cell_set_total[n_sets, ncells], gene_n, gene_total, gene_sumsq)."""
    lib = library()
    out = [np.zeros(ncells, np.int64), np.zeros(ncells, np.int64), np.zeros((n_sets, ncells), np.int64),
           np.zeros(ngenes, np.int64), np.zeros(ngenes, np.int64), np.zeros(ngenes, np.int64)]
    _lib.check(lib.schpf_axis_stats(device, ncells, ngenes, len(vals), _p(indptr), _p(indices), _p(vals),
                                    NUMPY_VALUE_KINDS[vals.dtype], n_sets, _p(flags), *[_p(a) for a in out]))
    return out


def _submatrix_host(ncells, ngenes, indptr, indices, vals, rows, keep, device):
    """schpf_submatrix on NumPy arrays, the sizing call and the filling call: (out_ngenes, out_indptr, out_indices, out_values)."""
    lib = library()
    n_rows = ncells if rows is None else len(rows)
    if rows is not None and n_rows == 0:                  # an empty list is still a list: NULL would ask for all rows
        rows = np.zeros(1, np.int32)
    kept, out_indptr = ctypes.c_int64(0), np.zeros(n_rows + 1, np.int64)
    args = (device, ncells, ngenes, len(vals), _p(indptr), _p(indices), _p(vals), NUMPY_VALUE_KINDS[vals.dtype], n_rows,
            _p(rows), _p(keep), ctypes.byref(kept), _p(out_indptr))
    _lib.check(lib.schpf_submatrix(*(args + (None, None, 0))))                               # the sizes
    total = int(out_indptr[-1])
    out_indices, out_values = np.empty(max(total, 1), np.int32), np.empty(max(total, 1), vals.dtype)
    _lib.check(lib.schpf_submatrix(*(args + (_p(out_indices), _p(out_values), total))))
    return int(kept.value), out_indptr, out_indices[:total], out_values[:total]


def _moments(out, ncells):
    """gene_mean and gene_var (over all cells, zeros included; ddof = 1) in float64 on the host."""
    total, sumsq = _host(out["gene_total"]).astype(np.float64), _host(out["gene_sumsq"]).astype(np.float64)
    out["gene_mean"] = total / ncells if ncells else np.zeros_like(total)
    out["gene_var"] = (sumsq - total * total / ncells) / (ncells - 1) if ncells > 1 else np.zeros_like(total)
    return out


def qc_metrics(X, gene_sets=None, device=None):
    """The sums a quality filter asks of a cells x genes count matrix X: a dict.

    X: non-negative integer counts <= 2^24.  A torch sparse CSR or COO tensor on a GPU stays there -- a COO is brought to
    canonical CSR with torch on that GPU -- the sums run on torch's current stream and int64 tensors on that GPU come back.
    Anything else goes through SciPy (`tocsr()` and `sum_duplicates()` on a copy) and the GPU `device` ($SCHPF_DEVICE or
    0), and NumPy arrays come back.  gene_sets: a dict from a name to a boolean mask or an index array over the genes
    (mitochondrial, ribosomal, ...), at most 32.

    Keys, all int64 and in the bit contract: `cell_n_genes` (the genes with a count > 0; a stored zero is no expression, the
    rule of min_cells_expressing_mask), `cell_total`, `cell_set_total` (a dict, name -> the counts of the cell inside the
    set); `gene_n_cells`, `gene_total`, `gene_sumsq`.  Not in it, float64 NumPy worked out from those on the host:
    `gene_mean` and `gene_var` (over all cells, zeros included, ddof = 1).  What the library refuses raises ValueError
    naming the smallest offending row or entry."""
    if on_gpu(X):
        import torch
        lib = library()
        inp, dev = gpu_csr(X, device)
        N, J = inp.shape
        names, flags = _flags(gene_sets, J)
        with torch.cuda.device(dev):
            stream = stream_of(dev)
            d_flags = torch.from_numpy(flags.view(np.int32)).to(dev)
            cell = torch.zeros((2 + len(names), N), dtype=torch.int64, device=dev)
            gene = torch.zeros((3, J), dtype=torch.int64, device=dev)
            _lib.check(lib.schpf_axis_stats_device(inp.device, stream, N, J, inp.nnz, ptr(inp.major), inp.major_kind, ptr(inp.minor),
                                                   inp.minor_kind, ptr(inp.values), inp.value_kind, len(names), ptr(d_flags),
                                                   ptr(cell[0]), ptr(cell[1]), ptr(cell[2:]), ptr(gene[0]), ptr(gene[1]),
                                                   ptr(gene[2])))
        found = [cell[0], cell[1], cell[2:], gene[0], gene[1], gene[2]]
    else:
        C = host_csr(X, canonical=True)
        N, J = C.shape
        names, flags = _flags(gene_sets, J)
        found = _axis_stats_host(N, J, *(host_csr_arrays(C) + (len(names), flags, device_of(device))))
    out = {"cell_n_genes": found[0], "cell_total": found[1],
           "cell_set_total": {name: found[2][s] for s, name in enumerate(names)},
           "gene_n_cells": found[3], "gene_total": found[4], "gene_sumsq": found[5]}
    return _moments(out, N)


def submatrix(X, cells=None, genes=None, device=None):
    """X[cells][:, genes] of a cells x genes sparse matrix X, without leaving the memory X lives in.

    cells: a boolean mask over the rows, or an integer array of rows in any order, repeats allowed (a subsample, a
    bootstrap, a validation split); None: all.  genes: a boolean mask or a strictly ascending index array; None: all.  The
    kept genes are renumbered in ascending order.  A torch sparse CSR or COO tensor on a GPU stays there (a COO is brought
    to canonical CSR with torch) and a torch sparse CSR tensor on that GPU comes back, one that `fit` and `project` take as
    it is; anything else goes through SciPy (`tocsr()`) and the GPU `device`, and a SciPy csr_matrix comes back.  Within
    a row the entries keep their stored order, and the values are copied byte for byte in their own dtype."""
    if on_gpu(X):
        import torch
        lib = library()
        inp, dev = gpu_csr(X, device)
        N, J = inp.shape
        if is_torch_tensor(cells) and cells.device == dev and cells.dtype in (torch.bool, torch.int32) and cells.dim() == 1:
            if cells.dtype == torch.bool and cells.shape[0] != N:
                raise ValueError("a boolean cell mask must have shape (%d,), got %s" % (N, tuple(cells.shape)))
            rows = (torch.nonzero(cells).flatten().to(torch.int32) if cells.dtype == torch.bool else cells).contiguous()
        else:
            rows = _rows(cells, N)
            rows = None if rows is None else torch.from_numpy(rows).to(dev)
        keep = None if genes is None else torch.from_numpy(_mask(genes, J, "gene", ascending=True).view(np.uint8)).to(dev)
        n_rows = N if rows is None else int(rows.shape[0])
        with torch.cuda.device(dev):
            stream = stream_of(dev)
            if rows is not None and n_rows == 0:          # an empty list is still a list: NULL would ask for all rows
                rows = torch.zeros(1, dtype=torch.int32, device=dev)
            kept, out_indptr = ctypes.c_int64(0), torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
            args = (inp.device, stream, N, J, inp.nnz, ptr(inp.major), inp.major_kind, ptr(inp.minor), inp.minor_kind,
                    ptr(inp.values), inp.value_kind, n_rows, ptr(rows), ptr(keep), ctypes.byref(kept), ptr(out_indptr))
            _lib.check(lib.schpf_submatrix_device(*(args + (None, None, 0))))               # the sizes
            total = int(out_indptr[-1])
            out_indices = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            out_values = torch.empty(max(total, 1), dtype=inp.values.dtype, device=dev)
            _lib.check(lib.schpf_submatrix_device(*(args + (ptr(out_indices), ptr(out_values), total))))
            return torch.sparse_csr_tensor(out_indptr, out_indices[:total].to(torch.int64), out_values[:total],
                                           size=(n_rows, int(kept.value)))
    from scipy.sparse import csr_matrix
    C = host_csr(X, canonical=False)
    N, J = C.shape
    rows = _rows(cells, N)
    keep = None if genes is None or J == 0 else np.ascontiguousarray(_mask(genes, J, "gene", ascending=True)).view(np.uint8)
    indptr, indices, vals = host_csr_arrays(C)
    kept, out_indptr, out_indices, out_values = _submatrix_host(N, J, indptr, indices, vals, rows, keep, device_of(device))
    return csr_matrix((out_values.astype(C.data.dtype, copy=False), out_indices, out_indptr), shape=(len(out_indptr) - 1, kept))


def filter_counts(X, min_cells=0, min_genes=0, min_counts=0, max_counts=None, max_set_fraction=None, gene_sets=None,
                  device=None):
    """(X_filtered, cell_keep, gene_keep, metrics): the usual quality filter of a cells x genes count matrix, on the GPU.

    Genes: kept where at least `min_cells` cells hold a count > 0 -- the rule of preprocessing.min_cells_expressing_mask,
    also for a value strictly between 0 and 1, a proportion: the threshold is then round(min_cells * ncells).
    Cells: kept with at least `min_genes` genes with a count > 0, a total count of at least `min_counts` and, where given,
    at most `max_counts`, and for every (name, fraction) of the dict `max_set_fraction` at most that share of the total
    inside the gene set `name` of `gene_sets` (say, mitochondrial counts).

    One pass, not iterated: the genes are judged on the statistics of ALL cells and the cells on the statistics of ALL
    genes, those of `metrics = qc_metrics(X, gene_sets)`, which describe X and not X_filtered; a gene may end below
    `min_cells` among the cells that were kept.  X_filtered = submatrix(X, cell_keep, gene_keep).  The masks are boolean
    tensors on the GPU of X where X is a tensor there, else NumPy arrays."""
    metrics = qc_metrics(X, gene_sets=gene_sets, device=device)
    ncells = int(X.shape[0])
    if 0 < min_cells < 1:
        min_cells = round(min_cells * ncells)
    f64 = lambda a: a.double() if is_torch_tensor(a) else a.astype(np.float64)  # noqa: E731
    gene_keep = metrics["gene_n_cells"] >= min_cells
    total = metrics["cell_total"]
    cell_keep = (metrics["cell_n_genes"] >= min_genes) & (total >= min_counts)
    if max_counts is not None:
        cell_keep = cell_keep & (total <= max_counts)
    for name, fraction in (max_set_fraction or {}).items():
        if name not in metrics["cell_set_total"]:
            raise ValueError("max_set_fraction names the gene set %r, which gene_sets does not hold" % (name,))
        cell_keep = cell_keep & (f64(metrics["cell_set_total"][name]) <= float(fraction) * f64(total))
    return submatrix(X, cells=cell_keep, genes=gene_keep, device=device), cell_keep, gene_keep, metrics
