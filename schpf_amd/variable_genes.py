"""Highly variable genes on the GPU: the variance of every gene's analytic Pearson residuals.

Choosing the genes is the one step before `fit` that works on all N J pairs of the count matrix, zeros included.  Under a
negative-binomial null with the cell's depth and the gene's share as the only parameters (Lause et al. 2021; scanpy's
highly_variable_genes(flavor="pearson_residuals")), the residual of a zero entry depends on the cell only through its total
count: the library (schpf_residual_var[_device]) sums the clipped residuals and their squares per gene over the DISTINCT
cell totals and corrects the stored entries, without ever making the matrix dense.  `residual_variance` hands the count
matrix over; `highly_variable_genes` ranks the genes and returns the mask that `submatrix(X, genes=mask)` takes:

    found = highly_variable_genes(X, n_top_genes=2000)
    model = scHPF(K).fit(submatrix(X, genes=found["highly_variable"]))
"""
import math

import numpy as np

from . import _lib
from ._call import array_ptr as _p, device_of, library, same_device, stream_of, tensor_ptr as ptr
from .device_input import to_numpy as host
from .gene_major import gpu_arrays, held_on_gpu, host_arrays, refuse_gene_major

__all__ = ["residual_variance", "highly_variable_genes"]

NAMES = ("residual_sum", "residual_sumsq", "residual_var", "gene_total", "cell_total", "n_distinct_totals")


def _parameters(theta, clip, ncells):
    """(inv_theta, clip) as the library takes them: theta in (0, inf], clip in (0, inf] with the default sqrt(N)."""
    theta = float(theta)
    if not theta > 0:
        raise ValueError("theta must be in (0, inf], got %r" % (theta,))
    clip = math.sqrt(ncells) if clip is None else float(clip)
    if ncells and not clip > 0:
        raise ValueError("clip must be in (0, inf], got %r" % (clip,))
    return (0.0 if math.isinf(theta) else 1.0 / theta), (clip if clip > 0 else 1.0)   # no cells: any clip gives zeros


def residual_variance(X, theta=100.0, clip=None, device=None):
    """The variance of every gene's clipped Pearson residuals under a negative-binomial null, over all cells: a dict.

    X: cells x genes, integer counts in [0, 2^24].  A torch sparse COO or CSR tensor on a GPU is converted to CSC with torch
    on that GPU (duplicates summed) and scored on torch's current stream; tensors on that GPU come back.  Anything else goes
    through SciPy (`tocsc()` on a copy, duplicates summed) and the GPU `device` ($SCHPF_DEVICE or 0); NumPy comes back.
    theta: the overdispersion of the null in (0, inf]; inf is the Poisson null.  clip: the bound of a residual's size in
    (0, inf], default sqrt(N).

    With n_c, s_g, T the totals of cell c, of gene g and of all:  mu_cg = n_c s_g / T,  r_cg = clip((x_cg - mu_cg) /
    sqrt(mu_cg + mu_cg^2 / theta)), 0 where mu_cg = 0.  Keys: `residual_sum` and `residual_sumsq` (float64: the sums of r and
    r^2 per gene, the library's outputs, the same bits on every call), `residual_var` = sumsq / N - (sum / N)^2 (ddof = 0,
    as NumPy's var and scanpy), `gene_total` and `cell_total` (int64, exact) and `n_distinct_totals`, the number of
    different cell totals the dense part of the sum walked.  What the library refuses raises ValueError naming the smallest
    offending gene.  A `GeneMajor` (`gene_major(X)`) in place of X skips the conversion."""
    if held_on_gpu(X):
        import torch
        lib = library()
        dev = X.device
        same_device(dev.index, device, "X")
        N, J = int(X.shape[0]), int(X.shape[1])
        inv_theta, clip = _parameters(theta, clip, N)
        with torch.cuda.device(dev):
            indptr, cells, values = gpu_arrays(X)
            s1, s2 = torch.zeros(J, dtype=torch.float64, device=dev), torch.zeros(J, dtype=torch.float64, device=dev)
            cell_total = torch.zeros(N, dtype=torch.int64, device=dev)
            gene_total = torch.zeros(J, dtype=torch.int64, device=dev)
            _lib.check(lib.schpf_residual_var_device(dev.index, stream_of(dev), N, J, int(values.shape[0]), ptr(indptr),
                                                     ptr(cells), ptr(values), inv_theta, clip, ptr(s1), ptr(s2), ptr(cell_total),
                                                     ptr(gene_total)))
            var = s2 / N - (s1 / N) ** 2 if N else torch.zeros_like(s2)
            distinct = int(torch.unique(cell_total).numel())
        return dict(zip(NAMES, (s1, s2, var, gene_total, cell_total, distinct)))

    N, J, indptr, indices, data = host_arrays(X)
    inv_theta, clip = _parameters(theta, clip, N)
    lib = library()
    s1, s2 = np.zeros(J, np.float64), np.zeros(J, np.float64)
    cell_total, gene_total = np.zeros(N, np.int64), np.zeros(J, np.int64)
    _lib.check(lib.schpf_residual_var(device_of(device), N, J, len(data), _p(indptr), _p(indices), _p(data),
                                      inv_theta, clip, _p(s1), _p(s2), _p(cell_total), _p(gene_total)))
    var = s2 / N - (s1 / N) ** 2 if N else np.zeros(J)
    return dict(zip(NAMES, (s1, s2, var, gene_total, cell_total, int(np.unique(cell_total).size))))


def _ranks(var):
    """rank[g] of every gene, 0 the most variable: the order by (-var, gene index)."""
    order = np.argsort(-var, kind="stable")
    rank = np.empty(len(var), np.int64)
    rank[order] = np.arange(len(var))
    return rank


def highly_variable_genes(X, n_top_genes=2000, theta=100.0, clip=None, batch=None, device=None):
    """The `n_top_genes` genes of the cells x genes count matrix X whose Pearson residuals vary most: a dict.

    X, theta, clip, device: as `residual_variance`.  Keys: `highly_variable` (a bool mask over the genes, what
    `submatrix(X, genes=mask)` takes), `rank` (int64; 0 is the most variable gene; the genes are ordered by (-residual_var,
    gene index), so ties are settled), `residual_var` and `means` (float64: the mean count of the gene over all cells).

    batch: one label per cell.  Every batch b is scored on its own, on submatrix(X, cells=batch == b), with `clip`
    defaulting to the square root of that batch's cells.  Per gene: `n_batches`, in how many batches it ranks below
    n_top_genes; `median_rank`, the median of those ranks (NaN where there is none); `residual_var`, the mean over the
    batches.  The genes are ordered by n_batches descending, then median_rank ascending, then gene index -- scanpy's rule --
    and `rank` is the place in that order.

    Where X is a tensor on a GPU the arrays come back as tensors on that GPU, else as NumPy arrays; the ranking itself, J
    numbers, is done in NumPy on the host."""
    n_top_genes = int(n_top_genes)
    if n_top_genes < 0:
        raise ValueError("n_top_genes must be >= 0, got %d" % n_top_genes)
    N, J = int(X.shape[0]), int(X.shape[1])
    if batch is None:
        found = residual_variance(X, theta=theta, clip=clip, device=device)
        var = host(found["residual_var"])
        rank = _ranks(var)
        out = {"highly_variable": rank < n_top_genes, "rank": rank, "residual_var": var,
               "means": host(found["gene_total"]) / float(N) if N else np.zeros(J)}
    else:
        from .qc import submatrix
        refuse_gene_major(X, "highly_variable_genes(batch=...)")
        batch = host(batch)
        if batch.shape != (N,):
            raise ValueError("batch must hold one label per cell: %d, got shape %s" % (N, tuple(batch.shape)))
        labels = np.unique(batch)
        ranks, total = np.empty((len(labels), J), np.float64), np.zeros(J, np.int64)
        var = np.zeros(J, np.float64)
        for b, label in enumerate(labels):
            found = residual_variance(submatrix(X, cells=batch == label, device=device), theta=theta, clip=clip, device=device)
            var_b = host(found["residual_var"])
            ranks[b] = _ranks(var_b)
            var += var_b
            total += host(found["gene_total"])
        ranks[ranks >= n_top_genes] = np.nan
        n_batches = (~np.isnan(ranks)).sum(axis=0)
        median = np.full(J, np.nan)
        for g in np.flatnonzero(n_batches):
            median[g] = np.median(ranks[~np.isnan(ranks[:, g]), g])
        order = np.lexsort((np.arange(J), np.where(n_batches > 0, median, np.inf), -n_batches))
        rank = np.empty(J, np.int64)
        rank[order] = np.arange(J)
        out = {"highly_variable": rank < n_top_genes, "rank": rank, "residual_var": var / max(len(labels), 1),
               "means": total / float(N) if N else np.zeros(J), "n_batches": n_batches.astype(np.int64), "median_rank": median}
    if held_on_gpu(X):
        import torch
        out = {name: torch.from_numpy(np.ascontiguousarray(a)).to(X.device) for name, a in out.items()}
    return out
