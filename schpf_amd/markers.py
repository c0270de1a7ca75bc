"""Marker genes per cluster on the GPU: exact Wilcoxon rank sums of every gene for every group of cells.

"Which genes mark each cluster?" is a rank-sum test of every gene, each group of cells against the rest.  With average
ranks for ties, twice a rank is an integer: the library (schpf_rank_sums[_device]) returns the rank sums, the tie terms and
the counts as exact int64 sums, the same bits however the work was scheduled.  `rank_sums` hands the count matrix over;
`rank_genes_groups` turns the integers into z-scores, p-values, Benjamini-Hochberg adjusted p-values, fold changes and
the fractions of expressing cells -- plain NumPy / SciPy on G x J numbers, not part of the bit contract.
"""
import numpy as np

from . import _lib
from ._call import array_ptr as _p, device_of, library, same_device, stream_of, tensor_ptr as ptr
from .device_input import classify, gpu_coo, int32_labels, is_torch_tensor, on_gpu
from .gene_major import gpu_arrays, held_on_gpu, host_arrays, refuse_gene_major

__all__ = ["rank_sums", "rank_genes_groups", "benjamini_hochberg", "pair_rank_sums", "rank_genes_pairs"]

NAMES = ("n", "zeros", "ties", "nexpr", "rank2")
PAIR_NAMES = ("n", "nexpr", "u2", "ties")
PAIR_STATISTICS = ("scores", "pvals", "pvals_adj", "logfoldchanges", "pct_a", "pct_b", "mean_a", "mean_b")
STATISTICS = ("scores", "pvals", "pvals_adj", "logfoldchanges", "pct_in", "pct_out", "mean_in", "mean_out")
MAX_CELLS = 1 << 21


def _rank_sums_host(ncells, ngenes, indptr, indices, data, labels, ngroups, device):
    """schpf_rank_sums on the C-contiguous arrays of a CSC matrix (int64, int32, float32) and int32 labels -> the five int64
    arrays n[G], zeros[J], ties[J], nexpr[G, J], rank2[G, J]."""
    lib = library()
    out = _outputs(ngroups, ngenes)
    _lib.check(lib.schpf_rank_sums(device_of(device), ncells, ngenes, _p(indptr), _p(indices), _p(data), _p(labels), ngroups,
                                   *[_p(a) for a in out]))
    return out


def _outputs(ngroups, ngenes):
    return (np.zeros(ngroups, np.int64), np.zeros(ngenes, np.int64), np.zeros(ngenes, np.int64),
            np.zeros((ngroups, ngenes), np.int64), np.zeros((ngroups, ngenes), np.int64))


def _groups(labels, ngroups, ncells):
    """(labels as they are, G): one label per cell, G = ngroups or the largest label + 1, at least 1."""
    if len(labels.shape) != 1 or labels.shape[0] != ncells:
        raise ValueError("labels must hold one label per cell: %d, got shape %s" % (ncells, tuple(labels.shape)))
    if ngroups is None:
        ngroups = max(1, int(labels.max()) + 1) if ncells else 1
    ngroups = int(ngroups)
    if ngroups < 1:
        raise ValueError("ngroups must be at least 1, got %d" % ngroups)
    return ngroups


def _check_sizes(ncells, ngenes, ngroups):
    if ncells >= MAX_CELLS:          # what the library refuses before it reads anything, said before anything is converted
        raise ValueError("ncells must be in [0, 2^21), got %d" % ncells)
    if ngroups * ngenes >= 2 ** 31:
        raise ValueError("ngroups * ngenes must be below 2^31, got %d * %d" % (ngroups, ngenes))


def _gpu_inputs(X, labels, ngroups, device):
    """What a call on a matrix in GPU memory hands to the library: (the library, torch device, N, J, G, int32 labels on that
    GPU, the CSC arrays of `gene_major`, torch's current stream there)."""
    import torch
    lib = library()
    dev = X.device
    same_device(dev.index, device, "X")
    N, J = int(X.shape[0]), int(X.shape[1])
    with torch.cuda.device(dev):
        lab = (labels if is_torch_tensor(labels) else torch.tensor(np.asarray(labels))).detach()
        G = _groups(lab, ngroups, N)
        _check_sizes(N, J, G)
        lab = lab.to(device=dev, dtype=torch.int32).contiguous()
        indptr, cells, values = gpu_arrays(X)
        stream = stream_of(dev)
    return lib, dev, N, J, G, lab, indptr, cells, values, stream


def _host_inputs(X, labels, ngroups):
    """What a call on a matrix in host memory hands to the library: (N, J, G, the C-contiguous arrays of the canonical CSC
    form -- int64, int32, float32 -- and the int32 labels)."""
    if is_torch_tensor(labels):
        labels = labels.detach().cpu().numpy()
    labels = np.asarray(labels)
    N, J, indptr, indices, data = host_arrays(X)
    G = _groups(labels, ngroups, N)
    _check_sizes(N, J, G)
    return N, J, G, indptr, indices, data, int32_labels(labels, np.iinfo(np.int32).min, "labels must be in [-1, ngroups)")


def rank_sums(X, labels, ngroups=None, device=None):
    """The exact integers of the rank-sum test of every gene for every group of cells: a dict of int64 arrays
    n[G] (cells per group), zeros[J] (cells that tie at zero), ties[J] (the sum of t^3 - t over the tie groups, the zeros
    included), nexpr[G, J] (cells of the group with a positive value) and rank2[G, J] (twice the sum of the group's average
    ranks).  Twice the Mann-Whitney U of group g against the rest is rank2[g] - n[g] (n[g] + 1).

    X: cells x genes.  A SciPy sparse matrix is converted with tocsc() on a copy, duplicates summed; NumPy arrays come back.
    A torch sparse COO or CSR tensor on a GPU is converted to CSC with torch on that GPU and ranked on torch's current
    stream; tensors on that GPU come back.  Values are ranked as float32 (counts up to 2^24 are exact), must be finite and
    >= 0; stored zeros are zeros like the implicit ones.  A `GeneMajor` (`gene_major(X)`) in place of X skips the conversion.

    labels: one integer per cell in [-1, G), NumPy or a tensor; -1 ranks the cell with all the others but puts it in no
    group.  ngroups: G, default the largest label + 1.  Fewer than 2^21 cells, and G * J < 2^31.  What the library refuses
    raises ValueError naming the smallest offending gene or cell."""
    if held_on_gpu(X):
        import torch
        lib, dev, N, J, G, lab, indptr, cells, values, stream = _gpu_inputs(X, labels, ngroups, device)
        with torch.cuda.device(dev):
            out = [torch.zeros(s, dtype=torch.int64, device=dev) for s in ((G,), (J,), (J,), (G, J), (G, J))]
            _lib.check(lib.schpf_rank_sums_device(dev.index, stream, N, J, ptr(indptr), ptr(cells), ptr(values),
                                                  ptr(lab), G, *[ptr(t) for t in out]))
        return dict(zip(NAMES, out))

    N, J, G, indptr, indices, data, labels = _host_inputs(X, labels, ngroups)
    out = _rank_sums_host(N, J, indptr, indices, data, labels, G, device)
    return dict(zip(NAMES, out))


def benjamini_hochberg(pvals):
    """Benjamini-Hochberg adjusted p-values along the last axis: p_(i) J / i, made monotone from the largest down, at most 1.
    A row that holds a NaN is NaN."""
    p = np.asarray(pvals, dtype=np.float64)
    J = p.shape[-1]
    if J == 0:
        return p.copy()
    order = np.argsort(p, axis=-1)
    ranked = np.take_along_axis(p, order, axis=-1) * (float(J) / np.arange(1, J + 1))
    ranked = np.minimum(np.minimum.accumulate(ranked[..., ::-1], axis=-1)[..., ::-1], 1.0)
    out = np.empty_like(p)
    np.put_along_axis(out, order, ranked, axis=-1)
    out[np.isnan(p).any(axis=-1)] = np.nan
    return out


def _scaled(X, target_sum):
    """Every cell's counts scaled to `target_sum` ("median": the median depth of the cells), in float32."""
    if on_gpu(X):
        import torch
        rows, cols, values = gpu_coo(X)
        values = values.to(torch.float32)
        depth = torch.zeros(X.shape[0], dtype=torch.float32, device=X.device).index_add_(0, rows, values)
        target = float(torch.median(depth)) if isinstance(target_sum, str) and target_sum == "median" else float(target_sum)
        factor = torch.where(depth > 0, torch.tensor(target, dtype=torch.float32, device=X.device) / depth, torch.zeros_like(depth))
        return torch.sparse_coo_tensor(torch.stack([rows, cols]), values * factor[rows], size=tuple(X.shape)).coalesce()
    from scipy.sparse import csr_matrix
    R = csr_matrix(X, dtype=np.float32, copy=True)
    R.sum_duplicates()
    depth = np.asarray(R.sum(axis=1), dtype=np.float32).ravel()
    target = np.float32(np.median(depth)) if isinstance(target_sum, str) and target_sum == "median" else np.float32(target_sum)
    factor = np.zeros_like(depth)
    np.divide(target, depth, out=factor, where=depth > 0)
    R.data *= np.repeat(factor, np.diff(R.indptr))
    return R


def _group_sums(X, labels, G):
    """sums[g, j] = the sum of X[i, j] over the cells of group g, and the sums over all cells: one sparse product with the
    group indicator."""
    if on_gpu(X):
        import torch
        lab = (labels if is_torch_tensor(labels) else torch.tensor(np.asarray(labels))).to(X.device).to(torch.int64)
        rows, cols, values = gpu_coo(X)
        values = values.to(torch.float64)
        onehot = torch.zeros((X.shape[0], G + 1), dtype=torch.float64, device=X.device)
        onehot[torch.arange(X.shape[0], device=X.device), torch.where(lab >= 0, lab, torch.full_like(lab, G))] = 1.0
        both = torch.sparse.mm(torch.sparse_coo_tensor(torch.stack([cols, rows]), values, size=(X.shape[1], X.shape[0])), onehot)
        both = both.t().cpu().numpy()
        return both[:G], both.sum(axis=0)
    from scipy.sparse import csr_matrix
    labels = np.asarray(labels)
    inside = np.flatnonzero(labels >= 0)
    indicator = csr_matrix((np.ones(len(inside)), (labels[inside], inside)), shape=(G, len(labels)))
    Xd = csr_matrix(X, dtype=np.float64)
    return np.asarray((indicator @ Xd).todense()), np.asarray(Xd.sum(axis=0)).ravel()


def rank_genes_groups(X, labels, tie_correct=True, target_sum=None, device=None, reference=None):
    """The Wilcoxon rank-sum test of every gene, each group of cells against all the other cells: a dict of (G, J) float64
    arrays `scores`, `pvals`, `pvals_adj`, `logfoldchanges`, `pct_in`, `pct_out`, `mean_in`, `mean_out`, and `n`, the cells
    per group.  G is the largest label + 1; cells labelled -1 are in no group and count among "all the others".

    From the exact integers of `rank_sums`, with n_o = N - n_g:
        d = rank2 - n_g (N + 1);  var = n_g n_o ((N + 1) - tie) / 12,  tie = ties / (N (N - 1)) if tie_correct else 0
        scores = d / (2 sqrt(var)), 0 where var == 0;  pvals = erfc(|scores| / sqrt 2)
    -- the normal approximation of scipy.stats.mannwhitneyu without continuity correction; tie_correct=False is the
    z-score of scanpy's default.  pvals_adj: Benjamini-Hochberg within each group.  pct_in / pct_out: the fraction of
    cells with a positive value inside and outside the group; mean_in / mean_out the mean values;
    logfoldchanges = log2((mean_in + 1e-9) / (mean_out + 1e-9)).  A group that is empty or holds all the cells gets NaN.

    target_sum: scale every cell's counts to that total before ranking ("median": the median depth), in float32.

    reference: None, or a group r: every other group is then tested against group r alone (scanpy's `reference=`) -- the
    result of `rank_genes_pairs` for the pairs (g, r), g != r, laid out as (G, J) with NaN in row r; the keys are those of
    `rank_genes_pairs` (pct_a, pct_b, mean_a, mean_b: a is the row's group, b the reference), `n` the cells per group."""
    refuse_gene_major(X, "rank_genes_groups")
    if reference is not None:
        return _against_reference(X, labels, int(reference), tie_correct, target_sum, device)
    if is_torch_tensor(X) and not on_gpu(X):      # a tensor in host memory: as SciPy
        X = classify(X).matrix
    if is_torch_tensor(labels) and not on_gpu(X):
        labels = labels.detach().cpu().numpy()
    if target_sum is not None:
        X = _scaled(X, target_sum)
    sums = rank_sums(X, labels, device=device)
    n, zeros, ties, nexpr, rank2 = [np.asarray(sums[k].cpu() if is_torch_tensor(sums[k]) else sums[k]) for k in NAMES]
    G, J = rank2.shape
    N = int(X.shape[0])
    n_g = n.astype(np.float64)[:, None]
    n_o = N - n_g
    with np.errstate(divide="ignore", invalid="ignore"):
        tie = ties.astype(np.float64)[None, :] / (float(N) * (N - 1)) if tie_correct and N > 1 else 0.0
        var = n_g * n_o * ((N + 1) - tie) / 12.0
        d = rank2.astype(np.float64) - n_g * (N + 1)      # exact: both are below 2^53
        scores = np.where(var > 0, d / (2.0 * np.sqrt(np.where(var > 0, var, 1.0))), 0.0)
        scores = np.where((n_g > 0) & (n_o > 0), scores, np.nan)
        from scipy.special import erfc
        pvals = erfc(np.abs(scores) / np.sqrt(2.0))
        group_sums, all_sums = _group_sums(X, labels, G)
        mean_in = group_sums / n_g
        mean_out = (all_sums[None, :] - group_sums) / n_o
        pct_in = nexpr / n_g
        pct_out = ((N - zeros)[None, :] - nexpr) / n_o
        logfoldchanges = np.log2((mean_in + 1e-9) / (mean_out + 1e-9))
    return {"scores": scores, "pvals": pvals, "pvals_adj": benjamini_hochberg(pvals), "logfoldchanges": logfoldchanges,
            "pct_in": pct_in, "pct_out": pct_out, "mean_in": mean_in, "mean_out": mean_out, "n": n}


def _pair_rank_sums_host(ncells, ngenes, indptr, indices, data, labels, ngroups, pairs, device):
    """schpf_pair_rank_sums on the C-contiguous arrays of a CSC matrix, int32 labels and int32 pairs[P, 2] -> the four int64
    arrays n[G], nexpr[G, J], u2[P, J], ties[P, J]."""
    lib = library()
    P = pairs.shape[0]
    out = (np.zeros(ngroups, np.int64), np.zeros((ngroups, ngenes), np.int64), np.zeros((P, ngenes), np.int64),
           np.zeros((P, ngenes), np.int64))
    _lib.check(lib.schpf_pair_rank_sums(device_of(device), ncells, ngenes, _p(indptr), _p(indices), _p(data), _p(labels), ngroups,
                                        _p(pairs), P, *[_p(a) for a in out]))
    return out


def _pairs(pairs, ngroups, ngenes):
    """The int32 P x 2 array of a `pairs` argument: "all" is every a < b."""
    if isinstance(pairs, str):
        if pairs != "all":
            raise ValueError('pairs must be "all" or rows (a, b), got %r' % (pairs,))
        a, b = np.triu_indices(ngroups, 1)
        pairs = np.stack([a, b], axis=1)
    if is_torch_tensor(pairs):
        pairs = pairs.detach().cpu().numpy()
    pairs = np.asarray(pairs)
    if pairs.size == 0:
        pairs = pairs.reshape(0, 2)
    if pairs.ndim != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must be rows (a, b), got shape %s" % (tuple(pairs.shape),))
    if pairs.shape[0] * ngenes >= 2 ** 31:
        raise ValueError("npairs * ngenes must be below 2^31, got %d * %d" % (pairs.shape[0], ngenes))
    if pairs.size and (pairs.min() < 0 or pairs.max() >= ngroups or (pairs[:, 0] == pairs[:, 1]).any()):
        wrong = (pairs < 0).any(axis=1) | (pairs >= ngroups).any(axis=1) | (pairs[:, 0] == pairs[:, 1])
        raise ValueError("pairs must name two different groups in [0, ngroups); offending pair %d" % int(np.flatnonzero(wrong)[0]))
    return np.ascontiguousarray(pairs, dtype=np.int32)


def pair_rank_sums(X, labels, pairs="all", ngroups=None, device=None):
    """The exact integers of the rank-sum test of every gene between pairs of groups of cells, each pair ranked alone: a dict
    of int64 arrays n[G] (cells per group), nexpr[G, J] (cells of the group with a positive value), u2[P, J] (twice the
    Mann-Whitney U of the pair's first group over its second; twice the rank sum of the first group within the two is
    u2 + n_a (n_a + 1)) and ties[P, J] (the sum of t^3 - t over the tie groups of the two groups' cells, the zeros
    included), and `pairs`, the int32 P x 2 array that was used.  Cells labelled -1 or in a third group do not exist for a
    pair.  One sort on the GPU serves all pairs.

    pairs: "all" -- every a < b -- or rows (a, b) of two different groups; a row may be repeated or reversed.  X, labels,
    ngroups and device as for `rank_sums`: a torch sparse COO or CSR tensor on a GPU is ranked there on torch's current
    stream and tensors come back (`pairs` too); anything else goes through SciPy and NumPy arrays come back.  A `GeneMajor`
    (`gene_major(X)`) in place of X skips the conversion."""
    if held_on_gpu(X):
        import torch
        lib, dev, N, J, G, lab, indptr, cells, values, stream = _gpu_inputs(X, labels, ngroups, device)
        pairs = _pairs(pairs, G, J)
        P = pairs.shape[0]
        with torch.cuda.device(dev):
            d_pairs = torch.tensor(pairs, device=dev)
            out = [torch.zeros(s, dtype=torch.int64, device=dev) for s in ((G,), (G, J), (P, J), (P, J))]
            _lib.check(lib.schpf_pair_rank_sums_device(dev.index, stream, N, J, ptr(indptr), ptr(cells),
                                                       ptr(values), ptr(lab), G, ptr(d_pairs), P, *[ptr(t) for t in out]))
        return dict(zip(PAIR_NAMES + ("pairs",), out + [d_pairs]))

    N, J, G, indptr, indices, data, labels = _host_inputs(X, labels, ngroups)
    pairs = _pairs(pairs, G, J)
    out = _pair_rank_sums_host(N, J, indptr, indices, data, labels, G, pairs, device)
    return dict(zip(PAIR_NAMES + ("pairs",), tuple(out) + (pairs,)))


def _group_means_input(X, labels, G, target_sum, device):
    """sums[g, j] of X over the cells of group g as float64: the exact integer sums of schpf_amd.group_stats for counts, one
    sparse product in float64 for a matrix scaled to a target sum (its values are no integers)."""
    if target_sum is not None:
        return _group_sums(X, labels, G)[0]
    from .aggregate import group_stats
    total = group_stats(X, labels, ngroups=G, sumsq=False, device=device)["total"]
    return np.asarray(total.cpu() if is_torch_tensor(total) else total).astype(np.float64)


def rank_genes_pairs(X, labels, pairs="all", tie_correct=True, target_sum=None, device=None):
    """The Wilcoxon rank-sum (Mann-Whitney) test of every gene between pairs of groups of cells, the first group of a pair
    against the second and no other cell: a dict of (P, J) float64 arrays `scores`, `pvals`, `pvals_adj`, `logfoldchanges`,
    `pct_a`, `pct_b`, `mean_a`, `mean_b`, and `pairs` (int32 P x 2, as used) and `n`, the cells per group.  G is the largest
    label + 1.  This is scanpy's rank_genes_groups(reference=...) and Seurat's FindMarkers(ident.1, ident.2) for any list of
    pairs at once.

    From the exact integers of `pair_rank_sums`, with n = n_a + n_b:
        var = n_a n_b ((n + 1) - tie) / 12,  tie = ties / (n (n - 1)) if tie_correct else 0
        scores = (u2 - n_a n_b) / (2 sqrt(var)), 0 where var == 0, NaN if either group is empty
        pvals = erfc(|scores| / sqrt 2)
    -- the normal approximation of scipy.stats.mannwhitneyu(xa, xb) without continuity correction.  pvals_adj:
    Benjamini-Hochberg within each pair.  pct_a / pct_b: the fraction of the group's cells with a positive value; mean_a /
    mean_b: the mean values, from the exact sums of schpf_amd.group_stats (X must then hold counts; with target_sum, from a
    float64 product); logfoldchanges = log2((mean_a + 1e-9) / (mean_b + 1e-9)).

    pairs: "all" or rows (a, b).  target_sum: scale every cell's counts to that total before ranking ("median": the median
    depth), in float32; nearly every entry is then its own value, the slowest case of the kernels."""
    refuse_gene_major(X, "rank_genes_pairs")
    if is_torch_tensor(X) and not on_gpu(X):      # a tensor in host memory: as SciPy
        X = classify(X).matrix
    if is_torch_tensor(labels) and not on_gpu(X):
        labels = labels.detach().cpu().numpy()
    if target_sum is not None:
        X = _scaled(X, target_sum)
    sums = pair_rank_sums(X, labels, pairs=pairs, device=device)
    n, nexpr, u2, ties, pairs = [np.asarray(sums[k].cpu() if is_torch_tensor(sums[k]) else sums[k]) for k in PAIR_NAMES + ("pairs",)]
    G = n.shape[0]
    a, b = pairs[:, 0], pairs[:, 1]
    n_a, n_b = n[a].astype(np.float64)[:, None], n[b].astype(np.float64)[:, None]
    both = n_a + n_b
    with np.errstate(divide="ignore", invalid="ignore"):
        tie = ties.astype(np.float64) / np.where(both > 1, both * (both - 1), 1.0) if tie_correct else 0.0
        var = n_a * n_b * ((both + 1) - tie) / 12.0
        d = u2.astype(np.float64) - n_a * n_b             # exact: both are below 2^53
        scores = np.where(var > 0, d / (2.0 * np.sqrt(np.where(var > 0, var, 1.0))), 0.0)
        scores = np.where((n_a > 0) & (n_b > 0), scores, np.nan)
        from scipy.special import erfc
        pvals = erfc(np.abs(scores) / np.sqrt(2.0))
        group_sums = _group_means_input(X, labels, G, target_sum, device)
        mean_a, mean_b = group_sums[a] / n_a, group_sums[b] / n_b
        pct_a, pct_b = nexpr[a] / n_a, nexpr[b] / n_b
        logfoldchanges = np.log2((mean_a + 1e-9) / (mean_b + 1e-9))
    return {"scores": scores, "pvals": pvals, "pvals_adj": benjamini_hochberg(pvals), "logfoldchanges": logfoldchanges,
            "pct_a": pct_a, "pct_b": pct_b, "mean_a": mean_a, "mean_b": mean_b, "pairs": pairs, "n": n}


def _against_reference(X, labels, reference, tie_correct, target_sum, device):
    """rank_genes_groups(reference=r): the pairs (g, r), g != r, of rank_genes_pairs as (G, J) arrays, NaN in row r."""
    lab = labels.detach().cpu().numpy() if is_torch_tensor(labels) else np.asarray(labels)
    G = max(1, int(lab.max()) + 1) if lab.size else 1
    if not 0 <= reference < G:
        raise ValueError("reference must be a group in [0, %d), got %d" % (G, reference))
    others = np.array([g for g in range(G) if g != reference], dtype=np.int32)
    pairs = np.stack([others, np.full(len(others), reference, np.int32)], axis=1).reshape(-1, 2)
    found = rank_genes_pairs(X, labels, pairs=pairs, tie_correct=tie_correct, target_sum=target_sum, device=device)
    out = {"n": found["n"]}
    for name in PAIR_STATISTICS:
        full = np.full((G, found[name].shape[1]), np.nan)
        full[others] = found[name]
        out[name] = full
    return out
