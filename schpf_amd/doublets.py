"""Doublet scores on the GPU: simulate doublets, project them, count neighbours.

In droplet data a few percent of the rows of a count matrix are two cells.  Scrublet (Wolock, Lopez & Klein 2019) finds
them by adding the counts of random pairs of observed cells, embedding observed and simulated cells together, and scoring
every cell by the share of simulated doublets among its nearest neighbours.  The first step runs in the library
(schpf_doublet_parents[_device], schpf_doublet_rows[_device]): the parents are a counter-based draw and the sum of two
sorted sparse rows is integer work, so `simulate_doublets` returns the same bits wherever the matrix lives and however the
work was scheduled.  The embedding is `project()` against the frozen gene factors and the neighbours are `knn`, exact: given
the embedding, `k_sim` -- an integer -- is in the bit contract too.  The score itself is a few lines of NumPy in float64 on
the host (`scrublet_score`), not part of it.
"""
import math

import numpy as np

from . import _lib
from ._call import array_ptr as _p, device_of, library, stream_of, tensor_ptr as ptr
from .device_input import NUMPY_VALUE_KINDS, classify, gpu_csr, host_csr, host_csr_arrays, is_torch_tensor, on_gpu
from .thinning import _seed       # one rule for a seed, whichever Philox stream it starts

__all__ = ["simulate_doublets", "doublet_scores", "scrublet_score"]

MAX_K = 128        # the longest neighbour list schpf_knn gives


def _n_sim(n_sim, ratio, n_obs):
    n_sim = int(round(float(ratio) * n_obs)) if n_sim is None else int(n_sim)
    if not 0 <= n_sim < 2 ** 31:
        raise ValueError("n_sim must be in [0, 2^31), got %d" % n_sim)
    return n_sim


def _check_parents(shape, n_obs):
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError("parents must be an (n_sim, 2) array of rows of X, got shape %s" % (tuple(shape),))
    if n_obs >= 2 ** 31:
        raise ValueError("ncells must be in [0, 2^31), got %d" % n_obs)


def simulate_doublets(X, n_sim=None, ratio=2.0, seed=0, parents=None, device=None):
    """X -> (X_sim, parents): row s of X_sim is X[parents[s, 0]] + X[parents[s, 1]].

    X: cells x genes counts, non-negative integers <= 2^24.  A torch sparse CSR or COO tensor on a GPU stays there -- a COO
    is brought to canonical CSR (duplicates summed, columns ascending) with torch on that GPU -- the sum runs on torch's
    current stream, and a torch sparse CSR tensor and an (n_sim, 2) int32 tensor on that GPU come back.  Anything else goes
    through SciPy (`tocsr()` and `sum_duplicates()` on a copy) and the GPU `device` ($SCHPF_DEVICE or 0), and a SciPy
    csr_matrix and a NumPy array come back.  Values keep the input's dtype.

    n_sim: the number of simulated rows, default round(ratio * ncells).  parents=None: the pairs are drawn, pair s from
    (seed, ncells, s) alone -- Philox4x32-10 with the counter (s, 0, 1), unrelated to the thinning stream of the same seed;
    a cell may meet itself, as in Scrublet.  parents given (n_sim x 2 rows of X): the draw is skipped and the caller chooses
    the pairs, for instance only cells from different clusters; they come back as they are.

    In the bit contract: parents and all three arrays of X_sim -- every column stored in either parent is stored in the
    sum, columns ascending, also where the sum is 0, so the structure depends on the indices alone.  The columns of a CSR
    must be strictly ascending within a row; what the library refuses raises ValueError naming the smallest offending row,
    entry or pair."""
    lib = library()
    seed = _seed(seed)
    if on_gpu(X):
        import torch
        inp, dev = gpu_csr(X, device)
        N, J = inp.shape
        with torch.cuda.device(dev):
            stream = stream_of(dev)
            if parents is None:
                n_pairs = _n_sim(n_sim, ratio, N)
                if n_pairs and N < 1:
                    raise ValueError("ncells must be in (0, 2^31) to draw parents, got %d" % N)
                parents = torch.empty((n_pairs, 2), dtype=torch.int32, device=dev)
                if n_pairs:
                    _lib.check(lib.schpf_doublet_parents_device(inp.device, stream, 0, n_pairs, N, seed, ptr(parents)))
            else:
                if not is_torch_tensor(parents):
                    parents = torch.tensor(np.asarray(parents))
                parents = parents.detach().to(device=dev, dtype=torch.int32).contiguous()
                _check_parents(parents.shape, N)
                n_pairs = int(parents.shape[0])
            out_indptr = torch.zeros(n_pairs + 1, dtype=torch.int64, device=dev)
            args = (inp.device, stream, N, J, inp.nnz, ptr(inp.major), inp.major_kind, ptr(inp.minor), inp.minor_kind,
                    ptr(inp.values), inp.value_kind, n_pairs, ptr(parents), ptr(out_indptr))
            _lib.check(lib.schpf_doublet_rows_device(*(args + (None, None, 0))))          # the sizes
            total = int(out_indptr[-1])
            out_indices = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            out_values = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            _lib.check(lib.schpf_doublet_rows_device(*(args + (ptr(out_indices), ptr(out_values), total))))
            X_sim = torch.sparse_csr_tensor(out_indptr, out_indices[:total].to(torch.int64),
                                            out_values[:total].to(inp.values.dtype), size=(n_pairs, J))
        return X_sim, parents

    from scipy.sparse import csr_matrix
    C = host_csr(X, canonical=True)
    N, J = C.shape
    if parents is None:
        n_pairs = _n_sim(n_sim, ratio, N)
        parents = np.empty((n_pairs, 2), np.int32)
        if n_pairs:
            _lib.check(lib.schpf_doublet_parents(0, n_pairs, N, seed, _p(parents)))
    else:
        if is_torch_tensor(parents):
            parents = parents.detach().cpu().numpy()
        given = np.asarray(parents)
        _check_parents(given.shape, N)
        if given.size and (given.min() < 0 or given.max() >= N):      # before the cast to int32 could hide it
            raise ValueError("doublets: parents must be in [0, ncells); offending pair %d"
                             % int(np.flatnonzero(((given < 0) | (given >= N)).any(axis=1))[0]))
        parents = np.ascontiguousarray(given, dtype=np.int32)
        n_pairs = parents.shape[0]
    indptr, indices, vals = host_csr_arrays(C)
    out_indptr = np.zeros(n_pairs + 1, np.int64)
    args = (device_of(device), N, J, C.nnz, _p(indptr), _p(indices), _p(vals), NUMPY_VALUE_KINDS[vals.dtype], n_pairs,
            _p(parents), _p(out_indptr))
    _lib.check(lib.schpf_doublet_rows(*(args + (None, None, 0))))                          # the sizes
    total = int(out_indptr[-1])
    out_indices, out_values = np.empty(max(total, 1), np.int32), np.empty(max(total, 1), np.int32)
    _lib.check(lib.schpf_doublet_rows(*(args + (_p(out_indices), _p(out_values), total))))
    return csr_matrix((out_values[:total].astype(C.data.dtype), out_indices[:total], out_indptr), shape=(n_pairs, J)), parents


def scrublet_score(k_sim, k_adj, ratio, expected_rate=0.06, rate_sd=0.02):
    """(score, se) of Scrublet's Bayesian doublet score from k_sim, the simulated rows among a cell's k_adj nearest
    neighbours, with ratio = n_sim / n_obs and rho = expected_rate, in float64:
        q = (k_sim + 1) / (k_adj + 2);  d = 1 - rho - q (1 - rho - rho / ratio);  score = q rho / ratio / d
        se = score / d * sqrt((se_q / q (1 - rho))^2 + (se_rho / rho (1 - q))^2),  se_q = sqrt(q (1 - q) / (k_adj + 3))
    Plain NumPy on the host, not part of the bit contract."""
    k_sim = np.asarray(k_sim, dtype=np.float64)
    rho, r, se_rho = float(expected_rate), float(ratio), float(rate_sd)
    q = (k_sim + 1.0) / (k_adj + 2.0)
    d = 1.0 - rho - q * (1.0 - rho - rho / r)
    score = q * rho / r / d
    se_q = np.sqrt(q * (1.0 - q) / (k_adj + 3.0))
    se = score / d * np.sqrt((se_q / q * (1.0 - rho)) ** 2 + (se_rho / rho * (1.0 - q)) ** 2)
    return score, se


def _stack(X, X_sim):
    """X over X_sim as one matrix `project` takes: plumbing, with torch on the GPU of X or with SciPy."""
    if on_gpu(X):
        import torch
        inp = gpu_csr(X)[0]
        crow, sim_crow = inp.major.to(torch.int64), X_sim.crow_indices()
        return torch.sparse_csr_tensor(torch.cat([crow, sim_crow[1:] + crow[-1]]),
                                       torch.cat([inp.minor.to(torch.int64), X_sim.col_indices()]),
                                       torch.cat([inp.values, X_sim.values()]),
                                       size=(inp.shape[0] + X_sim.shape[0], inp.shape[1]))
    from scipy.sparse import csr_matrix, issparse, vstack
    if is_torch_tensor(X):
        X = classify(X).matrix
    return vstack([X.tocsr() if issparse(X) else csr_matrix(X), X_sim]).tocoo()


def doublet_scores(model, X, ratio=2.0, expected_rate=0.06, rate_sd=0.02, k=None, metric="euclidean", seed=0,
                   threshold=None, device=None, **project_kwargs):
    """Scrublet's doublet score of every cell of X under a fitted model: a dict.

    1. `simulate_doublets(X, ratio=ratio, seed=seed)` adds the counts of random pairs of cells.
    2. X stacked over the simulated rows goes through ONE `model.project(...)` against the frozen gene factors
       (project_kwargs go there): observed and simulated cells are embedded by the same procedure -- the fitted theta of
       the observed cells is not used.
    3. `cell_score()` of the projection, `knn` of the stack against itself (a row is not its own neighbour) with
       k_adj = round(k (1 + n_sim / n_obs)) neighbours, k_sim = the simulated rows among them, `scrublet_score`.
    k: default round(0.5 sqrt(n_obs)), lowered where k_adj would pass the 128 neighbours `knn` gives; a k given is taken as
    it is and refused if k_adj passes them.  expected_rate, rate_sd: the doublet rate expected and its standard deviation.

    Keys: `scores`, `se`, `k_sim` for the observed cells; `scores_sim`, `k_sim_sim`, `parents` for the simulated ones;
    `k_adj`; with a threshold also `calls` (scores > threshold) and `detectable_fraction` (the share of scores_sim >
    threshold).  Picking the threshold, and Scrublet's UMI subsampling of the doublets, are not done here.

    In the bit contract: `parents`, and `k_sim` / `k_sim_sim` given the embedding (integers, from exact neighbours under the
    key of DESIGN.md 16).  Not in it: the embedding itself (a float fit) and the scores (float64 NumPy)."""
    n_obs = int(X.shape[0])
    X_sim, parents = simulate_doublets(X, ratio=ratio, seed=seed, device=device)
    n_sim = int(X_sim.shape[0])
    if n_obs < 1 or n_sim < 1:
        raise ValueError("doublet scores need at least one cell and one simulated row, got %d and %d" % (n_obs, n_sim))
    r = n_sim / float(n_obs)
    if k is None:
        k = max(1, int(round(0.5 * math.sqrt(n_obs))))
        while k > 1 and int(round(k * (1.0 + r))) > MAX_K:
            k -= 1
    k = int(k)
    k_adj = int(round(k * (1.0 + r)))
    if not 1 <= k_adj <= min(MAX_K, n_obs + n_sim - 1):
        raise ValueError("k_adj = round(k (1 + n_sim / n_obs)) must be in [1, min(128, n_obs + n_sim - 1)], got %d from k = %d"
                         % (k_adj, k))
    from .neighbors import knn
    if device is not None:
        project_kwargs.setdefault("device", int(device))
    embedded = model.project(_stack(X, X_sim), **project_kwargs).cell_score()
    indices, _ = knn(embedded, k=k_adj, metric=metric, device=device)
    k_all = (np.asarray(indices) >= n_obs).sum(axis=1).astype(np.int64)
    score, se = scrublet_score(k_all, k_adj, r, expected_rate, rate_sd)
    if is_torch_tensor(parents):
        parents = parents.cpu().numpy()
    out = {"scores": score[:n_obs], "se": se[:n_obs], "k_sim": k_all[:n_obs], "scores_sim": score[n_obs:],
           "k_sim_sim": k_all[n_obs:], "parents": parents, "k_adj": k_adj}
    if threshold is not None:
        out["calls"] = out["scores"] > threshold
        out["detectable_fraction"] = float(np.mean(out["scores_sim"] > threshold))
    return out
