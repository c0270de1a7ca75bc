"""Loss functions, evaluated on the GPU.

Mirror of /root/reference/schpf/loss.py: `pois_llh_pointwise` (:107-139) and
`mean_negative_pois_llh` (:142-168) plus the two higher-order helpers
`loss_function_for_data` (:17-34) and `projection_loss_function` (:37-102).
As in the reference every loss takes the data positionally/as `X` and everything
else as keyword arguments, ignoring the ones it does not use.
"""
import functools

import numpy as np

from ._call import device_of
from .hpf_hip import compute_pois_llh

__all__ = ["loss_function_for_data", "projection_loss_function", "pois_llh_pointwise",
           "mean_negative_pois_llh", "elbo", "cellmean_negative_pois_llh", "genemean_negative_pois_llh",
           "thinned_mean_negative_pois_llh", "predictive_check"]

# what predictive_check returns, in the column order of `scHPF score --ppc`
PPC_COLUMNS = ("pred_mean", "pred_var", "pred_zero_frac", "obs_mean", "obs_var", "obs_zero_frac")


def loss_function_for_data(loss_function, X):
    """Bind the data argument `X` of a loss function."""
    return functools.partial(loss_function, X=X)


def projection_loss_function(loss_function, X, nfactors, model_kwargs={}, proj_kwargs={}, device=None):
    """Loss of held-out cells `X` after projecting them onto the model being trained.

    `device` (an addition to the reference's signature): HIP device the held-out cells live on;
    default $SCHPF_DEVICE or 0, like project().  The returned function has a `.close()` that
    releases the engine it keeps between checks.

    Returns f(*, a, ap, bp, c, cp, dp, eta, beta, **ignored): it copies the
    hyperparameters and gene distributions into a private scHPF, runs project(X,
    replace=True) (defaults reinit=False, max_iter=min_iter=10, no intermediate
    loss checks) and evaluates `loss_function` on the projection.
    """
    from .scHPF_ import scHPF   # late import: scHPF_ imports this module
    from .engine import DeviceCAVI

    pmodel = scHPF(nfactors=nfactors, **model_kwargs)
    from .device_input import as_matrix
    X = as_matrix(X)
    device = device_of(device)
    held = {}    # the held-out cells stay on the device between checks: one upload, one pair of plans

    def _projection_loss_function(*, a, ap, bp, c, cp, dp, eta, beta, **kwargs):
        assert eta.dims[0] == beta.dims[0]
        assert beta.dims[1] == nfactors
        pmodel.a, pmodel.ap, pmodel.bp = a, ap, bp
        pmodel.c, pmodel.cp, pmodel.dp = c, cp, dp
        pmodel.eta, pmodel.beta = eta, beta

        proj_kwargs.setdefault("reinit", False)
        proj_kwargs.setdefault("max_iter", 10)
        proj_kwargs.setdefault("min_iter", 10)
        proj_kwargs.setdefault("check_freq", proj_kwargs["max_iter"] + 1)
        dtype = np.dtype(pmodel.dtype)
        eng = held.get("engine")
        if eng is None or eng.dtype != dtype or "engine" in proj_kwargs:
            eng = proj_kwargs.get("engine")
            if eng is None:
                old = held.pop("engine", None)
                if old is not None:
                    old.close()
                eng = DeviceCAVI(X.shape[0], X.shape[1], nfactors, dtype=dtype, device=device)
                eng.upload(X)
                held["engine"] = eng
        pmodel.project(X, replace=True, **dict(proj_kwargs, engine=eng, device=device))

        if getattr(loss_function, "func", loss_function) is mean_negative_pois_llh:   # also a functools.partial of it
            # the engine holds exactly the state project() just returned: evaluate there (one scalar back)
            return eng.mean_negative_pois_llh()
        return loss_function(X, a=pmodel.a, ap=pmodel.ap, bp=pmodel.bp, c=pmodel.c, cp=pmodel.cp,
                             dp=pmodel.dp, xi=pmodel.xi, eta=pmodel.eta, theta=pmodel.theta,
                             beta=pmodel.beta)

    def close():
        eng = held.pop("engine", None)
        if eng is not None:
            eng.close()
    _projection_loss_function.close = close
    return _projection_loss_function


def pois_llh_pointwise(X, *, theta, beta, single_process=False, **kwargs):
    """Poisson log-likelihood of each stored nonzero of X, in X's COO order.

    `single_process` is accepted for signature compatibility and ignored: there is
    one execution path, the GPU.
    """
    return compute_pois_llh(X.data, X.row, X.col, theta.vi_shape, theta.vi_rate,
                            beta.vi_shape, beta.vi_rate)


def mean_negative_pois_llh(X, *, theta, beta, single_process=False, **kwargs):
    """Mean over the stored nonzeros of X of the negative Poisson log-likelihood."""
    return np.mean(-pois_llh_pointwise(X=X, theta=theta, beta=beta))


def thinned_mean_negative_pois_llh(X_test, *, theta, beta, frac, device=None, **kwargs):
    """Held-out loss of a model fitted to the train part of a thinned matrix (thinning.thin_counts): the
    mean over the stored entries of X_test of -log Poisson(x_test | s E[theta_i] E[beta_g]), s = frac / (1 - frac) -- the
    test counts have frac / (1 - frac) times the rate of the train counts.  No kernel of its own: the usual device loss
    on a theta whose rate is divided by s.  X_test: a SciPy matrix, or a torch sparse tensor (one in GPU memory is
    uploaded from there; `device` as for the per-row means)."""
    from .scHPF_ import HPF_Gamma   # late import: scHPF_ imports this module
    from .device_input import as_matrix, is_torch_tensor
    if not 0.0 < frac < 1.0:
        raise ValueError("frac must be in (0, 1), got %r" % (frac,))
    s = theta.vi_rate.dtype.type(frac / (1.0 - frac))
    scaled = HPF_Gamma(theta.vi_shape, theta.vi_rate / s)
    X_test = as_matrix(X_test)
    if not is_torch_tensor(X_test):
        return mean_negative_pois_llh(X_test, theta=scaled, beta=beta)
    from .engine import DeviceCAVI
    device = device_of(device)
    with DeviceCAVI(X_test.shape[0], X_test.shape[1], theta.dims[1], dtype=theta.dtype, device=device) as eng:
        eng.upload(X_test)
        eng.set_gamma("theta", scaled.vi_shape, scaled.vi_rate)
        eng.set_gamma("beta", beta.vi_shape, beta.vi_rate)
        return eng.mean_negative_pois_llh()


def elbo(X, *, a, ap, bp, c, cp, dp, xi, eta, theta, beta, terms=False, device=None, **kwargs):
    """The evidence lower bound of the variational state (xi, eta, theta, beta) on X, with the responsibilities at
    their optimum, evaluated on the GPU: X is uploaded, the state set and the ELBO computed.  X: a SciPy
    sparse matrix or a torch sparse COO / CSR tensor (DeviceCAVI.upload), as for the per-row means below.

    terms=True returns the dict {'data', 'logfac', 'rate', 'cell', 'gene', 'elbo'}, else the total.  `device`: HIP
    device ordinal, default $SCHPF_DEVICE or 0.
    """
    from .engine import DeviceCAVI   # late import, as in projection_loss_function
    device = device_of(device)
    from .device_input import as_matrix
    X = as_matrix(X)          # a SciPy matrix or a torch sparse tensor (in GPU memory: uploaded from there)
    with DeviceCAVI(X.shape[0], X.shape[1], theta.dims[1], dtype=theta.dtype, device=device) as eng:
        eng.upload(X)
        eng.set_hypers(a, c, bp, dp)
        for name, g in (("xi", xi), ("theta", theta), ("eta", eta), ("beta", beta)):
            eng.set_gamma(name, g.vi_shape, g.vi_rate)
        out = eng.elbo_terms(ap, cp)
    return out if terms else out["elbo"]


def _rowmean_on_device(X, theta, beta, by, device):
    """X uploaded once, theta / beta set, the per-row loss of axis `by` evaluated on the device."""
    from .engine import DeviceCAVI   # late import, as in projection_loss_function
    device = device_of(device)
    from .device_input import as_matrix
    X = as_matrix(X)          # a SciPy matrix or a torch sparse tensor (in GPU memory: uploaded from there)
    with DeviceCAVI(X.shape[0], X.shape[1], theta.dims[1], dtype=theta.dtype, device=device) as eng:
        eng.upload(X)
        eng.set_gamma("theta", theta.vi_shape, theta.vi_rate)
        eng.set_gamma("beta", beta.vi_shape, beta.vi_rate)
        return eng.cellmean_negative_pois_llh() if by == "cell" else eng.genemean_negative_pois_llh()


def cellmean_negative_pois_llh(X, *, theta, beta, device=None, **kwargs):
    """Mean negative Poisson log-likelihood of the stored entries of each cell of X (NaN for a cell without any),
    float64 [ncells], evaluated on the GPU.  `device`: HIP device ordinal, default $SCHPF_DEVICE or 0."""
    return _rowmean_on_device(X, theta, beta, "cell", device)


def genemean_negative_pois_llh(X, *, theta, beta, device=None, **kwargs):
    """Mean negative Poisson log-likelihood of the stored entries of each gene of X (NaN for a gene without any),
    float64 [ngenes], evaluated on the GPU.  `device`: HIP device ordinal, default $SCHPF_DEVICE or 0."""
    return _rowmean_on_device(X, theta, beta, "gene", device)


def observed_moments(X, by):
    """Per row of the axis `by` of X ("cell": rows, "gene": columns), over ALL its entries, stored or not: (mean,
    population variance, fraction of zeros), float64 -- from sum x, sum x^2 and the number of entries with x > 0, after
    duplicate coordinates have been summed.  SciPy input: on the host.  A torch sparse tensor: with torch ops where it
    lives (in GPU memory nothing of O(nnz) comes to the host)."""
    from .device_input import is_torch_tensor
    if by not in ("cell", "gene"):
        raise ValueError("by must be 'cell' or 'gene', got %r" % (by,))
    axis = 0 if by == "cell" else 1
    n_rows, n = int(X.shape[axis]), int(X.shape[1 - axis])
    if is_torch_tensor(X):
        import torch
        if X.layout != torch.sparse_coo:
            X = X.to_sparse_coo()
        X = X.coalesce()                       # duplicates summed
        major, x = X.indices()[axis], X.values().to(torch.float64)
        sums = [torch.zeros(n_rows, dtype=torch.float64, device=x.device).index_add_(0, major, v)
                for v in (x, x * x, (x > 0).to(torch.float64))]
        s1, s2, pos = (v.cpu().numpy() for v in sums)
    else:
        from scipy.sparse import coo_matrix
        C = X.tocoo() if not hasattr(X, "row") else X
        C = coo_matrix((np.asarray(C.data, np.float64), (C.row, C.col)), shape=C.shape)   # a copy: X stays as it is
        C.sum_duplicates()
        major = C.row if axis == 0 else C.col
        s1 = np.bincount(major, weights=C.data, minlength=n_rows)
        s2 = np.bincount(major, weights=C.data * C.data, minlength=n_rows)
        pos = np.bincount(major, weights=(C.data > 0).astype(np.float64), minlength=n_rows)
    mean = s1 / n
    return mean, s2 / n - mean * mean, (n - pos) / n


def predictive_check(X, *, theta, beta, by="gene", device=None, **kwargs):
    """Posterior predictive check of a Poisson factor model without zero inflation: per gene (by="gene")
    or per cell (by="cell"), what the model predicts for the mean, the variance and the fraction of zeros of the row's
    entries -- over ALL cell x gene pairs, from lambda = E[theta] . E[beta], summed on the GPU -- next to what X shows.

    Returns a dict of float64 arrays, one value per row of the axis: pred_mean, pred_var, pred_zero_frac and, unless X is
    None, obs_mean, obs_var (population variance), obs_zero_frac.  X: a SciPy sparse matrix or a torch sparse tensor
    (duplicate coordinates are summed first); it is not uploaded.  A theta whose rate is divided by frac / (1 - frac)
    gives the check for the test part of thinned counts.  `device`: HIP device ordinal, default $SCHPF_DEVICE or 0."""
    from .engine import DeviceCAVI, predicted_moments   # late import, as in projection_loss_function
    if by not in ("cell", "gene"):
        raise ValueError("by must be 'cell' or 'gene', got %r" % (by,))
    ncells, ngenes = theta.vi_shape.shape[0], beta.vi_shape.shape[0]
    if X is not None and tuple(int(v) for v in X.shape) != (ncells, ngenes):
        raise ValueError("X has shape %s, theta and beta describe %d cells x %d genes" % (tuple(X.shape), ncells, ngenes))
    device = device_of(device)
    with DeviceCAVI(ncells, ngenes, theta.dims[1], dtype=theta.dtype, device=device) as eng:
        eng.set_gamma("theta", theta.vi_shape, theta.vi_rate)
        eng.set_gamma("beta", beta.vi_shape, beta.vi_rate)
        sums = eng.predictive_rows(by)
    out = dict(zip(PPC_COLUMNS[:3], predicted_moments(sums, ngenes if by == "cell" else ncells)))
    if X is not None:
        out.update(zip(PPC_COLUMNS[3:], observed_moments(X, by)))
    return out

