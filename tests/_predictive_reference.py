"""Host yardstick of the posterior predictive check: NumPy float64 on the dense N x G matrix of rates.

A Gamma is a pair (vi_shape, vi_rate) of arrays in the model dtype; they are converted to float64 as they are, so the
yardstick sees exactly the values the engine stores.  lambda = (theta_shape / theta_rate) @ (beta_shape / beta_rate).T;
per row of the axis `by` ("cell": major = cell, "gene": major = gene) the three sums over ALL rows of the other axis."""
import numpy as np

SUMS = ("zeros", "rate", "rate2")
COLUMNS = ("pred_mean", "pred_var", "pred_zero_frac", "obs_mean", "obs_var", "obs_zero_frac")


def expected(gamma):
    shape, rate = gamma
    return np.asarray(shape).astype(np.float64) / np.asarray(rate).astype(np.float64)


def rates(theta, beta):
    """lambda, dense float64 [ncells, ngenes]."""
    return expected(theta) @ expected(beta).T


def sums_of(lam, by):
    """{"zeros", "rate", "rate2"} per row of the axis from a dense lambda [ncells, ngenes]."""
    axis = {"cell": 1, "gene": 0}[by]
    return {"zeros": np.exp(-lam).sum(axis=axis), "rate": lam.sum(axis=axis), "rate2": (lam * lam).sum(axis=axis)}


def sums(theta, beta, by):
    return sums_of(rates(theta, beta), by)


def predicted(s, n):
    """(mean, variance, fraction of zeros) of an entry of each row, n = entries per row: Poisson given lambda, so the
    variance is E[lambda] + Var[lambda] = rate/n + rate2/n - (rate/n)^2."""
    mean = s["rate"] / n
    return mean, mean + s["rate2"] / n - mean * mean, s["zeros"] / n


def observed(dense, by):
    """(mean, population variance, fraction of zeros) per row of the axis from a dense copy of X, through the integer
    sums sum x, sum x^2 and #(x > 0) -- exact in float64 below 2^53."""
    axis = {"cell": 1, "gene": 0}[by]
    D = np.asarray(dense, np.float64)
    n = D.shape[axis]
    s1, s2, pos = D.sum(axis=axis), (D * D).sum(axis=axis), (D > 0).sum(axis=axis).astype(np.float64)
    mean = s1 / n
    return mean, s2 / n - mean * mean, (n - pos) / n


def check(theta, beta, dense, by):
    """What predictive_check returns, from the yardstick (dense=None: the predicted half only)."""
    n = np.asarray(beta[0] if by == "cell" else theta[0]).shape[0]
    out = dict(zip(COLUMNS[:3], predicted(sums(theta, beta, by), n)))
    if dense is not None:
        out.update(zip(COLUMNS[3:], observed(dense, by)))
    return out


def random_gammas(N, G, K, dtype, seed):
    rng = np.random.RandomState(seed)
    g = lambda *d: (rng.uniform(0.2, 3.0, d).astype(dtype), rng.uniform(0.5, 2.0, d).astype(dtype))  # noqa: E731
    return {"xi": g(N), "theta": g(N, K), "eta": g(G), "beta": g(G, K)}
