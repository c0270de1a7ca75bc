"""Host yardstick of the per-row Poisson loss: float64 NumPy / SciPy from (X, theta, beta).  Every stored
entry is an observation of its own -- duplicates are not summed, explicit zeros count -- and a row without stored
entries has no mean (NaN).  Never calls the code under test."""
import numpy as np
from scipy.special import gammaln


def _rates(X, theta, beta):
    """x and r = sum_k E[theta][row, k] E[beta][col, k] of every stored entry, float64."""
    ts, tr = (np.asarray(v, np.float64) for v in theta)
    bs, br = (np.asarray(v, np.float64) for v in beta)
    r = np.einsum("ik,ik->i", (ts / tr)[X.row], (bs / br)[X.col])
    return np.asarray(X.data, np.float64), r


def loss_rows(X, theta, beta, by="cell"):
    """theta, beta: (shape, rate) pairs.  Per row of axis `by`: {llh: sum x log r - r, gl: sum gammaln(x + 1),
    count: stored entries, scale: sum |x log r| + r (what a tolerance on llh is relative to)}."""
    x, r = _rates(X, theta, beta)
    with np.errstate(divide="ignore", invalid="ignore"):
        xlogr = np.where(x > 0, x * np.log(r), 0.0)   # an explicit zero: x log r = 0 whatever r
    idx, n = (X.row, X.shape[0]) if by == "cell" else (X.col, X.shape[1])
    return {"llh": np.bincount(idx, weights=xlogr - r, minlength=n),
            "gl": np.bincount(idx, weights=gammaln(x + 1.0), minlength=n),
            "count": np.bincount(idx, minlength=n).astype(np.int64),
            "scale": np.bincount(idx, weights=np.abs(xlogr) + r, minlength=n)}


def rowmean_negative(X, theta, beta, by="cell"):
    """Mean over the row's stored entries of -(x log r - r - gammaln(x + 1)); NaN for a row without any."""
    t = loss_rows(X, theta, beta, by)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(t["llh"] - t["gl"]) / t["count"]
