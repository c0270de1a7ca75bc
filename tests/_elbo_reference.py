"""Host yardstick of the ELBO: its five terms in float64 NumPy / SciPy from (X, hypers, four Gammas),
the data term with scipy.special.logsumexp, so that it is right where the device's product form underflows."""
import numpy as np
from scipy.special import digamma, gammaln, logsumexp, softmax


def gamma_parts(shape, rate):
    """(E[x], E[log x], entropy) of Gamma(shape, rate), in float64."""
    s, r = np.asarray(shape, np.float64), np.asarray(rate, np.float64)
    psi = digamma(s)
    return s / r, psi - np.log(r), s - np.log(r) + gammaln(s) + (1.0 - s) * psi


def _loading_terms(shape, rate, cap_shape, cap_rate, prior, cap_prior_shape, cap_prior_rate):
    E, L, H = gamma_parts(shape, rate)
    cE, cL, cH = gamma_parts(cap_shape, cap_rate)
    per_factor = prior * cL[:, None] - gammaln(prior) + (prior - 1.0) * L - cE[:, None] * E + H
    per_row = (cap_prior_shape * np.log(cap_prior_rate) - gammaln(cap_prior_shape) + (cap_prior_shape - 1.0) * cL
               - cap_prior_rate * cE + cH)
    return per_factor.sum() + per_row.sum(), E.sum(0)


def _log_weights(X, theta_shape, theta_rate, beta_shape, beta_rate):
    """Stored entries with x > 0 (explicit zeros contribute nothing), and their L_theta + L_beta rows."""
    x = np.asarray(X.data, np.float64)
    keep = x > 0
    Lt = gamma_parts(theta_shape, theta_rate)[1]
    Lb = gamma_parts(beta_shape, beta_rate)[1]
    return x[keep], Lt[X.row[keep]] + Lb[X.col[keep]]


def elbo_terms(X, a, ap, bp, c, cp, dp, xi, theta, eta, beta):
    """xi, theta, eta, beta: (shape, rate) pairs.  Returns {data, logfac, rate, cell, gene, elbo}."""
    x, l = _log_weights(X, theta[0], theta[1], beta[0], beta[1])
    data = float(np.sum(x * logsumexp(l, axis=1)))
    logfac = float(np.sum(gammaln(np.asarray(X.data, np.float64) + 1.0)))
    cell, s_theta = _loading_terms(theta[0], theta[1], xi[0], xi[1], a, ap, bp)
    gene, s_beta = _loading_terms(beta[0], beta[1], eta[0], eta[1], c, cp, dp)
    rate = float(np.dot(s_theta, s_beta))
    return {"data": data, "logfac": logfac, "rate": rate, "cell": float(cell), "gene": float(gene),
            "elbo": data - logfac - rate + cell + gene}


def explicit_phi_likelihood(X, theta, beta, phi=None):
    """E_q[log p(x | z) + log p(z | theta, beta)] - E_q[log q(z)] summed over the nonzeros with the responsibilities
    phi (default: their optimum, the softmax of L_theta + L_beta), i.e. sum x phi_k (Lt + Lb - log phi_k) - logfac - rate
    -- the form the data term is derived from."""
    x, l = _log_weights(X, theta[0], theta[1], beta[0], beta[1])
    if phi is None:
        phi = softmax(l, axis=1)
    data = float(np.sum(x[:, None] * phi * (l - np.log(phi))))
    logfac = float(np.sum(gammaln(np.asarray(X.data, np.float64) + 1.0)))
    rate = float(np.dot(gamma_parts(*theta)[0].sum(0), gamma_parts(*beta)[0].sum(0)))
    return data - logfac - rate


def scale(terms):
    """sum of |terms|: the yardstick the tolerances are relative to."""
    return sum(abs(terms[k]) for k in ("data", "logfac", "rate", "cell", "gene"))
