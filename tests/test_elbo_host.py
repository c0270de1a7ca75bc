"""The ELBO's host yardstick (tests/_elbo_reference.py) checked against its own derivation, and the C ABI's argument
errors of schpf_elbo_terms -- no GPU needed."""
import ctypes

import numpy as np
import pytest
from scipy.special import softmax

from conftest import synthetic_counts
import _elbo_reference as ref


def _state(X, K, seed):
    rng = np.random.RandomState(seed)
    N, G = X.shape
    g = lambda *d: (rng.uniform(0.2, 3.0, d), rng.uniform(0.5, 2.0, d))  # noqa: E731
    return g(N), g(N, K), g(G), g(G, K)


@pytest.mark.parametrize("K", [3, 10])
def test_phi_optimal_data_term_equals_the_explicit_phi_form(K):
    X = synthetic_counts(60, 80, 0.1, seed=K)
    xi, theta, eta, beta = _state(X, K, K)
    t = ref.elbo_terms(X, 0.3, 1.0, 1.5, 0.3, 1.0, 2.0, xi, theta, eta, beta)
    explicit = ref.explicit_phi_likelihood(X, theta, beta)
    assert abs((t["data"] - t["logfac"] - t["rate"]) - explicit) <= 1e-12 * ref.scale(t)
    # any other phi is strictly worse: the softmax is the maximiser
    x, l = ref._log_weights(X, theta[0], theta[1], beta[0], beta[1])
    rng = np.random.RandomState(1)
    phi = softmax(np.log(softmax(l, axis=1)) + 0.3 * rng.standard_normal(l.shape), axis=1)
    assert ref.explicit_phi_likelihood(X, theta, beta, phi) < explicit - 1e-9 * ref.scale(t)


def test_reference_entropy_is_the_models():
    from schpf_amd.scHPF_ import HPF_Gamma
    rng = np.random.RandomState(0)
    s, r = rng.uniform(1e-3, 50.0, (30, 4)), rng.uniform(1e-2, 20.0, (30, 4))
    np.testing.assert_allclose(ref.gamma_parts(s, r)[2], HPF_Gamma(s, r).entropy, rtol=1e-14, atol=1e-13)


def test_elbo_terms_null_arguments_are_errors():
    from schpf_amd import _lib
    lib = _lib.load()
    terms = (ctypes.c_double * 5)()
    assert lib.schpf_elbo_terms(None, 1.0, 1.0, terms) != 0
    assert b"NULL" in lib.schpf_last_error()
