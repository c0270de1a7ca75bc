"""Posterior predictive check, the parts that need no GPU: the yardstick the device is held to
(tests/_predictive_reference.py) against a closed form and against a Poisson draw, the observed-moment helper of
schpf_amd.loss.predictive_check, and the declaration of the C entry point."""
import os
import re

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.sparse import coo_matrix

from conftest import ROOT
import _predictive_reference as ref


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rate_is_the_closed_form(dtype):
    """rate[r] = sum_m sum_k E_rk E_mk = E_r . (sum_m E_m): the dense sum against the factored one."""
    st = ref.random_gammas(130, 70, 7, dtype, seed=1)
    et, eb = ref.expected(st["theta"]), ref.expected(st["beta"])
    assert_allclose(ref.sums(st["theta"], st["beta"], "cell")["rate"], et @ eb.sum(axis=0), rtol=1e-13)
    assert_allclose(ref.sums(st["theta"], st["beta"], "gene")["rate"], eb @ et.sum(axis=0), rtol=1e-13)
    for name in ref.SUMS:        # every sum has the same total whichever axis it is taken along
        assert_allclose(ref.sums(st["theta"], st["beta"], "cell")[name].sum(),
                        ref.sums(st["theta"], st["beta"], "gene")[name].sum(), rtol=1e-13)


def test_predicted_moments_match_a_poisson_draw():
    """x_m ~ Poisson(lambda_m) independently, m < n.  About the predicted mean mu the statistic T = mean (x_m - mu)^2
    has E[T] = mean(lambda + (lambda - mu)^2) = rate/n + rate2/n - mu^2, the predicted variance, exactly, and
    Var[T] = sum_m Var[(x_m - mu)^2] / n^2 with, for d = lambda - mu and the Poisson central moments (l, l, l + 3 l^2),
    E[(x - mu)^4] = l + 3 l^2 + 4 d l + 6 d^2 l + d^4.  The mean and the fraction of zeros are sample means of
    variables with variance lambda and p (1 - p).  Each is held to 6 sigma of its own sampling error."""
    n = 200000
    st = ref.random_gammas(n, 4, 3, np.float64, seed=7)
    lam = ref.rates(st["theta"], st["beta"])                    # [n, 4]: four genes, n cells each
    mean, var, zero = ref.predicted(ref.sums_of(lam, "gene"), n)
    x = np.random.RandomState(11).poisson(lam).astype(np.float64)
    d = lam - mean
    second = lam + d * d
    fourth = lam + 3 * lam ** 2 + 4 * d * lam + 6 * d * d * lam + d ** 4
    sigma_t = np.sqrt((fourth - second ** 2).sum(axis=0)) / n
    t = ((x - mean) ** 2).mean(axis=0)
    assert np.all(np.abs(t - var) <= 6 * sigma_t), (t, var, sigma_t)
    assert np.all(sigma_t < 0.02 * var)                         # the bound is a tight one
    assert np.all(np.abs(x.mean(axis=0) - mean) <= 6 * np.sqrt(lam.sum(axis=0)) / n)
    p = np.exp(-lam)
    assert np.all(np.abs((x == 0).mean(axis=0) - zero) <= 6 * np.sqrt((p * (1 - p)).sum(axis=0)) / n)


def matrix_with_stored_zeros_and_duplicates(N=57, G=43, seed=2):
    rng = np.random.RandomState(seed)
    nnz = 600
    row, col = rng.randint(0, N, nnz), rng.randint(0, G, nnz)
    val = rng.randint(0, 6, nnz)                                # explicit zeros among the values
    row[:50], col[:50] = row[50:100], col[50:100]               # repeated coordinates
    row[100:110], col[100:110] = row[110:120], col[110:120]
    val[100:120] = 0                                            # ... some of which sum to a stored zero
    row[-1], col[-1], val[-1] = N - 1, G - 1, 3
    return coo_matrix((val, (row, col)), shape=(N, G))


@pytest.mark.parametrize("fmt", ["coo", "csr", "csc"])
def test_observed_moments_of_a_scipy_matrix(fmt):
    from schpf_amd.loss import observed_moments
    X = matrix_with_stored_zeros_and_duplicates()
    assert (X.data == 0).any() and X.nnz > len(set(zip(X.row, X.col)))
    dense = np.zeros(X.shape)
    np.add.at(dense, (X.row, X.col), X.data)                    # duplicates summed
    before = (X.row.copy(), X.col.copy(), X.data.copy())
    given = X if fmt == "coo" else X.asformat(fmt)
    for by in ("cell", "gene"):
        got = observed_moments(given, by)
        for g, w in zip(got, ref.observed(dense, by)):
            assert g.dtype == np.float64
            assert_array_equal(g, w)                            # integer sums in float64: exact
        assert_allclose(got[1], dense.var(axis=1 if by == "cell" else 0), rtol=1e-12, atol=1e-14)
    for a, b in zip(before, (X.row, X.col, X.data)):            # the caller's matrix is left as it was
        assert_array_equal(a, b)
    with pytest.raises(ValueError):
        observed_moments(X, "factor")


def test_observed_moments_of_a_cpu_tensor():
    torch = pytest.importorskip("torch")
    from schpf_amd.loss import observed_moments
    X = matrix_with_stored_zeros_and_duplicates()
    dense = np.zeros(X.shape)
    np.add.at(dense, (X.row, X.col), X.data)
    T = torch.sparse_coo_tensor(np.stack([X.row, X.col]).astype(np.int64), torch.as_tensor(X.data.astype(np.int64)), X.shape)
    for by in ("cell", "gene"):
        for g, w in zip(observed_moments(T, by), ref.observed(dense, by)):
            assert_array_equal(g, w)


def test_the_header_declares_the_entry_point():
    """... and the binding table knows it; tests/test_capi_host.py then holds the library's exports to the header."""
    from schpf_amd import _lib, loss
    text = open(os.path.join(ROOT, "include", "schpf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+schpf_predictive_rows\s*\(\s*schpf_ctx\s*\*\s*ctx\s*,\s*int\s+by\s*,\s*double\s*\*\s*zeros\s*,"
                     r"\s*double\s*\*\s*rate\s*,\s*double\s*\*\s*rate2\s*\)\s*;", text)
    assert len(_lib.SIGNATURES["schpf_predictive_rows"]) == 5
    assert hasattr(_lib.load(), "schpf_predictive_rows")
    assert "predictive_check" in loss.__all__
    assert tuple(loss.PPC_COLUMNS) == ref.COLUMNS


def test_score_ppc_is_opt_in():
    from schpf_amd import cli
    p = cli._parser()
    assert p.parse_args(["score", "-m", "m.joblib"]).ppc is False
    assert p.parse_args(["score", "-m", "m.joblib", "-i", "x.mtx", "--ppc"]).ppc is True
