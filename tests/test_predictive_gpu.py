"""Posterior predictive row sums on the GPU (schpf_predictive_rows) against the float64 host yardstick
(tests/_predictive_reference.py).

Tolerance: 1e-11 relative on every output in BOTH model dtypes -- the project's float64 ELBO tolerance; the device does
all arithmetic in double from the stored shape / rate, so a float32 engine owes the yardstick the same.  Every term of
the three sums is >= 0, so relative error is well defined; a sum of n terms in double is good to about n * 1.1e-16
(n <= 70001 here: 8e-12 in the worst case, a few 1e-14 in practice), the exponential to 2 ulp (special.h)."""
import ctypes
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from conftest import GOLDEN, load_golden, golden_coo, synthetic_counts
import _predictive_reference as ref

pytestmark = pytest.mark.gpu

RTOL = 1e-11
NAMES = ("xi", "theta", "eta", "beta")
# a lone row; strips and tiles that stick out by one either way; several strips and several tiles (the issue's four)
# -- all of them walk strips of 32 rows.  70001 x 67: the cell axis is long enough for strips of 64 (kernels.h
# predictive_strip), whose tiles of 64 genes stick out by 3; the gene axis walks 547 tiles of 128 cells
SHAPES = [(1, 1), (63, 65), (130, 70), (257, 129)]
LONG = (70001, 67)
# every K of the issue on its shapes (1: a lone factor; 5, 20: one pass over the factors; 50: two passes); the long
# shape with one K of each kind
CASES = [(shape, K) for shape in SHAPES for K in (1, 5, 20, 50)] + [(LONG, 5), (LONG, 50)]


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def engine_with(amd, N, G, K, dtype, st, X=None):
    eng = amd.DeviceCAVI(N, G, K, dtype=dtype)
    if X is not None:
        eng.upload(X, warn=False)
    eng.set_hypers(0.3, 0.3, 1.3, 0.8)
    for name in NAMES:
        eng.set_gamma(name, *st[name])
    return eng


def state_of(eng):
    return {n: eng.get_gamma(n) for n in NAMES}


def check_against_yardstick(eng, st, label):
    got = {}
    for by in ("cell", "gene"):
        want = ref.sums(st["theta"], st["beta"], by)
        got[by] = eng.predictive_rows(by)
        assert set(got[by]) == set(ref.SUMS)
        for name in ref.SUMS:
            g, w = got[by][name], want[name]
            assert g.dtype == np.float64 and g.shape == w.shape
            err = np.abs(g - w) / w
            print("%s by %s %s: largest relative error %.3g" % (label, by, name, err.max()))
            assert_allclose(g, w, rtol=RTOL, atol=0, err_msg="%s %s by %s" % (label, name, by))
    return got


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape, K", CASES)
def test_parity(amd, shape, K, dtype):
    """A random Gamma state, no upload: every output of both axes against the yardstick, and the identities that tie
    them together -- rate is the closed form E_r . sum_m E_m, and each sum has one total whichever axis it runs along."""
    N, G = shape
    st = ref.random_gammas(N, G, K, dtype, seed=K + N)
    with engine_with(amd, N, G, K, dtype, st) as eng:
        got = check_against_yardstick(eng, st, "%dx%d/K%d/%s" % (N, G, K, np.dtype(dtype).name))
        down = state_of(eng)
    et, eb = ref.expected(down["theta"]), ref.expected(down["beta"])
    assert_allclose(got["cell"]["rate"], et @ eb.sum(axis=0), rtol=RTOL)
    assert_allclose(got["gene"]["rate"], eb @ et.sum(axis=0), rtol=RTOL)
    for name in ref.SUMS:
        assert_allclose(got["cell"][name].sum(), got["gene"][name].sum(), rtol=RTOL, err_msg=name)


@pytest.mark.parametrize("dtype, huge", [(np.float64, 1e120), (np.float32, 1e30)])
def test_extremes(amd, dtype, huge):
    N, G, K = 130, 70, 5
    st = ref.random_gammas(N, G, K, dtype, seed=3)
    ts, tr = (a.copy() for a in st["theta"])
    drowned, empty, mixed = slice(10, 20), slice(40, 45), 100
    ts[drowned] = 1e5                                # lambda >= 5e4 * min E[beta] > 800 in every gene
    ts[empty] = np.finfo(dtype).tiny                 # lambda ~ 1e-300 (1e-37 in float32): exp(-lambda) == 1
    tr[mixed, 0], tr[mixed, 1] = huge, 1 / huge      # E = 1 / huge beside E = huge in one row
    st["theta"] = (ts, tr)
    with engine_with(amd, N, G, K, dtype, st) as eng:
        cell, gene = eng.predictive_rows("cell"), eng.predictive_rows("gene")
    lam = ref.rates(st["theta"], st["beta"])
    assert lam[drowned].min() > 800 and lam[empty].max() < 1e-30 and lam[mixed].min() > 1e-2 * huge
    for out in (cell, gene):
        for name in ref.SUMS:
            assert np.all(np.isfinite(out[name])), name
    assert_array_equal(cell["zeros"][drowned], 0.0)
    assert_array_equal(cell["zeros"][empty], float(G))
    assert cell["zeros"][mixed] == 0.0
    rest = np.ones(N, bool)
    rest[drowned] = False
    rest[mixed] = False
    assert_allclose(gene["zeros"], np.exp(-lam[rest]).sum(axis=0), rtol=RTOL)
    for by, out in (("cell", cell), ("gene", gene)):          # and everything else is still the yardstick's
        want = ref.sums_of(lam, by)
        for name in ref.SUMS:
            assert_allclose(out[name], want[name], rtol=RTOL, err_msg="%s by %s" % (name, by))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_leaves_no_trace(amd, dtype):
    N, G, K = 130, 70, 5
    X = synthetic_counts(N, G, 0.1, seed=4)
    st = ref.random_gammas(N, G, K, dtype, seed=5)
    with engine_with(amd, N, G, K, dtype, st) as eng:         # no matrix
        before = state_of(eng)
        first = {by: eng.predictive_rows(by) for by in ("cell", "gene")}
        again = {by: eng.predictive_rows(by) for by in ("cell", "gene")}
        after = state_of(eng)
    for by in first:
        for name in ref.SUMS:
            assert_array_equal(first[by][name], again[by][name])
    for n in NAMES:
        for a, b in zip(before[n], after[n]):
            assert_array_equal(a, b, err_msg=n)
    finals = []
    for probe in (False, True):
        with engine_with(amd, N, G, K, dtype, st, X) as eng:
            eng.steps(2)
            if probe:
                eng.predictive_rows("cell")
                eng.predictive_rows("gene")
            eng.steps(2)
            finals.append((state_of(eng), eng.loss_terms()))
    for n in NAMES:
        for a, b in zip(finals[0][0][n], finals[1][0][n]):
            assert_array_equal(a, b, err_msg=n)
    assert finals[0][1] == finals[1][1]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_after_real_iterations(amd, dtype, monkeypatch):
    """Upload, three iterations with every SCHPF_ switch at its default (the small problem then fuses the column sums:
    tables and sums older than the parameters are what the engine holds), then the sums of the downloaded state."""
    for v in [v for v in os.environ if v.startswith("SCHPF_") and v not in ("SCHPF_DEVICE", "SCHPF_LIB_PATH",
                                                                          "SCHPF_HIP_RUNTIME", "SCHPF_RCCL_PATH")]:
        monkeypatch.delenv(v)
    N, G, K = 257, 129, 20
    X = synthetic_counts(N, G, 0.1, seed=6)
    st = ref.random_gammas(N, G, K, dtype, seed=7)
    with engine_with(amd, N, G, K, dtype, st, X) as eng:
        eng.steps(3)
        got = check_against_yardstick(eng, state_of(eng), "stepped/%s" % np.dtype(dtype).name)
        eng.set_gamma("theta", *st["theta"])                 # parameters newer than the tables
        fresh = check_against_yardstick(eng, dict(state_of(eng)), "reset/%s" % np.dtype(dtype).name)
    assert not np.array_equal(got["cell"]["rate"], fresh["cell"]["rate"])


def test_refusals(amd):
    from schpf_amd import _lib
    st = ref.random_gammas(9, 7, 3, np.float64, seed=8)
    with engine_with(amd, 9, 7, 3, np.float64, st) as eng:
        with pytest.raises(_lib.SchpfHipError, match="SCHPF_BY_CELL"):
            eng.predictive_rows(2)
        with pytest.raises(_lib.SchpfHipError, match="NULL"):
            eng.predictive_rows("gene", which=())
        out = np.empty(9)
        p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert eng._lib.schpf_predictive_rows(eng._h, -1, p, p, p) != 0
        assert eng._lib.schpf_predictive_rows(None, 0, p, p, p) != 0
        for bad in ("factor", None, 1.0, True):
            with pytest.raises(ValueError):
                eng.predictive_rows(bad)
        with pytest.raises(ValueError):
            eng.predictive_rows("cell", which=("zeros", "mean"))
        only = eng.predictive_rows("cell", which=("rate2",))      # a NULL output is skipped
        assert list(only) == ["rate2"]
        assert_array_equal(only["rate2"], eng.predictive_rows("cell")["rate2"])   # the process lives, the engine works


@pytest.fixture(scope="module")
def golden():
    import joblib
    model = joblib.load(os.path.join(GOLDEN, "ref_model_f64.joblib"))
    X = golden_coo(load_golden("fit_data_k5_s0_f64.npz"))    # the matrix it was fitted to
    theta, beta = (model.theta.vi_shape, model.theta.vi_rate), (model.beta.vi_shape, model.beta.vi_rate)
    want = {by: ref.check(theta, beta, X.toarray(), by) for by in ("cell", "gene")}
    return model, X, want


def assert_check(got, want, observed=True):
    assert set(got) == set(ref.COLUMNS if observed else ref.COLUMNS[:3])
    for name in ref.COLUMNS[:3]:
        assert got[name].dtype == np.float64
        assert_allclose(got[name], want[name], rtol=RTOL, atol=0, err_msg=name)
    if observed:
        for name in ref.COLUMNS[3:]:
            assert_array_equal(got[name], want[name], err_msg=name)


@pytest.mark.parametrize("by", ["gene", "cell"])
def test_check_on_the_golden_model(amd, golden, by):
    import torch
    from schpf_amd import loss
    model, X, want = golden
    assert_check(model.predictive_check(X, by=by), want[by])
    assert_check(loss.predictive_check(X.tocsr(), theta=model.theta, beta=model.beta, by=by, a=0.3), want[by])
    assert_check(model.predictive_check(by=by), want[by], observed=False)
    idx = torch.as_tensor(np.stack([X.row, X.col]).astype(np.int64), device="cuda")
    T = torch.sparse_coo_tensor(idx, torch.as_tensor(X.data, device="cuda"), X.shape)
    assert_check(loss.predictive_check(T, theta=model.theta, beta=model.beta, by=by), want[by])
    twice = torch.sparse_coo_tensor(torch.cat([idx, idx[:, :100]], 1),     # duplicates are summed first
                                    torch.cat([T._values(), T._values()[:100]]), X.shape)
    dense = X.toarray().astype(np.float64)
    np.add.at(dense, (X.row[:100], X.col[:100]), X.data[:100])
    got = loss.predictive_check(twice, theta=model.theta, beta=model.beta, by=by)
    for name, w in zip(ref.COLUMNS[3:], ref.observed(dense, by)):
        assert_array_equal(got[name], w, err_msg=name)
    if by == "gene":
        assert model.predictive_check(X)["pred_mean"].shape == (X.shape[1],)     # the default axis
        with pytest.raises(ValueError):
            model.predictive_check(X.tocsr()[:-1])


def test_score_ppc_writes_both_files(amd, golden, tmp_path):
    from scipy.io import mmwrite
    from schpf_amd import cli
    model, X, want = golden
    path = os.path.join(GOLDEN, "ref_model_f64.joblib")
    mmwrite(str(tmp_path / "x.mtx"), X, field="integer")
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "plain"), "-i", str(tmp_path / "x.mtx")]) == 0
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "ppc"), "-i", str(tmp_path / "x.mtx"), "--ppc"]) == 0
    plain, with_ppc = set(os.listdir(str(tmp_path / "plain"))), set(os.listdir(str(tmp_path / "ppc")))
    assert with_ppc == plain | {"gene_ppc.txt", "cell_ppc.txt"} and not plain & {"gene_ppc.txt", "cell_ppc.txt"}
    import json
    assert "ppc" not in json.load(open(str(tmp_path / "plain" / "score_commandline_args.json")))
    for by, n in (("gene", X.shape[1]), ("cell", X.shape[0])):
        table = np.loadtxt(str(tmp_path / "ppc" / (by + "_ppc.txt")))
        assert table.shape == (n, 6)
        assert_check(dict(zip(ref.COLUMNS, table.T.copy())), want[by])
        direct = model.predictive_check(X, by=by)
        for j, name in enumerate(ref.COLUMNS):
            assert_array_equal(table[:, j], direct[name], err_msg=name)       # the same numbers, digit for digit
    with pytest.raises(ValueError):
        cli.main(["score", "-m", path, "-o", str(tmp_path / "bad"), "--ppc"])
