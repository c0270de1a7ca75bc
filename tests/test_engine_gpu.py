"""GPU parity of the device-resident CAVI engine and of scHPF.fit()/project() built on
it, against the CPU oracle and the golden traces produced by the reference.

Stated tolerances (DESIGN.md "parity"): after one iteration from identical state,
rtol 1e-11 (f64) / 2e-5 (f32) on every shape/rate; whole fits from identical seeds:
per-check loss rtol 1e-9 (f64) / 1e-4 (f32), final theta/beta/xi/eta rtol 1e-6 (f64) /
2e-2 (f32, 40-60 iterations of f32 round-off through a non-convex iteration).
"""
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose

from conftest import load_golden, golden_coo, synthetic_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["tile", "half", "gather"])
def plan_kind(request, monkeypatch):
    """Every engine test runs on all sweep implementations: the LDS-staged tile plan with the
    schedule the library picks ("tile", what ships), with the half-window schedule forced ("half":
    SCHPF_HALF=2), with balanced windows forced ("balanced": SCHPF_BALANCE=1 -- the library itself only
    balances sparse, wide problems like the C5 share), and the L2-gather plan (selected by the library
    from SCHPF_PLAN when the engine is created).  A test that belongs to some of them narrows the list with
    `only_plans(...)` -- no ids that can only skip -- and the tests of the iteration itself add "balanced"
    (`every_plan`)."""
    monkeypatch.setenv("SCHPF_PLAN", "tile" if request.param in ("half", "balanced") else request.param)
    monkeypatch.delenv("SCHPF_HALF", raising=False)
    monkeypatch.delenv("SCHPF_BALANCE", raising=False)
    if request.param == "half":
        monkeypatch.setenv("SCHPF_HALF", "2")
    monkeypatch.delenv("SCHPF_WPB", raising=False)
    if request.param == "balanced":
        monkeypatch.setenv("SCHPF_BALANCE", "1")
        monkeypatch.setenv("SCHPF_WPB", "16")     # the balanced kernels are the 1024-thread ones
    return request.param


def only_plans(*kinds):
    return pytest.mark.parametrize("plan_kind", list(kinds), indirect=True)


every_plan = only_plans("tile", "half", "gather", "balanced")


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def random_state(oracle, X, K, dtype, seed, a=0.3, c=0.3, ap=1.0, cp=1.0):
    np.random.seed(seed)
    bp, dp, st = oracle.setup_state(X, K, np.dtype(dtype), a, ap, c, cp)
    st.xi_shape[:] = ap + K * a
    st.eta_shape[:] = cp + K * c
    return bp, dp, st


def load_engine(amd, X, K, dtype, st, a, c, bp, dp):
    eng = amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=dtype)
    eng.upload(X)
    eng.set_hypers(a, c, bp, dp)
    eng.set_gamma("xi", st.xi_shape, st.xi_rate)
    eng.set_gamma("theta", st.theta_shape, st.theta_rate)
    eng.set_gamma("eta", st.eta_shape, st.eta_rate)
    eng.set_gamma("beta", st.beta_shape, st.beta_rate)
    return eng


def compare_state(eng, st, rtol):
    for name in ("xi", "theta", "eta", "beta"):
        s, r = eng.get_gamma(name)
        assert_allclose(s, getattr(st, name + "_shape"), rtol=rtol, err_msg=name + " shape")
        assert_allclose(r, getattr(st, name + "_rate"), rtol=rtol, err_msg=name + " rate")


CASES = [  # (ncells, ngenes, density, K)
    (300, 1000, 0.03, 4),
    (513, 777, 0.05, 20),
    (1000, 400, 0.10, 10),
    (200, 300, 0.20, 50),
    (64, 90, 0.30, 1),
    (150, 200, 0.10, 100),
]


@every_plan
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("flags", [{}, {"simultaneous": True}, {"freeze_genes": True}])
def test_iterations_match_oracle(amd, oracle, dtype, case, flags, plan_kind):
    N, G, dens, K = case
    X = synthetic_counts(N, G, dens, seed=N + K)
    a, c = 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, dtype, seed=K)
    f32 = np.dtype(dtype) == np.float32
    with load_engine(amd, X, K, dtype, st, a, c, bp, dp) as eng:
        loss0 = eng.mean_negative_pois_llh()
        want0 = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                              st.beta_shape, st.beta_rate)
        assert_allclose(loss0, want0, rtol=2e-6 if f32 else 1e-12)
        for it in range(3):
            eng.step(**flags)
            oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp, **flags)
            compare_state(eng, st, rtol=(2e-5 * (it + 1)) if f32 else 1e-11)
        loss = eng.mean_negative_pois_llh()
        want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                             st.beta_shape, st.beta_rate)
        assert_allclose(loss, want, rtol=1e-5 if f32 else 1e-11)


def _fuzz_matrix(rng):
    """A random small problem: shape, K, fill, row / column skew, value range, COO order."""
    from scipy.sparse import coo_matrix
    N = int(rng.choice([2, 3, 7, 63, 64, 65, 200, 513, 1200]))       # one row has no variance: bp would be inf
    G = int(rng.choice([2, 3, 31, 128, 129, 400, 1031, 2500]))
    K = int(rng.choice([1, 2, 3, 5, 8, 13, 16, 20, 33, 50, 64, 100]))
    want = max(1, int(N * G * rng.choice([0.005, 0.03, 0.1, 0.4])))
    want = min(want, 60000)
    # skewed marginals: a few heavy cells / genes (what makes rows of a wave uneven)
    pr = rng.gamma(rng.choice([0.3, 1.0, 5.0]), 1.0, N) + 1e-9
    pc = rng.gamma(rng.choice([0.3, 1.0, 5.0]), 1.0, G) + 1e-9
    row = rng.choice(N, want, p=pr / pr.sum()).astype(np.int32)
    col = rng.choice(G, want, p=pc / pc.sum()).astype(np.int32)
    top = int(rng.choice([3, 60, 65535, 200000]))                    # beyond 65535: the unpacked entry format
    val = np.minimum(rng.negative_binomial(1, 0.3, want) + 1, top).astype(np.int64)
    if top > 65535:
        val[rng.randint(0, want, 3)] = top
    X = coo_matrix((val, (row, col)), shape=(N, G))
    X.sum_duplicates()
    while np.var(X.sum(1)) == 0 or np.var(X.sum(0)) == 0:            # the empirical hyperparameters need a spread
        X = (X + coo_matrix(([1], ([0], [0])), shape=(N, G))).tocoo()
    order = rng.permutation(X.nnz)                                   # COO order is not guaranteed sorted
    return coo_matrix((X.data[order], (X.row[order], X.col[order])), shape=(N, G)), K


@every_plan
@pytest.mark.parametrize("seed", range(24))
def test_random_problems_match_oracle(amd, oracle, seed, plan_kind):
    """Seeded fuzz over shapes (1 x 1 upwards, off-by-one around the 64-lane and window sizes), K from 1 to
    100, fill 0.5-40 %, heavy-tailed rows and columns, counts beyond 16 bits, shuffled COO order, both
    dtypes and every ordering flag (1 x n matrices are left out: the reference's bp = mean / var of the row sums
    is infinite there): two iterations and the loss against the oracle."""
    rng = np.random.RandomState(1000 + seed)
    X, K = _fuzz_matrix(rng)
    dtype = [np.float64, np.float32][seed % 2]
    flags = [{}, {"simultaneous": True}, {"freeze_genes": True}, {}][(seed // 2) % 4]
    a, c = float(rng.choice([0.3, 1.0])), float(rng.choice([0.3, 0.05]))
    bp, dp, st = random_state(oracle, X, K, dtype, seed=seed, a=a, c=c)
    f32 = np.dtype(dtype) == np.float32
    with load_engine(amd, X, K, dtype, st, a, c, bp, dp) as eng:
        for it in range(2):
            eng.step(**flags)
            oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp, **flags)
            compare_state(eng, st, rtol=(3e-5 * (it + 1)) if f32 else 1e-11)
        loss = eng.mean_negative_pois_llh()
        st64 = st.cast(np.float64)
        want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st64.theta_shape, st64.theta_rate,
                                             st64.beta_shape, st64.beta_rate)
        assert_allclose(loss, want, rtol=2e-5 if f32 else 1e-11)


@every_plan
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_random_phi_first_iteration_matches_oracle(amd, oracle, dtype, plan_kind):
    """t == 0: responsibilities drawn on the host (reference scHPF_.py:652-655)."""
    X = synthetic_counts(300, 500, 0.05, seed=3)
    K, a, c = 6, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, dtype, seed=1)
    xphi = X.data[:, None] * np.random.dirichlet(np.ones(K), X.nnz)
    with load_engine(amd, X, K, dtype, st, a, c, bp, dp) as eng:
        eng.init_phi_host(xphi)
        eng.step()
        st64 = st.cast(np.float64)
        oracle.cavi_iteration(X.data, X.row, X.col, st64, a, c, bp, dp, xphi=xphi)
        compare_state(eng, st64.cast(dtype), rtol=1e-6 if np.dtype(dtype) == np.float32 else 1e-12)


def test_device_random_phi_is_a_valid_start(amd, oracle):
    """Device-generated t=0 responsibilities: each nonzero's phi sums to one, so
    sum_k (shape - prior) over cells == over genes == sum of counts; cell and gene sweeps
    regenerate the same draws (cross-checked through the k-marginals)."""
    X = synthetic_counts(400, 300, 0.08, seed=9)
    K, a, c = 8, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, np.float64, seed=2)
    with load_engine(amd, X, K, np.float64, st, a, c, bp, dp) as eng:
        eng.init_phi_device(1234)
        eng.step()
        ths, _ = eng.get_gamma("theta")
        bes, _ = eng.get_gamma("beta")
    assert_allclose((ths - a).sum(), X.data.sum(), rtol=1e-12)
    assert_allclose((bes - c).sum(), X.data.sum(), rtol=1e-12)
    assert_allclose((ths - a).sum(0), (bes - c).sum(0), rtol=1e-12)
    assert_allclose((ths - a).sum(1), np.asarray(X.sum(1)).ravel(), rtol=1e-12)
    assert np.all(ths > a * 0.999) and np.all(bes >= c)


@every_plan
def test_underflow_fallback_matches_log_domain_oracle(amd, oracle, plan_kind):
    """Factors whose E[log] differ by thousands make the product form underflow; the
    kernel must fall back to the reference's max-shifted form (hpf_numba.py:98-112)."""
    X = synthetic_counts(120, 150, 0.15, seed=21)
    K, a, c = 4, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, np.float64, seed=5)
    # cell i strongly prefers factor i%K, gene g factor (g+1)%K: shapes 1e-4 elsewhere
    st.theta_shape[:] = 1e-4
    st.beta_shape[:] = 1e-4
    st.theta_shape[np.arange(120), np.arange(120) % K] = 5.0
    st.beta_shape[np.arange(150), (np.arange(150) + 1) % K] = 5.0
    with load_engine(amd, X, K, np.float64, st, a, c, bp, dp) as eng:
        eng.step()
        oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
        compare_state(eng, st, rtol=1e-10)
        eng.step()      # and the fallback accumulators were cleaned up
        oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
        compare_state(eng, st, rtol=1e-10)


@every_plan
def test_empty_rows_and_columns_keep_the_prior(amd, oracle, plan_kind):
    """The reference's own test matrix has 77 all-zero genes; shapes stay at the prior."""
    g = load_golden("pbmc_like_data.npz")
    X = golden_coo(g)
    K, a, c = 5, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, np.float64, seed=0)
    empty = np.asarray(X.sum(0)).ravel() == 0
    assert empty.sum() == 77
    with load_engine(amd, X, K, np.float64, st, a, c, bp, dp) as eng:
        eng.step()
        bes, _ = eng.get_gamma("beta")
        assert np.all(bes[empty] == c)
        oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
        compare_state(eng, st, rtol=1e-11)


E_RTOL_F32 = 1e-3

FITS = [
    ("fit_data_k5_s0_f64.npz", np.float64, {}),
    ("fit_data_k5_s1_f64.npz", np.float64, {}),
    ("fit_conf_k4_s0_f64.npz", np.float64, {}),
    ("fit_data_k5_s0_f64_simul.npz", np.float64, {"beta_theta_simultaneous": True}),
    ("fit_data_k5_s0_f64_single.npz", np.float64, {"single_process": True}),
    ("fit_data_k5_s0_f32.npz", np.float32, {}),
    ("fit_conf_k4_s0_f32.npz", np.float32, {}),
]


@every_plan
@pytest.mark.parametrize("fname,dtype,kw", FITS)
def test_fit_reproduces_reference_trace(amd, fname, dtype, kw, plan_kind):
    """scHPF.fit() from the reference's seed reproduces the reference's run: same bp/dp,
    same number of loss checks (same stop decision), same losses, same final model."""
    from schpf import scHPF
    g = load_golden(fname)
    X = golden_coo(g)
    np.random.seed(int(g["seed"]))
    model = scHPF(int(g["nfactors"]), dtype=dtype, max_iter=int(g["max_iter"]), verbose=False)
    model.fit(X, **kw)
    f32 = np.dtype(dtype) == np.float32
    assert model.bp == float(g["bp"]) and model.dp == float(g["dp"])
    assert len(model.loss) == len(g["loss"])
    assert_allclose(model.loss, g["loss"], rtol=1e-4 if f32 else 1e-9)
    for name in ("xi", "theta", "eta", "beta"):
        got = getattr(model, name)
        assert got.vi_shape.dtype == np.dtype(dtype)
        # float32: 2e-2 on the RAW parameters protects the factors a cell / gene has nearly switched off (shape -> the
        # prior 0.3, its tiny remainder is a difference of float32 sums after 40-60 iterations); their number is
        # asserted small right below, and the EXPECTATIONS the north star names are held to 1e-3 further down
        assert_allclose(got.vi_shape, g[name + "_shape"], rtol=2e-2 if f32 else 1e-6, err_msg=name)
        assert_allclose(got.vi_rate, g[name + "_rate"], rtol=2e-2 if f32 else 1e-6, err_msg=name)
        if f32:
            for part, want in ((got.vi_shape, g[name + "_shape"]), (got.vi_rate, g[name + "_rate"])):
                rel = np.abs(part.astype(np.float64) - want.astype(np.float64)) / np.abs(want.astype(np.float64))
                assert np.mean(rel > 1e-3) <= 0.01, "%s: more than 1 %% of the raw parameters beyond 1e-3" % name
    assert_allclose(model.cell_score(), (g["theta_shape"] / g["theta_rate"])
                    * (g["xi_shape"] / g["xi_rate"])[:, None], rtol=2e-2 if f32 else 1e-6)
    # theta/beta EXPECTATIONS within 1e-6 (f64) / 1e-3 (f32) of the reference's
    for name in ("theta", "beta"):
        got = getattr(model, name)
        want = g[name + "_shape"].astype(np.float64) / g[name + "_rate"].astype(np.float64)
        assert_allclose(got.e_x, want, rtol=E_RTOL_F32 if f32 else 1e-6, atol=0, err_msg="E[%s]" % name)


def test_project_reproduces_reference_trace(amd):
    from schpf import load_model
    import os
    from conftest import GOLDEN
    g = load_golden("project_data_k5_f64.npz")
    X = golden_coo(g)
    model = load_model(os.path.join(GOLDEN, "ref_model_f64.joblib"))   # written by the reference
    model.verbose = False
    beta_before = model.beta.vi_shape.copy()
    np.random.seed(int(g["seed"]))
    proj = model.project(X, max_iter=20)
    assert len(proj.loss) == len(g["loss"])
    assert_allclose(proj.loss, g["loss"], rtol=1e-9)
    assert_allclose(proj.theta.vi_shape, g["theta_shape"], rtol=1e-6)
    assert_allclose(proj.theta.vi_rate, g["theta_rate"], rtol=1e-6)
    assert_allclose(proj.xi.vi_rate, g["xi_rate"], rtol=1e-6)
    assert proj.beta == model.beta and np.array_equal(model.beta.vi_shape, beta_before)
    assert proj.bp == model.bp
    # replace=True returns the loss and swaps xi/theta in place of the model's
    np.random.seed(int(g["seed"]))
    loss = model.project(X, max_iter=20, replace=True)
    assert_allclose(loss, g["loss"], rtol=1e-9)
    assert model.theta.dims == (40, 5)


def test_custom_loss_and_checkstep_receive_host_gammas(amd):
    from schpf import scHPF, HPF_Gamma
    import schpf.loss as ls
    g = load_golden("fit_data_k5_s0_f64.npz")
    X = golden_coo(g)
    seen = []

    def checkstep(bp, dp, xi, eta, theta, beta, t):
        assert isinstance(theta, HPF_Gamma) and theta.dims == (100, 5)
        seen.append(t)

    np.random.seed(0)
    model = scHPF(5, max_iter=25, verbose=False)
    model.fit(X, loss_function=ls.loss_function_for_data(ls.mean_negative_pois_llh, X),
              checkstep_function=checkstep)
    assert seen == [0, 10, 20]
    assert_allclose(model.loss, g["loss"][:3], rtol=1e-9)


def test_mass_conservation_at_benchmark_shape(amd, oracle):
    """Size-independent property at BASELINE config C2 (10k x 5k, 3 %, K=10): every
    nonzero's responsibilities sum to one, so after any iteration
    sum_k (theta.shape - a)[i,:] = row sum of X and sum_k (beta.shape - c)[g,:] = column sum,
    and both k-marginals agree (the cell sweep and the gene sweep saw the same phi)."""
    X = synthetic_counts(10000, 5000, 0.03, seed=42)
    K, a, c = 10, 0.3, 0.3
    for dtype, tol in ((np.float64, 1e-11), (np.float32, 2e-5)):
        bp, dp, st = random_state(oracle, X, K, dtype, seed=0)
        with load_engine(amd, X, K, dtype, st, a, c, bp, dp) as eng:
            for _ in range(3):
                eng.step()
            ths, thr = eng.get_gamma("theta")
            bes, ber = eng.get_gamma("beta")
            loss = eng.mean_negative_pois_llh()
        rows = np.asarray(X.sum(1)).ravel(); cols = np.asarray(X.sum(0)).ravel()
        assert_allclose((ths.astype(np.float64) - a).sum(1), rows, rtol=tol, atol=tol)
        assert_allclose((bes.astype(np.float64) - c).sum(1), cols, rtol=tol, atol=tol * 10)
        assert_allclose((ths.astype(np.float64) - a).sum(0), (bes.astype(np.float64) - c).sum(0), rtol=tol * 10)
        want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, ths, thr, bes, ber, nthreads=8)
        assert_allclose(loss, want, rtol=1e-5 if dtype == np.float32 else 1e-11)
        assert np.all(np.isfinite(ths)) and np.all(thr > 0) and np.all(ber > 0)


@only_plans("tile")
def test_mass_conservation_at_headline_shape(amd, oracle, plan_kind):
    """The same size-independent properties at the headline shape (BASELINE C3: 100k x 20k, K=20,
    1024-thread workgroups, 152 KiB windows, the dual launch) with 1 % of the entries filled, in
    float64: row / column sums, agreeing k-marginals, the loss against the oracle."""
    X = synthetic_counts(100000, 20000, 0.01, seed=42)
    K, a, c = 20, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, np.float64, seed=0)
    with load_engine(amd, X, K, np.float64, st, a, c, bp, dp) as eng:
        assert eng.plan_info()["chunk_len"] == -972          # 152 KiB / (20 x 8 B) rows per window
        for _ in range(2):
            eng.step()
        ths, thr = eng.get_gamma("theta")
        bes, ber = eng.get_gamma("beta")
        loss = eng.mean_negative_pois_llh()
    rows = np.asarray(X.sum(1)).ravel(); cols = np.asarray(X.sum(0)).ravel()
    assert_allclose((ths - a).sum(1), rows, rtol=1e-11, atol=1e-11)
    assert_allclose((bes - c).sum(1), cols, rtol=1e-11, atol=1e-10)
    assert_allclose((ths - a).sum(0), (bes - c).sum(0), rtol=1e-10)
    want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, ths, thr, bes, ber, nthreads=8)
    assert_allclose(loss, want, rtol=1e-11)


@only_plans("tile", "half", "balanced")
def test_persistent_dual_launch_equals_one_workgroup_per_task_bitwise(amd, oracle, plan_kind, monkeypatch):
    """The dual sweep launch as persistent workgroups that draw tasks from a device counter (default)
    against one workgroup per task (SCHPF_PERSISTENT=0), with more tasks than the device holds at once so
    that the counter is actually used, over several launches (the counter re-arms itself): bitwise equal."""
    X = synthetic_counts(20000, 8000, 0.015, seed=12)        # 40 blocks x 9 windows + 16 x 21: > 256 tasks
    K, a, c = 20, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, np.float64, seed=4)
    got = []
    for persistent in ("1", "0"):
        monkeypatch.setenv("SCHPF_PERSISTENT", persistent)
        monkeypatch.setenv("SCHPF_TASKS", "2000")
        monkeypatch.setenv("SCHPF_WPB", "16")
        with load_engine(amd, X, K, np.float64, st, a, c, bp, dp) as eng:
            for _ in range(3):
                eng.step()
            eng.steps(4)                                     # and inside a captured graph
            info = eng.plan_info()
            got.append((eng.get_gamma("theta"), eng.get_gamma("beta"), info["n_waves_cell"] + info["n_waves_gene"]))
    assert got[0][2] == got[1][2] and got[0][2] > 300        # tasks of both orientations
    for x, y in zip(got[0][:2], got[1][:2]):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


@every_plan
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_matrix_without_stored_entries_keeps_the_priors(amd, oracle, dtype, plan_kind):
    """The empty input: no stored entry at all.  Every shape stays at its prior, the rates follow from the capacities
    and the column sums exactly as in the oracle's iteration over zero nonzeros (hpf_numba.py:151 with an empty loop),
    inside a captured stretch too; the mean loss over no entries is NaN like the reference's np.mean of an empty array."""
    from scipy.sparse import coo_matrix
    N, G, K, a, c = 70, 45, 6, 0.3, 0.3
    X = coo_matrix((np.zeros(0, np.int32), (np.zeros(0, np.int32), np.zeros(0, np.int32))), shape=(N, G))
    np.random.seed(2)
    _, _, st = oracle.setup_state(synthetic_counts(N, G, 0.2, seed=1), K, np.dtype(dtype), a, 1.0, c, 1.0)
    bp, dp = 0.7, 0.02
    st.xi_shape[:] = 1.0 + K * a
    st.eta_shape[:] = 1.0 + K * c
    f32 = np.dtype(dtype) == np.float32
    with load_engine(amd, X, K, dtype, st, a, c, bp, dp) as eng:
        assert eng.nnz == 0
        for it in range(2):
            eng.step()
            oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
            compare_state(eng, st, rtol=(2e-5 * (it + 1)) if f32 else 1e-11)
        eng.steps(4)
        for _ in range(4):
            oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
        compare_state(eng, st, rtol=2e-4 if f32 else 1e-11)
        ths, _ = eng.get_gamma("theta")
        bes, _ = eng.get_gamma("beta")
        assert np.all(ths == np.dtype(dtype).type(a)) and np.all(bes == np.dtype(dtype).type(c))
        assert np.isnan(eng.mean_negative_pois_llh())


@pytest.mark.parametrize("plan_kind,dtype", [("gather", np.float64), ("gather", np.float32), ("tile", np.float32)],
                         indirect=["plan_kind"])
def test_largest_supported_number_of_factors(amd, oracle, dtype, plan_kind):
    """K = 256, the most the update kernel's one-thread-per-(row, factor) mapping takes; 257 is refused.
    Rows of 2 KiB (float64) are beyond the LDS-staged plan's 1 KiB rows: the library takes the L2-gather plan for them
    by itself (policy.cpp choose_config), which is the plan forced here; float32 rows (1 KiB) run on either."""
    N, G, K, a, c = 90, 120, 256, 0.3, 0.3
    X = synthetic_counts(N, G, 0.15, seed=8)
    bp, dp, st = random_state(oracle, X, K, dtype, seed=12)
    f32 = np.dtype(dtype) == np.float32
    with load_engine(amd, X, K, dtype, st, a, c, bp, dp) as eng:
        for it in range(2):
            eng.step()
            oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
            compare_state(eng, st, rtol=(2e-5 * (it + 1)) if f32 else 1e-11)
        want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                             st.beta_shape, st.beta_rate)
        assert_allclose(eng.mean_negative_pois_llh(), want, rtol=1e-5 if f32 else 1e-11)
    with pytest.raises(ValueError):
        amd.DeviceCAVI(N, G, 257, dtype=dtype)


def test_engine_argument_errors(amd):
    X = synthetic_counts(50, 60, 0.1)
    with pytest.raises(ValueError):
        amd.DeviceCAVI(50, 60, 300)                       # nfactors > 256
    with amd.DeviceCAVI(50, 60, 3) as eng:
        with pytest.raises(Exception):
            eng.step()                                    # nothing uploaded
        with pytest.raises(ValueError):
            eng.upload(synthetic_counts(51, 60, 0.1))     # wrong shape
        for poison in (-1.0, np.nan, np.inf):
            bad = X.copy(); bad.data = bad.data.astype(np.float64); bad.data[0] = poison
            with pytest.raises(ValueError):
                eng.upload(bad)                           # not a Poisson observation
        eng.upload(X)
        with pytest.raises(ValueError):
            eng.set_gamma("theta", np.ones((50, 2)), np.ones((50, 2)))


@every_plan
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_real_valued_data_and_stored_zeros_match_oracle(amd, oracle, dtype, plan_kind):
    """The reference fits any non-negative X.data (normalised / down-weighted counts, explicitly
    stored zeros, counts beyond 2^24; hpf_numba.py:98-112 only multiplies by it).  Values travel
    as float32 (a RuntimeWarning says so when that rounds); a stored zero adds nothing to the
    updates and -r to the loss, and counts in the mean (hpf_numba.py:43-50, loss.py:167)."""
    from scipy.sparse import coo_matrix
    X0 = synthetic_counts(300, 400, 0.06, seed=21)
    rng = np.random.RandomState(1)
    data = X0.data.astype(np.float64) * rng.uniform(0.25, 3.0, X0.nnz)     # not float32-representable
    data[::11] = 0.0                                                        # stored zeros
    data[5] = 2.0 ** 25 + 2.0                                               # a huge "count"
    X = coo_matrix((data, (X0.row, X0.col)), shape=X0.shape)
    K, a, c = 7, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, dtype, seed=2)
    eng = amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=dtype)
    with eng:
        with pytest.warns(RuntimeWarning, match="rounded"):
            eng.upload(X)
        info = eng.upload_info()
        assert info["zeros"] == len(data[::11]) and info["rounded"] > 0 and info["nnz"] == X.nnz
        eng.set_hypers(a, c, bp, dp)
        for n in ("xi", "theta", "eta", "beta"):
            eng.set_gamma(n, getattr(st, n + "_shape"), getattr(st, n + "_rate"))
        f32 = np.dtype(dtype) == np.float32
        for it in range(2):
            eng.step()
            oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
            # the float32 rounding of the data (6e-8 relative) is the floor in float64
            compare_state(eng, st, rtol=(2e-5 * (it + 1)) if f32 else 5e-7)
        loss = eng.mean_negative_pois_llh()
        # float64 evaluation of the same state: with a 3e7 "count" in the data the float32 form of
        # the pointwise llh (x log r - r - lgamma(x+1) ~ 5e8) is only good to ~40 absolute
        s64 = st.cast(np.float64)
        want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, s64.theta_shape, s64.theta_rate,
                                             s64.beta_shape, s64.beta_rate)
        assert_allclose(loss, want, rtol=1e-5 if f32 else 5e-7)


@only_plans("tile", "balanced")
@pytest.mark.parametrize("device_plan", ["1", "0"])
def test_duplicate_entries_match_oracle(amd, oracle, plan_kind, device_plan, monkeypatch):
    """A COO may hold an entry twice; the reference treats every stored entry as a nonzero of its own
    (hpf_numba.py:97-112 runs over X.data) and so does the engine -- with both plan builders, and with the
    balancing pass, whose keys (block, minor, lane group) then repeat."""
    from scipy.sparse import coo_matrix
    monkeypatch.setenv("SCHPF_DEVICE_PLAN", device_plan)
    X0 = synthetic_counts(700, 900, 0.05, seed=31)
    rng = np.random.RandomState(2)
    pick = rng.choice(X0.nnz, 3000, replace=False)
    row = np.concatenate([X0.row, X0.row[pick], X0.row[pick[:500]]])
    col = np.concatenate([X0.col, X0.col[pick], X0.col[pick[:500]]])
    data = np.concatenate([X0.data, X0.data[pick] + 1, np.ones(500, X0.data.dtype)])
    perm = rng.permutation(len(data))
    X = coo_matrix((data[perm], (row[perm], col[perm])), shape=X0.shape)    # NOT summed: nnz counts the repeats
    assert X.nnz == X0.nnz + 3500
    K, a, c = 12, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, np.float64, seed=3)
    with load_engine(amd, X, K, np.float64, st, a, c, bp, dp) as eng:
        for it in range(2):
            eng.step()
            oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
            compare_state(eng, st, rtol=1e-11)
        want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate, st.beta_shape, st.beta_rate)
        assert_allclose(eng.mean_negative_pois_llh(), want, rtol=1e-11)


def _subproblem_check(oracle, X, st_before, got, a, c, bp, dp, cells, genes, rtol, simultaneous=False):
    """Oracle comparison that scales to the benchmark sizes.  theta.shape[i] depends only on row
    i's nonzeros and the old tables, beta.shape[g] only on column g's; the rate updates need the
    column sums of E[theta] (old) and E[beta] (new), which are O((N+G)K) numpy.  So: run the
    oracle's own iteration on the sub-matrices the sampled rows / columns define and compare."""
    from scipy.sparse import coo_matrix
    dt = st_before.theta_shape.dtype
    # the oracle runs in float64 for both model dtypes: at N = 1e5 its float32 form (serial float32
    # column sums, like the reference's loops) is itself only good to ~1e-4, so the float64
    # evaluation of the same formulas is the sharper reference for a float32 engine
    st_before = st_before.cast(np.float64)
    ths, thr, bes, ber = st_before.theta_shape, st_before.theta_rate, st_before.beta_shape, st_before.beta_rate
    # gene side: sampled columns, all cells (the oracle's beta update is exact for them: beta.shape
    # needs the column's nonzeros, beta.rate the sum over ALL cells of the old E[theta])
    keep = np.isin(X.col, genes)
    remap = np.full(X.shape[1], -1, np.int64); remap[genes] = np.arange(len(genes))
    Xg = coo_matrix((X.data[keep], (X.row[keep], remap[X.col[keep]])), shape=(X.shape[0], len(genes)))
    sg = oracle.State(st_before.xi_shape.copy(), st_before.xi_rate.copy(), ths.copy(), thr.copy(),
                      st_before.eta_shape[genes].copy(), st_before.eta_rate[genes].copy(),
                      np.ascontiguousarray(bes[genes]), np.ascontiguousarray(ber[genes]))
    oracle.cavi_iteration(Xg.data, Xg.row, Xg.col, sg, a, c, bp, dp, simultaneous=simultaneous, nthreads=8)
    assert_allclose(got["beta"][0][genes], sg.beta_shape, rtol=rtol, err_msg="beta shape (sampled genes)")
    assert_allclose(got["beta"][1][genes], sg.beta_rate, rtol=rtol, err_msg="beta rate (sampled genes)")
    assert_allclose(got["eta"][1][genes], sg.eta_rate, rtol=rtol, err_msg="eta rate (sampled genes)")
    # cell side: sampled rows, all genes.  theta.rate needs sum_g E[beta_gk] of the NEW beta (old
    # beta when simultaneous): take the engine's new beta for it -- verified on the sample above
    # and globally by the mass-conservation checks -- and run the oracle's cell block with it.
    keep = np.isin(X.row, cells)
    remap = np.full(X.shape[0], -1, np.int64); remap[cells] = np.arange(len(cells))
    Xc = coo_matrix((X.data[keep], (remap[X.row[keep]], X.col[keep])), shape=(len(cells), X.shape[1]))
    sc = oracle.State(st_before.xi_shape[cells].copy(), st_before.xi_rate[cells].copy(),
                      np.ascontiguousarray(ths[cells]), np.ascontiguousarray(thr[cells]),
                      st_before.eta_shape.copy(), st_before.eta_rate.copy(), bes.copy(), ber.copy())
    # frozen genes + responsibilities from the OLD beta: first the shape part ...
    oracle.cavi_iteration(Xc.data, Xc.row, Xc.col, sc, a, c, bp, dp, freeze_genes=True, nthreads=8)
    assert_allclose(got["theta"][0][cells], sc.theta_shape, rtol=rtol, err_msg="theta shape (sampled cells)")
    # ... then the rates, which the reference computes from the new beta (scHPF_.py:711-714)
    new_beta = (got["beta"][0].astype(np.float64) / got["beta"][1].astype(np.float64)) if not simultaneous \
        else (bes.astype(np.float64) / ber.astype(np.float64))
    want_rate = (st_before.xi_shape[cells].astype(np.float64) / st_before.xi_rate[cells].astype(np.float64))[:, None] \
        + new_beta.sum(0)[None, :]
    assert_allclose(got["theta"][1][cells], want_rate, rtol=rtol, err_msg="theta rate (sampled cells)")
    want_xi = bp + (got["theta"][0][cells].astype(np.float64) / got["theta"][1][cells].astype(np.float64)).sum(1)
    assert_allclose(got["xi"][1][cells], want_xi, rtol=rtol, err_msg="xi rate (sampled cells)")
    assert got["theta"][0].dtype == dt


from conftest import bench_matrix as _bench_matrix   # shared with tests/test_trajectory_gpu.py (drawn once per session)


BENCH_SHAPES = [   # the workloads bench.py times (BASELINE.json configs[2] and the per-GPU share of configs[4])
    pytest.param(100000, 20000, 0.05, 20, np.float64, id="C3-f64"),
    pytest.param(100000, 20000, 0.05, 20, np.float32, id="C3-f32"),
    pytest.param(125000, 25000, 0.02, 50, np.float64, id="C5share-f64"),
    pytest.param(125000, 25000, 0.02, 50, np.float32, id="C5share-f32"),
    # ALL of C5 (BASELINE.json configs[4]: 1M x 25k, 2 %, K=50, nnz 4.95e8) on one GPU, in the default run
    pytest.param(1000000, 25000, 0.02, 50, np.float64, id="C5whole-f64"),
]


_C3_UNSHARDED = {}


def _c3_unsharded_run(amd, oracle, dtype):
    """Two iterations + the loss of ONE engine on the C3 matrix from the seed-0 start: the states after each
    iteration and the loss, computed once per dtype and kept for the shard counts of the test below."""
    key = np.dtype(dtype).name
    if key not in _C3_UNSHARDED:
        X = _bench_matrix(100000, 20000, 0.05)
        bp, dp, st = random_state(oracle, X, 20, dtype, seed=0)
        states = []
        with load_engine(amd, X, 20, dtype, st, 0.3, 0.3, bp, dp) as eng:
            for _ in range(2):
                eng.step()
                states.append({n: eng.get_gamma(n) for n in ("xi", "theta", "eta", "beta")})
            loss = eng.mean_negative_pois_llh()
        _C3_UNSHARDED[key] = (states, loss)
    return _C3_UNSHARDED[key]


@only_plans("tile")
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nshards", [2, 4, 8])
def test_c4_row_shards_of_c3_match_oracle_and_the_unsharded_engine(amd, oracle, plan_kind, nshards, dtype):
    """BASELINE.json configs[3] AT ITS SIZE on the one GPU a test box has: the C3 matrix (100k x 20k, 5 %, K = 20,
    nnz 9.75e7) split by the product's nnz-balanced row_partition into 2 / 4 / 8 shard engines on device 0
    (ThreadedShards: hint_sharded plans, the two-launch sharded iteration, the packing and update-from-exchange
    kernels; comm="emulated": the all-reduce is the sum of the shards' exchange buffers, because RCCL refuses
    several ranks on one device).  Two iterations, each checked (i) against the oracle's own iteration on ~500
    sampled cells and ~500 sampled genes and (ii) against the unsharded DeviceCAVI on ALL rows -- the sharded
    sum order differs, hence round-off tolerances: rtol 1e-11 (f64) / 2e-5 (f32); then the loss over all
    nonzeros against the unsharded engine and the oracle."""
    from schpf_amd.sharded import ThreadedShards
    N, G, K, a, c = 100000, 20000, 20, 0.3, 0.3
    X = _bench_matrix(N, G, 0.05)
    f32 = np.dtype(dtype) == np.float32
    tol = 2e-5 if f32 else 1e-11
    bp, dp, st = random_state(oracle, X, K, dtype, seed=0)
    ref_states, ref_loss = _c3_unsharded_run(amd, oracle, dtype)
    rng = np.random.RandomState(11 + nshards)
    cells = np.sort(rng.choice(N, 500, replace=False))
    genes = np.sort(rng.choice(G, 500, replace=False))
    with ThreadedShards(X, K, dtype, devices=[0] * nshards, comm="emulated") as shards:
        assert shards.world == nshards and int(shards.bounds[-1]) == N
        per_shard = np.diff(np.concatenate([[0], np.cumsum(np.bincount(X.row, minlength=N))])[shards.bounds])
        assert per_shard.max() - per_shard.min() <= 2 * np.bincount(X.row, minlength=N).max()   # nnz-balanced
        shards.set_hypers(a, c, bp, dp)
        for name in ("xi", "theta", "eta", "beta"):
            shards.set_gamma(name, getattr(st, name + "_shape"), getattr(st, name + "_rate"))
        for it in range(2):
            shards.steps(1)
            got = {n: shards.get_gamma(n) for n in ("xi", "theta", "eta", "beta")}
            _subproblem_check(oracle, X, st, got, a, c, bp, dp, cells, genes, rtol=tol)
            for name in ("xi", "theta", "eta", "beta"):
                assert_allclose(got[name][0], ref_states[it][name][0], rtol=tol, err_msg="%s shape vs unsharded" % name)
                assert_allclose(got[name][1], ref_states[it][name][1], rtol=tol, err_msg="%s rate vs unsharded" % name)
            for e in shards.engines[1:]:     # the replicas of beta / eta agree bitwise with shard 0's
                for name in ("eta", "beta"):
                    s_r = e.get_gamma(name)
                    assert np.array_equal(s_r[0], got[name][0]) and np.array_equal(s_r[1], got[name][1])
            st = oracle.State(got["xi"][0], got["xi"][1], got["theta"][0], got["theta"][1],
                              got["eta"][0], got["eta"][1], got["beta"][0], got["beta"][1])
        loss = shards.mean_negative_pois_llh()
    assert_allclose(loss, ref_loss, rtol=1e-5 if f32 else 1e-11)
    want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                         st.beta_shape, st.beta_rate, nthreads=16)
    assert_allclose(loss, want, rtol=1e-5 if f32 else 1e-11)


SHARD_SHAPES = [   # what a rank of bench.py --gpus 8 / 4 / 2 holds of C3 (bench.py CONFIGS c4-shard, -shard4, -shard2)
    pytest.param(12500, id="1of8"), pytest.param(25000, id="1of4"), pytest.param(50000, id="1of2"),
]


@only_plans("tile")
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("ncells", SHARD_SHAPES)
def test_shard_shapes_with_sharded_plans_match_oracle_on_sampled_rows(amd, oracle, plan_kind, ncells, dtype):
    """The row-shard shapes of C3 with the plans a rank really gets (schpf_hint_sharded: task ranges for two sweep
    launches, the half-window rule from 256 (block, window) pairs) through the library-driven sharded iteration
    (one-rank RCCL communicator: gene sweep, packing, all-reduce, cell sweep, update from the exchange buffer):
    sampled rows against the oracle, conservation over all rows, the loss over all nonzeros."""
    from schpf_amd.sharded import NativeShard
    G, K, a, c = 20000, 20, 0.3, 0.3
    X = synthetic_counts(ncells, G, 0.05, seed=42)
    f32 = np.dtype(dtype) == np.float32
    tol = 2e-5 if f32 else 1e-11
    bp, dp, st = random_state(oracle, X, K, dtype, seed=0)
    rng = np.random.RandomState(5)
    cells = np.sort(rng.choice(ncells, 400, replace=False))
    genes = np.sort(rng.choice(G, 400, replace=False))
    rows = np.asarray(X.sum(1)).ravel(); cols = np.asarray(X.sum(0)).ravel()
    with load_shard_engine(amd, X, K, dtype, st, a, c, bp, dp) as eng:
        shard = NativeShard(eng, amd.DeviceCAVI.comm_unique_id(), 0, 1)
        for it in range(2):
            shard.steps(1)
            got = {n: eng.get_gamma(n) for n in ("xi", "theta", "eta", "beta")}
            _subproblem_check(oracle, X, st, got, a, c, bp, dp, cells, genes, rtol=tol)
            ths, bes = got["theta"][0].astype(np.float64), got["beta"][0].astype(np.float64)
            assert_allclose((ths - a).sum(1), rows, rtol=tol, atol=tol)
            assert_allclose((bes - c).sum(1), cols, rtol=tol, atol=tol * 10)
            st = oracle.State(got["xi"][0], got["xi"][1], got["theta"][0], got["theta"][1],
                              got["eta"][0], got["eta"][1], got["beta"][0], got["beta"][1])
        loss = shard.mean_negative_pois_llh()
    want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                         st.beta_shape, st.beta_rate, nthreads=16)
    assert_allclose(loss, want, rtol=1e-5 if f32 else 1e-11)


@only_plans("tile")
@pytest.mark.parametrize("N,G,dens,K,dtype", BENCH_SHAPES)
def test_benchmarked_workloads_match_oracle_on_sampled_rows(amd, oracle, plan_kind, N, G, dens, K, dtype):
    """Parity AT the sizes bench.py reports: BASELINE C3 as stated (100k x 20k, 5 %, K=20) and
    the per-GPU share of C5 (125k x 25k, 2 %, K=50), f64 and f32.  Two iterations on the device;
    each is checked (i) against the oracle's own iteration on ~500 random cells and ~500 random
    genes (every updated quantity of those rows, small-case tolerances), (ii) by the
    size-independent conservation laws over ALL rows, (iii) the loss against the oracle's
    threaded compute_pois_llh over all nonzeros."""
    X = _bench_matrix(N, G, dens)
    a, c = 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, dtype, seed=0)
    f32 = np.dtype(dtype) == np.float32
    rng = np.random.RandomState(7)
    cells = np.sort(rng.choice(N, 500, replace=False))
    genes = np.sort(rng.choice(G, 500, replace=False))
    rows = np.asarray(X.sum(1)).ravel(); cols = np.asarray(X.sum(0)).ravel()
    with load_engine(amd, X, K, dtype, st, a, c, bp, dp) as eng:
        for it in range(2):
            eng.step()
            got = {n: eng.get_gamma(n) for n in ("xi", "theta", "eta", "beta")}
            _subproblem_check(oracle, X, st, got, a, c, bp, dp, cells, genes, rtol=2e-5 if f32 else 1e-11)
            ths, bes = got["theta"][0].astype(np.float64), got["beta"][0].astype(np.float64)
            tol = 2e-5 if f32 else 1e-11
            assert_allclose((ths - a).sum(1), rows, rtol=tol, atol=tol)
            assert_allclose((bes - c).sum(1), cols, rtol=tol, atol=tol * 10)
            assert_allclose((ths - a).sum(0), (bes - c).sum(0), rtol=tol * 10)
            # next iteration starts from the device's own state on both sides
            st = oracle.State(got["xi"][0], got["xi"][1], got["theta"][0], got["theta"][1],
                              got["eta"][0], got["eta"][1], got["beta"][0], got["beta"][1])
        loss = eng.mean_negative_pois_llh()
    want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                         st.beta_shape, st.beta_rate, nthreads=16)
    assert_allclose(loss, want, rtol=1e-5 if f32 else 1e-11)


@pytest.mark.parametrize("flags", [{}, {"simultaneous": True}, {"freeze_genes": True}])
def test_sharded_protocol_two_engines_on_one_gpu(amd, oracle, flags):
    """Cells split over two engines (as two ranks would hold them); the all-reduce is played by
    adding the two exchange buffers through torch views of the library's device memory -- the
    same views bench.py hands to RCCL.  Result must match the unsharded oracle."""
    import torch
    from schpf_amd.sharded import row_partition, take_rows, exchange_tensor_of
    X = synthetic_counts(600, 400, 0.08, seed=13)
    K, a, c = 12, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, np.float64, seed=4)
    xphi0 = X.data[:, None] * np.random.dirichlet(np.ones(K), X.nnz)
    bounds = row_partition(X, 2)
    engines, views = [], []
    for r in range(2):
        lo, hi = int(bounds[r]), int(bounds[r + 1])
        Xl, keep = take_rows(X, lo, hi)
        eng = amd.DeviceCAVI(hi - lo, X.shape[1], K, dtype=np.float64)
        eng.upload(Xl)
        eng.set_hypers(a, c, bp, dp)
        eng.set_gamma("xi", st.xi_shape[lo:hi], st.xi_rate[lo:hi])
        eng.set_gamma("theta", st.theta_shape[lo:hi], st.theta_rate[lo:hi])
        eng.set_gamma("eta", st.eta_shape, st.eta_rate)
        eng.set_gamma("beta", st.beta_shape, st.beta_rate)
        eng.init_phi_host(xphi0[keep])
        engines.append(eng)
        views.append(exchange_tensor_of(eng, 0))
    assert views[0].numel() == 400 * K + K and views[0].dtype == torch.float64
    for t in range(3):
        for eng in engines:
            eng.step_local(**flags)
            eng.synchronize()
        if not flags.get("freeze_genes"):
            total = views[0] + views[1]
            views[0].copy_(total); views[1].copy_(total)
            torch.cuda.synchronize()
        for eng in engines:
            eng.step_finish(**flags)
        oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp, xphi=xphi0 if t == 0 else None, **flags)
    ths = np.concatenate([e.get_gamma("theta")[0] for e in engines])
    thr = np.concatenate([e.get_gamma("theta")[1] for e in engines])
    assert_allclose(ths, st.theta_shape, rtol=1e-11)
    assert_allclose(thr, st.theta_rate, rtol=1e-11)
    for e in engines:
        bes, ber = e.get_gamma("beta")
        assert_allclose(bes, st.beta_shape, rtol=1e-11)
        assert_allclose(ber, st.beta_rate, rtol=1e-11)
        assert_allclose(e.get_gamma("eta")[1], st.eta_rate, rtol=1e-11)
    terms = [e.loss_terms() for e in engines]
    loss = -(sum(t[0] for t in terms) - sum(t[1] for t in terms)) / sum(t[2] for t in terms)
    want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                         st.beta_shape, st.beta_rate)
    assert_allclose(loss, want, rtol=1e-11)
    for e in engines:
        e.close()


PACKED_ROW_LENGTHS = (0, 1, 16, 17, 64, 65, 144)   # stored entries of a shard's gene row: 0, 1, 1, 2, 4, 5, 9 chunks of 16


def _matrix_with_gene_rows_of_pinned_lengths(shard_cells=144, ngenes=42, seed=5):
    """Two row shards of `shard_cells` cells each.  In EACH shard gene g holds PACKED_ROW_LENGTHS[(g + 3 * shard) % 7]
    stored entries, in distinct cells of the shard drawn at random.  144 entries need 144 cells in the shard; both
    shards hold the same number of entries (the same lengths, rotated; 42 = 6 x 7 genes), so the nnz-balanced
    partition cuts between them."""
    from scipy.sparse import coo_matrix
    rng = np.random.RandomState(seed)
    row, col, lengths = [], [], np.zeros((2, ngenes), np.int64)
    for shard in range(2):
        for g in range(ngenes):
            n = PACKED_ROW_LENGTHS[(g + 3 * shard) % len(PACKED_ROW_LENGTHS)]
            lengths[shard, g] = n
            row.append(shard * shard_cells + np.sort(rng.choice(shard_cells, n, replace=False)))
            col.append(np.full(n, g))
    row, col = np.concatenate(row).astype(np.int32), np.concatenate(col).astype(np.int32)
    perm = rng.permutation(len(row))
    X = coo_matrix((rng.randint(1, 6, len(row)), (row[perm], col[perm])), shape=(2 * shard_cells, ngenes))
    return X, lengths


@only_plans("gather")
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("K", [5, 20])
def test_gather_shards_pack_gene_rows_of_0_to_9_chunks(amd, oracle, plan_kind, K, dtype):
    """The packing of a sharded rank's gene-side partial rows on GATHER plans, at the row lengths its fixed-order sum
    (kernels.h sum_strided: four terms in flight, then a tail) tells apart: gene rows of 0, 1, 1, 2, 4, 5 and 9 chunks
    in each of two row shards on one GPU (ThreadedShards, comm="emulated").  plan_info says that these chunk counts
    were really built.  Two iterations: all rows against the unsharded engine at the shard tests' tolerances (rtol
    1e-11 f64 / 2e-5 f32: the sharded sum order differs) and against the oracle at the iteration tests'."""
    from schpf_amd.sharded import ThreadedShards
    X, lengths = _matrix_with_gene_rows_of_pinned_lengths()
    N, a, c = X.shape[0], 0.3, 0.3
    f32 = np.dtype(dtype) == np.float32
    tol = 2e-5 if f32 else 1e-11
    bp, dp, st = random_state(oracle, X, K, dtype, seed=K)
    names = ("xi", "theta", "eta", "beta")
    ref_states = []
    with load_engine(amd, X, K, dtype, st, a, c, bp, dp) as eng:
        for _ in range(2):
            eng.step()
            ref_states.append({n: eng.get_gamma(n) for n in names})
    with ThreadedShards(X, K, dtype, devices=[0, 0], comm="emulated") as shards:
        assert list(shards.bounds) == [0, N // 2, N]
        for r, e in enumerate(shards.engines):
            info = e.plan_info()
            assert info["chunk_len"] == 16
            assert info["n_chunks_gene"] == int(((lengths[r] + 15) // 16).sum())
            assert sorted(set((lengths[r] + 15) // 16)) == [0, 1, 2, 4, 5, 9]
        shards.set_hypers(a, c, bp, dp)
        for name in names:
            shards.set_gamma(name, getattr(st, name + "_shape"), getattr(st, name + "_rate"))
        for it in range(2):
            shards.steps(1)
            oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
            got = {n: shards.get_gamma(n) for n in names}
            for name in names:
                assert_allclose(got[name][0], ref_states[it][name][0], rtol=tol, err_msg="%s shape vs unsharded" % name)
                assert_allclose(got[name][1], ref_states[it][name][1], rtol=tol, err_msg="%s rate vs unsharded" % name)
                assert_allclose(got[name][0], getattr(st, name + "_shape"), rtol=(2e-5 * (it + 1)) if f32 else 1e-11,
                                err_msg="%s shape vs oracle" % name)
                assert_allclose(got[name][1], getattr(st, name + "_rate"), rtol=(2e-5 * (it + 1)) if f32 else 1e-11,
                                err_msg="%s rate vs oracle" % name)


@only_plans("tile", "half")
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("coo_order", ["canonical", "shuffled"])
def test_rows_gathered_on_the_device_equal_a_host_slice(amd, oracle, plan_kind, dtype, coo_order):
    """Minibatch rows without re-uploads (schpf_keep_rows / schpf_upload_rows): a batch engine whose rows
    were gathered from the source engine's resident copy iterates BITWISE like one that was handed
    X.tocsr()[rows].tocoo() by the host (the reference's own slicing, scHPF_.py:643-650) -- rows in any
    order, repeated batches, empty rows included; and the batch engine refuses to score itself."""
    from scipy.sparse import coo_matrix
    X = synthetic_counts(3000, 1500, 0.04, seed=21)
    X.data[::11] += 70000 if np.dtype(dtype) == np.float64 else 0      # f64 case: unpacked 16-byte entries
    if coo_order == "shuffled":
        perm = np.random.RandomState(1).permutation(X.nnz)
        X = coo_matrix((X.data[perm], (X.row[perm], X.col[perm])), shape=X.shape)
    K, a, c, nb = 12, 0.3, 0.3, 700
    bp, dp, st = random_state(oracle, X, K, dtype, seed=9)
    Xcsr = X.tocsr()
    Xcsr.sort_indices()
    rng = np.random.RandomState(5)
    with amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=dtype) as source, \
            amd.DeviceCAVI(nb, X.shape[1], K, dtype=dtype) as dev, amd.DeviceCAVI(nb, X.shape[1], K, dtype=dtype) as host:
        source.keep_rows()
        host.hint_transient()          # like scHPF._fit_minibatch: a batch engine plans the cheap way, by either route
        source.upload(X)
        assert source.upload_info()["rows"]
        for eng in (dev, host):
            eng.set_hypers(a, c, bp, dp)
            eng.set_gamma("eta", st.eta_shape, st.eta_rate)
            eng.set_gamma("beta", st.beta_shape, st.beta_rate)
        for it in range(3):
            rows = rng.permutation(X.shape[0])[:nb].astype(np.int32)
            dev.upload_rows(source, rows)
            host.upload(Xcsr[rows, :].tocoo())
            assert dev.nnz == host.nnz
            for eng in (dev, host):
                eng.set_gamma("xi", st.xi_shape[rows], st.xi_rate[rows])
                eng.set_gamma("theta", st.theta_shape[rows], st.theta_rate[rows])
                eng.step(cells_first=True)
                eng.step()
            for name in ("xi", "theta", "eta", "beta"):
                (s0, r0), (s1, r1) = dev.get_gamma(name), host.get_gamma(name)
                assert np.array_equal(s0, s1) and np.array_equal(r0, r1), name
        with pytest.raises(Exception, match="source"):
            dev.mean_negative_pois_llh()
        with pytest.raises(ValueError):
            dev.upload_rows(source, np.arange(nb - 1, dtype=np.int32))
        with pytest.raises(ValueError):
            dev.upload_rows(source, np.full(nb, X.shape[0], dtype=np.int32))
        with pytest.raises(Exception, match="keeps no rows"):
            dev.upload_rows(host, np.arange(nb, dtype=np.int32))


def test_minibatch_fit_reproduces_reference_trace(amd):
    """batchsize=32 (reference scHPF_.py:626-650, 688-704): cell block first, genes from the
    batch; same shuffle, same Dirichlet draws, same losses and parameters."""
    from schpf import scHPF
    g = load_golden("fit_data_k5_s3_f64_batch.npz")
    X = golden_coo(g)
    np.random.seed(int(g["seed"]))
    model = scHPF(5, max_iter=int(g["max_iter"]), verbose=False)
    model.fit(X, batchsize=32)
    assert model.bp == float(g["bp"]) and model.dp == float(g["dp"])
    assert len(model.loss) == len(g["loss"])
    assert_allclose(model.loss, g["loss"], rtol=1e-9)
    for name in ("xi", "theta", "eta", "beta"):
        assert_allclose(getattr(model, name).vi_shape, g[name + "_shape"], rtol=1e-7, err_msg=name)
        assert_allclose(getattr(model, name).vi_rate, g[name + "_rate"], rtol=1e-7, err_msg=name)


def test_run_trials_reproduces_reference_selection(amd, capsys):
    """run_trials / run_trials_pool (reference scHPF_.py:968-1332): same seeds -> same winner,
    same losses for the winner and the rejected restarts."""
    from schpf import run_trials, run_trials_pool
    g = load_golden("trials_data_k5_f64.npz")
    X = golden_coo(g)
    np.random.seed(int(g["seed"]))
    best, rest = run_trials(X, 5, ntrials=3, max_iter=30, verbose=False, return_all=True)
    assert_allclose(best.loss, g["loss"], rtol=1e-9)
    assert_allclose([m.loss[-1] for m in rest], g["rejected_final"], rtol=1e-9)
    assert_allclose(best.theta.vi_shape, g["theta_shape"], rtol=1e-6)
    assert_allclose(best.beta.vi_rate, g["beta_rate"], rtol=1e-6)
    assert best.loss[-1] <= min(m.loss[-1] for m in rest)
    np.random.seed(12)
    bests = run_trials_pool(X, [4, 6], ntrials=2, njobs=1, max_iter=20, verbose=False)
    assert [m.nfactors for m in bests] == list(g["pool_nfactors"])
    assert [len(m.loss) for m in bests] == list(g["pool_checks"])
    # reproject=True appends the projection's loss list and selects on its last value
    np.random.seed(1)
    m = run_trials(X, 4, ntrials=2, max_iter=12, verbose=False, reproject=True)
    assert isinstance(m.loss[-1], list) and m.theta.dims == (100, 4)
    # validation cells through projection_loss_function
    np.random.seed(2)
    m = run_trials(X, 4, ntrials=1, max_iter=12, verbose=False, vcells=X.tocsr()[:30].tocoo())
    assert len(m.loss) == 2 and np.isfinite(m.loss[-1])


def test_run_trials_pool_threads_per_device(amd):
    """run_trials_pool(devices=[...]): the restarts of every K are dealt to the devices, one host
    thread and one resident upload per (K, device).  Two "devices" that are both GPU 0 exercise
    the threaded path on a one-GPU box (the threads share NumPy's global RNG, so the draws
    interleave: selection properties are checked, not a golden trace)."""
    from schpf import run_trials_pool
    X = golden_coo(load_golden("trials_data_k5_f64.npz"))
    np.random.seed(5)
    best, rejected = run_trials_pool(X, [4, 6], ntrials=4, max_iter=25, verbose=False, devices=[0, 0],
                                     return_all=True)
    assert [m.nfactors for m in best] == [4, 6] and [len(r) for r in rejected] == [3, 3]
    for m, rest in zip(best, rejected):
        finals = [m.loss[-1]] + [r.loss[-1] for r in rest]
        assert np.all(np.isfinite(finals)) and finals == sorted(finals)       # winner first, rest ascending
        for trial in [m] + rest:
            assert trial.loss[-1] < trial.loss[0] and trial.theta.dims == (100, trial.nfactors)
            assert np.all(trial.beta.vi_shape > 0) and np.all(trial.theta.vi_rate > 0)


@pytest.mark.parametrize("stream_kind", ["engine-owned", "torch-default", "torch-side"])
def test_rccl_all_reduce_accepts_the_exchange_buffer(amd, oracle, stream_kind):
    """One-rank NCCL(=RCCL) process group on the GPU box: the sharded driver's all_reduce runs
    on a torch view of library-owned HBM (same HIP runtime, see schpf_amd/_lib.py) and the
    sharded step equals the plain step -- whichever stream the engine enqueues on (its own,
    torch's default stream whose handle is 0, or a torch side stream): ShardedCAVI makes that
    stream torch's current stream around the collective, which is what orders the two."""
    import os
    import socket
    import torch
    import torch.distributed as dist
    from schpf_amd.sharded import ShardedCAVI, exchange_tensor_of
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        X = synthetic_counts(700, 500, 0.06, seed=17)
        K, a, c = 20, 0.3, 0.3
        bp, dp, st = random_state(oracle, X, K, np.float64, seed=6)
        side = torch.cuda.Stream(device=0)
        stream = {"engine-owned": None, "torch-default": torch.cuda.current_stream().cuda_stream,
                  "torch-side": side.cuda_stream}[stream_kind]
        eng = amd.DeviceCAVI(700, 500, K, dtype=np.float64, device=0, stream=stream)
        assert (eng.stream_handle() == 0) == (stream_kind == "torch-default")
        if stream_kind == "torch-side":
            assert eng.stream_handle() == side.cuda_stream
        eng.upload(X)
        eng.set_hypers(a, c, bp, dp)
        for name in ("xi", "theta", "eta", "beta"):
            eng.set_gamma(name, getattr(st, name + "_shape"), getattr(st, name + "_rate"))
        drv = ShardedCAVI(eng, exchange_tensor_of(eng, 0))
        for _ in range(3):
            drv.step()
            oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
        compare_state(eng, st, rtol=1e-11)
        want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                             st.beta_shape, st.beta_rate)
        assert_allclose(drv.mean_negative_pois_llh(), want, rtol=1e-11)
        eng.close()
    finally:
        dist.destroy_process_group()


@every_plan
def test_skewed_expression_matrix_matches_oracle(amd, oracle, plan_kind):
    """Real count matrices are heavy-tailed: a few genes are seen in almost every cell, most in
    a handful, and cell depths vary several-fold.  Zipf-distributed gene popularity, log-normal
    depths, a few all-zero cells and genes, counts up to the thousands (and one above 65535, which
    forces the unpacked entry format)."""
    rng = np.random.RandomState(23)
    N, G, K = 900, 1300, 10
    pop = 1.0 / np.arange(1, G + 1) ** 1.1
    pop[rng.permutation(G)[:40]] = 0.0                       # never-seen genes
    depth = np.exp(rng.normal(5.0, 0.7, N)).astype(int)
    depth[rng.permutation(N)[:15]] = 0                       # empty cells
    rows, cols = [], []
    cdf = np.cumsum(pop) / pop.sum()
    for i in range(N):
        g = np.searchsorted(cdf, rng.random_sample(depth[i]))
        rows.append(np.full(g.shape, i, np.int32)); cols.append(g.astype(np.int32))
    row, col = np.concatenate(rows), np.minimum(np.concatenate(cols), G - 1)
    from scipy.sparse import coo_matrix
    X = coo_matrix((np.ones(row.shape[0], np.int64), (row, col)), shape=(N, G))
    X.sum_duplicates()
    for big in (False, True):
        if big:
            X.data[np.argmax(X.data)] = 70000                # > 16 bits: unpacked entries
        a, c = 0.3, 0.3
        bp, dp, st = random_state(oracle, X, K, np.float64, seed=8)
        with load_engine(amd, X, K, np.float64, st, a, c, bp, dp) as eng:
            for _ in range(3):
                eng.step()
                oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp)
            compare_state(eng, st, rtol=1e-10)
            want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                                 st.beta_shape, st.beta_rate)
            assert_allclose(eng.mean_negative_pois_llh(), want, rtol=1e-10)


@only_plans("tile", "half", "balanced")
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dual_launch_equals_two_launches_bitwise(amd, oracle, dtype, plan_kind, monkeypatch):
    """One launch for both orientations (tile_sweep_dual_kernel) runs the same tasks with the same
    fixed-order reductions as one launch per orientation: identical bits, and run-to-run
    deterministic (no atomics anywhere)."""
    X = synthetic_counts(3000, 2500, 0.04, seed=5)
    K = 20
    bp, dp, st = random_state(oracle, X, K, dtype, seed=2)
    results = []
    for dual in ("1", "0", "1"):
        monkeypatch.setenv("SCHPF_DUAL", dual)
        with load_engine(amd, X, K, dtype, st, 0.3, 0.3, bp, dp) as eng:
            for _ in range(3):
                eng.step()
            results.append([eng.get_gamma(n) for n in ("xi", "theta", "eta", "beta")])
    for other in results[1:]:
        for (s0, r0), (s1, r1) in zip(results[0], other):
            assert np.array_equal(s0, s1) and np.array_equal(r0, r1)


@only_plans("tile", "half", "balanced")
@pytest.mark.parametrize("dtype,K", [(np.float64, 20), (np.float32, 20), (np.float64, 50)])
def test_loss_is_the_same_on_either_plan(amd, oracle, plan_kind, monkeypatch, dtype, K):
    """The loss pass sweeps ONE tile plan -- the cell-side one, or the gene-side one when the cell side has too few
    tasks to fill the device (policy.cpp loss_side): both hold every nonzero and r = sum_k E[theta] E[beta] is
    symmetric, so the two must agree to summation order, with the oracle's loss (hpf_numba.py:24-51) and explicitly
    stored zeros (counted by the reference's loss) included."""
    from scipy.sparse import coo_matrix
    X = synthetic_counts(1500, 900, 0.06, seed=23)
    data = X.data.copy()
    data[::11] = 0          # explicit zeros
    X = coo_matrix((data, (X.row, X.col)), shape=X.shape)
    bp, dp, st = random_state(oracle, X, K, dtype, seed=9)
    got = []
    for side in ("0", "1"):
        monkeypatch.setenv("SCHPF_LOSS_SIDE", side)
        with load_engine(amd, X, K, dtype, st, 0.3, 0.3, bp, dp) as eng:
            eng.step()
            got.append(eng.mean_negative_pois_llh())
            state = [eng.get_gamma(n) for n in ("theta", "beta")]
    want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, state[0][0], state[0][1], state[1][0], state[1][1])
    f32 = np.dtype(dtype) == np.float32
    assert_allclose(got[0], got[1], rtol=1e-6 if f32 else 1e-12)
    assert_allclose(got[0], want, rtol=1e-5 if f32 else 1e-10)


@only_plans("tile", "half", "balanced")
@pytest.mark.parametrize("dtype,K", [(np.float64, 20), (np.float32, 20), (np.float64, 50)])
@pytest.mark.parametrize("side", ["0", "1"])
def test_loss_pass_on_finer_tasks_matches_oracle(amd, oracle, plan_kind, monkeypatch, dtype, K, side):
    """The loss pass keeps no partial rows, so the library cuts the iteration's tasks into sub-ranges of their windows
    for it (capi.hip loss_tasks; round 5: C3's cell side has ONE task per block, 196 for 256 compute units).  With the
    iteration's tasks long (one range per block) every task is cut; the loss must agree with the uncut pass
    (SCHPF_LOSS_SPLIT=0) to summation order and with the oracle (hpf_numba.py:24-51) -- on either plan, with the
    half-window schedule (whose entries may point one sub-window beyond a sub-task), balanced windows and K = 50's
    one-nonzero-at-a-time loop, stored zeros included; the iteration itself must not notice."""
    from scipy.sparse import coo_matrix
    X = synthetic_counts(6000, 5000, 0.02, seed=29)
    data = X.data.copy()
    data[::13] = 0          # explicit zeros
    X = coo_matrix((data, (X.row, X.col)), shape=X.shape)
    bp, dp, st = random_state(oracle, X, K, dtype, seed=6)
    monkeypatch.setenv("SCHPF_LOSS_SIDE", side)
    monkeypatch.setenv("SCHPF_TASKS", "1")          # one window range per block: tasks as long as they get
    monkeypatch.setenv("SCHPF_WPB", "16")
    got, states = [], []
    for split in ("1", "0"):
        monkeypatch.setenv("SCHPF_LOSS_SPLIT", split)
        with load_engine(amd, X, K, dtype, st, 0.3, 0.3, bp, dp) as eng:
            eng.step()
            first = eng.mean_negative_pois_llh()
            eng.step()                               # the sweep after a loss pass sees the iteration's own tasks again
            got.append((first, eng.mean_negative_pois_llh()))
            states.append([eng.get_gamma(n) for n in ("theta", "beta")])
    for (s0, r0), (s1, r1) in zip(states[0], states[1]):
        assert np.array_equal(s0, s1) and np.array_equal(r0, r1)
    th, be = states[0]
    want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, th[0], th[1], be[0], be[1])
    f32 = np.dtype(dtype) == np.float32
    assert_allclose(got[0], got[1], rtol=1e-6 if f32 else 1e-12)
    assert_allclose(got[0][1], want, rtol=1e-5 if f32 else 1e-10)


@only_plans("tile", "half", "balanced")
@pytest.mark.parametrize("coo_order", ["canonical", "shuffled", "col-major"])
@pytest.mark.parametrize("dtype,K,big", [(np.float64, 20, False), (np.float32, 12, False), (np.float64, 5, True),
                                         (np.float64, 50, False)])
@pytest.mark.parametrize("bank_order", [2, 1])
def test_device_plan_equals_host_plan(amd, oracle, plan_kind, monkeypatch, coo_order, dtype, K, big, bank_order):
    """The plan built by device passes (plan_device.hip: radix sort, step counts, bank-ordered
    fill) is the host builder's plan bit for bit: same entry order => same summation order => the
    engines agree in every bit after three iterations, from a host-drawn t=0 included (that path
    uses the plan's sort permutation).  bank_order 2 = the joint assignment over the lane groups of an
    LDS pass (wave-parallel fill_joint_kernel against the sequential plan.cpp::bank_order_joint; one, two
    and four lanes per row), 1 = the per-row rule (also what segments of > 128 nonzeros fall back to:
    the col-major case has them)."""
    monkeypatch.setenv("SCHPF_BANK_ORDER", str(bank_order))
    from scipy.sparse import coo_matrix
    # col-major input also gets long segments (40 % filled: > 192 nonzeros per row and window)
    X = synthetic_counts(600, 2600, 0.4, seed=11) if coo_order == "col-major" else synthetic_counts(2500, 1800, 0.05, seed=11)
    data = X.data.copy()
    if big:
        data[::7] += 70000          # counts beyond 16 bits: unpacked 16-byte entries
    perm = {"canonical": np.arange(X.nnz), "shuffled": np.random.RandomState(3).permutation(X.nnz),
            "col-major": np.lexsort((X.row, X.col))}[coo_order]
    Xp = coo_matrix((data[perm], (X.row[perm], X.col[perm])), shape=X.shape)
    bp, dp, st = random_state(oracle, Xp, K, dtype, seed=4)
    phi = np.random.RandomState(5).dirichlet(np.ones(K), Xp.nnz)
    results = []
    for device_plan in ("1", "0"):
        monkeypatch.setenv("SCHPF_DEVICE_PLAN", device_plan)
        with load_engine(amd, Xp, K, dtype, st, 0.3, 0.3, bp, dp) as eng:
            eng.init_phi_host(Xp.data[:, None] * phi)
            for _ in range(3):
                eng.step()
            results.append([eng.get_gamma(n) for n in ("xi", "theta", "eta", "beta")] + [eng.plan_info()])
    assert results[0][4] == results[1][4]
    for (s0, r0), (s1, r1) in zip(results[0][:4], results[1][:4]):
        assert np.array_equal(s0, s1) and np.array_equal(r0, r1)


@every_plan
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("flags", [{}, {"simultaneous": True}, {"freeze_genes": True}])
def test_steps_call_equals_single_steps_bitwise(amd, oracle, dtype, flags, plan_kind):
    """schpf_steps(n) -- the stretch between two loss checks as one call, replayed as a hipGraph
    from the second call on -- gives the bits of n schpf_step calls: eager first call, graph
    capture, graph replay, an odd count (graph + one eager iteration), and after new
    hyperparameters (which are baked into the captured launches and must invalidate them)."""
    X = synthetic_counts(900, 700, 0.06, seed=31)
    K, a, c = 20, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, dtype, seed=3)
    with load_engine(amd, X, K, dtype, st, a, c, bp, dp) as one, load_engine(amd, X, K, dtype, st, a, c, bp, dp) as many:
        def same():
            for n in ("xi", "theta", "eta", "beta"):
                (s0, r0), (s1, r1) = one.get_gamma(n), many.get_gamma(n)
                assert np.array_equal(s0, s1) and np.array_equal(r0, r1), n
        # (.., 5, 5, 4, 4, 5, 4): odd counts leave the sum-of-beta buffers swapped on the host, so the
        # graph of 4 is captured at one parity and must not be replayed at the other (round-2 advisor
        # finding: with simultaneous=True the replay read the sums of one iteration earlier)
        for count in (1, 4, 4, 4, 5, 2, 5, 5, 4, 4, 5, 4):
            for _ in range(count):
                one.step(**flags)
            many.steps(count, **flags)
            same()
        one.set_hypers(a, c, bp * 1.5, dp * 0.5)
        many.set_hypers(a, c, bp * 1.5, dp * 0.5)
        for _ in range(4):
            one.step(**flags)
        many.steps(4, **flags)
        same()
        assert one.mean_negative_pois_llh() == many.mean_negative_pois_llh()


def test_validation_cells_reproduce_reference_trace(amd):
    """run_trials(vcells=...) (reference scHPF_.py:1097-1106, loss.py:37-102): held-out cells are
    projected onto the model at every check, warm-started, and THEIR loss drives the stop rule.
    Here the held-out cells stay resident in one engine between checks; the trace is the
    reference's."""
    from schpf import run_trials
    g = load_golden("trials_validation_k5_f64.npz")
    full = golden_coo(load_golden("pbmc_like_data.npz")).tocsr()
    n_train = int(g["n_train"])
    Xt, Xv = full[:n_train].tocoo(), full[n_train:].tocoo()
    assert np.array_equal(Xt.data, g["x"]) and np.array_equal(Xt.col, g["col"])
    np.random.seed(int(g["seed"]))
    model = run_trials(Xt, 5, ntrials=1, max_iter=40, verbose=False, vcells=Xv)
    assert len(model.loss) == len(g["loss"])
    assert_allclose(model.loss, g["loss"], rtol=1e-9)
    assert_allclose(model.theta.vi_shape, g["theta_shape"], rtol=1e-6)
    assert_allclose(model.beta.vi_rate, g["beta_rate"], rtol=1e-6)


@pytest.mark.parametrize("fname,dtype,kw", [FITS[0], FITS[3], FITS[5]])
def test_fit_over_devices_reproduces_reference_trace(amd, monkeypatch, fname, dtype, kw):
    """scHPF.fit(X, devices=[...]): cells row-sharded over the listed GPUs, one all-reduce of the
    gene-side sums per iteration (schpf_amd.sharded.ThreadedShards).  The one-GPU test box cannot
    host two RCCL ranks, so both shards sit on device 0 and the all-reduce is played through torch
    views of the exchange buffers (SCHPF_SHARD_COMM=emulated); partitioning, packing, update
    kernels and the estimator plumbing are the product's.  Same stop iteration and losses as the
    reference's single-process run; parameters to the sharded summation order."""
    from schpf import scHPF
    monkeypatch.setenv("SCHPF_SHARD_COMM", "emulated")
    g = load_golden(fname)
    X = golden_coo(g)
    np.random.seed(int(g["seed"]))
    model = scHPF(int(g["nfactors"]), dtype=dtype, max_iter=int(g["max_iter"]), verbose=False)
    model.fit(X, devices=[0, 0], **kw)
    f32 = np.dtype(dtype) == np.float32
    assert model.bp == float(g["bp"]) and model.dp == float(g["dp"])
    assert len(model.loss) == len(g["loss"])
    assert_allclose(model.loss, g["loss"], rtol=1e-4 if f32 else 1e-9)
    for name in ("xi", "theta", "eta", "beta"):
        got = getattr(model, name)
        assert got.vi_shape.shape == g[name + "_shape"].shape
        assert_allclose(got.vi_shape, g[name + "_shape"], rtol=2e-2 if f32 else 1e-6, err_msg=name)
        assert_allclose(got.vi_rate, g[name + "_rate"], rtol=2e-2 if f32 else 1e-6, err_msg=name)


def load_shard_engine(amd, X, K, dtype, st, a, c, bp, dp):
    """load_engine for a rank of a sharded fit: hint_sharded() before the upload, as ThreadedShards and
    bench.py do -- the task ranges are then chosen for two sweep launches per iteration."""
    eng = amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=dtype)
    eng.hint_sharded()
    eng.upload(X)
    eng.set_hypers(a, c, bp, dp)
    eng.set_gamma("xi", st.xi_shape, st.xi_rate)
    eng.set_gamma("theta", st.theta_shape, st.theta_rate)
    eng.set_gamma("eta", st.eta_shape, st.eta_rate)
    eng.set_gamma("beta", st.beta_shape, st.beta_rate)
    return eng


@pytest.mark.parametrize("hinted", [False, True])
def test_library_rccl_one_rank_equals_plain_steps(amd, oracle, hinted):
    """The collective inside the library (schpf_comm_init / schpf_steps_sharded / schpf_loss_terms_all,
    RCCL bound at run time to the copy already in the process): a one-rank communicator on the GPU
    box.  The sharded iteration -- two sweep launches, packing, all-reduce on the communicator's
    stream ordered by events, update from the exchange buffer -- must equal the oracle, with the plans
    of a plain engine and with those of a hinted rank."""
    from schpf_amd.sharded import NativeShard
    X = synthetic_counts(700, 500, 0.06, seed=17)
    K, a, c = 20, 0.3, 0.3
    bp, dp, st = random_state(oracle, X, K, np.float64, seed=6)
    with (load_shard_engine if hinted else load_engine)(amd, X, K, np.float64, st, a, c, bp, dp) as eng:
        shard = NativeShard(eng, amd.DeviceCAVI.comm_unique_id(), 0, 1)
        shard.steps(2)
        shard.step(simultaneous=True)
        shard.step(freeze_genes=True)
        for flags in ({}, {}, {"simultaneous": True}, {"freeze_genes": True}):
            oracle.cavi_iteration(X.data, X.row, X.col, st, a, c, bp, dp, **flags)
        compare_state(eng, st, rtol=1e-11)
        want = oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                             st.beta_shape, st.beta_rate)
        assert_allclose(shard.mean_negative_pois_llh(), want, rtol=1e-11)


@only_plans("tile")
def test_a_new_communicator_drops_the_captured_stretch(amd, oracle, plan_kind):
    """A captured sharded stretch holds an all-reduce bound to the communicator it was captured with: joining a new
    communicator (or leaving one) on a live engine must drop the cached graphs, and the same (flags, n) stretch
    is then captured again with the new one (round-4 advisor finding: replay against a freed communicator)."""
    from schpf_amd.sharded import NativeShard
    X = synthetic_counts(3000, 1500, 0.04, seed=3)
    K, a, c = 12, 0.3, 0.3
    bp, dp, ref = random_state(oracle, X, K, np.float64, seed=2)
    with load_shard_engine(amd, X, K, np.float64, ref, a, c, bp, dp) as eng:
        done = 0
        for _ in range(3):
            shard = NativeShard(eng, amd.DeviceCAVI.comm_unique_id(), 0, 1)   # comm_init on the live engine
            shard.steps(1)
            shard.steps(4)      # captured (one-rank communicator: the graph is the default)
            shard.steps(4)      # replayed
            done += 9
            for _ in range(9):
                oracle.cavi_iteration(X.data, X.row, X.col, ref, a, c, bp, dp)
            compare_state(eng, ref, rtol=1e-10)
        amd._lib.check(eng._lib.schpf_comm_destroy(eng._h))
        with pytest.raises(amd._lib.SchpfHipError):
            eng.steps_sharded(4)                                              # no communicator, no stale graph


@only_plans("tile", "half", "balanced")
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("graph", ["0", "1"])
def test_sharded_stretches_with_mode_switches_match_oracle(amd, oracle, plan_kind, dtype, graph, monkeypatch):
    """The library-driven sharded iteration (schpf_steps_sharded, one-rank communicator) at a size with
    several rounds of tasks per compute unit, eager and with the stretch captured as a hipGraph (both
    streams, the events between them and the RCCL call), through mode switches: simultaneous, frozen
    genes, plain single-GPU steps in between, odd and even stretch lengths (the per-parity graph cache)."""
    from schpf_amd.sharded import NativeShard
    monkeypatch.setenv("SCHPF_GRAPH_SHARDED", graph)
    X = synthetic_counts(20000, 8000, 0.015, seed=12)
    K, a, c = 20, 0.3, 0.3
    f32 = np.dtype(dtype) == np.float32
    bp, dp, ref = random_state(oracle, X, K, dtype, seed=4)
    seq = [(1, {}), (4, {}), (4, {}), (5, {}), (4, {}), (1, {"simultaneous": True}), (2, {"freeze_genes": True}), (3, {})]
    with load_shard_engine(amd, X, K, dtype, ref, a, c, bp, dp) as eng:
        shard = NativeShard(eng, amd.DeviceCAVI.comm_unique_id(), 0, 1)
        done = 0
        for n, flags in seq:
            shard.steps(n, **flags)
            for _ in range(n):
                oracle.cavi_iteration(X.data, X.row, X.col, ref, a, c, bp, dp, **flags)
            done += n
            compare_state(eng, ref, rtol=(2e-5 * done) if f32 else 1e-10)
        eng.step()
        oracle.cavi_iteration(X.data, X.row, X.col, ref, a, c, bp, dp)
        shard.steps(2)
        for _ in range(2):
            oracle.cavi_iteration(X.data, X.row, X.col, ref, a, c, bp, dp)
        compare_state(eng, ref, rtol=(2e-5 * (done + 3)) if f32 else 1e-10)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_column_sums_and_mode_switches_match_oracle(amd, oracle, dtype, monkeypatch):
    """Small problems skip the two column-sum reduce launches of an iteration: the update kernels
    sum the other side's per-block partials themselves (default ordering only).  Switching between
    the default ordering and the orderings that read the reduced sums (simultaneous, freeze_genes)
    must bring those sums up to date; with the fusion off the results agree to round-off."""
    X = synthetic_counts(700, 450, 0.07, seed=41)
    K, a, c = 9, 0.3, 0.3
    f32 = np.dtype(dtype) == np.float32
    bp, dp, st = random_state(oracle, X, K, dtype, seed=8)
    seq = [{}, {}, {"simultaneous": True}, {}, {"freeze_genes": True}, {}, {"simultaneous": True}]
    states = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("SCHPF_FUSE_SUMS", fuse)
        ref = st.copy()
        with load_engine(amd, X, K, dtype, ref, a, c, bp, dp) as eng:
            for it, flags in enumerate(seq):
                eng.step(**flags)
                oracle.cavi_iteration(X.data, X.row, X.col, ref, a, c, bp, dp, **flags)
                compare_state(eng, ref, rtol=(2e-5 * (it + 1)) if f32 else 1e-11)
            states[fuse] = [eng.get_gamma(n) for n in ("xi", "theta", "eta", "beta")]
    for (s1, r1), (s0, r0) in zip(states["1"], states["0"]):
        assert_allclose(s1, s0, rtol=1e-5 if f32 else 1e-13)
        assert_allclose(r1, r0, rtol=1e-5 if f32 else 1e-13)
