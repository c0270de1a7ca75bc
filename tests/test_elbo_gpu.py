"""The ELBO on the GPU: every term against the float64 host yardstick (tests/_elbo_reference.py), on
every sweep plan and on either side of the loss pass; monotone over whole fits; no effect on the fit; sharded sums.

Tolerances: each term within rtol * sum|terms|, rtol 1e-11 (f64) / 1e-5 (f32).  Monotonicity (f64): every step of
the ELBO >= -1e-11 * sum|terms| (a failure is a finding about an update or a schedule, not a tolerance to widen)."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix

from conftest import load_golden, golden_coo, synthetic_counts
import _elbo_reference as ref

pytestmark = pytest.mark.gpu

TERMS = ("data", "logfac", "rate", "cell", "gene")
RTOL = {np.dtype(np.float64): 1e-11, np.dtype(np.float32): 1e-5}


@pytest.fixture(autouse=True, params=["tile-0", "tile-1", "half-0", "half-1", "balanced-0", "balanced-1", "gather"])
def plan_kind(request, monkeypatch):
    """The plan kinds of tests/test_engine_gpu.py (tile, the half-window schedule, balanced windows, the L2-gather
    plan) times the side of the matrix the ELBO pass sweeps (SCHPF_LOSS_SIDE, tile plans; the gather plan has one)."""
    kind, _, side = request.param.partition("-")
    monkeypatch.setenv("SCHPF_PLAN", "gather" if kind == "gather" else "tile")
    for v in ("SCHPF_HALF", "SCHPF_BALANCE", "SCHPF_WPB", "SCHPF_LOSS_SIDE"):
        monkeypatch.delenv(v, raising=False)
    if kind == "half":
        monkeypatch.setenv("SCHPF_HALF", "2")
    if kind == "balanced":
        monkeypatch.setenv("SCHPF_BALANCE", "1")
        monkeypatch.setenv("SCHPF_WPB", "16")     # the balanced kernels are the 1024-thread ones
    if side:
        monkeypatch.setenv("SCHPF_LOSS_SIDE", side)
    return request.param


def only_plans(*kinds):
    return pytest.mark.parametrize("plan_kind", list(kinds), indirect=True)


plans_default_side = only_plans("tile-0", "half-1", "balanced-0", "gather")


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


HYP = dict(a=0.3, ap=1.0, bp=1.3, c=0.3, cp=1.0, dp=0.8)


def random_state(N, G, K, dtype, seed):
    rng = np.random.RandomState(seed)
    g = lambda *d: (rng.uniform(0.2, 3.0, d).astype(dtype), rng.uniform(0.5, 2.0, d).astype(dtype))  # noqa: E731
    return {"xi": g(N), "theta": g(N, K), "eta": g(G), "beta": g(G, K)}


def engine_with(amd, X, K, dtype, st, hyp=HYP):
    eng = amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=dtype)
    eng.upload(X)
    eng.set_hypers(hyp["a"], hyp["c"], hyp["bp"], hyp["dp"])
    for name in ("xi", "theta", "eta", "beta"):
        eng.set_gamma(name, *st[name])
    return eng


def reference(X, st, hyp=HYP):
    return ref.elbo_terms(X, hyp["a"], hyp["ap"], hyp["bp"], hyp["c"], hyp["cp"], hyp["dp"],
                          st["xi"], st["theta"], st["eta"], st["beta"])


def assert_terms_close(got, want, rtol):
    tol = rtol * ref.scale(want)
    for k in TERMS + ("elbo",):
        assert abs(got[k] - want[k]) <= tol, "%s: device %.17g, reference %.17g (tol %.3g)" % (k, got[k], want[k], tol)


def with_zeros_and_duplicates(X, seed):
    """X plus explicitly stored zeros and repeated (cell, gene) entries, kept as given (no sum_duplicates)."""
    rng = np.random.RandomState(seed)
    n = max(4, X.nnz // 20)
    pick = rng.randint(0, X.nnz, n)
    zr, zc = rng.randint(0, X.shape[0], n), rng.randint(0, X.shape[1], n)
    row = np.concatenate([X.row, X.row[pick], zr]).astype(np.int32)
    col = np.concatenate([X.col, X.col[pick], zc]).astype(np.int32)
    val = np.concatenate([X.data, rng.randint(1, 5, n), np.zeros(n, X.data.dtype)])
    return coo_matrix((val, (row, col)), shape=X.shape)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", [5, 10, 20, 50])
def test_terms_match_the_host_reference(amd, K, dtype, plan_kind):
    X = with_zeros_and_duplicates(synthetic_counts(230, 310, 0.06, seed=K), K)
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=K + 1)
    with engine_with(amd, X, K, dtype, st) as eng:
        got = eng.elbo_terms(HYP["ap"], HYP["cp"])
        again = eng.elbo_terms(HYP["ap"], HYP["cp"])
    assert got == again                                   # bitwise: fixed-order sums, no atomics
    assert_terms_close(got, reference(X, st), RTOL[np.dtype(dtype)])


def test_terms_of_the_reference_fitted_golden_state(amd, plan_kind):
    g = load_golden("fit_data_k5_s0_f64.npz")
    X = golden_coo(g)
    K = int(g["nfactors"])
    hyp = dict(HYP, bp=float(g["bp"]), dp=float(g["dp"]))
    st = {n: (g[n + "_shape"], g[n + "_rate"]) for n in ("xi", "theta", "eta", "beta")}
    with engine_with(amd, X, K, np.float64, st, hyp) as eng:
        got = eng.elbo_terms(hyp["ap"], hyp["cp"])
    assert_terms_close(got, reference(X, st, hyp), 1e-11)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K, shape", [(5, (120, 90, 0.08)), (50, (1500, 1200, 0.03))])
def test_underflowed_normalisers_take_the_log_domain_path(amd, K, shape, dtype, plan_kind):
    """Cells 0-3 are tiny on every factor but 0 and four genes spread over the table on factor 0 only: for their 16
    nonzeros every product of the exp-shifted rows underflows (psi(alpha) ~ -1/alpha: E[log] ~ -800 at alpha = 1.25e-3
    in f64, ~ -100 at 1e-2 in f32), so s = 0 and only the log-domain cold path gives the finite value logsumexp does.
    K = 50 reaches the wide-row loops (f64: the rolling one) and, on the larger matrix, tasks over several windows."""
    N, G, dens = shape
    tiny_shape = 1.25e-3 if dtype == np.float64 else 1e-2
    cells, genes = np.arange(4), np.array([0, G // 3, 2 * G // 3, G - 1])
    X = synthetic_counts(N, G, dens, seed=3)
    ci, gi = [a.ravel() for a in np.meshgrid(cells, genes)]
    X = coo_matrix((np.concatenate([X.data, np.arange(1, 17)]), (np.concatenate([X.row, ci]), np.concatenate([X.col, gi]))),
                   shape=X.shape)
    st = random_state(N, G, K, dtype, seed=4)
    st["theta"][0][cells, 1:] = tiny_shape
    st["beta"][0][genes, 0] = tiny_shape
    want = reference(X, st)
    assert np.isfinite(want["data"])
    with engine_with(amd, X, K, dtype, st) as eng:
        got = eng.elbo_terms(HYP["ap"], HYP["cp"])
        print("ELBO-UNDERFLOW K=%d plan=%s %s" % (K, plan_kind, eng.sweep_bytes()))
    assert_terms_close(got, want, RTOL[np.dtype(dtype)])


def _worst_step(elbos, scale):
    d = np.diff(np.asarray(elbos))
    return float(d.min() / scale) if d.size else 0.0


@plans_default_side
@pytest.mark.parametrize("K", [10, 20, 50])
@pytest.mark.parametrize("matrix", ["synthetic", "planted"])
def test_elbo_never_decreases_over_a_fit(amd, K, matrix, plan_kind):
    if matrix == "synthetic":
        X = synthetic_counts(300, 400, 0.05, seed=K)
    else:
        from benchlib.data import planted_block
        X = planted_block(300, 400, K, 6000, seed=K)
        X = X if hasattr(X, "row") else X.tocoo()
    np.random.seed(K)
    model = amd.scHPF(K, min_iter=200, max_iter=200, check_freq=1, verbose=False)
    model.fit(X, record_elbo=True)
    assert len(model.elbo_) == len(model.loss) == 200
    scale = ref.scale(model.elbo(X, terms=True))
    worst = _worst_step(model.elbo_, scale)
    print("ELBO-WORST fit %s K=%d plan=%s: %.3e" % (matrix, K, plan_kind, worst))
    assert worst >= -1e-11, worst


@plans_default_side
def test_elbo_never_decreases_over_cells_first_steps(amd, plan_kind):
    K = 20
    X = synthetic_counts(300, 400, 0.05, seed=7)
    st = random_state(X.shape[0], X.shape[1], K, np.float64, seed=8)
    st["xi"][0][:] = HYP["ap"] + K * HYP["a"]           # the capacities' shapes are constants of the model
    st["eta"][0][:] = HYP["cp"] + K * HYP["c"]
    with engine_with(amd, X, K, np.float64, st) as eng:
        np.random.seed(0)
        eng.init_phi_host(X.data[:, None] * np.random.dirichlet(np.ones(K), X.nnz))
        eng.step(cells_first=True)
        elbos, scale = [], None
        for _ in range(100):
            eng.step(cells_first=True)
            t = eng.elbo_terms(HYP["ap"], HYP["cp"])
            elbos.append(t["elbo"])
            scale = ref.scale(t)
    worst = _worst_step(elbos, scale)
    print("ELBO-WORST cells_first K=%d plan=%s: %.3e" % (K, plan_kind, worst))
    assert worst >= -1e-11, worst


@plans_default_side
def test_float32_fit_ends_above_where_it_started(amd, plan_kind):
    X = synthetic_counts(300, 400, 0.05, seed=11)
    np.random.seed(11)
    model = amd.scHPF(10, min_iter=60, max_iter=60, check_freq=5, dtype=np.float32, verbose=False)
    model.fit(X, record_elbo=True)
    assert len(model.elbo_) == len(model.loss)
    assert model.elbo_[-1] > model.elbo_[0]


@only_plans("tile-0", "gather")
def test_recording_the_elbo_changes_nothing_in_the_fit(amd, plan_kind):
    X = synthetic_counts(300, 400, 0.05, seed=5)
    fits = []
    for record in (False, True):
        np.random.seed(5)
        m = amd.scHPF(10, min_iter=30, max_iter=30, check_freq=3, verbose=False)
        m.fit(X, record_elbo=record)
        fits.append(m)
    plain, recorded = fits
    assert not hasattr(plain, "elbo_") and len(recorded.elbo_) == len(recorded.loss)
    assert plain.loss == recorded.loss
    for name in ("xi", "theta", "eta", "beta"):
        assert getattr(plain, name) == getattr(recorded, name), name       # HPF_Gamma.__eq__: bitwise arrays
    assert plain.get_params() == recorded.get_params()
    # a later fit that records nothing leaves no trace of the earlier one
    np.random.seed(5)
    recorded.fit(X, record_elbo=False, max_iter=6, min_iter=6)
    assert not hasattr(recorded, "elbo_")


@only_plans("tile-0", "half-1", "gather")
def test_steps_after_an_elbo_evaluation_are_unchanged(amd, plan_kind):
    """Eager steps and graph replays (the second schpf_steps call with the same count) after an ELBO evaluation equal
    the same steps without one, bitwise."""
    K = 10
    X = synthetic_counts(300, 400, 0.05, seed=9)
    st = random_state(X.shape[0], X.shape[1], K, np.float64, seed=9)
    out = []
    for evaluate in (False, True):
        with engine_with(amd, X, K, np.float64, st) as eng:
            for _ in range(3):
                eng.step()
                eng.steps(4)
                if evaluate:
                    eng.elbo(HYP["ap"], HYP["cp"])
            out.append([eng.get_gamma(n) for n in ("xi", "theta", "eta", "beta")])
    for (s0, r0), (s1, r1) in zip(*out):
        assert np.array_equal(s0, s1) and np.array_equal(r0, r1)


@only_plans("tile-0", "gather")
@pytest.mark.parametrize("n", [2, 4])
def test_sharded_terms_equal_the_unsharded_engine(amd, n, plan_kind):
    from schpf_amd.sharded import ThreadedShards
    K = 10
    X = synthetic_counts(400, 300, 0.05, seed=n)
    st = random_state(X.shape[0], X.shape[1], K, np.float64, seed=n)
    with engine_with(amd, X, K, np.float64, st) as eng:
        whole = eng.elbo_terms(HYP["ap"], HYP["cp"])
    shards = ThreadedShards(X, K, np.float64, devices=[0] * n, comm="emulated")
    try:
        shards.set_hypers(HYP["a"], HYP["c"], HYP["bp"], HYP["dp"])
        for name in ("xi", "theta", "eta", "beta"):
            shards.set_gamma(name, *st[name])
        parts = shards.elbo_terms(HYP["ap"], HYP["cp"])
    finally:
        shards.close()
    for k in TERMS:
        assert abs(parts[k] - whole[k]) <= 1e-12 * abs(whole[k]), (k, parts[k], whole[k])
    assert abs(parts["elbo"] - whole["elbo"]) <= 1e-12 * ref.scale(whole)


@only_plans("tile-0")
def test_batch_engines_and_minibatch_fits_refuse(amd, plan_kind):
    from schpf_amd import _lib
    K = 5
    X = synthetic_counts(200, 150, 0.05, seed=1)
    src = amd.DeviceCAVI(X.shape[0], X.shape[1], K)
    try:
        src.keep_rows()
        src.upload(X)
        with amd.DeviceCAVI(50, X.shape[1], K) as batch:
            batch.upload_rows(src, np.arange(50))
            batch.set_hypers(HYP["a"], HYP["c"], HYP["bp"], HYP["dp"])
            with pytest.raises(_lib.SchpfHipError):
                batch.elbo_terms(HYP["ap"], HYP["cp"])
    finally:
        src.close()
    with pytest.raises(ValueError):
        amd.scHPF(K, max_iter=3, verbose=False).fit(X, batchsize=50, record_elbo=True)
