"""The per-cell and per-gene Poisson loss on the GPU against the float64 host yardstick
(tests/_loss_rows_reference.py), on every sweep plan; its sums against the scalar loss; read-only; bit-reproducible.

Tolerances.  Counts: exact.  gammaln_sum: rtol 1e-12 (float64 arithmetic on float32-exact counts on both sides).
llh_sum of a row: |got - want| <= tol * sum_row(|x log r| + r) with the engine tests' loss tolerance, tol = 1e-11
(float64) / 1e-5 (float32) -- relative to the row's absolute scale, so that cancellation in a short row neither hides
nor fakes an error.  Rows without stored entries (fewer than 5 % of an axis in every case, asserted) are compared by
the position of their NaN alone."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.sparse import coo_matrix

from conftest import load_golden, golden_coo, synthetic_counts
import _loss_rows_reference as ref

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float64): 1e-11, np.dtype(np.float32): 1e-5}
PLANS = ["gather", "tile", "half", "balanced", "hostplan"]
WORST = {}   # dtype name -> largest scaled llh error seen in this session (printed by the last test)


@pytest.fixture(autouse=True, params=PLANS)
def plan_kind(request, monkeypatch):
    """The plan kinds of tests/test_engine_gpu.py -- the L2-gather plan, the tile plan with the window schedule, with
    SCHPF_HALF slots, with balanced windows -- and the tile plan built on the host (SCHPF_DEVICE_PLAN=0)."""
    kind = request.param
    monkeypatch.setenv("SCHPF_PLAN", "gather" if kind == "gather" else "tile")
    for v in ("SCHPF_HALF", "SCHPF_BALANCE", "SCHPF_WPB", "SCHPF_LOSS_SIDE", "SCHPF_DEVICE_PLAN", "SCHPF_TASKS"):
        monkeypatch.delenv(v, raising=False)
    if kind == "half":
        monkeypatch.setenv("SCHPF_HALF", "2")
    if kind == "balanced":
        monkeypatch.setenv("SCHPF_BALANCE", "1")
        monkeypatch.setenv("SCHPF_WPB", "16")     # the balanced kernels are the 1024-thread ones
    if kind == "hostplan":
        monkeypatch.setenv("SCHPF_DEVICE_PLAN", "0")
    return kind


def only_plans(*kinds):
    return pytest.mark.parametrize("plan_kind", list(kinds), indirect=True)


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def random_state(N, G, K, dtype, seed):
    rng = np.random.RandomState(seed)
    g = lambda *d: (rng.uniform(0.2, 3.0, d).astype(dtype), rng.uniform(0.5, 2.0, d).astype(dtype))  # noqa: E731
    return {"xi": g(N), "theta": g(N, K), "eta": g(G), "beta": g(G, K)}


def engine_with(amd, X, K, dtype, st, cls=None):
    eng = (cls or amd.DeviceCAVI)(X.shape[0], X.shape[1], K, dtype=dtype)
    eng.upload(X, warn=False)
    eng.set_hypers(0.3, 0.3, 1.3, 0.8)
    for name in ("xi", "theta", "eta", "beta"):
        eng.set_gamma(name, *st[name])
    return eng


def state_of(eng):
    return {n: eng.get_gamma(n) for n in ("xi", "theta", "eta", "beta")}


def without_some_rows_and_columns(X, rows, cols):
    keep = ~(np.isin(X.row, rows) | np.isin(X.col, cols))
    return coo_matrix((X.data[keep], (X.row[keep], X.col[keep])), shape=X.shape)


def base_matrix(seed=5):
    """1500 x 1300, about 5 % filled, integer counts (the packed entry format), three empty cells and three empty genes."""
    X = synthetic_counts(1500, 1300, 0.05, seed=seed)
    return without_some_rows_and_columns(X, [0, 77, 1499], [3, 640, 1299])


def edge_matrix(seed=6):
    """base_matrix plus explicitly stored zeros (some in otherwise empty rows), repeated (cell, gene) entries kept as
    separate observations, and one non-integer value (so: the unpacked entry format)."""
    X = base_matrix(seed)
    rng = np.random.RandomState(seed)
    n = X.nnz // 25
    pick = rng.randint(0, X.nnz, n)
    zr, zc = rng.randint(0, X.shape[0], n), rng.randint(0, X.shape[1], n)
    zr[:2], zc[:2] = 77, [3, 5]                    # a cell / a gene whose only entries are stored zeros
    row = np.concatenate([X.row, X.row[pick], zr]).astype(np.int32)
    col = np.concatenate([X.col, X.col[pick], zc]).astype(np.int32)
    val = np.concatenate([X.data.astype(np.float64), rng.randint(1, 5, n), np.zeros(n)])
    val[11] = 2.5
    perm = rng.permutation(val.shape[0])           # unsorted COO
    return coo_matrix((val[perm], (row[perm], col[perm])), shape=X.shape)


MATRICES = {"packed": base_matrix, "edge": edge_matrix}


def check_rows(eng, X, st, dtype, label=""):
    """loss_rows on both axes against the yardstick; returns the device arrays {by: (llh, gl, count)}."""
    dt = np.dtype(dtype)
    theta, beta = st["theta"], st["beta"]
    out = {}
    for by in ("cell", "gene"):
        want = ref.loss_rows(X, theta, beta, by)
        llh, gl, cnt = eng.loss_rows(by)
        assert llh.dtype == np.float64 and gl.dtype == np.float64 and cnt.dtype == np.int64
        assert_array_equal(cnt, want["count"], err_msg="%s count by %s" % (label, by))
        empty = want["count"] == 0
        assert empty.mean() < 0.05, "%s: %d of %d rows by %s are empty" % (label, empty.sum(), empty.size, by)
        assert_allclose(gl, want["gl"], rtol=1e-12, atol=0, err_msg="%s gammaln by %s" % (label, by))
        err = np.abs(llh - want["llh"])[~empty] / want["scale"][~empty]
        WORST[dt.name] = max(WORST.get(dt.name, 0.0), float(err.max()))
        print("%s by %s %s: largest scaled llh error %.3g" % (label, by, dt.name, err.max()))
        assert err.max() <= TOL[dt], "%s llh by %s: scaled error %.3g in row %d" % (label, by, err.max(),
                                                                                   np.flatnonzero(~empty)[err.argmax()])
        assert_array_equal(llh[empty], 0.0)
        mean = eng.cellmean_negative_pois_llh() if by == "cell" else eng.genemean_negative_pois_llh()
        assert_array_equal(np.isnan(mean), empty)
        out[by] = (llh, gl, cnt)
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", [5, 20, 50])
@pytest.mark.parametrize("matrix", ["packed", "edge"])
def test_rows_match_the_yardstick(amd, matrix, K, dtype, plan_kind):
    """A random state, then the state a few iterations later; sums against the scalar loss; bitwise repeatable."""
    X = MATRICES[matrix]()
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=K)
    with engine_with(amd, X, K, dtype, st) as eng:
        info = eng.upload_info()
        assert (info["zeros"] > 0) == (matrix == "edge")
        if matrix == "edge":
            assert info["packed"] == 0          # a non-integer value: the unpacked entry format
        for stage in ("random", "stepped"):
            if stage == "stepped":
                eng.steps(3)
                st = state_of(eng)
            got = check_rows(eng, X, st, dtype, "%s/%s/K%d/%s" % (plan_kind, matrix, K, stage))
            for by in ("cell", "gene"):                     # two calls, the same bits
                for a, b in zip(got[by], eng.loss_rows(by)):
                    assert_array_equal(a, b)
            # consistency with the scalar loss of the same engine
            tol = TOL[np.dtype(dtype)]
            llh, gl, nnz = eng.loss_terms()
            scale = ref.loss_rows(X, st["theta"], st["beta"], "cell")["scale"].sum()
            for by in ("cell", "gene"):
                assert got[by][2].sum() == nnz == X.nnz
                assert abs(got[by][0].sum() - llh) <= tol * scale
                assert_allclose(got[by][1].sum(), gl, rtol=1e-12)
                assert_allclose(-(got[by][0].sum() - got[by][1].sum()) / nnz, eng.mean_negative_pois_llh(),
                                rtol=tol * scale / abs(llh - gl) + 1e-15)


def test_rows_span_several_tasks_on_both_axes(amd, plan_kind, monkeypatch):
    """A matrix whose rows lie in several tasks (tile plans) / chunks (gather plan) on BOTH axes: the row reduction
    then really sums several records per row."""
    if plan_kind != "gather":
        monkeypatch.setenv("SCHPF_TASKS", "2000")
    X = synthetic_counts(2600, 2300, 0.04, seed=9)
    for dtype, K in ((np.float64, 20), (np.float32, 50)):
        st = random_state(X.shape[0], X.shape[1], K, dtype, seed=2)
        with engine_with(amd, X, K, dtype, st) as eng:
            p = eng.plan_info()
            if plan_kind == "gather":
                assert p["n_chunks_cell"] > X.shape[0] and p["n_chunks_gene"] > X.shape[1]
            else:
                gpb = 64 // p["LPC"] * p["waves_per_block"]
                for n, tasks in ((X.shape[0], p["n_waves_cell"]), (X.shape[1], p["n_waves_gene"])):
                    blocks = -(-n // gpb)
                    assert tasks >= 2 * blocks, "every block should be cut into several tasks (pcount > 1): %s" % (p,)
            check_rows(eng, X, st, dtype, "%s/multi-task/K%d" % (plan_kind, K))


@pytest.mark.parametrize("fname, dtype", [("f64", np.float64), ("f32", np.float32)])
def test_golden_state_and_the_reference_cellmean(amd, fname, dtype, plan_kind):
    """The state the reference fitted (ops_*.npz): rows against the yardstick, and the reference's own
    cellmean_negative_pois_llh vector at test_ops_gpu.py's tolerance for it."""
    g = load_golden("ops_%s.npz" % fname)
    X = golden_coo(g)
    K = g["theta_shape"].shape[1]
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=0)
    st["theta"], st["beta"] = (g["theta_shape"], g["theta_rate"]), (g["beta_shape"], g["beta_rate"])
    with engine_with(amd, X, K, dtype, st) as eng:
        got = eng.cellmean_negative_pois_llh()
        lr = eng.loss_rows("cell")
    want = g["cellmean_neg_llh"]
    keep = lr[2] > 0
    assert_allclose(got[keep], want[keep], rtol=1e-5 if dtype == np.float32 else 1e-7)
    assert_array_equal(np.isnan(got), ~keep)
    t = ref.loss_rows(X, st["theta"], st["beta"], "cell")
    assert_array_equal(lr[2], t["count"])
    assert np.all(np.abs(lr[0] - t["llh"]) <= TOL[np.dtype(dtype)] * np.maximum(t["scale"], 1e-300))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fitted_golden_state(amd, dtype, plan_kind):
    g = load_golden("fit_data_k5_s0_f64.npz")
    X = golden_coo(g)
    st = {n: (g[n + "_shape"].astype(dtype), g[n + "_rate"].astype(dtype)) for n in ("xi", "theta", "eta", "beta")}
    with engine_with(amd, X, int(g["nfactors"]), dtype, st) as eng:
        for by in ("cell", "gene"):
            want = ref.loss_rows(X, st["theta"], st["beta"], by)
            llh, gl, cnt = eng.loss_rows(by)
            assert_array_equal(cnt, want["count"])
            assert_allclose(gl, want["gl"], rtol=1e-12)
            some = want["count"] > 0
            err = np.abs(llh - want["llh"])[some] / want["scale"][some]
            WORST[np.dtype(dtype).name] = max(WORST.get(np.dtype(dtype).name, 0.0), float(err.max()))
            assert err.max() <= TOL[np.dtype(dtype)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", [5, 20, 50])
def test_loss_rows_only_reads_the_state(amd, K, dtype, plan_kind):
    """steps(3); loss_rows on both axes; steps(3) leaves every Gamma bit-identical to steps(3); steps(3) -- and the same
    between init_phi_host and the first step."""
    X = edge_matrix(seed=8)
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=3)
    rng = np.random.RandomState(4)
    phi = rng.dirichlet(np.ones(K), X.nnz) * np.asarray(X.data, np.float64)[:, None]
    finals = []
    for probe in (False, True):
        with engine_with(amd, X, K, dtype, st) as eng:
            eng.init_phi_host(phi)
            if probe:
                eng.loss_rows("cell"); eng.loss_rows("gene")
            eng.steps(3)
            if probe:
                eng.loss_rows("cell"); eng.loss_rows("gene")
            eng.steps(3)
            if probe:
                eng.loss_rows("gene")
            finals.append((state_of(eng), eng.loss_terms()))
    for name in ("xi", "theta", "eta", "beta"):
        for a, b in zip(finals[0][0][name], finals[1][0][name]):
            assert_array_equal(a, b, err_msg=name)
    assert finals[0][1] == finals[1][1]


@only_plans("tile", "gather")
def test_python_surface(amd, plan_kind):
    from schpf_amd import HPF_Gamma, loss, scHPF, _lib
    X = edge_matrix(seed=10)
    K, dtype = 5, np.float64
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=1)
    theta, beta = HPF_Gamma(*st["theta"]), HPF_Gamma(*st["beta"])
    with engine_with(amd, X, K, dtype, st) as eng:
        cell, gene = eng.cellmean_negative_pois_llh(), eng.genemean_negative_pois_llh()
        for bad in ("factor", 2, None):
            with pytest.raises((ValueError, _lib.SchpfHipError)):
                eng.loss_rows(bad)
        out, cnt = np.empty(X.shape[0]), np.empty(X.shape[0], np.int64)
        import ctypes
        p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))  # noqa: E731
        status = eng._lib.schpf_loss_rows(eng._h, 7, p(out, ctypes.c_double), p(out, ctypes.c_double), p(cnt, ctypes.c_int64))
        assert status != 0 and b"SCHPF_BY_CELL" in eng._lib.schpf_last_error()
    assert_array_equal(loss.cellmean_negative_pois_llh(X, theta=theta, beta=beta, a=0.3), cell)
    assert_array_equal(loss.genemean_negative_pois_llh(X, theta=theta, beta=beta), gene)
    m = scHPF(K, dtype=dtype)
    m.theta, m.beta = theta, beta
    assert_array_equal(m.genemean_negative_pois_llh(X), gene)
    assert_allclose(cell, ref.rowmean_negative(X, st["theta"], st["beta"], "cell"), rtol=1e-9, equal_nan=True)
    # the estimator's host route (unchanged) gives the same means on a matrix without duplicates or stored zeros
    Y = base_matrix(seed=10)
    on_device = loss.cellmean_negative_pois_llh(Y, theta=theta, beta=beta)
    with np.errstate(divide="ignore", invalid="ignore"):
        on_host = m.cellmean_negative_pois_llh(Y)
    some = ~np.isnan(on_device)
    assert some.sum() == Y.shape[0] - 3
    assert_allclose(on_device[some], on_host[some], rtol=1e-7)


@only_plans("tile")
def test_batch_engine_raises(amd, plan_kind):
    from schpf_amd import _lib
    X = base_matrix(seed=12)
    K, dtype = 5, np.float64
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=1)
    src = amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=dtype)
    try:
        src.keep_rows()
        src.upload(X)
        rows = np.arange(10, 210, dtype=np.int32)
        with amd.DeviceCAVI(rows.size, X.shape[1], K, dtype=dtype) as batch:
            batch.upload_rows(src, rows)
            for n in ("eta", "beta"):
                batch.set_gamma(n, *st[n])
            with pytest.raises(_lib.SchpfHipError, match="batch rows"):
                batch.loss_rows("cell")
            with pytest.raises(_lib.SchpfHipError, match="batch rows"):
                batch.loss_terms()
    finally:
        src.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_row_shards_on_one_gpu_add_up(amd, dtype, plan_kind):
    """The nnz-balanced row blocks of ThreadedShards on separate engines (hint_sharded) of one GPU: cells concatenated
    and genes summed equal the whole-matrix engine -- counts exactly, sums at the loss tolerance."""
    from schpf_amd.sharded import row_partition, take_rows
    X = edge_matrix(seed=14)
    K = 20
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=5)
    with engine_with(amd, X, K, dtype, st) as eng:
        whole = {by: eng.loss_rows(by) for by in ("cell", "gene")}
    bounds = row_partition(X, 3)
    parts = []
    for r in range(3):
        lo, hi = int(bounds[r]), int(bounds[r + 1])
        sub, _ = take_rows(X, lo, hi)
        sst = dict(st, xi=tuple(v[lo:hi] for v in st["xi"]), theta=tuple(v[lo:hi] for v in st["theta"]))
        eng = amd.DeviceCAVI(hi - lo, X.shape[1], K, dtype=dtype)
        try:
            eng.hint_sharded()
            eng.upload(sub, warn=False)
            for name in ("xi", "theta", "eta", "beta"):
                eng.set_gamma(name, *sst[name])
            parts.append({by: eng.loss_rows(by) for by in ("cell", "gene")})
        finally:
            eng.close()
    tol = TOL[np.dtype(dtype)]
    cells = [np.concatenate([p["cell"][i] for p in parts]) for i in range(3)]
    genes = [sum(p["gene"][i] for p in parts) for i in range(3)]
    for by, got in (("cell", cells), ("gene", genes)):
        scale = np.maximum(ref.loss_rows(X, st["theta"], st["beta"], by)["scale"], 1e-300)
        assert_array_equal(got[2], whole[by][2])
        assert np.all(np.abs(got[0] - whole[by][0]) <= tol * scale)
        assert_allclose(got[1], whole[by][1], rtol=1e-12)


@only_plans("tile")
def test_threaded_shards_over_two_gpus(amd, plan_kind):
    from schpf_amd import _lib
    from schpf_amd.sharded import ThreadedShards
    if _lib.device_count() < 2:
        pytest.skip("needs two GPUs")
    X = edge_matrix(seed=16)
    K, dtype = 20, np.float64
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=6)
    sh = ThreadedShards(X, K, dtype, [0, 1])
    try:
        sh.set_hypers(0.3, 0.3, 1.3, 0.8)
        for name in ("xi", "theta", "eta", "beta"):
            sh.set_gamma(name, *st[name])
        for by in ("cell", "gene"):
            want = ref.loss_rows(X, st["theta"], st["beta"], by)
            llh, gl, cnt = sh.loss_rows(by)
            assert_array_equal(cnt, want["count"])
            assert np.all(np.abs(llh - want["llh"]) <= 1e-11 * np.maximum(want["scale"], 1e-300))
            assert_allclose(gl, want["gl"], rtol=1e-12)
    finally:
        sh.close()


@only_plans("hostplan")
def test_zz_report_largest_scaled_error(plan_kind):
    """Not a check of its own: prints the largest scaled llh error the tests above saw, per dtype."""
    print("largest scaled llh error per dtype:", WORST)
    for name, tol in (("float64", 1e-11), ("float32", 1e-5)):
        assert WORST.get(name, 0.0) <= tol
