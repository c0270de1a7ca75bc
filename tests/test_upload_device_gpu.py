"""Uploading a count matrix that already lies in GPU memory against the host upload of the same build on
the same matrix: the engine must end up holding the same thing, so every comparison here is for equal bits.  The host
path is the reference; the existing tests pin it to the oracle."""
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.sparse import coo_matrix

from conftest import bench_matrix, load_golden, golden_coo, synthetic_counts

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
NAMES = ("xi", "theta", "eta", "beta")
PLAN_VARS = ("SCHPF_HALF", "SCHPF_BALANCE", "SCHPF_WPB", "SCHPF_LOSS_SIDE", "SCHPF_DEVICE_PLAN", "SCHPF_TASKS")


def set_plan(monkeypatch, kind):
    """The plan kinds of tests/test_loss_rows_gpu.py, with its environment settings."""
    monkeypatch.setenv("SCHPF_PLAN", "gather" if kind == "gather" else "tile")
    for v in PLAN_VARS:
        monkeypatch.delenv(v, raising=False)
    if kind == "half":
        monkeypatch.setenv("SCHPF_HALF", "2")
    if kind == "balanced":
        monkeypatch.setenv("SCHPF_BALANCE", "1")
        monkeypatch.setenv("SCHPF_WPB", "16")
    if kind == "hostplan":
        monkeypatch.setenv("SCHPF_DEVICE_PLAN", "0")


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def without_some_rows_and_columns(X, rows, cols):
    keep = ~(np.isin(X.row, rows) | np.isin(X.col, cols))
    return coo_matrix((X.data[keep], (X.row[keep], X.col[keep])), shape=X.shape)


def base_matrix(seed=5):
    """1500 x 1300, about 5 % filled, integer counts, three empty cells and three empty genes, sorted by (row, col)."""
    X = synthetic_counts(1500, 1300, 0.05, seed=seed)
    return without_some_rows_and_columns(X, [0, 77, 1499], [3, 640, 1299])


def edge_matrix(seed=6):
    """base_matrix plus stored zeros (some in otherwise empty rows), repeated entries, one non-integer value; unsorted."""
    X = base_matrix(seed)
    rng = np.random.RandomState(seed)
    n = X.nnz // 25
    pick = rng.randint(0, X.nnz, n)
    zr, zc = rng.randint(0, X.shape[0], n), rng.randint(0, X.shape[1], n)
    zr[:2], zc[:2] = 77, [3, 5]
    row = np.concatenate([X.row, X.row[pick], zr]).astype(np.int32)
    col = np.concatenate([X.col, X.col[pick], zc]).astype(np.int32)
    val = np.concatenate([X.data.astype(np.float64), rng.randint(1, 5, n), np.zeros(n)])
    val[11] = 2.5
    perm = rng.permutation(val.shape[0])
    return coo_matrix((val[perm], (row[perm], col[perm])), shape=X.shape)


_MATRICES = {}


def matrix(name):
    if name not in _MATRICES:
        _MATRICES[name] = {"packed": base_matrix, "edge": edge_matrix}[name]()
    return _MATRICES[name]


def on_gpu(X, fmt):
    """The SciPy COO X as a GPU tensor: 'coo64' / 'coo32' (uncoalesced: the entries as they are, in their order) or
    'csr32' / 'csr64' (X must be sorted by (row, col); entries kept as they are)."""
    it = torch.int32 if fmt.endswith("32") else torch.int64
    val = torch.tensor(X.data).cuda()
    if fmt.startswith("coo"):
        ind = torch.tensor(np.stack([X.row, X.col])).to(it).cuda()
        return torch.sparse_coo_tensor(ind, val, X.shape, check_invariants=False, is_coalesced=False)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(X.row, minlength=X.shape[0]))])
    return torch.sparse_csr_tensor(torch.tensor(indptr).to(it).cuda(), torch.tensor(X.col).to(it).cuda(), val, size=X.shape)


def random_state(N, G, K, dtype, seed):
    rng = np.random.RandomState(seed)
    g = lambda *d: (rng.uniform(0.2, 3.0, d).astype(dtype), rng.uniform(0.5, 2.0, d).astype(dtype))  # noqa: E731
    return {"xi": g(N), "theta": g(N, K), "eta": g(G), "beta": g(G, K)}


def engine_with(amd, X, shape, K, dtype, st, prepare=None):
    eng = amd.DeviceCAVI(shape[0], shape[1], K, dtype=dtype)
    if prepare:
        prepare(eng)
    eng.upload(X, warn=False)
    eng.set_hypers(0.3, 0.3, 1.3, 0.8)
    for name in NAMES:
        eng.set_gamma(name, *st[name])
    return eng


def assert_same_engine(host, dev, steps=3, rows=True):
    assert dev.upload_info() == host.upload_info()
    assert dev.plan_info() == host.plan_info()
    assert dev.sweep_bytes() == host.sweep_bytes()
    for e in (host, dev):
        e.init_phi_device(7)
    for _ in range(steps):
        host.steps(1); dev.steps(1)
    for name in NAMES:
        for a, b in zip(host.get_gamma(name), dev.get_gamma(name)):
            assert_array_equal(a, b, err_msg=name)
    if rows:
        assert dev.loss_terms() == host.loss_terms()
        assert dev.elbo_terms(1.0, 1.0) == host.elbo_terms(1.0, 1.0)
        for by in ("cell", "gene"):
            for a, b in zip(host.loss_rows(by), dev.loss_rows(by)):
                assert_array_equal(a, b, err_msg=by)


# every format, value dtype, plan kind and K = 50 at least once; the CSR formats on the sorted matrix only; the edge
# matrix holds 2.5, so only with float values
CASES = [
    ("packed", "coo64", np.int32, 5, np.float64, "tile"),
    ("packed", "coo32", np.int64, 20, np.float32, "half"),
    ("packed", "csr32", np.float32, 20, np.float64, "balanced"),
    ("packed", "csr64", np.float64, 50, np.float64, "tile"),
    ("packed", "csr32", np.int32, 5, np.float32, "gather"),
    ("packed", "coo64", np.float64, 20, np.float64, "hostplan"),
    ("edge", "coo64", np.float64, 20, np.float64, "tile"),
    ("edge", "coo32", np.float64, 50, np.float32, "half"),
    ("edge", "coo64", np.float32, 5, np.float64, "gather"),
    ("edge", "coo32", np.float64, 20, np.float64, "balanced"),
    ("edge", "coo64", np.float64, 5, np.float32, "hostplan"),
]


@pytest.mark.parametrize("name, fmt, vdtype, K, dtype, plan", CASES)
def test_device_upload_equals_host_upload(amd, monkeypatch, name, fmt, vdtype, K, dtype, plan):
    set_plan(monkeypatch, plan)
    X = matrix(name)
    X = coo_matrix((X.data.astype(vdtype), (X.row, X.col)), shape=X.shape)
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=K)
    with engine_with(amd, X, X.shape, K, dtype, st) as host, engine_with(amd, on_gpu(X, fmt), X.shape, K, dtype, st) as dev:
        assert (host.upload_info()["zeros"] > 0) == (name == "edge")
        assert_same_engine(host, dev)


def test_task_range_model_from_device_histograms(amd, monkeypatch, capfd):
    """A matrix large enough for policy.cpp choose_ranges to run its sampled histograms with stride 2: 40 * 21 + 20 * 42
    block x half-window pairs >= 6 * 256 and nnz / 4e6 = 2."""
    for v in PLAN_VARS + ("SCHPF_PLAN",):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("SCHPF_VERBOSE", "1")
    X = bench_matrix(20000, 10000, 0.05)
    assert X.nnz >= 8000000
    K, dtype = 20, np.float64
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=1)
    with engine_with(amd, X, X.shape, K, dtype, st) as host:
        assert "task ranges from the list-schedule model" in capfd.readouterr().err
        with engine_with(amd, on_gpu(X, "coo64"), X.shape, K, dtype, st) as dev:
            err = capfd.readouterr().err
            assert "task ranges from the list-schedule model" in err and "upload_coo_device" in err
            assert_same_engine(host, dev, steps=2, rows=False)


def test_marginals(amd, monkeypatch):
    from schpf_amd import hpf_hip, _lib
    set_plan(monkeypatch, "tile")
    K, dtype = 5, np.float64
    X = matrix("packed")
    with amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=dtype) as eng:
        eng.upload(on_gpu(X, "csr32"))
        for got, want in zip(eng.marginals(), hpf_hip.coo_marginals(X)):
            assert_array_equal(got, want)
    E = matrix("edge")
    v32 = E.data.astype(np.float32).astype(np.float64)
    with amd.DeviceCAVI(E.shape[0], E.shape[1], K, dtype=dtype) as eng:
        eng.upload(on_gpu(E, "coo64"), warn=False)
        rows, cols = eng.marginals()
        assert_allclose(rows, np.bincount(E.row, weights=v32, minlength=E.shape[0]), rtol=1e-12)
        assert_allclose(cols, np.bincount(E.col, weights=v32, minlength=E.shape[1]), rtol=1e-12)
    src = amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=dtype)
    try:
        src.keep_rows()
        src.upload(on_gpu(X, "coo64"))
        rows = np.arange(10, 210, dtype=np.int32)
        with amd.DeviceCAVI(rows.size, X.shape[1], K, dtype=dtype) as batch:
            batch.upload_rows(src, rows)
            with pytest.raises(_lib.SchpfHipError, match="batch rows"):
                batch.marginals()
    finally:
        src.close()


@pytest.mark.parametrize("fmt", ["coo64", "csr32"])
def test_keep_rows_source_uploaded_from_the_device(amd, monkeypatch, fmt):
    set_plan(monkeypatch, "tile")
    X = matrix("packed")
    K, dtype = 20, np.float64
    st = random_state(X.shape[0], X.shape[1], K, dtype, seed=2)
    rows = np.random.RandomState(0).permutation(X.shape[0])[:300].astype(np.int32)
    bst = dict(st, xi=tuple(v[rows] for v in st["xi"]), theta=tuple(v[rows] for v in st["theta"]))
    finals = []
    for M in (X, on_gpu(X, fmt)):
        with engine_with(amd, M, X.shape, K, dtype, st, prepare=lambda e: e.keep_rows()) as src:
            assert src.upload_info()["rows"]
            with amd.DeviceCAVI(rows.size, X.shape[1], K, dtype=dtype) as batch:
                batch.upload_rows(src, rows)
                batch.set_hypers(0.3, 0.3, 1.3, 0.8)
                for name in NAMES:
                    batch.set_gamma(name, *bst[name])
                batch.step(cells_first=True)
                finals.append((batch.plan_info(), {n: batch.get_gamma(n) for n in NAMES}))
    assert finals[0][0] == finals[1][0]
    for name in NAMES:
        for a, b in zip(finals[0][1][name], finals[1][1][name]):
            assert_array_equal(a, b, err_msg=name)


def small_coo(n=4000, N=300, G=200, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, N, n).astype(np.int64), rng.randint(0, G, n).astype(np.int64),
            rng.randint(1, 9, n).astype(np.float64), (N, G))


def gpu_coo(row, col, val, shape):
    return torch.sparse_coo_tensor(torch.tensor(np.stack([row, col])).cuda(), torch.tensor(val).cuda(), shape,
                                   check_invariants=False, is_coalesced=False)


def assert_no_matrix(eng):
    from schpf_amd import _lib
    with pytest.raises(_lib.SchpfHipError, match="no count matrix"):
        eng.steps(1)


@pytest.mark.parametrize("what, entries, message", [
    ("col", {1234: 200}, "COO index out of range at entry 1234"),                       # == ngenes
    ("row", {77: -1, 900: -5}, "COO index out of range at entry 77"),                   # negative; the smallest entry
    ("col", {3999: 2 ** 33}, "COO index out of range at entry 3999"),                   # an int64 beyond int32
    ("val", {2100: np.nan, 7: -1.0, 3000: np.inf}, "offending entry 7"),
    ("val", {2100: np.inf}, "offending entry 2100"),
    ("val", {64: np.nan}, "offending entry 64"),
    ("both", {5: -2.0, 3100: 10 ** 6}, "COO index out of range at entry 3100"),         # an index error goes first
])
def test_bad_entries_are_refused(amd, monkeypatch, what, entries, message):
    set_plan(monkeypatch, "tile")
    row, col, val, shape = small_coo()
    with amd.DeviceCAVI(shape[0], shape[1], 5) as eng:
        eng.upload(gpu_coo(row, col, val, shape))           # a matrix the failed upload must take away
        for j, v in entries.items():
            target = {"row": row, "col": col, "val": val}.get(what) if what != "both" else (val if v < 0 else row)
            target[j] = v
        with pytest.raises(ValueError, match=message):
            eng.upload(gpu_coo(row, col, val, shape))
        assert_no_matrix(eng)
        row, col, val, shape = small_coo()
        eng.upload(gpu_coo(row, col, val, shape))           # and the engine is as usable as before
        eng.steps(1)


@pytest.mark.parametrize("damage", ["decreasing", "short", "start"])
def test_bad_csr_row_pointers_are_refused(amd, monkeypatch, damage):
    from schpf_amd import _lib
    set_plan(monkeypatch, "tile")
    row, col, val, shape = small_coo()
    order = np.lexsort((col, row))
    row, col, val = row[order], col[order], val[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=shape[0]))]).astype(np.int64)
    if damage == "decreasing":
        indptr[100] = indptr[101] + 3
    elif damage == "short":
        indptr[-1] -= 1
    else:
        indptr[0] = 1
    d_ptr, d_col, d_val = (torch.tensor(a).cuda() for a in (indptr, col, val))
    torch.cuda.synchronize()
    with amd.DeviceCAVI(shape[0], shape[1], 5) as eng:
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        status = eng._lib.schpf_upload_csr_device(eng._h, val.shape[0], p(d_ptr), _lib.IDX_I64, p(d_col), _lib.IDX_I64,
                                                  p(d_val), _lib.VAL_F64)
        assert status == 1 and b"indptr" in eng._lib.schpf_last_error()
        assert_no_matrix(eng)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_state_round_trip_on_the_device(amd, dtype):
    N, G, K = 70, 50, 5
    st = random_state(N, G, K, dtype, seed=4)
    with amd.DeviceCAVI(N, G, K, dtype=dtype) as eng, amd.DeviceCAVI(N, G, K, dtype=dtype) as other:
        for name in NAMES:
            eng.set_gamma(name, *st[name])
            s, r = eng.get_gamma(name, device=True)
            assert s.is_cuda and tuple(s.shape) == st[name][0].shape
            for a, b in zip((s, r), eng.get_gamma(name)):
                assert_array_equal(a.cpu().numpy(), b)
            other.set_gamma(name, s, r)
            for a, b in zip(other.get_gamma(name), st[name]):
                assert_array_equal(a, b)
        with pytest.raises(ValueError):
            other.set_gamma("theta", *eng.get_gamma("beta", device=True))
        wrong = torch.float32 if dtype == np.float64 else torch.float64
        with pytest.raises(ValueError):
            other.set_gamma("xi", *[t.to(wrong) for t in eng.get_gamma("xi", device=True)])


def test_inputs_the_engine_refuses(amd):
    X = matrix("packed")
    with amd.DeviceCAVI(X.shape[0], X.shape[1], 5) as eng:
        with pytest.raises(TypeError, match="sparse COO"):
            eng.upload(torch.zeros(X.shape, device="cuda"))
        with pytest.raises(ValueError, match="engine was created for"):
            eng.upload(on_gpu(coo_matrix((X.data, (X.row, X.col)), shape=(X.shape[0] + 1, X.shape[1])), "coo64"))
        with pytest.raises(TypeError, match="float16"):
            t = on_gpu(X, "coo64")
            eng.upload(torch.sparse_coo_tensor(t._indices(), t._values().to(torch.float16), X.shape))
        eng.upload(on_gpu(X, "coo64").cpu())        # a CPU tensor: the host path
        assert eng.upload_info()["nnz"] == X.nnz


def test_schpf_fits_a_matrix_in_gpu_memory(amd):
    from schpf_amd import scHPF
    g = load_golden("fit_data_k5_s0_f64.npz")
    X = golden_coo(g)
    Xg = on_gpu(X, "coo64")
    models = []
    for M, kw in ((Xg, {}), (X, {"init": "device"})):
        np.random.seed(0)
        models.append(scHPF(5, verbose=False).fit(M, **kw))
    a, b = models
    assert (a.bp, a.dp) == (b.bp, b.dp)
    assert a.loss == b.loss and len(a.loss) > 3
    assert_array_equal(a.theta.e_x, b.theta.e_x)
    assert_array_equal(a.beta.e_x, b.beta.e_x)
    for n in NAMES:
        assert getattr(a, n) == getattr(b, n)
    projected = []
    for M, kw in ((on_gpu(X, "csr32" if is_sorted(X) else "coo32"), {}), (X, {"init": "device"})):
        np.random.seed(1)
        projected.append(a.project(M, **kw))
    assert projected[0].loss == projected[1].loss
    assert_array_equal(projected[0].theta.e_x, projected[1].theta.e_x)
    assert_array_equal(projected[0].xi.e_x, projected[1].xi.e_x)
    assert a.elbo(Xg) == a.elbo(X)
    assert a.elbo(Xg, terms=True) == a.elbo(X, terms=True)
    assert_array_equal(a.genemean_negative_pois_llh(Xg), a.genemean_negative_pois_llh(X))
    from schpf_amd import loss
    assert_array_equal(loss.cellmean_negative_pois_llh(Xg, theta=a.theta, beta=a.beta),
                       loss.cellmean_negative_pois_llh(X, theta=a.theta, beta=a.beta))
    for kw in ({"init": "numpy"}, {"batchsize": 100}, {"devices": [0, 1]}):
        with pytest.raises(ValueError):
            scHPF(5, verbose=False).fit(Xg, **kw)
    # run_trials' shared upload: an engine that was uploaded from the device
    with amd.DeviceCAVI(X.shape[0], X.shape[1], 5) as eng:
        eng.upload(Xg)
        np.random.seed(0)
        c = scHPF(5, verbose=False).fit(Xg, engine=eng)
        np.random.seed(0)
        d = scHPF(5, verbose=False).fit(X, engine=eng, init="device")
    assert c.loss == a.loss == d.loss
    assert_array_equal(c.theta.e_x, a.theta.e_x)


def is_sorted(X):
    key = X.row.astype(np.int64) * X.shape[1] + X.col
    return bool(np.all(np.diff(key) >= 0))
