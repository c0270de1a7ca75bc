"""The yardstick of the stateless operator mirrors, checked without a device (tests/_ops_reference.py): its longdouble
references reproduce the golden vectors and the oracle, a NumPy emulation of every kernel's operation order stays
inside every bound on every case tests/test_ops_shapes_gpu.py runs (so no bound is vacuous, and none is met by roundings
alone), and the wrappers and the C ABI refuse arguments whose sizes do not fit before they touch a pointer."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

import _ops_reference as ref
from conftest import load_golden, synthetic_counts

LD = ref.LD


@pytest.fixture(scope="module")
def golden():
    return load_golden("ops_f64.npz")


def test_references_reproduce_the_golden_vectors(golden):
    """The rtols are those tests/test_ops_gpu.py holds the device to in float64 (1e-7; row sums 1e-13)."""
    g = golden
    N, G = (int(v) for v in g["shape"])
    coo = (g["x"], g["row"], g["col"], g["theta_shape"], g["theta_rate"], g["beta_shape"], g["beta_rate"])
    want = ref.xphi(*coo)[0]
    assert_allclose(want.astype(np.float64), g["xphi"], rtol=1e-7, atol=0)
    assert_allclose(want.astype(np.float64), g["xphi_numpy"], rtol=1e-7, atol=0)
    assert_allclose(want.sum(axis=1).astype(np.float64), g["x"], rtol=1e-13)
    assert_allclose(ref.llh(*coo)[0].astype(np.float64), g["llh"], rtol=1e-7, atol=0)
    assert_allclose(ref.llh(*coo)[0].astype(np.float64), g["llh_numpy"], rtol=1e-7, atol=0)
    for keep, n, prior, key in ((g["row"], N, g["a"], "theta_shape_upd"), (g["col"], G, g["c"], "beta_shape_upd")):
        assert_allclose(ref.shape_update(g["xphi_in"], keep, n, float(prior))[0].astype(np.float64), g[key],
                        rtol=1e-7, atol=0)
    th = ref.rate_update(g["xi_shape"], g["xi_rate"], g["beta_shape"], g["beta_rate"])[0]
    be = ref.rate_update(g["eta_shape"], g["eta_rate"], g["theta_shape"], g["theta_rate"])[0]
    assert_allclose(th.astype(np.float64), g["theta_rate_upd"], rtol=1e-7)
    assert_allclose(be.astype(np.float64), g["beta_rate_upd"], rtol=1e-7)
    eta = ref.capacity_rate(g["beta_shape"], g["beta_rate"], float(g["dp"]))[0]
    xi = ref.capacity_rate(g["theta_shape"], g["theta_rate"], float(g["bp"]))[0]
    assert_allclose(eta.astype(np.float64), g["eta_rate_upd"], rtol=1e-7, atol=0)
    assert_allclose(xi.astype(np.float64), g["xi_rate_upd"], rtol=1e-7, atol=0)


@pytest.mark.parametrize("K", [1, 7, 50])
def test_references_match_the_oracle_seeded(oracle, K):
    """The seeded 2000 x 1500 case of tests/test_ops_gpu.py test_ops_vs_oracle_seeded, float64, its rtol 1e-12; the
    capacity update, which that test leaves out, as well."""
    X = synthetic_counts(2000, 1500, 0.02, seed=11)
    rng = np.random.RandomState(K)
    perm = rng.permutation(X.nnz)
    x, row, col = X.data[perm].astype(np.int64), X.row[perm], X.col[perm]
    N, G = X.shape
    ths = rng.uniform(0.15, 3.0, (N, K)); thr = rng.uniform(0.1, 2.0, (N, K))
    bes = rng.uniform(0.15, 3.0, (G, K)); ber = rng.uniform(0.1, 2.0, (G, K))
    coo = (x, row, col, ths, thr, bes, ber)
    f = lambda a: a.astype(np.float64)   # noqa: E731
    want = oracle.compute_Xphi_data(*coo)
    assert_allclose(f(ref.xphi(*coo)[0]), want, rtol=1e-12, atol=0)
    assert_allclose(f(ref.llh(*coo)[0]), oracle.compute_pois_llh(*coo), rtol=1e-12)
    assert_allclose(f(ref.shape_update(want, col, G, 0.3)[0]), oracle.compute_loading_shape_update(want, col, G, 0.3),
                    rtol=1e-12)
    ps, pr = ths[:, 0].copy(), thr[:, 0].copy()
    assert_allclose(f(ref.rate_update(ps, pr, bes, ber)[0]), oracle.compute_loading_rate_update(ps, pr, bes, ber),
                    rtol=1e-12)
    assert_allclose(f(ref.capacity_rate(bes, ber, 0.7)[0]), oracle.compute_capacity_rate_update(bes, ber, 0.7),
                    rtol=1e-12)


def test_emulations_stay_inside_the_bounds():
    """Every (state, K, dtype) of tests/test_ops_shapes_gpu.py: the kernels' operation order in NumPy, with SciPy's
    digamma / gammaln and NumPy's log / exp in the device functions' place, may use at most 0.9 of any bound; the rest
    is the special functions'.  One exception, stated in _ops_reference: an X * phi result in T's denormal range lies on
    a grid and roundings alone can put it the whole (x + 1) / 2 spacings of its bound away, so those results
    ("xphi_denormal") are held to the bound itself and the 0.9 is asked of all the others.  Prints the largest fraction
    per operator, dtype and state."""
    worst = {}

    def note(op, dt, state, frac, tag):
        key = (op, np.dtype(dt).name, state)
        if frac > worst.get(key, (-1.0, ""))[0]:
            worst[key] = (frac, tag)

    for state in ref.STATES:
        for dt in (np.float64, np.float32):
            for K in ref.LAYOUT_KS + [ref.BIG_K]:
                for op, tag, got, want, bound in ref.operator_checks(ref.problem(K, dt, state), ref.emulation):
                    if op == "xphi":
                        low = want < LD(np.finfo(dt).smallest_normal)
                        if low.any():
                            note("xphi_denormal", dt, state, ref.fraction(got[low], want[low], bound[low]), tag)
                        got, want, bound = got[~low], want[~low], bound[~low]
                    note(op, dt, state, ref.fraction(got, want, bound), tag)
    for K, m in ref.SECOND_TRIP:
        for dt in (np.float64, np.float32):
            a = ref.second_trip_problem(K, m, dt, "mild")
            want, bound = ref.rate_update(*a)
            note("rate_update", dt, "mild", ref.fraction(ref.emulate_rate_update(*a), want, bound), "K%d/m%d" % (K, m))
            a = ref.second_trip_problem(K, m, dt, "exact")       # and the exact case is exact in this order as well
            got = ref.emulate_rate_update(*a)
            assert np.array_equal(got, ref.rate_update(*a)[0].astype(dt)), (K, m)
    for key, (frac, tag) in sorted(worst.items()):
        print("emulated %-14s %-8s %-8s largest error %.3g of its bound (%s)" % (key + (frac, tag)))
    assert len([key for key in worst if key[0] != "xphi_denormal"]) == 6 * 2 * 2
    assert ("xphi_denormal", "float64", "extreme") in worst and ("xphi_denormal", "float32", "extreme") in worst
    for key, (frac, tag) in worst.items():
        assert 0.0 < frac <= (1.0 if key[0] == "xphi_denormal" else 0.9), (key, frac, tag)


def test_extreme_state_has_the_structure_the_gpu_tests_rely_on():
    """Entry 0 of every problem sits at (0, 0), where both sides alternate shape 1e-4 and 5: the reference's phi there is
    exactly 0 on the small factors and x / (number of large factors) on the others."""
    for dt in (np.float64, np.float32):
        p = ref.problem(7, dt, "extreme")
        assert (p["ths"] >= 1e-4).all() and (p["bes"] >= 1e-4).all()
        want = ref.xphi(*ref.coo_args(p))[0]
        assert (p["row"][:4] == 0).all() and (p["col"][:4] == 0).all()
        assert (want[:4, 0::2] == 0).all()
        assert_allclose((want[:4, 1::2] / p["x"][:4, None]).astype(np.float64), 1.0 / 3, rtol=1e-15)
        assert np.isfinite(want.astype(np.float64)).all()


# ------------------------------------------------------------------------------------------------------- refusals
class NoPointers(object):
    """Stands in for the loaded library: a wrapper that reaches a library call has taken pointers already."""

    def __getattr__(self, name):
        return lambda *args: pytest.fail("the wrapper called %s" % name)


@pytest.fixture
def hip(monkeypatch):
    from schpf_amd import hpf_hip, _lib
    monkeypatch.setattr(_lib, "load", lambda: NoPointers())
    monkeypatch.setattr(hpf_hip, "_p", lambda a: pytest.fail("the wrapper took a pointer"))
    return hpf_hip


def _coo(K=3, dt=np.float64):
    p = ref.problem(K, dt, "mild", n_cells=6, n_genes=5, nnz=60)
    return dict(X_data=p["x"], X_row=p["row"], X_col=p["col"], theta_vi_shape=p["ths"], theta_vi_rate=p["thr"],
                beta_vi_shape=p["bes"], beta_vi_rate=p["ber"])


@pytest.mark.parametrize("op", ["compute_Xphi_data", "compute_pois_llh"])
@pytest.mark.parametrize("arg,cut", [("theta_vi_rate", lambda a: a[:-1]), ("theta_vi_rate", lambda a: a[:, :-1]),
                                     ("beta_vi_rate", lambda a: a[:-1]), ("beta_vi_rate", lambda a: a.ravel()),
                                     ("X_row", lambda a: a[:-1]), ("X_col", lambda a: a[:-1]),
                                     ("X_col", lambda a: a[:0])])
def test_coo_wrappers_refuse_arrays_of_another_size(hip, op, arg, cut):
    kw = _coo()
    kw[arg] = cut(kw[arg])
    with pytest.raises(ValueError, match=arg):
        getattr(hip, op)(**kw)


@pytest.mark.parametrize("op", ["compute_Xphi_data", "compute_pois_llh"])
def test_coo_wrappers_refuse_no_factors(hip, op):
    kw = _coo()
    for name in ("theta_vi_shape", "theta_vi_rate", "beta_vi_shape", "beta_vi_rate"):
        kw[name] = kw[name][:, :0]
    with pytest.raises(ValueError, match="theta_vi_shape.*nfactors must be at least 1"):
        getattr(hip, op)(**kw)
    kw = _coo()
    kw["theta_vi_shape"] = kw["theta_vi_shape"][:, 0]
    with pytest.raises(ValueError, match="theta_vi_shape"):
        getattr(hip, op)(**kw)


def test_update_wrappers_refuse_arrays_of_another_size(hip):
    xphi = np.ones((10, 3))
    keep = np.zeros(10, np.int32)
    with pytest.raises(ValueError, match="X_keep"):
        hip.compute_loading_shape_update(xphi, keep[:9], 4, 0.3)
    with pytest.raises(ValueError, match="Xphi_data.*nfactors must be at least 1"):
        hip.compute_loading_shape_update(xphi[:, :0], keep, 4, 0.3)
    with pytest.raises(ValueError, match="Xphi_data"):
        hip.compute_loading_shape_update(xphi[:, 0], keep, 4, 0.3)
    with pytest.raises(ValueError, match="nkeep"):
        hip.compute_loading_shape_update(xphi, keep, -1, 0.3)
    ps, pr, os_, or_ = np.ones(4), np.ones(4), np.ones((7, 3)), np.ones((7, 3))
    with pytest.raises(ValueError, match="prior_vi_rate"):
        hip.compute_loading_rate_update(ps, pr[:3], os_, or_)
    with pytest.raises(ValueError, match="other_loading_vi_rate"):
        hip.compute_loading_rate_update(ps, pr, os_, or_[:6])
    with pytest.raises(ValueError, match="other_loading_vi_rate"):
        hip.compute_loading_rate_update(ps, pr, os_, or_.T)
    with pytest.raises(ValueError, match="other_loading_vi_shape.*nfactors must be at least 1"):
        hip.compute_loading_rate_update(ps, pr, os_[:, :0], or_[:, :0])
    with pytest.raises(ValueError, match="loading_vi_rate"):
        hip.compute_capacity_rate_update(os_, or_[:6], 0.3)
    with pytest.raises(ValueError, match="loading_vi_shape.*nfactors must be at least 1"):
        hip.compute_capacity_rate_update(os_[:, :0], or_[:, :0], 0.3)


@pytest.mark.parametrize("K", [0, -1])
@pytest.mark.parametrize("dtype", ["F64", "F32"])
def test_abi_refuses_no_factors_before_anything_is_uploaded(K, dtype):
    """Every pointer is NULL and the sizes are large: had an entry point read an index, allocated or uploaded before it
    looked at nfactors, it would have crashed here or answered with another message (without a device: a HIP error)."""
    from schpf_amd import _lib
    lib = _lib.load()
    code = getattr(_lib, dtype)
    n = 1 << 20
    calls = {
        "schpf_xphi": (code, n, n, n, K) + (None,) * 8,
        "schpf_pois_llh_pointwise": (code, n, n, n, K) + (None,) * 8,
        "schpf_shape_update": (code, n, K, None, None, n, 0.3, None),
        "schpf_capacity_rate_update": (code, n, K, None, None, 0.3, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) != 0, name
        assert lib.schpf_last_error() == b"nfactors must be at least 1", name
        with pytest.raises(ValueError):
            _lib.check(1)
    for k in (K, 257):
        assert lib.schpf_rate_update(code, n, n, k, None, None, None, None, None) != 0
        assert lib.schpf_last_error() == b"nfactors must be in [1, 256]"
    # the dtype is still asked first
    assert lib.schpf_xphi(7, n, n, n, K, *(None,) * 8) != 0
    assert b"dtype" in lib.schpf_last_error()
