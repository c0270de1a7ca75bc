"""Every instantiated sweep shape once: one case per (plan, dtype, (NV, LPC) pair, layout), at the pair's smallest K.

The engine picks the pair from K and the dtype alone (policy.cpp choose_config); the table of tests/_sweep_shapes.py --
pinned against the library by tests/test_sweep_shapes_host.py -- names the K that reaches each pair, and each case
asserts through plan_info() / upload_info() that it ran on the shape it names.  A pair's kernels are reached through
the layouts of _sweep_shapes (256 / 1024 threads, balanced windows, half windows; 8-byte and 16-byte entries); the
two-launch iteration (SCHPF_DUAL=0) and the device-drawn first iteration ride on the packed cases.  Matrices are the
smallest with more than one block of major rows and more than one LDS window in both orientations.

What a case checks, against the CPU oracle and the float64 yardsticks of the ELBO and the per-row loss, with the
tolerances of the tests it restates per pair (test_iterations_match_oracle, test_terms_match_the_host_reference,
test_loss_rows_gpu.check_rows, test_dual_launch_equals_two_launches_bitwise, test_device_random_phi_is_a_valid_start):
  loss before any step 1e-12 (float64) / 2e-6 (float32), after two steps 1e-11 / 1e-5; state after step `it`
  1e-11 / 2e-5 * (it + 1); ELBO terms 1e-11 / 1e-5 of sum |terms|; a row's loss 1e-11 / 1e-5 of its sum |x log r| + r,
  counts exact; two launches: the same bits; device-drawn start: conservation at rtol 1e-12 / 2e-5 of the sums' scale.
The last test prints the largest error seen per plan, dtype and quantity as a fraction of its bound (DESIGN.md "parity")."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _elbo_reference as elbo_ref
import _loss_rows_reference as rows_ref
import _sweep_shapes as shapes

pytestmark = pytest.mark.gpu

A, C, AP, CP = 0.3, 0.3, 1.0, 1.0
NAMES = ("xi", "theta", "eta", "beta")
TERMS = ("data", "logfac", "rate", "cell", "gene")
WORST = {}     # (plan, dtype, quantity) -> [largest error / bound, the case it came from]


def record(case, quantity, err, bound):
    w = WORST.setdefault((case.plan, case.dtype, quantity), [0.0, ""])
    if err / bound >= w[0]:
        w[0], w[1] = float(err / bound), case.id
    return err <= bound


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


class Reference(object):
    """What the oracle and the yardsticks say of one (matrix, K, dtype): computed once, shared by the layouts, read-only."""

    def __init__(self, oracle, X, K, dtype):
        dt = np.dtype(dtype)
        np.random.seed(K)
        self.bp, self.dp, st = oracle.setup_state(X, K, dt, A, AP, C, CP)
        st.xi_shape[:] = AP + K * A
        st.eta_shape[:] = CP + K * C
        loss = lambda s: float(oracle.mean_negative_pois_llh(X.data, X.row, X.col, s.theta_shape, s.theta_rate,  # noqa: E731
                                                            s.beta_shape, s.beta_rate))
        pair = lambda s, n: (getattr(s, n + "_shape"), getattr(s, n + "_rate"))  # noqa: E731
        self.states = [st.copy()]
        self.loss0 = loss(st)
        self.elbo = elbo_ref.elbo_terms(X, A, AP, self.bp, C, CP, self.dp, *[pair(st, n) for n in NAMES])
        self.rows = {by: rows_ref.loss_rows(X, pair(st, "theta"), pair(st, "beta"), by) for by in ("cell", "gene")}
        for _ in range(2):
            oracle.cavi_iteration(X.data, X.row, X.col, st, A, C, self.bp, self.dp)
            self.states.append(st.copy())
        self.loss2 = loss(st)
        for s in self.states:
            for a in s.arrays():
                a.setflags(write=False)


@functools.lru_cache(maxsize=2)
def _reference(oracle, N, G, K, packed, dtype):
    return Reference(oracle, shapes.case_matrix(N, G, K, packed), K, dtype)


def reference(oracle, case):
    return _reference(oracle, case.N, case.G, case.K, case.layout.packed, case.dtype)


def set_layout(monkeypatch, case):
    monkeypatch.setenv("SCHPF_PLAN", case.plan)
    for v in shapes.CLEARED:
        monkeypatch.delenv(v, raising=False)
    for k, v in case.layout.env.items():
        monkeypatch.setenv(k, v)


def load_engine(amd, X, case, ref):
    st = ref.states[0]
    eng = amd.DeviceCAVI(X.shape[0], X.shape[1], case.K, dtype=np.dtype(case.dtype))
    eng.upload(X)
    eng.set_hypers(A, C, ref.bp, ref.dp)
    for n in NAMES:
        eng.set_gamma(n, getattr(st, n + "_shape"), getattr(st, n + "_rate"))
    return eng


def assert_shape(eng, case):
    """The engine runs the kernels the case names; anything else fails the case."""
    info, up = eng.plan_info(), eng.upload_info()
    vec = 16 // shapes.ITEMSIZE[case.dtype]
    got = (info["LPC"], info["KL"] // vec, info["KP"])
    assert got == (case.LPC, case.NV, case.NV * vec * case.LPC) and info["KL"] % vec == 0, (case.id, info)
    assert info["waves_per_block"] == case.layout.wpb, (case.id, info)
    assert (info["ring_cell"], info["ring_gene"]) == (case.layout.ring, case.layout.ring), (case.id, info)
    if case.plan == "tile":
        assert info["chunk_len"] < 0                      # a tile plan: minus the rows per LDS window / slot
        assert up["packed"] == case.layout.packed, (case.id, up)
        if case.layout.ring == 1:
            assert -info["chunk_len"] == case.win_rows, (case.id, info)
        if case.several_windows:
            assert info["windows_cell"] >= 2 and info["windows_gene"] >= 2, (case.id, info)
    else:
        assert info["chunk_len"] > 0 and up["packed"] == 0, (case.id, info, up)    # the gather plan has one entry format
    assert up["nnz"] == eng.nnz and up["rounded"] == 0 and up["zeros"] == 0


def check_state(eng, case, want, it):
    f32 = case.dtype == "float32"
    rtol = 2e-5 * (it + 1) if f32 else 1e-11
    bad = []
    for n in NAMES:
        for part, got in zip(("shape", "rate"), eng.get_gamma(n)):
            w = getattr(want, n + "_" + part)
            err = float(np.max(np.abs(got.astype(np.float64) - w.astype(np.float64)) / np.abs(w.astype(np.float64))))
            if not record(case, "state, step %d" % (it + 1), err, rtol):
                bad.append("%s %s: %.3g" % (n, part, err))
    assert not bad, "%s step %d, relative errors beyond %.3g: %s" % (case.id, it + 1, rtol, ", ".join(bad))


def check_loss(eng, case, want, rtol, label):
    got = eng.mean_negative_pois_llh()
    ok = record(case, label, abs(got - want) / abs(want), rtol)
    assert ok, "%s %s: device %.17g, oracle %.17g (rtol %.3g)" % (case.id, label, got, want, rtol)


def check_elbo(eng, case, want):
    got, again = eng.elbo_terms(AP, CP), eng.elbo_terms(AP, CP)
    assert got == again                                   # bitwise: fixed-order sums, no atomics
    rtol = 1e-5 if case.dtype == "float32" else 1e-11
    tol = rtol * elbo_ref.scale(want)
    bad = ["%s: device %.17g, reference %.17g" % (k, got[k], want[k]) for k in TERMS + ("elbo",)
           if not record(case, "ELBO terms", abs(got[k] - want[k]), tol)]
    assert not bad, "%s (tol %.3g): %s" % (case.id, tol, "; ".join(bad))


def check_rows(eng, case, ref):
    """tests/test_loss_rows_gpu.py check_rows."""
    tol = 1e-5 if case.dtype == "float32" else 1e-11
    for by in ("cell", "gene"):
        want = ref.rows[by]
        llh, gl, cnt = eng.loss_rows(by)
        assert llh.dtype == np.float64 and gl.dtype == np.float64 and cnt.dtype == np.int64
        assert_array_equal(cnt, want["count"], err_msg="%s count by %s" % (case.id, by))
        empty = want["count"] == 0
        assert empty.mean() < 0.05
        assert_allclose(gl, want["gl"], rtol=1e-12, atol=0, err_msg="%s gammaln by %s" % (case.id, by))
        err = np.abs(llh - want["llh"])[~empty] / want["scale"][~empty]
        ok = record(case, "row loss", float(err.max()), tol)
        assert ok, "%s llh by %s: scaled error %.3g in row %d" % (case.id, by, err.max(), np.flatnonzero(~empty)[err.argmax()])
        assert_array_equal(llh[empty], 0.0)
        mean = eng.cellmean_negative_pois_llh() if by == "cell" else eng.genemean_negative_pois_llh()
        assert_array_equal(np.isnan(mean), empty)


def check_two_launches(amd, monkeypatch, X, case, ref, bits):
    """test_dual_launch_equals_two_launches_bitwise: one launch per orientation leaves the same bits."""
    monkeypatch.setenv("SCHPF_DUAL", "0")
    with load_engine(amd, X, case, ref) as eng:
        assert_shape(eng, case)
        eng.step()
        eng.step()
        for n, (s0, r0) in zip(NAMES, bits):
            s1, r1 = eng.get_gamma(n)
            assert np.array_equal(s0, s1) and np.array_equal(r0, r1), "%s: %s differs between one launch and two" % (case.id, n)
    monkeypatch.delenv("SCHPF_DUAL")


def check_random_start(amd, X, case, ref):
    """test_device_random_phi_is_a_valid_start: every nonzero's drawn responsibilities sum to one, and both sweeps
    regenerate the same draws.  float64: that test's rtol 1e-12.  float32: 2e-5 (one iteration) of the compared sums'
    scale -- the counts they hold plus the priors that were subtracted."""
    K, f32 = case.K, case.dtype == "float32"
    with load_engine(amd, X, case, ref) as eng:
        eng.init_phi_device(1234 + K)
        eng.step()
        ths, bes = eng.get_gamma("theta")[0].astype(np.float64), eng.get_gamma("beta")[0].astype(np.float64)
    N, G = X.shape
    a, c = (np.float64(np.float32(A)), np.float64(np.float32(C))) if f32 else (A, C)
    total = float(X.data.sum())
    cell_sums = np.asarray(X.sum(1)).ravel().astype(np.float64)
    checks = [("all cells", (ths - a).sum(), total, total + N * K * a),
              ("all genes", (bes - c).sum(), total, total + G * K * c),
              ("per factor", (ths - a).sum(0), (bes - c).sum(0), (bes - c).sum(0) + (N * a + G * c)),
              ("per cell", (ths - a).sum(1), cell_sums, cell_sums + K * a)]
    for label, got, want, scale in checks:
        bound = 2e-5 * scale if f32 else 1e-12 * np.abs(want)
        err = np.abs(got - want)
        where = np.asarray(bound) > 0
        if np.any(where):
            record(case, "random start", float(np.max(np.asarray(err)[where] / np.asarray(bound)[where])), 1.0)
        assert np.all(err <= bound), "%s random start, %s: largest error %.3g" % (case.id, label, np.max(err))
    assert np.all(ths > a * 0.999) and np.all(bes >= c)


def run_case(amd, oracle, monkeypatch, case):
    set_layout(monkeypatch, case)
    X, ref = case.matrix(), reference(oracle, case)
    f32 = case.dtype == "float32"
    with load_engine(amd, X, case, ref) as eng:
        assert_shape(eng, case)
        check_loss(eng, case, ref.loss0, 2e-6 if f32 else 1e-12, "loss before")
        check_elbo(eng, case, ref.elbo)
        check_rows(eng, case, ref)
        for it in range(2):
            eng.step()
            check_state(eng, case, ref.states[it + 1], it)
        check_loss(eng, case, ref.loss2, 1e-5 if f32 else 1e-11, "loss after")
        bits = [eng.get_gamma(n) for n in NAMES]
    packed_plain = case.layout.packed and case.layout.name in ("t256", "t1024")
    if packed_plain:
        check_two_launches(amd, monkeypatch, X, case, ref, bits)
    if case.layout.packed and case.layout.name in ("t256", "gather"):
        check_random_start(amd, X, case, ref)


TILE_CASES, GATHER_CASES = shapes.cases("tile"), shapes.cases("gather")


@pytest.mark.parametrize("case", TILE_CASES, ids=[c.id for c in TILE_CASES])
def test_tile_shape(amd, oracle, monkeypatch, case):
    run_case(amd, oracle, monkeypatch, case)


@pytest.mark.parametrize("case", GATHER_CASES, ids=[c.id for c in GATHER_CASES])
def test_gather_shape(amd, oracle, monkeypatch, case):
    run_case(amd, oracle, monkeypatch, case)


def test_zz_report_largest_scaled_errors():
    """Not a check of its own: the largest error the cases above saw per plan, dtype and quantity, as a fraction of its
    bound, and the case it came from."""
    print("largest errors of the sweep shapes, as a fraction of the bound:")
    for (plan, dtype, quantity), (frac, cid) in sorted(WORST.items()):
        print("  SHAPE-WORST %-6s %s %-14s %.3g  (%s)" % (plan, dtype, quantity, frac, cid))
    for key, (frac, cid) in WORST.items():
        assert frac <= 1.0, (key, cid)
