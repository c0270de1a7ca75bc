"""The log-domain fallback of the phi sweeps on every instantiated shape, and at its threshold.

When the product-form normaliser s of a nonzero underflows, the tile plans' reciprocal is inf and the accumulators of
the row's lane group turn inf / NaN (the gather plans test s in the loop), and after the task or chunk the group
recomputes the row from the E[log] tables in the reference's max-shifted form (sweep_impl.h slow_task_row, slow_chunk, slow_nonzero;
MODE_ELBO: slow_task_elbo, slow_chunk_elbo).  That code decodes entries, pads and masks on its own and is the only
caller of group_max.  One case per case of tests/_sweep_shapes.py (plan, dtype, (NV, LPC) pair, layout) with K' =
max(K, 2) factors, from the start state of tests/_fallback_reference.py: a third of the rows flat, a third with hard
zeros, a third around the format's smallest number -- cold rows, mixed rows and fast rows in every task
(tests/test_fallback_host.py holds the state to its conditions).  A case, in order:
  asserts the pair, workgroup, schedule and entry format it runs on (test_sweep_shapes_gpu.assert_shape);
  reads the device's tab_log of the start state; loss before any step against the oracle (1e-12 / 2e-6);
  the five ELBO terms against tests/_elbo_reference.py at test_elbo_gpu's 1e-11 / 1e-5 of sum |terms|, twice: same bits;
  one step: every element of theta's and beta's shape against the longdouble reference, by the derived bound;
  the whole state (eight arrays) against the oracle's iteration from the same state: float64 rtol 1e-10 (the figure of
    test_underflow_fallback_matches_log_domain_oracle), float32 rtol 1.142e-3 -- the larger of the iteration tests'
    2e-5 and twice 5.71e-4, the largest distance of the float32 oracle's iteration from the float64 oracle's from the
    same state over these cases (a hard row's E[log] of 1e4 is known to 6e-4 in float32; measured by
    tests/test_fallback_host.py, which pins the figure);
  a second step against the oracle at twice those figures: what the cold path stored is a clean accumulator;
  the loss of the device's own state after two steps against the oracle's formula on that state (1e-11 / 1e-5);
  packed 256- and 1024-thread cases: SCHPF_DUAL=0 (the single-orientation kernels' cold path) leaves the same bits;
  four tile cases: SCHPF_DEVICE_PLAN=0 (host-built plans) leaves the same bits.
Every half-window case runs a second time with one window range per block (SCHPF_TASKS=1): only then do rows work ahead
of their epoch and the cold path decodes entries that live in the other slot (entry_minor's ring branch with ahead > 0).
The threshold test runs the same on seven layouts of six pairs where every row is a threshold row, d on a grid of step
0.25 across the format's log-tiny and counts from {1, 3, 1000, 65535, 70000}: s walks from normal numbers through the
denormal binades to 0, and x rcp(s) overflows for the large counts first.
The last test prints the largest error / bound per plan, dtype and quantity."""
import numpy as np
import pytest

import _elbo_reference as elbo_ref
import _fallback_reference as fr
import _sweep_shapes as shapes
from test_sweep_shapes_gpu import NAMES, TERMS, assert_shape, load_engine, set_layout

pytestmark = pytest.mark.gpu

WORST = {}     # (plan, dtype, quantity) -> [largest error / bound, the case it came from]
DEVICE_PLAN_CASES = {("float64", (5, 2), "t1024"), ("float64", (7, 4), "balanced"), ("float32", (5, 1), "t1024"),
                     ("float32", (4, 8), "half")}


def record(case, quantity, err, bound):
    w = WORST.setdefault((case.plan, case.dtype, quantity), [0.0, ""])
    frac = float(err / bound) if np.isfinite(err) else float("inf")
    if frac >= w[0]:
        w[0], w[1] = frac, case.id
    return frac <= 1.0


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


class Reference(object):
    """What the oracle and the ELBO yardstick say of one (matrix, K', dtype): computed once, shared by the layouts."""

    def __init__(self, oracle, case):
        self.X, self.bp, self.dp, st = fr.case_inputs(oracle, case)
        X = self.X
        pair = lambda s, n: (getattr(s, n + "_shape"), getattr(s, n + "_rate"))  # noqa: E731
        self.states = [st.copy()]
        self.loss0 = float(oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                                         st.beta_shape, st.beta_rate))
        self.elbo = elbo_ref.elbo_terms(X, fr.A, fr.AP, self.bp, fr.C, fr.CP, self.dp, *[pair(st, n) for n in NAMES])
        for _ in range(2):
            oracle.cavi_iteration(X.data, X.row, X.col, st, fr.A, fr.C, self.bp, self.dp)
            self.states.append(st.copy())
        for s in self.states:
            for a in s.arrays():
                a.setflags(write=False)
        self.tables, self.ld = None, None

    def longdouble(self, log_c, log_g):
        """The longdouble reference from the device's tab_log: once per distinct pair of tables."""
        if self.tables is None or not (np.array_equal(self.tables[0], log_c) and np.array_equal(self.tables[1], log_g)):
            self.tables, self.ld = (log_c, log_g), fr.reference(self.X, log_c, log_g)
        return self.ld


_CACHE = {}


def reference(oracle, case):
    """One Reference at a time: the cases that share one are next to each other."""
    key = (type(case).__name__, case.N, case.G, case.K0, case.K, case.layout.packed, case.dtype)
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = Reference(oracle, case)
    return _CACHE[key]


def check_state(eng, case, want, it):
    rtol = (fr.F32_STATE_RTOL if case.dtype == "float32" else 1e-10) * (it + 1)
    bad = []
    for n in NAMES:
        for part, got in zip(("shape", "rate"), eng.get_gamma(n)):
            w = getattr(want, n + "_" + part).astype(np.float64)
            err = float(np.max(np.abs(got.astype(np.float64) - w) / np.abs(w)))
            print("  %s %s %s step %d: %.3g of %.3g" % (case.id, n, part, it + 1, err, rtol))
            if not record(case, "state, step %d" % (it + 1), err, rtol):
                bad.append("%s %s: %.3g" % (n, part, err))
    assert not bad, "%s step %d, relative errors beyond %.3g: %s" % (case.id, it + 1, rtol, ", ".join(bad))


def check_loss(case, got, want, rtol, label):
    print("  %s %s: device %.17g, oracle %.17g" % (case.id, label, got, want))
    ok = record(case, label, abs(got - want) / abs(want), rtol)
    assert ok, "%s %s: device %.17g, oracle %.17g (rtol %.3g)" % (case.id, label, got, want, rtol)


def check_elbo(eng, case, want):
    got, again = eng.elbo_terms(fr.AP, fr.CP), eng.elbo_terms(fr.AP, fr.CP)
    assert got == again                                   # bitwise: fixed-order sums, no atomics
    tol = (1e-5 if case.dtype == "float32" else 1e-11) * elbo_ref.scale(want)
    bad = ["%s: device %.17g, reference %.17g" % (k, got[k], want[k]) for k in TERMS + ("elbo",)
           if not record(case, "ELBO terms", abs(got[k] - want[k]), tol)]
    assert not bad, "%s (tol %.3g): %s" % (case.id, tol, "; ".join(bad))


def check_elements(eng, case, ref):
    """Every element of theta's and beta's shape after the first step against the longdouble reference."""
    bad = []
    for name in ("theta", "beta"):
        got = eng.get_gamma(name)[0]
        frac, at = fr.scaled_error(got, ref, name)
        if not np.all(np.isfinite(got)):
            frac = float("inf")
        print("  %s %s shape: %.3g of the bound at %s" % (case.id, name, frac, at))
        if not record(case, "shape elements", frac, 1.0):
            bad.append("%s: %.3g of the bound at %s (device %r, reference %r)"
                       % (name, frac, at, got[at], float(ref[name][at])))
    assert not bad, "%s: %s" % (case.id, "; ".join(bad))


def check_same_bits(amd, monkeypatch, X, case, ref, bits, switch):
    monkeypatch.setenv(switch, "0")
    with load_engine(amd, X, case, ref) as eng:
        assert_shape(eng, case)
        eng.step()
        eng.step()
        for n, (s0, r0) in zip(NAMES, bits):
            s1, r1 = eng.get_gamma(n)
            assert np.array_equal(s0, s1) and np.array_equal(r0, r1), "%s: %s differs under %s=0" % (case.id, n, switch)
    monkeypatch.delenv(switch)


def run_case(amd, oracle, monkeypatch, case):
    """Every check of a case runs, whatever an earlier one found: a failure names all the quantities that are off."""
    set_layout(monkeypatch, case)
    if getattr(case, "tasks", 0):
        monkeypatch.setenv("SCHPF_TASKS", str(case.tasks))      # one window range per block: rows work ahead
    ref = reference(oracle, case)
    X, K, f32 = ref.X, case.K, case.dtype == "float32"
    problems = []

    def check(fn, *args):
        try:
            fn(*args)
        except AssertionError as e:
            problems.append(str(e))

    with load_engine(amd, X, case, ref) as eng:
        assert_shape(eng, case)
        log_c, log_g = [eng._debug_tables(by)["log"][:, :K].copy() for by in ("cell", "gene")]
        check(check_loss, case, eng.mean_negative_pois_llh(), ref.loss0, 2e-6 if f32 else 1e-12, "loss before")
        check(check_elbo, eng, case, ref.elbo)
        ld = ref.longdouble(log_c, log_g)
        eng.step()
        check(check_elements, eng, case, ld)
        check(check_state, eng, case, ref.states[1], 0)
        eng.step()
        check(check_state, eng, case, ref.states[2], 1)
        bits = [eng.get_gamma(n) for n in NAMES]
        own = float(oracle.mean_negative_pois_llh(X.data, X.row, X.col, bits[1][0], bits[1][1], bits[3][0], bits[3][1]))
        check(check_loss, case, eng.mean_negative_pois_llh(), own, 1e-5 if f32 else 1e-11, "loss after")
    if case.layout.packed and case.layout.name in ("t256", "t1024"):
        check(check_same_bits, amd, monkeypatch, X, case, ref, bits, "SCHPF_DUAL")
    if case.layout.packed and (case.dtype, (case.NV, case.LPC), case.layout.name) in DEVICE_PLAN_CASES:
        check(check_same_bits, amd, monkeypatch, X, case, ref, bits, "SCHPF_DEVICE_PLAN")
    assert not problems, "\n".join(problems)


TILE_CASES = [fr.fallback_case(c) for c in shapes.cases("tile")]
LONG_TASK_CASES = [fr.long_task_case(c) for c in TILE_CASES if c.layout.name == "half"]
GATHER_CASES = [fr.fallback_case(c) for c in shapes.cases("gather")]
THRESHOLD_CASES = fr.threshold_cases()


@pytest.mark.parametrize("case", TILE_CASES, ids=[c.id for c in TILE_CASES])
def test_tile_fallback(amd, oracle, monkeypatch, case):
    run_case(amd, oracle, monkeypatch, case)


@pytest.mark.parametrize("case", LONG_TASK_CASES, ids=[c.id for c in LONG_TASK_CASES])
def test_half_windows_with_long_tasks(amd, oracle, monkeypatch, case):
    """entry_minor with ring > 1 and ahead > 0 in the cold path: see _fallback_reference.long_task_case."""
    run_case(amd, oracle, monkeypatch, case)


@pytest.mark.parametrize("case", GATHER_CASES, ids=[c.id for c in GATHER_CASES])
def test_gather_fallback(amd, oracle, monkeypatch, case):
    run_case(amd, oracle, monkeypatch, case)


@pytest.mark.parametrize("case", THRESHOLD_CASES, ids=[c.id for c in THRESHOLD_CASES])
def test_threshold(amd, oracle, monkeypatch, case):
    run_case(amd, oracle, monkeypatch, case)


def test_zz_report_largest_scaled_errors():
    """Not a check of its own: the largest error the cases above saw per plan, dtype and quantity, as a fraction of its
    bound, and the case it came from."""
    print("largest errors of the fallback cases, as a fraction of the bound:")
    for (plan, dtype, quantity), (frac, cid) in sorted(WORST.items()):
        print("  FALLBACK-WORST %-6s %s %-14s %.3g  (%s)" % (plan, dtype, quantity, frac, cid))
    for key, (frac, cid) in WORST.items():
        assert frac <= 1.0, (key, cid)
