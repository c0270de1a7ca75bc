"""What gamma_update_kernel (schpf_amd/csrc/kernels.hip) WRITES, element by element: the three [n, KP] tables every
sweep, the loss and the ELBO read, copied back by the test hook schpf_debug_tables (DeviceCAVI._debug_tables) and
compared with plain NumPy in longdouble computed from the shape and rate the engine returns -- so the check does not
pass through a sweep, and a table entry wrong by a few ulp, a wrong shift of tab_exp or a nonzero padding column
cannot hide behind the rtol of the state one iteration later.

Reference and bounds, each derived from special.h's stated accuracy (tests/test_special_gpu.py holds the device to it)
and the number formats; T = the engine's dtype, the terms in [] for float32 only (one rounding to T):
  tab_e   = shape / rate.  The kernel multiplies by fast_rcp(rate): relative error <= 2.3e-16 (the reciprocal)
            + 2**-53 (the product) [+ 2**-24].
  tab_log = psi(shape) - log(rate), psi from scipy.special.digamma, log in longdouble:
            |err| <= 4e-15 * max(1, |psi|, |log rate|) [+ 2**-24 |L|]  (special.h's bound for digamma_less_log).
  tab_exp = exp(d), d = tab_log - float32(max_k tab_log) computed from the RETURNED tab_log exactly as the kernel forms it
            (both are one double subtraction), so the exponential is isolated:
            |err| <= (4.5e-16 [+ 2**-24]) * exp(d) + half the denormal spacing of T (the result is rounded once into T's
            denormal range: ldexp in float64, the conversion in float32).  Exactly 0 where d < -1075 ln 2 = -745.1332...,
            below which exp(d) rounds to 0 in float64.  For d in (-745.1332, -745] the correctly rounded float64 value
            is the smallest denormal, not 0, and that is what the general bound above demands there (a 0 would be off by
            more than half a spacing) -- as tests/test_special_gpu.py demands of fast_exp at -745.  Row 1 of every
            state built by extreme_state puts an entry at d = -745.07 to pin that.
  every column k >= K of all three tables is exactly +0.
Every entry of every table is compared.

Which of gamma_update_kernel's 24 instantiations <T, SRC, WAVE_ROWS, MINW> each test launches.  T: both dtypes in
every test.  WAVE_ROWS (rows of K threads inside one wavefront) is on for K <= 64 with (64 / K) * K >= 56, i.e. of the
K used here for 1, 14, 19, 20, 64 and off for 13, 50, 65, 100, 256.  MINW is 4 iff the kernel sums the other side's
per-block column sums itself (capi.hip step_finish `fuse`: default update order on a small problem), else 8.
  test_refresh_at_extreme_state, test_fewer_rows_than_a_block, test_second_trip_of_the_group_loop
      <T, SRC_NONE, on / off, 8>: refresh_tables() after set_gamma.
  test_tables_after_a_step, test_other_side_with_many_update_blocks
      order "fused":          <T, SRC_STRIDED, on / off, 4>      order "simultaneous":          <T, SRC_STRIDED, on / off, 8>
      "fused" after init_phi_host: <T, SRC_DENSE, on / off, 4>   "simultaneous" after init_phi_host: <T, SRC_DENSE, on / off, 8>
      (K = 20, 64 on; K = 13, 50 off), each preceded by the <T, SRC_NONE, ., 8> refresh of the state set with set_gamma.
  Never launched by the engine: <T, SRC_NONE, ., 4>, four instantiations -- refresh_tables() passes no block partials
  of the other side (s_other_nb = 0), and launch_update_t picks MINW from that alone.  Not forced here.
"""
import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.optimize import brentq
from scipy.special import digamma

from conftest import synthetic_counts

pytestmark = pytest.mark.gpu

LD = np.longdouble
ZERO_BELOW = -1075 * np.log(2.0)       # exp(d) < half the smallest float64 denormal
RCP, EXP, PSI = 2.3e-16, 4.5e-16, 4e-15   # special.h's bounds
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
WORST = {}     # (table, dtype name) -> [largest error / bound, largest error in the bound's own unit]


@pytest.fixture(autouse=True, params=["tile", "gather"])
def plan_kind(request, monkeypatch):
    """The two table layouts: KP (the padded row length) is the tile plan's or the L2-gather plan's."""
    monkeypatch.setenv("SCHPF_PLAN", request.param)
    for v in ("SCHPF_HALF", "SCHPF_BALANCE", "SCHPF_WPB", "SCHPF_DEVICE_PLAN", "SCHPF_TASKS", "SCHPF_FUSE_SUMS"):
        monkeypatch.delenv(v, raising=False)
    return request.param


def only_plans(*kinds):
    return pytest.mark.parametrize("plan_kind", list(kinds), indirect=True)


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def rows_per_block(K):
    """kernels.hip update_rows_per_block"""
    return 4 * (64 // K) if K <= 64 and (64 // K) * K >= 56 else 256 // K


def record(table, dt, err, bound, unit_err):
    w = WORST.setdefault((table, dt.name), [0.0, 0.0])
    w[0] = max(w[0], float((err / bound).max()))
    w[1] = max(w[1], float(unit_err.max()))


def check_side(shape, rate, tabs, K, dt, label):
    """The three tables of one side against the state (shape, rate: [n, K] of dtype dt) they were built from."""
    n = shape.shape[0]
    KP = tabs["e"].shape[1]
    assert shape.shape == rate.shape == (n, K) and KP >= K
    bits = np.uint64 if dt == F64 else np.uint32
    for name, t in tabs.items():
        assert t.dtype == dt and t.shape == (n, KP)
        assert not t[:, K:].view(bits).any(), "%s: padding of tab_%s is not zero" % (label, name)
    cast = 0.0 if dt == F64 else 2.0 ** -24
    s, r = shape.astype(LD), rate.astype(LD)
    e, l, x = (tabs[k][:, :K].astype(LD) for k in ("e", "log", "exp"))

    E = s / r
    err, bound = np.abs(e - E), (RCP + 2.0 ** -53 + cast) * E
    record("e", dt, err, bound, err / E)
    print("%s tab_e: largest error %.3g of its bound" % (label, (err / bound).max()))
    assert (err <= bound).all(), "%s tab_e: %.3g of the bound at %s" % (
        label, np.nanmax(err / bound), np.unravel_index(np.nanargmax(err / bound), err.shape))

    psi, lr = digamma(shape.astype(np.float64)).astype(LD), np.log(r)
    L = psi - lr
    scale = np.maximum(1.0, np.maximum(np.abs(psi), np.abs(lr)))
    err, bound = np.abs(l - L), PSI * scale + cast * np.abs(L)
    record("log", dt, err, bound, err / scale)
    print("%s tab_log: largest error %.3g of its bound" % (label, (err / bound).max()))
    assert (err <= bound).all(), "%s tab_log: %.3g of the bound at %s" % (
        label, np.nanmax(err / bound), np.unravel_index(np.nanargmax(err / bound), err.shape))

    lt = tabs["log"][:, :K]
    d = lt.astype(np.float64) - lt.astype(np.float32).max(axis=1).astype(np.float64)[:, None]
    Et = np.exp(d.astype(LD))
    err, bound = np.abs(x - Et), (EXP + cast) * Et + 0.5 * LD(np.finfo(dt).smallest_subnormal)
    some = Et >= LD(np.finfo(dt).tiny)
    record("exp", dt, err, bound, (err / Et)[some])
    print("%s tab_exp: largest error %.3g of its bound; %d of %d arguments below -745" % (
        label, (err / bound).max(), (d <= -745.0).sum(), d.size))
    assert (err <= bound).all(), "%s tab_exp: %.3g of the bound at %s" % (
        label, np.nanmax(err / bound), np.unravel_index(np.nanargmax(err / bound), err.shape))
    assert not tabs["exp"][:, :K][d < ZERO_BELOW].view(bits).any(), "%s tab_exp: not 0 below -745.13" % label
    return d


def check_tables(eng, K, label):
    """Both sides' tables against the state the engine returns; the shifted arguments of tab_exp per side."""
    out = {}
    for by, name in (("cell", "theta"), ("gene", "beta")):
        shape, rate = eng.get_gamma(name)
        out[by] = check_side(shape, rate, eng._debug_tables(by), K, eng.dtype, "%s %s" % (label, name))
    return out


# psi(SLIVER_SHAPE) = psi(5) - 745.07: beside entries of shape 5 at the same rate its shifted argument lies in the middle
# of (-1075 ln 2, -745] = (-745.1332, -745], where exp(d) = 0.53 * 2**-1074 rounds to the smallest denormal.  The middle
# is 0.06 from either end; the rounding of the shape and of tab_log to float32 moves d by less than 1e-4.
SLIVER_SHAPE = brentq(lambda s: digamma(s) - (digamma(5.0) - 745.07), 1e-3, 2e-3, xtol=1e-15)


def extreme_state(n, K, dtype, seed):
    """Shapes log-uniform over [1e-4, 1e7] with a few at 1e8 and 3e9 (the branch without the shift), rates over
    [1e-6, 1e8]; row 0 alternates shapes 1e-4 and 5 at rate 1: psi(1e-4) ~ -1e4, so its small entries lie thousands below
    the row's maximum and their tab_exp must be 0; row 1 is SLIVER_SHAPE beside shapes of 5."""
    rng = np.random.RandomState(seed)
    shape = np.exp(rng.uniform(np.log(1e-4), np.log(1e7), (n, K)))
    rate = np.exp(rng.uniform(np.log(1e-6), np.log(1e8), (n, K)))
    big = rng.choice(n * K, min(6, n * K), replace=False)
    shape.flat[big] = np.resize([1e8, 3e9], big.size)
    if K >= 2:
        shape[0, 0::2], shape[0, 1::2], rate[0] = 1e-4, 5.0, 1.0
        if n >= 2:      # row 1: entry 0 lands in the sliver where exp(d) is the smallest float64 denormal, not yet 0
            shape[1], rate[1], shape[1, 0] = 5.0, 1.0, SLIVER_SHAPE
    shape = shape.astype(dtype)
    shape[shape < 1e-4] = np.nextafter(dtype(1e-4), dtype(1))     # float32(1e-4) lies below 1e-4
    return shape, rate.astype(dtype)


def refreshed(amd, N, G, K, dtype, seed):
    """An engine without a matrix whose theta and beta are extreme_state: the tables come from refresh_tables()."""
    eng = amd.DeviceCAVI(N, G, K, dtype=dtype)
    eng.set_gamma("theta", *extreme_state(N, K, dtype, seed))
    eng.set_gamma("beta", *extreme_state(G, K, dtype, seed + 1))
    return eng


KS = [1, 13, 14, 19, 20, 50, 64, 65, 100, 256]
# K = 256 on the plan / dtype pairs tests/test_engine_gpu.py test_largest_supported_number_of_factors runs
REFRESH = [(plan, dtype, K) for plan in ("tile", "gather") for dtype in (np.float64, np.float32) for K in KS
           if K < 256 or (plan, dtype) != ("tile", np.float64)]


@pytest.mark.parametrize("plan_kind,dtype,K", REFRESH, indirect=["plan_kind"])
def test_refresh_at_extreme_state(amd, plan_kind, dtype, K):
    N, G = 150, 97
    rb = rows_per_block(K)
    # 97 is prime: the gene side always ends in a partly filled group of rows; so does the cell side, except at
    # K = 50, 65 and 100 (rows_per_block 5, 3, 2)
    assert rb == 1 or G % rb
    assert rb == 1 or N % rb or K in (50, 65, 100)
    with refreshed(amd, N, G, K, dtype, seed=K) as eng:
        d = check_tables(eng, K, "%s/K%d/%s" % (plan_kind, K, np.dtype(dtype).name))
        if K >= 2:      # rows that span more than 745 in tab_log, and the alternating row 0
            for by in ("cell", "gene"):
                assert (d[by] <= -745.0).any() and (d[by][0, 0::2] < -5000).all()
                x = eng._debug_tables(by)["exp"]
                assert_array_equal(x[0, 0:K:2], 0.0)
                assert (x[0, 1:K:2] > 0.99).all()
                # row 1: d in (-745.1332, -745], where the float64 table holds the smallest denormal and not 0
                assert ZERO_BELOW + 0.05 < d[by][1, 0] < -745.05 and (d[by][1, 1:] > -1e-6).all()
                assert x[1, 0] == (5e-324 if np.dtype(dtype) == F64 else 0.0)


@only_plans("tile")
@pytest.mark.parametrize("dtype,K", [(np.float64, 20), (np.float32, 50)])
def test_fewer_rows_than_a_block(amd, plan_kind, dtype, K):
    N, G = 3, 2
    assert N < rows_per_block(K)
    with refreshed(amd, N, G, K, dtype, seed=7) as eng:
        check_tables(eng, K, "3x2/K%d/%s" % (K, np.dtype(dtype).name))


@only_plans("tile")
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K,N", [(20, 24589), (50, 10246)])
def test_second_trip_of_the_group_loop(amd, plan_kind, K, N, dtype):
    """More than 2048 groups of rows_per_block rows: the grid is capped at 2048 blocks (capi.hip UPD_BLOCKS), block 0
    takes groups 0 and 2048, and the last group holds a single row.  K = 20: rows inside a wavefront; K = 50: block-wide.
    All rows are compared: the first group, the last, partial one, and everything between."""
    rb = rows_per_block(K)
    assert N == 2048 * rb + rb + 1
    with refreshed(amd, N, 3, K, dtype, seed=K) as eng:
        check_tables(eng, K, "second trip/K%d/%s" % (K, np.dtype(dtype).name))


def mild_state(N, G, K, dtype, seed):
    rng = np.random.RandomState(seed)
    g = lambda *d: (rng.uniform(0.2, 3.0, d).astype(dtype), rng.uniform(0.5, 2.0, d).astype(dtype))  # noqa: E731
    return {"xi": g(N), "theta": g(N, K), "eta": g(G), "beta": g(G, K)}


def engine_with(amd, X, K, dtype, st):
    eng = amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=dtype)
    eng.upload(X, warn=False)
    eng.set_hypers(0.3, 0.3, 1.3, 0.8)
    for name in ("xi", "theta", "eta", "beta"):
        eng.set_gamma(name, *st[name])
    return eng


def random_phi(X, K, seed):
    return np.random.RandomState(seed).dirichlet(np.ones(K), X.nnz) * np.asarray(X.data, np.float64)[:, None]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", [13, 20, 50, 64])
@pytest.mark.parametrize("init", ["state", "phi"])
@pytest.mark.parametrize("order", ["fused", "simultaneous"])
def test_tables_after_a_step(amd, plan_kind, order, init, K, dtype):
    """One iteration -- from the state set with set_gamma, or with init_phi_host's dense sums -- in the default order
    (the update kernels sum the other side's block partials themselves) and with simultaneous=True (they do not); then
    the tables the kernel wrote beside the new shape and rate against that shape and rate."""
    X = synthetic_counts(150, 97, 0.1, seed=K)
    with engine_with(amd, X, K, dtype, mild_state(150, 97, K, dtype, seed=K + 1)) as eng:
        if init == "phi":
            eng.init_phi_host(random_phi(X, K, seed=K + 2))
        eng.step(simultaneous=(order == "simultaneous"))
        check_tables(eng, K, "%s/%s/%s/K%d/%s" % (plan_kind, order, init, K, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_other_side_with_many_update_blocks(amd, plan_kind, dtype):
    """1 100 cells at K = 20 are 92 update blocks, more than 7 * rows_per_block = 84: the gene update's fused column sums
    of E[theta] run the eight-way unrolled loop over the cell side's block partials, not only its tail.  The tables
    cannot see a wrong sum (they follow the rate the kernel stored), so the rates themselves are checked too:
    rate = E[capacity] + sum over the other side of shape / rate.  Bound, relative: a sum of n positive terms in any order
    is within n * 2**-53 of the exact one, and its terms and E[capacity] (a Newton reciprocal and a product each, 3.1 *
    2**-53) and the last addition fit another n * 2**-53 + 4 * 2**-53 [float32: + 2**-24 for the table entries that are
    summed, + 2**-24 for the stored rate]."""
    N, G, K = 1100, 97, 20
    assert -(-N // rows_per_block(K)) > 7 * rows_per_block(K)
    X = synthetic_counts(N, G, 0.1, seed=3)
    st = mild_state(N, G, K, dtype, seed=4)
    with engine_with(amd, X, K, dtype, st) as eng:
        eng.step()
        check_tables(eng, K, "%s/1100 cells/%s" % (plan_kind, np.dtype(dtype).name))
        new = {n: eng.get_gamma(n) for n in ("theta", "beta")}
    ratio = lambda sr: sr[0].astype(LD) / sr[1].astype(LD)  # noqa: E731
    cast = 0.0 if np.dtype(dtype) == F64 else 2.0 ** -23
    # beta from the OLD theta, theta from the NEW beta (scHPF_.py:697-714); capacities from the old xi / eta rates
    for name, cap, other, n_other in (("beta", "eta", st["theta"], N), ("theta", "xi", new["beta"], G)):
        want = ratio(st[cap])[:, None] + ratio(other).sum(axis=0)[None, :]
        err = np.abs(new[name][1].astype(LD) - want) / want
        print("%s rate %s: largest relative error %.3g" % (name, np.dtype(dtype).name, err.max()))
        assert err.max() <= 2 * n_other * 2.0 ** -53 + 4 * 2.0 ** -53 + cast, name


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reading_the_tables_changes_nothing(amd, plan_kind, dtype):
    """set state, [tables], step, [tables], step: every Gamma and the loss bit for bit as without the reads -- the first
    read rebuilds stale tables as the step after it would have, the second finds them fresh."""
    K = 20
    X = synthetic_counts(150, 97, 0.1, seed=11)
    st = mild_state(150, 97, K, dtype, seed=12)
    finals = []
    for probe in (False, True):
        with engine_with(amd, X, K, dtype, st) as eng:
            for _ in range(2):
                if probe:
                    first = {by: eng._debug_tables(by) for by in ("cell", "gene")}
                    for by in ("cell", "gene"):              # two reads, the same bits
                        for k, t in eng._debug_tables(by).items():
                            assert_array_equal(t, first[by][k])
                eng.step()
            finals.append(({n: eng.get_gamma(n) for n in ("xi", "theta", "eta", "beta")}, eng.loss_terms()))
    for name in ("xi", "theta", "eta", "beta"):
        for a, b in zip(finals[0][0][name], finals[1][0][name]):
            assert_array_equal(a, b, err_msg=name)
    assert finals[0][1] == finals[1][1]


@only_plans("tile")
def test_python_surface(amd, plan_kind):
    from schpf_amd import _lib
    with refreshed(amd, 5, 4, 3, np.float64, seed=1) as eng:
        with pytest.raises(ValueError):
            eng._debug_tables("theta")
        import ctypes
        assert eng._lib.schpf_debug_tables(eng._h, _lib.BY_GENE, None, None, None) == 0      # any pointer may be NULL
        only = np.empty((5, eng.plan_info()["KP"]))
        assert eng._lib.schpf_debug_tables(eng._h, _lib.BY_CELL, None, only.ctypes.data_as(ctypes.c_void_p), None) == 0
        assert_array_equal(only, eng._debug_tables("cell")["log"])
        assert eng._lib.schpf_debug_tables(eng._h, 2, None, None, None) != 0
        assert b"SCHPF_BY_CELL" in eng._lib.schpf_last_error()


@only_plans("gather")
def test_zz_report_largest_scaled_errors(plan_kind):
    """Not a check of its own: the largest table errors the tests above saw, as a fraction of the bound and in the
    bound's unit (tab_e: relative; tab_log: over max(1, |psi|, |log rate|); tab_exp: relative, normal results)."""
    print("largest table errors, fraction of the bound (in the bound's unit): " + ", ".join(
        "tab_%s %s %.3g (%.3g)" % (t, dt, w[0], w[1]) for (t, dt), w in sorted(WORST.items())))
    for key, w in WORST.items():
        assert w[0] <= 1.0, key
