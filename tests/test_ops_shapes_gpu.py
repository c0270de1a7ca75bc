"""The stateless operator mirrors (schpf_amd.hpf_hip -> ops.hip -> the "stateless operator mirrors" kernels of
kernels.hip) at every number of factors that changes a thread layout, at the grid cap of ratio_colsum_kernel, at block
edges and at states where the max-shift of the softmax matters -- element by element against the longdouble references
of tests/_ops_reference.py, inside the bounds derived there, and bit for bit where the inputs make every sum exact.
tests/test_ops_host.py shows without a device that the bounds are neither vacuous nor met by roundings alone.

What runs where (K = number of factors, rb = 256 // K rows per block of ratio_colsum_kernel):
  test_every_thread_layout      K in LAYOUT_KS: divisors of 256 (1, 2, 64, 128, 256: no idle thread), K that leave
                                256 - rb K threads idle (3, 7, 20, 50, 65, 100), rb = 1 (129, 255, 256); 193 x 217 with
                                3000 unsorted, partly repeated entries: n K straddles 256-thread blocks on both axes
  test_beyond_256_factors       K = 300 on the four operators without an upper limit; the rate update refuses it
  test_second_trip_*            m > 512 rb: blocks take a second group of rows, all 512 partials per factor are live in
                                colsum_reduce_kernel
  test_shape_update_exact_sums  a row of 5000 entries, rows without entries, n K in {255, 256, 257, 259}
  test_capacity_rate_exact      every K above
"""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _ops_reference as ref
from conftest import load_golden, synthetic_counts

pytestmark = pytest.mark.gpu

LD = ref.LD
DTYPES = [np.float64, np.float32]
WORST = {}     # (operator, dtype name) -> [largest error / bound, where]


@pytest.fixture(scope="module")
def hip():
    from schpf_amd import hpf_hip, _lib
    _lib.require_gpu()
    return hpf_hip


def hold(op, tag, got, want, bound, dt):
    """Every element of got within its bound of want; records and prints the largest fraction."""
    got = np.asarray(got)
    assert got.shape == want.shape, (op, tag, got.shape, want.shape)
    if op != "xphi_rowsum":
        assert got.dtype == np.dtype(dt), (op, tag, got.dtype)
    err = np.abs(got.astype(LD) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    worst = float(frac.max()) if frac.size else 0.0
    print("%s %s: largest error %.3g of its bound" % (op, tag, worst))
    assert np.isfinite(got).all(), "%s %s: %d outputs are not finite" % (op, tag, (~np.isfinite(got)).sum())
    assert (err <= bound).all(), "%s %s: %.3g of the bound at %s" % (
        op, tag, worst, np.unravel_index(np.argmax(frac), frac.shape))
    w = WORST.setdefault((op, np.dtype(dt).name), [0.0, ""])
    if worst > w[0]:
        w[0], w[1] = worst, tag


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_same_bits(got, want, msg=""):
    assert got.dtype == want.dtype and got.shape == want.shape, msg
    assert_array_equal(bits(got), bits(want), err_msg=msg)


# ------------------------------------------------------------------------------------------- every thread layout
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("state", ref.STATES)
@pytest.mark.parametrize("K", ref.LAYOUT_KS)
def test_every_thread_layout(hip, K, state, dtype):
    """All five operators on both axes; every element against its bound."""
    ops = []
    for op, tag, got, want, bound in ref.operator_checks(ref.problem(K, dtype, state), hip):
        hold(op, tag, got, want, bound, dtype)
        ops.append(op)
    assert ops == ["xphi", "xphi_rowsum", "llh"] + 2 * ["shape_update"] + 2 * ["rate_update"] + 2 * ["capacity_rate"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("state", ref.STATES)
def test_beyond_256_factors(hip, state, dtype):
    """K = 300: xphi, llh, the shape update and the capacity update loop over K and take it; the rate update's column
    sums deal 256 threads out over K factors and refuse it."""
    p = ref.problem(ref.BIG_K, dtype, state)
    ops = []
    for op, tag, got, want, bound in ref.operator_checks(p, hip):
        hold(op, tag, got, want, bound, dtype)
        ops.append(op)
    assert ops == ["xphi", "xphi_rowsum", "llh"] + 2 * ["shape_update"] + 2 * ["capacity_rate"]
    with pytest.raises(ValueError, match=r"nfactors must be in \[1, 256\]"):
        hip.compute_loading_rate_update(p["xi_s"], p["xi_r"], p["bes"], p["ber"])


# ----------------------------------------------------------------------- the second trip of ratio_colsum_kernel
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,m", ref.SECOND_TRIP)
def test_second_trip_exact(hip, K, m, dtype):
    """exact_state: every quotient is a multiple of 1/4 below 64 and every partial sum of them is exact in double, so the
    output is the exact rational sum rounded once to T, whatever the order -- bit for bit."""
    rb = 256 // K
    assert m > 512 * rb and m % (512 * rb)
    ps, pr, s, r = ref.second_trip_problem(K, m, dtype, "exact")
    want = ref.rate_update(ps, pr, s, r)[0]
    assert (want == want.astype(np.float64)).all()            # a multiple of 1/4 below 2**23: no rounding in the reference
    got = hip.compute_loading_rate_update(ps, pr, s, r)
    assert_same_bits(got, want.astype(dtype), "K=%d m=%d" % (K, m))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,m", ref.SECOND_TRIP)
def test_second_trip_mild(hip, K, m, dtype):
    a = ref.second_trip_problem(K, m, dtype, "mild")
    want, bound = ref.rate_update(*a)
    hold("rate_update", "K%d/m%d/%s/mild" % (K, m, np.dtype(dtype).name), hip.compute_loading_rate_update(*a),
         want, bound, dtype)


# ------------------------------------------------------------------------------------------ exact sums elsewhere
def _exact_shape_case(n, K, nnz, big_row, order, rng):
    """Integer entries 0...7 for n rows of which every third has none and big_row holds 5000."""
    allowed = np.array([r for r in range(n) if r % 3 != 1 or r == big_row], np.int32)
    keep = np.concatenate([rng.choice(allowed, nnz).astype(np.int32), np.full(5000, big_row, np.int32)])
    if order == "sorted":
        keep = np.sort(keep)
    elif order == "reversed":
        keep = np.sort(keep)[::-1].copy()
    else:
        keep = rng.permutation(keep)
    return keep, rng.randint(0, 8, (keep.size, K))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ["sorted", "reversed", "random"])
@pytest.mark.parametrize("n,K", [(85, 3), (255, 1), (128, 2), (256, 1), (257, 1), (37, 7), (1, 300)])
def test_shape_update_exact_sums(hip, n, K, order, dtype):
    """n K in {255, 256, 257, 259} (and 300 factors of a single row): the last block of shape_update_kernel is full, one
    short, one or three over.  Entries 0...7 on a prior of 0.25: every partial sum is a multiple of 1/4 below 2**16."""
    assert n * K in (255, 256, 257, 259, 300)
    rng = np.random.RandomState(n * K)
    big = n // 2
    keep, vals = _exact_shape_case(n, K, 600, big, order, rng)
    vals[np.nonzero(keep == big)[0][-1]] = 7      # the long row's last entry in position order counts
    counts = np.bincount(keep, minlength=n)
    assert counts[big] >= 5000 and (n < 3 or (counts == 0).any())
    want = np.full((n, K), 0.25)
    np.add.at(want, keep, vals.astype(np.float64))
    assert want.max() < 2 ** 16
    got = hip.compute_loading_shape_update(vals.astype(dtype), keep, n, 0.25)
    assert_same_bits(got, want.astype(dtype), "n=%d K=%d %s" % (n, K, order))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", ref.LAYOUT_KS + [ref.BIG_K])
def test_capacity_rate_exact(hip, K, dtype):
    """exact_state on a prior of 0.25, 515 rows (three blocks, the last with three rows): a multiple of 1/4 below
    0.25 + 60 K < 2**15 at every partial sum, exact in float32."""
    s, r = ref.exact_state(515, K, dtype, np.random.RandomState(K))
    want = 0.25 + (s.astype(np.float64) / r.astype(np.float64)).sum(axis=1)
    got = hip.compute_capacity_rate_update(s, r, 0.25)
    assert_same_bits(got, want.astype(dtype), "K=%d" % K)


# --------------------------------------------------------------------------------------------------- block edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nnz", [1, 255, 256, 257, 513])
def test_coo_block_edges(hip, nnz, dtype):
    p = ref.problem(7, dtype, "mild", n_cells=40, n_genes=30, nnz=nnz)
    tag = "nnz%d/%s" % (nnz, np.dtype(dtype).name)
    want, bound, rs_bound, _ = ref.xphi(*ref.coo_args(p))
    got = hip.compute_Xphi_data(*ref.coo_args(p))
    assert got.shape == (nnz, 7)
    hold("xphi", tag, got, want, bound, dtype)
    hold("xphi_rowsum", tag, got.astype(LD).sum(axis=1), p["x"].astype(LD), rs_bound, dtype)
    want, bound, _ = ref.llh(*ref.coo_args(p))
    got = hip.compute_pois_llh(*ref.coo_args(p))
    assert got.shape == (nnz,)
    hold("llh", tag, got, want, bound, dtype)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_special_block_edges(hip, n):
    """psi / cgammaln on n points of psi_gammaln.npz, the tolerances of tests/test_ops_gpu.py; the array's shape comes
    back, a scalar gives a float."""
    g = load_golden("psi_gammaln.npz")
    idx = np.linspace(0, len(g["x"]) - 1, n).astype(int)
    x = g["x"][idx]
    for fn, key, tol in ((hip.psi, "psi", 4e-15), (hip.cgammaln, "gammaln", 5e-15)):
        got = fn(x)
        assert isinstance(got, np.ndarray) and got.shape == (n,) and got.dtype == np.float64
        np.testing.assert_allclose(got, g[key][idx], rtol=tol, atol=tol)
        if n in (256, 0):
            two = fn(x.reshape(2, n // 2))
            assert two.shape == (2, n // 2)
            assert_array_equal(two.ravel(), got)
        if n == 1:
            one = fn(float(x[0]))
            assert type(one) is float and one == got[0]
            zero_d = fn(np.float64(x[0]))
            assert type(zero_d) is float and zero_d == got[0]


# ------------------------------------------------------------------------------------------- max-shift structure
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 2, 3, 7, 50, 256])
def test_max_shift_structure(hip, K, dtype):
    """extreme_state: E[log] spans thousands inside a row.  Every output is finite, every row of X * phi sums to x, and at
    (0, 0), where both sides alternate shape 1e-4 and 5 at rate 1, the small-shape factors are exactly 0 (they lie 2e4
    below the maximum) and the others carry x / (number of large factors)."""
    p = ref.problem(K, dtype, "extreme")
    tag = "structure/K%d/%s" % (K, np.dtype(dtype).name)
    got = hip.compute_Xphi_data(*ref.coo_args(p))
    assert np.isfinite(got).all() and (got >= 0).all()
    want, bound, rs_bound, _ = ref.xphi(*ref.coo_args(p))
    hold("xphi_rowsum", tag, got.astype(LD).sum(axis=1), p["x"].astype(LD), rs_bound, dtype)
    at00 = np.nonzero((p["row"] == 0) & (p["col"] == 0))[0]
    assert at00.size >= 4
    if K >= 2:
        assert not bits(got[at00][:, 0::2]).any(), "the small-shape factors of (0, 0) are not +0"
        n_large = K // 2
        share = p["x"][at00].astype(LD)[:, None] / n_large
        err = np.abs(got[at00][:, 1::2].astype(LD) - share)
        assert (np.abs(want[at00][:, 1::2] - share) <= 4 * ref.unit(dtype) * share).all()      # the reference agrees
        assert (err <= bound[at00][:, 1::2] + 4 * ref.unit(dtype) * share).all()
    else:
        assert_array_equal(got[:, 0], p["x"].astype(dtype))
    # one-hot rows: where the reference's phi is 0 (beyond exp's range even in longdouble) so is the device's
    dead = want == 0
    assert dead.any() or K == 1
    assert not bits(got)[dead].any()
    llh = hip.compute_pois_llh(*ref.coo_args(p))
    assert np.isfinite(llh).all()


# ------------------------------------------------------------------------------ stored zeros and large counts
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("state", ref.STATES + ("exact",))
@pytest.mark.parametrize("K", [1, 7, 50])
def test_llh_stored_zeros_and_large_counts(hip, K, state, dtype):
    """A stored x = 0 gives exactly -T(r): 0 * log r = 0 and lgamma(1) = 0, so the result is -(r summed in T), and
    counts up to 999 999 (x + 1 within the range lgamma is held to) stay inside the general bound.
    Where r's bits are known the zeros are compared bit for bit:
      K = 1, every state: r is one product of two correctly rounded quotients, rounded once -- the same with or
          without an fma;
      exact_state, every K: the quotients are multiples of 1/4 below 64, their products multiples of 1/16 below 4096 and
          every partial sum of 50 of them a multiple of 1/16 below 2**18: r is exact in float32 in any order, contracted
          or not.
    For K > 1 on the mild and extreme states the compiler may contract r += E_t E_b into one fma (the build sets no
    -ffp-contract), so r's bits are not predicted; there the zeros are held to r's own (K + 2) u alone -- without the
    log's, lgamma's or the store's share of the general bound."""
    p = ref.problem(K, dtype, state)
    x = p["x"].copy()
    x[0::3] = 0
    x[1::3] = np.random.RandomState(K).randint(1000, 1000000, x[1::3].size)
    x[1], x[4] = 999999, 999998
    args = (x,) + ref.coo_args(p)[1:]
    tag = "K%d/%s/%s" % (K, np.dtype(dtype).name, state)
    got = hip.compute_pois_llh(*args)
    want, bound, r = ref.llh(*args)
    hold("llh", "counts/" + tag, got, want, bound, dtype)
    hold("llh_zero", tag, got[0::3], -r[0::3], (K + 2) * ref.unit(dtype) * r[0::3], dtype)
    assert (got[0::3] < 0).all()
    if K == 1 or state == "exact":
        r_T = ((p["ths"] / p["thr"])[p["row"]] * (p["bes"] / p["ber"])[p["col"]]).sum(axis=1, dtype=dtype)   # in T
        assert r_T.dtype == np.dtype(dtype)
        if state == "exact":
            assert (r_T.astype(LD) == r).all()         # no rounding anywhere
        assert_same_bits(got[0::3], -r_T[0::3], "x = 0 is not -T(r): " + tag)
    # and the zeros do not depend on their neighbours' counts
    assert_same_bits(hip.compute_pois_llh(np.zeros_like(x), *args[1:])[0::3], got[0::3])


# ------------------------------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [7, 100, 256])
def test_every_operator_repeats_its_bits(hip, K, dtype):
    p = ref.problem(K, dtype, "mild")
    runs = []
    for _ in range(2):
        xphi = hip.compute_Xphi_data(*ref.coo_args(p))
        runs.append([xphi, hip.compute_pois_llh(*ref.coo_args(p)),
                     hip.compute_loading_shape_update(xphi, p["row"], p["N"], 0.3),
                     hip.compute_loading_shape_update(xphi, p["col"], p["G"], 0.3),
                     hip.compute_loading_rate_update(p["xi_s"], p["xi_r"], p["bes"], p["ber"]),
                     hip.compute_loading_rate_update(p["eta_s"], p["eta_r"], p["ths"], p["thr"]),
                     hip.compute_capacity_rate_update(p["ths"], p["thr"], 0.3),
                     hip.compute_capacity_rate_update(p["bes"], p["ber"], 0.3),
                     hip.psi(p["ths"].astype(np.float64)), hip.cgammaln(p["ths"].astype(np.float64))])
    for a, b in zip(*runs):
        assert_same_bits(a, b)
    a = ref.second_trip_problem(7, 18469, dtype, "mild")           # all 512 partials live
    assert_same_bits(hip.compute_loading_rate_update(*a), hip.compute_loading_rate_update(*a))


# --------------------------------------------------------------------------------------- no trace on a live engine
@pytest.mark.parametrize("dtype", DTYPES)
def test_operators_leave_no_trace_on_a_live_engine(hip, dtype):
    """step, step against step, <all five operators and the special functions>, step on the 150 x 97 matrix of
    tests/test_update_tables_gpu.py: the operators work on streams and buffers of their own, so every Gamma and the
    loss terms are the same bits."""
    import schpf_amd
    K, (N, G) = 20, (150, 97)
    X = synthetic_counts(N, G, 0.1, seed=11)
    rng = np.random.RandomState(12)
    st = {name: (rng.uniform(0.2, 3.0, d).astype(dtype), rng.uniform(0.5, 2.0, d).astype(dtype))
          for name, d in (("xi", N), ("theta", (N, K)), ("eta", G), ("beta", (G, K)))}
    p = ref.problem(K, dtype, "mild")
    finals = []
    for between in (False, True):
        with schpf_amd.DeviceCAVI(N, G, K, dtype=dtype) as eng:
            eng.upload(X, warn=False)
            eng.set_hypers(0.3, 0.3, 1.3, 0.8)
            for name in ("xi", "theta", "eta", "beta"):
                eng.set_gamma(name, *st[name])
            eng.step()
            if between:
                xphi = hip.compute_Xphi_data(*ref.coo_args(p))
                hip.compute_pois_llh(*ref.coo_args(p))
                hip.compute_loading_shape_update(xphi, p["col"], p["G"], 0.3)
                hip.compute_loading_rate_update(p["xi_s"], p["xi_r"], p["bes"], p["ber"])
                hip.compute_capacity_rate_update(p["ths"], p["thr"], 0.3)
                hip.psi(p["ths"].astype(np.float64))
                hip.cgammaln(p["ths"].astype(np.float64))
            eng.step()
            finals.append(({n: eng.get_gamma(n) for n in ("xi", "theta", "eta", "beta")}, eng.loss_terms()))
    for name in ("xi", "theta", "eta", "beta"):
        for a, b in zip(finals[0][0][name], finals[1][0][name]):
            assert_same_bits(a, b, name)
    assert finals[0][1] == finals[1][1]


def test_zz_report_largest_scaled_errors():
    """Not a check of its own: the largest error the tests above saw per operator and dtype, as a fraction of its bound."""
    print("largest operator errors, fraction of the bound: " + ", ".join(
        "%s %s %.3g (%s)" % (op, dt, w[0], w[1]) for (op, dt), w in sorted(WORST.items())))
    for key, w in WORST.items():
        assert w[0] <= 1.0, key
