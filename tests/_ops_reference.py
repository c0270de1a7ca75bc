"""Yardstick of the stateless operator mirrors (schpf_amd.hpf_hip; kernels.hip "stateless operator mirrors", ops.hip):
plain NumPy references in longdouble, the error bound of every operator, a NumPy emulation in dtype T of each kernel's
operation order, and the inputs.  Nothing here calls the device: tests/test_ops_host.py holds the references to the
golden vectors and the oracle and the emulations to the bounds, tests/test_ops_shapes_gpu.py holds the kernels to both.

Everything is computed from the shape and rate arrays AS GIVEN in dtype T (T = float64 or float32).
scipy.special.digamma and gammaln in float64 are taken as exact, as tests/test_update_tables_gpu.py does.
u = 2**-53 (float64) or 2**-24 (float32) is T's unit roundoff; cast = 0 (float64) or u (float32) is the rounding of a
value computed in double when it is stored in T.  A bound is first order in u; the emulations below must stay under
0.9 of it (tests/test_ops_host.py), which is also the room left for the second-order terms.

xphi (xphi_coo_kernel).  elt = psi(shape) - log(rate) per row and factor, computed in double and stored in T, the same
  for elb; s = max(1, |psi|, |log rate|).  v_k = elt_k + elb_k and v_k - mx are formed in T.  The argument of the
  exponential is therefore off by at most
      d_k = 5e-15 (s_t + s_b) + cast (|elt_k| + |elb_k|) + u (|v_k| + |v_k - mx|):
  digamma's 4e-15 (special.h) plus libm's log within 2 ulp, both relative to s, make the 5e-15 term; the two stores in
  T make the cast term; the sum and the difference in T make the u term.  With D = max_k d_k the kernel's maximum is
  within D of the true one, every e_k = exp(v_k - mx) is off by a factor within exp(+-(d_k + D)) and their sum by a
  factor within exp(+-2D); exp itself, its store in T, the K - 1 additions of the norm, the product, the quotient and
  the last store are K + 4 roundings.  So
      |got - want| <= (2 D + d_k + (K + 4) u) want exp(2 D) + (x + 1) / 2 smallest_subnormal(T).
  The last term is for T's denormal range, where a rounding is absolute: an e_k stored there is off by half a spacing,
  which x / norm (norm >= 1: the largest e_k is 1) scales to at most x / 2 spacings, and the result stored there is off
  by another half.  For counts x >= 1 that is at most x smallest_subnormal(T).  Roundings alone meet this term: a
  result in the denormal range lies on a grid and can sit the full (x + 1) / 2 spacings from the truth (the emulation:
  0.915 spacings at x = 1 on a float64 result of 3.8e-316, K = 255, extreme_state), so the rule that an emulation uses
  at most 0.9 of a bound is asked of the results in T's normal range, and the bound itself, 1.0, of the denormal ones
  (tests/test_ops_host.py) -- as tab_exp in tests/test_update_tables_gpu.py sits at 1.0 of its half spacing.
  Row sums.  sum_k got_k = x sum_k e_k / norm times one factor per entry for the product, the quotient and the store,
  with the SAME e_k above and below: D does not enter.  norm is the sum in T of K positive terms, within (K - 1) u of
  sum_k e_k; product and quotient are in double (2 * 2**-53 <= u) and the store is cast: three roundings of at most u
  between them in either dtype.  With half a denormal spacing per entry:
      |sum_k got_k - x| <= (K + 2) u x + K smallest_subnormal(T).

llh (llh_coo_kernel).  E = shape / rate is a correctly rounded quotient in T (ratio_kernel); r = sum_k E_t E_b in T: two
  quotients, a product and at most K - 1 additions per term, all terms positive, so r is within (K + 2) u relative.
  x log r - r - lgamma(x + 1) is formed in double and stored in T:
      |got - want| <= (K + 3) u (|x log r| + r) + 2**-52 |x log r| + 5e-15 max(1, lgamma(x + 1)) + cast |want|
                      + (K + 2) u x.
  The first four terms: r's own error and the roundings of the two products and differences, libm's
  log within 2 ulp of log r, lgamma within the tolerance tests/test_ops_gpu.py test_digamma_gammaln_vs_scipy_values
  enforces on psi_gammaln.npz (which spans [1e-4, 1e6]: keep x + 1 <= 1e6), the store.  The last term:
  d(x log r) = x dr / r, and dr / r is the (K + 2) u above whatever log r is -- (K + 3) u |x log r|
  covers it only where |log r| >= 1, and on mild_state at small K r lies around 1 (the emulation reaches 1.19 of the
  bound without the term at K = 1 in float32).

shape_update (shape_update_kernel).  T(prior) plus the row's n_r entries one after the other in T, in input position
  order (the counting sort of ops.hip is stable): n_r additions and the cast of the prior,
      |got - want| <= (n_r + 1) u (prior + sum |terms|).

rate_update (ratio_colsum_kernel, colsum_reduce_kernel, rate_update_kernel).  Correctly rounded quotients in T (u
  each), all positive, summed in double over the m rows in some order (m * 2**-53 relative), one more quotient, one more
  addition in double and one cast.  tests/test_update_tables_gpu.py test_other_side_with_many_update_blocks uses the
  same form:
      |got - want| <= (2 m 2**-53 + 4 u) want.

capacity_rate (capacity_rate_kernel).  T(prior) plus K quotients in T added one after the other in T, all positive: the
  cast, K quotients and K additions,
      |got - want| <= (2 K + 2) u want.

On exact_state no rounding happens at all and the tests ask for the exact value bit for bit: shapes are integers
1...15, rates powers of two in {1/4, ..., 4}, so every quotient is a multiple of 1/4 below 64, exact in float32; a sum
of m <= 131 075 of them is a multiple of 1/4 below 2**23, exact in double at every partial sum in any order; the sum of
K <= 300 of them on top of 0.25 is a multiple of 1/4 below 2**15, exact in float32 at every partial sum.
"""
import numpy as np
from scipy.special import digamma, gammaln

LD = np.longdouble
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
SPECIAL = 5e-15          # digamma's 4e-15 (special.h) + libm's log; also the lgamma tolerance of test_ops_gpu.py

N_CELLS, N_GENES, N_ENTRIES = 193, 217, 3000
# every K that changes ratio_colsum_kernel's thread layout: divisors of 256, K that leave idle threads, rb = 1
LAYOUT_KS = [1, 2, 3, 7, 20, 50, 64, 65, 100, 128, 129, 255, 256]
BIG_K = 300              # beyond the rate update's limit: the four operators that loop over K
# (K, m) with m > 512 * (256 // K) and no multiple of it: blocks of ratio_colsum_kernel take a second group of rows
SECOND_TRIP = [(256, 1031), (129, 700), (50, 5123), (7, 18469), (1, 131075)]
STATES = ("mild", "extreme")


def unit(dtype):
    return LD(2.0) ** (-53 if np.dtype(dtype) == F64 else -24)


def cast_unit(dtype):
    return LD(0) if np.dtype(dtype) == F64 else unit(dtype)


def tiny(dtype):
    return LD(np.finfo(np.dtype(dtype)).smallest_subnormal)


# ------------------------------------------------------------------------------------------------------- inputs
def mild_state(n, K, dtype, rng):
    """The seeded case of tests/test_ops_gpu.py: shape U[0.15, 3], rate U[0.1, 2]."""
    return rng.uniform(0.15, 3.0, (n, K)).astype(dtype), rng.uniform(0.1, 2.0, (n, K)).astype(dtype)


def extreme_state(n, K, dtype, rng):
    """Shapes log-uniform on [1e-4, 1e6] (the certified domain of special.h's digamma), rates log-uniform on
    [1e-6, 1e8]; row 0 alternates shape 1e-4 and 5 at rate 1: psi(1e-4) ~ -1e4, so where both sides are row 0 the small
    factors lie 2e4 below the maximum."""
    dtype = np.dtype(dtype).type
    shape = np.exp(rng.uniform(np.log(1e-4), np.log(1e6), (n, K)))
    rate = np.exp(rng.uniform(np.log(1e-6), np.log(1e8), (n, K)))
    shape[0, 0::2], shape[0, 1::2], rate[0] = 1e-4, 5.0, 1.0
    shape = shape.astype(dtype)
    shape[shape < 1e-4] = np.nextafter(dtype(1e-4), dtype(1))     # float32(1e-4) lies below 1e-4
    return shape, rate.astype(dtype)


def exact_state(n, K, dtype, rng):
    """Integer shapes 1...15 over rates in {1/4, 1/2, 1, 2, 4}: every quotient and every sum of them is exact."""
    return (rng.randint(1, 16, (n, K)).astype(dtype),
            np.ldexp(1.0, rng.randint(-2, 3, (n, K))).astype(dtype))


STATE = {"mild": mild_state, "extreme": extreme_state, "exact": exact_state}
ALL_STATES = ("mild", "extreme", "exact")


def entries(n_rows, n_cols, nnz, rng, hi=50):
    """nnz unsorted entries with repeated coordinates; the first four sit at (0, 0), where extreme_state alternates on
    both sides."""
    row = rng.randint(0, n_rows, nnz).astype(np.int32)
    col = rng.randint(0, n_cols, nnz).astype(np.int32)
    row[:4], col[:4] = 0, 0
    rep = min(50, nnz // 2)
    row[nnz // 2:nnz // 2 + rep] = row[:rep]        # the same coordinates again
    col[nnz // 2:nnz // 2 + rep] = col[:rep]
    return rng.randint(1, hi, nnz).astype(np.int64), row, col


def problem(K, dtype, state, n_cells=N_CELLS, n_genes=N_GENES, nnz=N_ENTRIES):
    """Everything the five operators take on both axes, seeded by (K, state)."""
    rng = np.random.RandomState(1000 * ALL_STATES.index(state) + K)
    x, row, col = entries(n_cells, n_genes, nnz, rng)
    p = dict(K=K, dtype=np.dtype(dtype), state=state, x=x, row=row, col=col, N=n_cells, G=n_genes)
    p["ths"], p["thr"] = STATE[state](n_cells, K, dtype, rng)
    p["bes"], p["ber"] = STATE[state](n_genes, K, dtype, rng)
    for name, n in (("xi", n_cells), ("eta", n_genes)):
        s, r = STATE[state](n, 1, dtype, rng)
        p[name + "_s"], p[name + "_r"] = s[:, 0].copy(), r[:, 0].copy()
    return p


def coo_args(p):
    return p["x"], p["row"], p["col"], p["ths"], p["thr"], p["bes"], p["ber"]


# ---------------------------------------------------------------------------- references (longdouble) and bounds
def _elog(shape, rate):
    psi = digamma(shape.astype(np.float64)).astype(LD)
    lr = np.log(rate.astype(LD))
    return psi - lr, np.maximum(1.0, np.maximum(np.abs(psi), np.abs(lr)))


def xphi(x, row, col, ths, thr, bes, ber):
    """(want, bound, row-sum bound, relative part of the bound) of compute_Xphi_data, each in longdouble."""
    dt = ths.dtype
    K = ths.shape[1]
    u, cast = unit(dt), cast_unit(dt)
    elt, st = _elog(ths, thr)
    elb, sb = _elog(bes, ber)
    elt, elb, st, sb = elt[row], elb[col], st[row], sb[col]
    v = elt + elb
    mx = v.max(axis=1, keepdims=True)
    e = np.exp(v - mx)
    xl = np.asarray(x).astype(LD)[:, None]
    want = xl * e / e.sum(axis=1, keepdims=True)
    d = SPECIAL * (st + sb) + cast * (np.abs(elt) + np.abs(elb)) + u * (np.abs(v) + np.abs(v - mx))
    D = d.max(axis=1, keepdims=True)
    rel = 2 * D + d + (K + 4) * u
    bound = rel * want * np.exp(2 * D) + (xl + 1) / 2 * tiny(dt)
    rowsum_bound = (K + 2) * u * xl[:, 0] + K * tiny(dt)
    return want, bound, rowsum_bound, rel


def llh(x, row, col, ths, thr, bes, ber):
    """(want, bound, r) of compute_pois_llh."""
    dt = ths.dtype
    K = ths.shape[1]
    u, cast = unit(dt), cast_unit(dt)
    r = ((ths.astype(LD) / thr.astype(LD))[row] * (bes.astype(LD) / ber.astype(LD))[col]).sum(axis=1)
    xl = np.asarray(x).astype(LD)
    lg = gammaln(np.asarray(x, np.float64) + 1.0).astype(LD)
    xlr = xl * np.log(r)
    want = xlr - r - lg
    bound = ((K + 3) * u * (np.abs(xlr) + r) + LD(2.0) ** -52 * np.abs(xlr) + SPECIAL * np.maximum(1.0, lg)
             + cast * np.abs(want) + (K + 2) * u * xl)
    return want, bound, r


def shape_update(xphi_data, keep, nkeep, prior):
    """(want, bound) of compute_loading_shape_update."""
    dt = xphi_data.dtype
    K = xphi_data.shape[1]
    t = xphi_data.astype(LD)
    s, a = np.zeros((nkeep, K), LD), np.zeros((nkeep, K), LD)
    np.add.at(s, keep, t)
    np.add.at(a, keep, np.abs(t))
    n_r = np.bincount(keep, minlength=nkeep).astype(LD)[:, None]
    return LD(prior) + s, (n_r + 1) * unit(dt) * (abs(LD(prior)) + a)


def rate_update(ps, pr, os_, or_):
    """(want, bound) of compute_loading_rate_update."""
    dt = os_.dtype
    m = os_.shape[0]
    want = (ps.astype(LD) / pr.astype(LD))[:, None] + (os_.astype(LD) / or_.astype(LD)).sum(axis=0)[None, :]
    return want, (2 * m * LD(2.0) ** -53 + 4 * unit(dt)) * want


def capacity_rate(shape, rate, prior):
    """(want, bound) of compute_capacity_rate_update."""
    dt = shape.dtype
    K = shape.shape[1]
    want = LD(prior) + (shape.astype(LD) / rate.astype(LD)).sum(axis=1)
    return want, (2 * K + 2) * unit(dt) * want


# --------------------------------------------------------------- emulations: the kernels' operation order in T
def emulate_xphi(x, row, col, ths, thr, bes, ber):
    dt = ths.dtype.type
    f = np.float64
    elt = (digamma(ths.astype(f)) - np.log(thr.astype(f))).astype(dt)       # elog_kernel
    elb = (digamma(bes.astype(f)) - np.log(ber.astype(f))).astype(dt)
    v = elt[row] + elb[col]                                                 # in T
    mx = v.max(axis=1, keepdims=True)
    e = np.exp((v - mx).astype(f)).astype(dt)
    norm = np.zeros(len(row), dt)
    for k in range(v.shape[1]):
        norm = norm + e[:, k]
    xv = np.asarray(x).astype(dt).astype(f)[:, None]
    return (xv * e.astype(f) / norm.astype(f)[:, None]).astype(dt)


def emulate_llh(x, row, col, ths, thr, bes, ber):
    dt = ths.dtype.type
    f = np.float64
    et, eb = (ths / thr)[row], (bes / ber)[col]                            # ratio_kernel, in T
    r = np.zeros(len(row), dt)
    for k in range(et.shape[1]):
        r = r + et[:, k] * eb[:, k]
    xv = np.asarray(x).astype(dt).astype(f)
    return (xv * np.log(r.astype(f)) - r.astype(f) - gammaln(xv + 1.0)).astype(dt)


def emulate_shape_update(xphi_data, keep, nkeep, prior):
    dt = xphi_data.dtype.type
    order = np.argsort(keep, kind="stable")                                 # counting_sort_positions
    counts = np.bincount(keep, minlength=nkeep)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    acc = np.full((nkeep, xphi_data.shape[1]), dt(prior), dt)
    for j in range(int(counts.max()) if len(keep) else 0):
        rows = np.nonzero(counts > j)[0]
        acc[rows] = acc[rows] + xphi_data[order[start[rows] + j]]
    return acc


def emulate_rate_update(ps, pr, os_, or_):
    dt = os_.dtype.type
    f = np.float64
    m, K = os_.shape
    rb = 256 // K
    nb = max(1, min(-(-m // rb), 512))
    trips = -(-m // (nb * rb))
    E = np.zeros((trips * nb * rb, K), f)                                   # rows past m add +0.0: no change
    E[:m] = (os_ / or_).astype(f)                                           # the quotient in T, then double
    E = E.reshape(trips, nb, rb, K)
    s = np.zeros((nb, rb, K), f)
    for t in range(trips):
        s = s + E[t]
    part = np.zeros((512, K), f)                                            # blocks past nb add +0.0
    for q in range(rb):
        part[:nb] = part[:nb] + s[:, q]
    red = part[:256] + part[256:]                                           # colsum_reduce_kernel
    half = 128
    while half >= 1:
        red = red[:half] + red[half:2 * half]
        half //= 2
    return ((ps / pr).astype(f)[:, None] + red[0][None, :]).astype(dt)


def emulate_capacity_rate(shape, rate, prior):
    dt = shape.dtype.type
    acc = np.full(shape.shape[0], dt(prior), dt)
    for k in range(shape.shape[1]):
        acc = acc + shape[:, k] / rate[:, k]
    return acc


# ---------------------------------------------------------------------------------------- the checks both files run
PRIOR = 0.3


def operator_checks(p, call):
    """Runs the five operators on both axes of problem p through `call` (a namespace with the seam's five callables or
    the emulations under the same names) and yields (operator, label, got, want, bound) with longdouble want / bound."""
    K, dt = p["K"], p["dtype"]
    tag = "K%d/%s/%s" % (K, dt.name, p["state"])
    want, bound, rs_bound, _ = xphi(*coo_args(p))
    xphi_in = want.astype(dt)       # the shape update's input (any (nnz, K) array of T would do)
    got = call.compute_Xphi_data(*coo_args(p))
    yield "xphi", tag, got, want, bound
    yield "xphi_rowsum", tag, got.astype(LD).sum(axis=1), p["x"].astype(LD), rs_bound
    want, bound, _ = llh(*coo_args(p))
    yield "llh", tag, call.compute_pois_llh(*coo_args(p)), want, bound
    for axis, keep, n in (("cell", p["row"], p["N"]), ("gene", p["col"], p["G"])):
        want, bound = shape_update(xphi_in, keep, n, PRIOR)
        yield "shape_update", tag + "/" + axis, call.compute_loading_shape_update(xphi_in, keep, n, PRIOR), want, bound
    for axis, cap, other in (("cell", "xi", "be"), ("gene", "eta", "th")):
        if K <= 256:
            a = (p[cap + "_s"], p[cap + "_r"], p[other + "s"], p[other + "r"])
            want, bound = rate_update(*a)
            yield "rate_update", tag + "/" + axis, call.compute_loading_rate_update(*a), want, bound
    for axis, name in (("cell", "th"), ("gene", "be")):
        want, bound = capacity_rate(p[name + "s"], p[name + "r"], PRIOR)
        yield ("capacity_rate", tag + "/" + axis,
               call.compute_capacity_rate_update(p[name + "s"], p[name + "r"], PRIOR), want, bound)


class emulation(object):
    """The emulations under the seam's names."""
    compute_Xphi_data = staticmethod(emulate_xphi)
    compute_pois_llh = staticmethod(emulate_llh)
    compute_loading_shape_update = staticmethod(emulate_shape_update)
    compute_loading_rate_update = staticmethod(emulate_rate_update)
    compute_capacity_rate_update = staticmethod(emulate_capacity_rate)


def second_trip_problem(K, m, dtype, state):
    """(prior shape, prior rate, other shape, other rate) of a rate update over m rows; 5 rows of output."""
    rng = np.random.RandomState(m)
    s, r = STATE[state](m, K, dtype, rng)
    ps, pr = STATE[state](5, 1, dtype, rng)
    return ps[:, 0].copy(), pr[:, 0].copy(), s, r


def fraction(got, want, bound):
    """The largest |got - want| / bound; an entry whose bound is 0 must be exact."""
    err = np.abs(np.asarray(got).astype(LD) - want)
    zero = bound == 0
    assert not (err[zero] > 0).any()
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
