"""Yardstick of the phi sweeps' log-domain fallback (sweep_impl.h slow_nonzero, slow_task_row, slow_chunk): the start
state that sends rows there, the classification of its nonzeros, one iteration's theta and beta shape in longdouble, a
bound per element and an emulation in T of both forms and of the hand-over.  Never calls the device:
tests/test_fallback_host.py holds the state to its conditions, the reference to the oracle and the emulations to the
bound; tests/test_fallback_gpu.py holds the kernels to all of it.

The state (start_state).  A case of _sweep_shapes.cases(plan) on its own matrix, with K' = max(K, 2) factors (at K = 1
the normaliser s is 1 and the cold path cannot be reached; K = 2 stays on the pair of K = 1).  The usual start
(oracle.setup_state, seed K'), then theta and beta by row class:
  r % 3 == 0  flat       shape 0.3 and one rate at every factor: every entry of the row's exp table is 1;
  r % 3 == 1  hard       5 at the row's own factors, 1e-4 elsewhere: E[log] ~ -1e4, the products are hard zeros;
  r % 3 == 2  threshold  5 at its own factors, 1/d elsewhere, d = lo + (hi - lo) frac(floor(r / 3) 0.6180339887) over
                         [697, 755] (float64) or [83, 108] (float32): E[log] ~ -d, s around the format's smallest number.
A row's own factors are the 16-byte vectors of factors (2 in float64, 4 in float32; single factors where K' has only
one vector) of the parity of floor(r / 3): two rows share all of them (s is about their number) or none (s = 0 between
hard rows, (K' / 2) exp(-d - 2.1) with a threshold row).  Whole vectors, because a lane of a row's group holds every
LPC-th vector: with LPC >= 2 a row's own factors then sit in some lanes of its group and not in the others, so an
accumulator that overflows (a finite x / s added up) does so in some lanes only and the hand-over has to be agreed on
by the group.  Rates stay as drawn except at own factors
and in flat rows, where the rate is the power of two next to the rate prior that leaves E[log] at least 1e-9 above its
float32 rounding (own_rate): the shift of the exp table is that rounding, so those entries are exp(+gap) >= 1 in float64
and exactly 1 in float32, on the host and -- the gap is a million times digamma's error -- on the device.
Why not the simpler state (one own factor r % K' per row, rates as drawn, class 0 untouched, d over [650, 800] and [70,
120]): it cannot meet the second condition below.  An entry of an exp table is at most exp(half a float32 step of
E[log]), so s >= 1 wants a product of two entries that are both 1 or above, and psi(5) - log(drawn rate) rounds up as
often as down; and with K' own factors a hard row of ~17 nonzeros rarely meets its own factor at all (K' = 225).  Here
a nonzero of a hard or threshold row has s >= 1 with every flat partner and every hard or threshold partner of its
parity, two partners in three, and the narrower range of d keeps 100 denormal nonzeros on the matrices of 1 500 nonzeros.

The classification (classify), from tab_exp restated in T (tables: Elog = fl_T(psi(shape) - log(rate)), shifted by the
row's largest entry rounded to float32 as gamma_update_kernel does, exp in double, rounded to T): s is the sum of the K
products formed in T.  A nonzero is `zero` if all K products are 0 in T and `denormal` if 0 < s < finfo(T).tiny.
CONDITIONS (check_conditions), per axis over non-empty rows: at least 35 % of rows hold a zero nonzero; every such row
also holds a nonzero with s >= 1; at least 25 % of rows hold no nonzero with s < tiny 2**40; and the case has at least
100 denormal nonzeros.

The reference (reference).  prior + sum x softmax_k(Elog_i,k + Elog_g,k) in np.longdouble from the E[log] tables AS
GIVEN in T -- the GPU test passes the device's own tab_log, so the sweep is judged apart from the rounding of the
tables (tests/test_update_tables_gpu.py bounds that).

The bound.  u = 2**-53 / 2**-24 is T's unit roundoff, cast = 0 / u the rounding of a double stored in T, dmin T's
smallest denormal, l_k = Elog_i,k + Elog_g,k, M = max_k l_k, phi the true responsibilities, m_i = float32(max_k
Elog_i,k) the shift of a row's exp table.  The device may serve a nonzero by either form, so a nonzero's relative
error on x phi_k is bounded by the larger of the two:
  cold (slow_nonzero).  fl_T(a + b) and fl_T(. - mx) put d_k = u (|l_k| + |l_k - M|) into the exponent's argument (the
    same mx shifts numerator and denominator, so its own error cancels); the double exp, the K additions of the sum in
    double, the quotient, the product and the store in T are K + 6 roundings of 2**-53 and one cast:
        e_cold,k = d_k + sum_j phi_j d_j + (K + 6) 2**-53 + cast.
  fast (the hot loop), where the true s = sum_k exp(l_k - m_i - m_g) is at least tiny / 8 -- below that the reciprocal
    has overflowed (1 / s > 4 / tiny > max) and the group is the cold path's.  A tab_exp entry is exp (4.5e-16,
    special.h) of a difference formed in double (2**-53 |Elog - m|), stored in T (cast): its relative error is
    t = 4.5e-16 + cast + 2**-53 |Elog - m|, and a product of two has D_k = t_i,k + t_g,k.  s adds K positive products
    with fmas ((K + 1) u); the reciprocal is within 2**-48 (float64: v_rcp_f64 and a Newton step) or 2 ulp = 4 u
    (float32); x rcp(s) and the product with tab_exp of the major row are two more roundings (the fma onto the
    accumulator is counted with the accumulation):
        e_fast,k = D_k + sum_j phi_j D_j + (K + 3) u + rcp + 1.6 K dmin / s.
    The last term is the lost low bits of a denormal s and of denormal tab_exp entries: an entry stored in the denormal
    range is off by dmin / 2 absolutely, a product that lands there by another dmin / 2, entries are at most e**5e-4 (the
    shift is the maximum rounded to float32), so s is off by at most 1.5 K dmin 1.001; denormals add exactly.  With
    s >= tiny / 8 that is K 2**-48 (float64) or K 2**-19 (float32): the reciprocal overflows before s loses many bits.
    The numerator's own denormal entries: x phi_k is off by x / s (dmin / 2) (a_k [b_k < tiny] + b_k [a_k < tiny]),
    added absolutely.
  Accumulation: a partial row adds its nonzeros one fma each in T and is scaled once, the update kernel sums partial
  rows and the prior in double and stores in T: with n nonzeros in the row at most n + 3 roundings of u on positive
  terms, (n + 3) u (prior + sum x phi_k), plus (n + 1) dmin for results in the denormal range.
      |got - want| <= sum_n x phi_k max(e_cold,k, e_fast,k) + absolute terms + (n + 3) u want + (n + 1) dmin.
  In float32 the cold form's d_k is large where E[log] is (u 2e4 = 1.2e-3 on hard rows): that is the reference form's
  own float32 error, which the float32 oracle shares.

The emulation (emulate).  Both forms in T with NumPy, nonzeros added in COO order, and the hand-over: a row goes to
the cold form if and only if an accumulator of its fast form is not finite (the tile plan's probe, which the lanes of
a row's group agree on) or, rule "tiny", a nonzero has s < GATHER_TINY (the gather plan's test in the loop, 1e-280 /
1e-30: with that margin above the smallest normal number x / s and its sums stay finite for every sum of counts below
1.8e28 / 3.4e8, so that plan needs no probe).  The device hands over per (row, task) piece, the
emulation per row; both lie within the bound, which holds for either form.  1 / s in T stands for the reciprocal: it
overflows when 1 / s, x / s or a partial sum exceeds the format.  denormal="kept" divides by a denormal s as it is,
"flushed" takes it for 0 (reciprocal inf: the group goes cold) -- float32 hardware may do either; float64 keeps.
The MI355X flushes: v_rcp_f32 of a denormal is inf while the fmas of the dot product keep their denormal results
(measured), so in float32 every nonzero with a denormal s goes to the cold path, as in "flushed".
"""
import copy

import numpy as np
from scipy.special import digamma

import _sweep_shapes as shapes

LD = np.longdouble
A, C, AP, CP = 0.3, 0.3, 1.0, 1.0
GOLDEN_FRAC = 0.6180339887
D_RANGE = {"float64": (697.0, 755.0), "float32": (83.0, 108.0)}
GATHER_TINY = {"float64": 1e-280, "float32": 1e-30}       # sweep_impl.h Vec16<T>::tiny()
EXP_ERR = 4.5e-16          # special.h: exp within 4.5e-16 relative where the result is normal
CHUNK = 4096


def fallback_case(case):
    """The case with K' = max(K, 2) factors on its own matrix (drawn with the seed of the case's K)."""
    out = copy.copy(case)
    out.K0, out.K = case.K, max(case.K, 2)
    out.id = case.id.replace("-K%d-" % out.K0, "-K%d-" % out.K)      # the id names the factor count that runs
    return out


def long_task_case(case):
    """A half-window case with one window range per block (SCHPF_TASKS=1, set by the test after the layout's switches).
    On these small matrices the planner otherwise gives every task one window, the horizon of the half-window schedule
    ends with the task, and no row works ahead: every entry lives in its epoch's own slot and entry_minor's `ahead` is 0.
    With tasks as long as they get, rows consume the next sub-window's entries within an epoch (`ahead` = 1)."""
    assert case.layout.name == "half"
    out = copy.copy(case)
    out.tasks = 1
    out.id = case.id + "-longtasks"
    return out


def case_matrix(case):
    return shapes.case_matrix(case.N, case.G, getattr(case, "K0", case.K), case.layout.packed)


# The threshold pairs: (plan, dtype, (NV, LPC), K, layout, packed).  Every row is a threshold row and d walks a grid.
THRESHOLD = [("tile", "float64", (5, 2), 20, "t1024", 1), ("tile", "float64", (5, 2), 20, "t1024", 0),
             ("tile", "float64", (7, 4), 50, "balanced", 0), ("tile", "float32", (5, 1), 20, "t1024", 0),
             ("tile", "float32", (7, 2), 50, "t1024", 0), ("gather", "float64", (5, 4), 33, "gather", 0),
             ("gather", "float32", (2, 4), 17, "gather", 0)]
LOG_TINY = {"float64": 708.4, "float32": 87.3}
COUNTS = (1, 3, 1000, 65535, 70000)


class ThresholdCase(shapes.Case):
    """One of THRESHOLD on a 560 x 600 matrix of 40 000 nonzeros: one LDS window, more than one block of rows where
    LPC >= 2."""
    several_windows = False

    def __init__(self, plan, dtype, pair, K, layout, packed):
        lay = [l for l in (shapes.tile_layouts() if plan == "tile" else shapes.gather_layouts())
               if l.name == layout and l.packed == packed][0]
        shapes.Case.__init__(self, plan, dtype, pair, K, lay)
        self.K0, self.N, self.G = K, 560, 600
        self.id = "threshold-" + self.id


def threshold_cases():
    return [ThresholdCase(*t) for t in THRESHOLD]


def threshold_matrix(case):
    """Uniformly placed nonzeros with counts from COUNTS (70 000, which needs the 16-byte entries, only where the case
    is not packed): x rcp(s) overflows for the large counts first."""
    from conftest import synthetic_counts
    X = synthetic_counts(case.N, case.G, 0.12, seed=case.K)
    rng = np.random.RandomState(case.K + 1)
    X.data[:] = rng.choice(COUNTS if not case.layout.packed else COUNTS[:-1], X.nnz)
    assert X.nnz <= 45000
    return X


LOG_DMIN = {"float64": 744.44, "float32": 103.28}
FINE = 64


def threshold_grid(case):
    """(d of the cells, d of the genes): steps of 0.25 from 40 below to 40 above the format's log-tiny, the genes' grid
    offset by half a step and walked with another stride, so that s = (K / 2) (exp(-d_i - 2.1) + exp(-d_g - 2.1)) of two
    rows of different parity goes from a normal number through the denormal binades to 0.  The lowest binades hold 1, 2
    and 4 values and the grid steps over them, so the last FINE cells walk d in steps of 0.07 across the level at which
    the largest single product is the smallest denormal (exp(-d - 2.1) rho = dmin, rho the ratio of two drawn rates, 1/3
    to 3), and the last 100 genes sit at the top of the grid, where their own term has vanished: s = dmin ... 8 dmin."""
    lt = LOG_TINY[case.dtype]
    d_c = lt - 40 + 0.25 * (np.arange(case.N) % 321)
    d_g = lt - 40 + 0.125 + 0.25 * ((np.arange(case.G) * 7) % 321)
    d_c[-FINE:] = LOG_DMIN[case.dtype] - 5.4 + 0.07 * np.arange(FINE)
    d_g[-100:] = lt + 40
    return d_c, d_g


def case_inputs(oracle, case):
    """(X, bp, dp, start state) of a fallback case or a threshold case."""
    if isinstance(case, ThresholdCase):
        X = threshold_matrix(case)
        d_c, d_g = threshold_grid(case)
        return (X,) + start_state(oracle, X, case.K, case.dtype, d_c, d_g, all_threshold=True)
    X = case_matrix(case)
    return (X,) + start_state(oracle, X, case.K, case.dtype)


# The float32 yardstick of the whole-state comparison: the largest relative distance of the float32
# oracle's iteration from the float64 oracle's from the same float32 state over the cases of test_fallback_gpu.py
# (tests/test_fallback_host.py measures it and pins this figure), and the bound made of it.
F32_ORACLE_DISTANCE = 5.71e-4      # step 1; 1.02e-3 after step 2
F32_STATE_RTOL = max(2e-5, 2 * F32_ORACLE_DISTANCE)


def threshold_d(n, dtype):
    lo, hi = D_RANGE[np.dtype(dtype).name]
    return lo + (hi - lo) * np.modf((np.arange(n) // 3) * GOLDEN_FRAC)[0]


def own_rate(shape, dtype, scale):
    """The power of two next to `scale` at which E[log] = psi(shape) - log(rate) lies at least 1e-9 above its float32
    rounding."""
    v = float(np.dtype(dtype).type(shape))
    e0 = int(np.round(np.log2(scale)))
    for e in (0, -1, 1, -2, 2, -3, 3, -4, 4, -5, 5):
        L = float(digamma(v)) - np.log(2.0 ** (e0 + e))
        if L - float(np.float32(L)) >= 1e-9:
            return 2.0 ** (e0 + e)
    raise AssertionError("no such rate")


def shape_rows(shape, rate, scale, d=None, all_threshold=False):
    """Overwrite the shapes (and the rates of own factors and flat rows) by row class in place; scale: the rate prior;
    d: per-row 1 / (shape elsewhere) of the threshold rows."""
    n, K = shape.shape
    dt = shape.dtype
    r = np.arange(n)
    cls = np.full(n, 2) if all_threshold else r % 3
    d = threshold_d(n, dt) if d is None else d
    flat, hard, thr = cls == 0, cls == 1, cls == 2
    shape[flat] = 0.3
    rate[flat] = own_rate(0.3, dt, scale)
    block = 16 // dt.itemsize if K > 16 // dt.itemsize else 1              # a 16-byte vector of factors, if K has two
    on = ((np.arange(K)[None, :] // block) % 2) == ((r // 3) % 2)[:, None]   # a row's own factors
    shape[hard] = np.where(on[hard], 5.0, 1e-4)
    shape[thr] = np.where(on[thr], 5.0, (1.0 / d[thr])[:, None]).astype(dt)
    rate[shape == dt.type(5.0)] = own_rate(5.0, dt, scale)


def start_state(oracle, X, K, dtype, d_cell=None, d_gene=None, all_threshold=False):
    """(bp, dp, state): the usual start with theta and beta overwritten by row class."""
    dt = np.dtype(dtype)
    np.random.seed(K)
    bp, dp, st = oracle.setup_state(X, K, dt, A, AP, C, CP)
    st.xi_shape[:] = AP + K * A
    st.eta_shape[:] = CP + K * C
    shape_rows(st.theta_shape, st.theta_rate, bp, d_cell, all_threshold)
    shape_rows(st.beta_shape, st.beta_rate, dp, d_gene, all_threshold)
    return bp, dp, st


def tables(shape, rate):
    """(tab_log, tab_exp) of one side restated in T = shape.dtype, as gamma_update_kernel forms them."""
    T = shape.dtype
    L = (digamma(shape.astype(np.float64)) - np.log(rate.astype(np.float64))).astype(T)
    return L, exp_table(L)


def row_shift(L):
    """float32(the row's largest E[log]) as a double: the shift of the row's exp table."""
    return L.astype(np.float64).astype(np.float32).max(axis=1).astype(np.float64)


def exp_table(L):
    with np.errstate(under="ignore"):
        return np.exp(L.astype(np.float64) - row_shift(L)[:, None]).astype(L.dtype)


def normalisers(X, exp_c, exp_g):
    """Per nonzero: s as the sum of the K products formed in T (float64), and whether all products are 0."""
    T = exp_c.dtype
    s, zero = np.empty(X.nnz), np.empty(X.nnz, dtype=bool)
    with np.errstate(under="ignore"):
        for i in range(0, X.nnz, CHUNK):
            p = exp_c[X.row[i:i + CHUNK]] * exp_g[X.col[i:i + CHUNK]]
            assert p.dtype == T
            s[i:i + CHUNK] = p.sum(axis=1, dtype=np.float64)
            zero[i:i + CHUNK] = ~p.any(axis=1)
    return s, zero


def classify(X, exp_c, exp_g):
    """The figures of the conditions: per axis the share of non-empty rows with a zero nonzero, whether each of them also
    holds a nonzero with s >= 1, the share of rows that are fast throughout; and the number of denormal nonzeros."""
    T = exp_c.dtype
    tiny = float(np.finfo(T).tiny)
    s, zero = normalisers(X, exp_c, exp_g)
    out = {"denormal": int(np.sum((s > 0) & (s < tiny))), "zero": int(zero.sum()), "s": s}
    for axis, idx, n in (("cell", X.row, X.shape[0]), ("gene", X.col, X.shape[1])):
        cnt = lambda mask: np.bincount(idx[mask], minlength=n)  # noqa: E731
        rows = cnt(np.ones(X.nnz, dtype=bool)) > 0
        has_zero, has_big, has_small = cnt(zero) > 0, cnt(s >= 1.0) > 0, cnt(s < tiny * 2.0 ** 40) > 0
        out[axis] = {"zero_rows": float(has_zero[rows].mean()), "mixed": bool(np.all(has_big[has_zero])),
                     "fast_rows": float((~has_small)[rows].mean())}
    return out


def check_conditions(cls, label=""):
    for axis in ("cell", "gene"):
        c = cls[axis]
        assert c["zero_rows"] >= 0.35, (label, axis, c)
        assert c["mixed"], (label, axis, c)
        assert c["fast_rows"] >= 0.25, (label, axis, c)
    assert cls["denormal"] >= 100, (label, cls["denormal"])


def _segments(keys):
    """(order, starts, unique keys) to sum the rows of a chunk by key with np.add.reduceat."""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    return order, starts, sk[starts]


def reference(X, log_c, log_g, a=A, c=C):
    """One iteration's theta and beta shape in longdouble from the E[log] tables as given in T (N x K and G x K), and
    the bound of every element.  {'theta', 'beta', 'bound_theta', 'bound_beta'} (longdouble) and 's' (the true s)."""
    T = log_c.dtype
    assert log_g.dtype == T and T in (np.float64, np.float32)
    f64 = T == np.float64
    fi = np.finfo(T)
    u, tiny, dmin = LD(fi.eps) / 2, LD(fi.tiny), LD(fi.smallest_subnormal)
    cast = LD(0) if f64 else u
    u53 = LD(2.0) ** -53
    rcp = LD(2.0) ** -48 if f64 else 4 * u
    N, G, K = log_c.shape[0], log_g.shape[0], log_c.shape[1]
    Lc, Lg = log_c.astype(LD), log_g.astype(LD)
    mc, mg = row_shift(log_c).astype(LD), row_shift(log_g).astype(LD)
    # a table entry's relative error and its value (fast form)
    tc, tg = EXP_ERR + cast + u53 * np.abs(Lc - mc[:, None]), EXP_ERR + cast + u53 * np.abs(Lg - mg[:, None])
    with np.errstate(under="ignore"):
        ec, eg = np.exp(Lc - mc[:, None]), np.exp(Lg - mg[:, None])
    x = X.data.astype(LD)
    out = {k: np.zeros(s, dtype=LD) for k, s in (("theta", (N, K)), ("beta", (G, K)), ("bound_theta", (N, K)),
                                                ("bound_beta", (G, K)))}
    s_true = np.empty(X.nnz, dtype=LD)
    with np.errstate(under="ignore", divide="ignore", over="ignore", invalid="ignore"):
        for i in range(0, X.nnz, CHUNK):
            r, g, xx = X.row[i:i + CHUNK], X.col[i:i + CHUNK], x[i:i + CHUNK, None]
            l = Lc[r] + Lg[g]
            M = l.max(axis=1, keepdims=True)
            p = np.exp(l - M)
            S = p.sum(axis=1, keepdims=True)
            phi = p / S
            s = S * np.exp(M - mc[r, None] - mg[g, None])
            s_true[i:i + CHUNK] = s[:, 0]
            d = u * (np.abs(l) + np.abs(l - M))
            e_cold = d + (phi * d).sum(axis=1, keepdims=True) + (K + 6) * u53 + cast
            D = tc[r] + tg[g]
            e_fast = D + (phi * D).sum(axis=1, keepdims=True) + (K + 3) * u + rcp + 1.6 * K * dmin / s
            eligible = s >= tiny / 8
            eps = np.where(eligible & (e_fast > e_cold), e_fast, e_cold)
            av, bv = ec[r], eg[g]
            absolute = np.where(eligible, xx / s * (dmin / 2) * (av * (bv < tiny) + bv * (av < tiny)), 0)
            contrib = xx * phi
            err = contrib * eps + absolute
            for keys, name in ((r, "theta"), (g, "beta")):
                order, starts, uniq = _segments(keys)
                out[name][uniq] += np.add.reduceat(contrib[order], starts, axis=0)
                out["bound_" + name][uniq] += np.add.reduceat(err[order], starts, axis=0)
    for name, prior, idx, n in (("theta", a, X.row, N), ("beta", c, X.col, G)):
        # the prior as the engine holds it: a double, rounded to T with the stored shape
        out[name] += LD(prior)
        nn = np.bincount(idx, minlength=n).astype(LD)[:, None]
        out["bound_" + name] += (nn + 3) * u * out[name] + (nn + 1) * dmin
    out["s"] = s_true
    return out


def emulate(X, log_c, log_g, rule="probe", denormal="kept", a=A, c=C):
    """One iteration's theta and beta shape as the sweeps form them, in T.  rule: "probe" (a row goes cold iff an
    accumulator of its fast form is not finite) or "tiny" (iff a nonzero has s < GATHER_TINY); denormal: "kept" or "flushed"
    (what the reciprocal makes of a denormal s).  {'theta', 'beta'} in T, and per axis 'cold_<axis>' (rows handed over)
    and 'fast_denormal_<axis>' (rows kept on the fast form that hold a nonzero with a denormal s)."""
    T = log_c.dtype
    tiny = T.type(np.finfo(T).tiny)
    exp_c, exp_g = exp_table(log_c), exp_table(log_g)
    K = log_c.shape[1]
    out = {}
    with np.errstate(all="ignore"):
        for name, axis, idx, oth, n, lt, lm, et, em, prior in (
                ("theta", "cell", X.row, X.col, X.shape[0], log_c, log_g, exp_c, exp_g, a),
                ("beta", "gene", X.col, X.row, X.shape[1], log_g, log_c, exp_g, exp_c, c)):
            fast, cold = np.zeros((n, K), dtype=T), np.zeros((n, K), dtype=T)
            den, small = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
            for i in range(0, X.nnz, CHUNK):
                r, g, xx = idx[i:i + CHUNK], oth[i:i + CHUNK], X.data[i:i + CHUNK].astype(T)
                b = em[g]
                s = (et[r] * b).sum(axis=1, dtype=T)
                is_den = (s > 0) & (s < tiny)
                np.logical_or.at(den, r, is_den)
                np.logical_or.at(small, r, s < T.type(GATHER_TINY[T.name]))
                if denormal == "flushed":
                    s = np.where(is_den, T.type(0), s)
                q = xx * (T.type(1) / s)
                np.add.at(fast, r, q[:, None] * b)
                l = lt[r] + lm[g]
                z = (l - l.max(axis=1, keepdims=True)).astype(np.float64)
                e = np.exp(z)
                scale = xx.astype(np.float64) / e.sum(axis=1)
                np.add.at(cold, r, (scale[:, None] * e).astype(T))
            go_cold = small if rule == "tiny" else ~np.isfinite(fast).all(axis=1)
            part = np.where(go_cold[:, None], cold, fast * et)
            out[name] = (prior + part.astype(np.float64)).astype(T)
            out["cold_" + axis] = go_cold
            out["fast_denormal_" + axis] = den & ~go_cold
    return out


def scaled_error(got, ref, name):
    """The largest |got - want| / bound over the elements of theta or beta, and where."""
    frac = np.abs(got.astype(LD) - ref[name]) / ref["bound_" + name]
    at = np.unravel_index(int(np.argmax(frac)), frac.shape)
    return float(frac[at]), at
