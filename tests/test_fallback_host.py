"""The yardstick of tests/test_fallback_gpu.py held to its own claims, without a device (tests/_fallback_reference.py):

  * the start state meets the class conditions on every case of both plans and both dtypes, and on the threshold pairs;
  * the longdouble reference agrees with oracle.cavi_iteration from the same state: float64 at the rtol 1e-10 of
    test_underflow_fallback_matches_log_domain_oracle (a hard row's E[log] of 1e4 carries 4e-15 * 1e4 into the exponent),
    float32 within the reference's own bound and the (2 K + 8) u of the oracle's float32 exp and sum;
  * the emulations in T stay within 0.9 of the bound on every case -- hand-over by the probe (tile plans) and by the
    gather plan's test of s in the loop, a denormal s kept and flushed;
  * wherever an emulation keeps a row with a denormal s on the fast form, that row is within the bound: the
    reciprocal's overflow is the guard of fast_div's "s known to be a normal positive number";
  * the float32 figure of the GPU module (F32_STATE_RTOL) is the larger of 2e-5 and twice the largest distance of the
    float32 oracle's iteration from the float64 oracle's on these cases.
One reference per distinct (matrix, K', dtype); the layouts of a pair share it."""
import functools

import numpy as np
import pytest

import _fallback_reference as fr
import _sweep_shapes as shapes

ALL = [fr.fallback_case(c) for c in shapes.cases("tile") + shapes.cases("gather")]
THRESHOLD = fr.threshold_cases()


def distinct(cases):
    seen, out = set(), []
    for c in cases:
        key = (c.N, c.G, c.K0, c.K, c.layout.packed, c.dtype)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


DISTINCT = distinct(ALL)
EVERY = DISTINCT + THRESHOLD
NAMES = ("xi", "theta", "eta", "beta")


@functools.lru_cache(maxsize=2)
def _setup(oracle, cid):
    X, bp, dp, st = fr.case_inputs(oracle, BY_ID[cid])
    log_c, exp_c = fr.tables(st.theta_shape, st.theta_rate)
    log_g, exp_g = fr.tables(st.beta_shape, st.beta_rate)
    return X, bp, dp, st, log_c, log_g, exp_c, exp_g


BY_ID = {c.id: c for c in EVERY}


def setup(oracle, c):
    return _setup(oracle, c.id)


def test_every_case_is_covered_and_keeps_its_pair():
    """One fallback case per sweep-shape case; K' differs from K only at K = 1, and K = 2 is on the pair of K = 1."""
    assert len(ALL) == len(shapes.cases("tile")) + len(shapes.cases("gather")) and len(DISTINCT) >= 200
    for c in ALL:
        assert c.K == max(c.K0, 2) and (c.K == c.K0 or c.K0 == 1)
        cfg = shapes.choose_config(c.dtype, c.K, c.plan)
        assert (cfg["NV"], cfg["LPC"]) == (c.NV, c.LPC), (c.id, cfg)


@pytest.mark.parametrize("case", DISTINCT, ids=[c.id for c in DISTINCT])
def test_start_state_meets_the_conditions(oracle, case):
    X, _, _, st, _, _, exp_c, exp_g = setup(oracle, case)
    assert X.nnz <= 45000
    fr.check_conditions(fr.classify(X, exp_c, exp_g), case.id)
    for a in st.arrays():
        assert np.all(np.isfinite(a)) and np.all(a > 0)


def test_threshold_grid_walks_through_every_denormal_binade(oracle):
    """On each threshold pair s takes normal values, values in every binade of the denormal range -- down to
    s = dmin -- and 0."""
    for case in THRESHOLD:
        X, _, _, _, _, _, exp_c, exp_g = setup(oracle, case)
        assert X.shape[0] <= 600 and X.shape[1] <= 600 and X.nnz <= 45000
        assert set(np.unique(X.data)) == set(fr.COUNTS if not case.layout.packed else fr.COUNTS[:-1])
        s, zero = fr.normalisers(X, exp_c, exp_g)
        fi = np.finfo(np.dtype(case.dtype))
        assert zero.sum() >= 20 and np.sum((s >= fi.tiny) & (s < fi.tiny * 2.0 ** 40)) >= 100 and np.sum(s >= 1) >= 100
        den = s[(s > 0) & (s < fi.tiny)]
        binades = np.unique(np.floor(np.log2(den)).astype(int))
        assert len(binades) == fi.nmant and binades.max() == fi.minexp - 1, (case.id, len(binades), binades[:4])
        smallest = float(np.finfo(np.dtype(case.dtype)).smallest_subnormal)
        assert den.min() == smallest, case.id         # the very bottom: s = dmin


@pytest.mark.parametrize("case", EVERY, ids=[c.id for c in EVERY])
def test_reference_oracle_and_emulations(oracle, case):
    X, bp, dp, st, log_c, log_g, _, _ = setup(oracle, case)
    f64 = case.dtype == "float64"
    ref = fr.reference(X, log_c, log_g)
    want = st.copy()
    oracle.cavi_iteration(X.data, X.row, X.col, want, fr.A, fr.C, bp, dp)
    for name, got in (("theta", want.theta_shape), ("beta", want.beta_shape)):
        if f64:
            rel = np.abs(got.astype(fr.LD) - ref[name]) / ref[name]
            assert float(rel.max()) <= 1e-10, (case.id, name, float(rel.max()))
        else:       # the float32 oracle also takes exp and the K additions in float32: (2 K + 8) u beside the bound
            extra = (2 * case.K + 8) * fr.LD(2.0) ** -24 * ref[name]
            frac = float(np.max(np.abs(got.astype(fr.LD) - ref[name]) / (ref["bound_" + name] + extra)))
            assert frac <= 1.0, (case.id, name, frac)
    for rule in ("probe", "tiny"):
        for denormal in ("kept", "flushed") if not f64 or rule == "probe" else ("kept",):
            em = fr.emulate(X, log_c, log_g, rule, denormal)
            for name, axis in (("theta", "cell"), ("beta", "gene")):
                frac, at = fr.scaled_error(em[name], ref, name)
                assert frac <= 0.9, (case.id, rule, denormal, name, frac, at)
                rows = em["fast_denormal_" + axis]
                assert not np.any(rows & em["cold_" + axis])
                if rule == "tiny":
                    assert not rows.any()       # the gather plan never divides by a denormal s
                elif rows.any():                # the probe kept them: the reciprocal did not overflow, and they are right
                    err = np.abs(em[name][rows].astype(fr.LD) - ref[name][rows]) / ref["bound_" + name][rows]
                    assert float(err.max()) <= 0.9, (case.id, denormal, name, float(err.max()))
                if denormal == "flushed":
                    assert not rows.any()


F32_DISTINCT = [c for c in EVERY if c.dtype == "float32"]
SEEN_F32 = {}


def oracle_distance(oracle, case):
    """[step 1, step 2]: the largest relative distance over the eight arrays of the float32 oracle's iteration from the
    float64 oracle's, both from the same (float32) state.  Once per case and process."""
    if case.id not in SEEN_F32:
        X, bp, dp, st, _, _, _, _ = setup(oracle, case)
        a32, a64 = st.copy(), st.cast(np.float64)
        worst = []
        for _ in range(2):
            oracle.cavi_iteration(X.data, X.row, X.col, a32, fr.A, fr.C, bp, dp)
            oracle.cavi_iteration(X.data, X.row, X.col, a64, fr.A, fr.C, bp, dp)
            worst.append(max(float(np.max(np.abs(g.astype(np.float64) - w) / np.abs(w)))
                             for g, w in zip(a32.arrays(), a64.arrays())))
        SEEN_F32[case.id] = worst
    return SEEN_F32[case.id]


@pytest.mark.parametrize("case", F32_DISTINCT, ids=[c.id for c in F32_DISTINCT])
def test_float32_oracle_distance(oracle, case):
    """The yardstick of the GPU module's float32 bound covers every case, at both steps."""
    worst = oracle_distance(oracle, case)
    assert 2 * worst[0] <= fr.F32_STATE_RTOL and 2 * worst[1] <= 2 * fr.F32_STATE_RTOL, (case.id, worst)


def test_zz_float32_figure_is_the_measured_one(oracle):
    """The figure is the largest over every float32 case: cases that did not run in this process are measured here."""
    seen = [oracle_distance(oracle, c) for c in F32_DISTINCT]
    largest = max(w[0] for w in seen)
    print("float32 oracle against float64 oracle, largest relative distance: step 1 %.3g, step 2 %.3g"
          % (largest, max(w[1] for w in seen)))
    assert fr.F32_ORACLE_DISTANCE * 0.99 <= largest <= fr.F32_ORACLE_DISTANCE
    assert fr.F32_STATE_RTOL == max(2e-5, 2 * fr.F32_ORACLE_DISTANCE)
