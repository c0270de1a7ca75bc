#!/usr/bin/env python
"""Generate tests/golden/special_edges.npz: arguments at which the special functions of schpf_amd/csrc/special.h can
go wrong, with their values computed by mpmath at 60 digits and rounded ONCE to double (round to nearest even,
denormals included).  Needs mpmath; the tests read only the .npz.

    python tests/golden/make_special_golden.py

Arrays (float64 throughout):
  rcp_x, rcp              1 / x: log-uniform over [1e-300, 1e300], powers of two, the neighbours of 1 and 2
  log_x, log              log x: log-uniform over the whole positive range (denormals included), [0.5, 2] densely, the
                          ends of the reduced range sqrt(1/2) / sqrt(2), the smallest denormal, the largest binade
  log_end_x, log_end      0, inf, nan -> -inf, inf, nan
  exp_x, exp              exp x: -uniform(0, 745), uniform(-1, 1), and the tail -744.5 ... -1e300 where the result is a
                          denormal or 0
  psi_x, psi              digamma: log-uniform over [1e-4, 1e6], and the points around the switch at 1e8
  pll_shape, pll_rate,    psi(shape) - log(rate), rounded once from the 60-digit difference, with its two terms:
  pll, pll_psi, pll_log   shape log-uniform over [1e-4, 1e7] plus the points around 1e8, rate over [1e-12, 1e12]
"""
import os
from fractions import Fraction

import mpmath as mp
import numpy as np

mp.mp.dps = 60
HERE = os.path.dirname(os.path.abspath(__file__))
TINY = mp.ldexp(mp.mpf(1), -1080)     # below half the smallest denormal: rounds to 0


def rounded(v):
    """The double nearest to the mpf v: through an exact fraction, because int / int is correctly rounded in Python over
    the whole range, denormals included (float(mpf) is not guaranteed to be)."""
    if mp.isnan(v):
        return float("nan")
    if mp.isinf(v):
        return float("inf") if v > 0 else float("-inf")
    if abs(v) < TINY:
        return 0.0
    sign, man, exp, _ = v._mpf_
    f = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return float(-f if sign else f)


def table(fn, *args):
    return np.array([rounded(fn(*[mp.mpf(float(a)) for a in row])) for row in zip(*args)], dtype=np.float64)


def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def main():
    rng = np.random.RandomState(20250)
    out = {}

    one, two = 1.0, 2.0
    out["rcp_x"] = np.concatenate([
        log_uniform(rng, 1e-300, 1e300, 1900),
        2.0 ** np.arange(-990, 991, 30),
        [np.nextafter(one, 0.0), one, np.nextafter(one, 2.0), np.nextafter(two, 0.0), two, np.nextafter(two, 3.0)]])
    out["rcp"] = table(lambda x: 1 / x, out["rcp_x"])

    r = np.sqrt(0.5)
    out["log_x"] = np.concatenate([
        np.exp(rng.uniform(np.log(5e-324), np.log(1.7976931348623157e308), 1500)),
        rng.uniform(0.5, 2.0, 500),
        [1.0, np.nextafter(r, 0.0), r, np.nextafter(r, 1.0), np.sqrt(2.0),
         5e-324, 1e-310, 2.2250738585072014e-308, 1.7e308]])
    out["log"] = table(mp.log, out["log_x"])
    out["log_end_x"] = np.array([0.0, np.inf, np.nan])
    out["log_end"] = np.array([-np.inf, np.inf, np.nan])

    out["exp_x"] = np.concatenate([
        -rng.uniform(0.0, 745.0, 1500), rng.uniform(-1.0, 1.0, 500),
        [0.0, -744.5, -745.0, -745.2, -746.0, -800.0, -999.9, -1000.0, -1000.1, -1e5, -1e300]])
    # far below the last denormal mpmath would carry an exponent of 1e300 bits: 0 at once
    out["exp"] = table(lambda x: mp.mpf(0) if x < -800 else mp.exp(x), out["exp_x"])

    around_switch = [9.99e7, np.nextafter(1e8, 0.0), 1e8, 1.01e8, 1e12, 1e15]
    out["psi_x"] = np.concatenate([log_uniform(rng, 1e-4, 1e6, 2000), around_switch])
    out["psi"] = table(mp.digamma, out["psi_x"])

    out["pll_shape"] = np.concatenate([log_uniform(rng, 1e-4, 1e7, 2000), around_switch, [3e9]])
    out["pll_rate"] = log_uniform(rng, 1e-12, 1e12, out["pll_shape"].size)
    out["pll"] = table(lambda s, q: mp.digamma(s) - mp.log(q), out["pll_shape"], out["pll_rate"])
    out["pll_psi"] = table(mp.digamma, out["pll_shape"])
    out["pll_log"] = table(mp.log, out["pll_rate"])

    path = os.path.join(HERE, "special_edges.npz")
    np.savez(path, **out)
    print("wrote %s: %d bytes, %s" % (path, os.path.getsize(path), {k: v.size for k, v in out.items()}))


if __name__ == "__main__":
    main()
