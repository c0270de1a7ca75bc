"""The special functions of the fused Gamma update (schpf_amd/csrc/special.h) evaluated ON THE DEVICE
(schpf_debug_special: one thread per element, the inline bodies gamma_update_kernel calls) against
tests/golden/special_edges.npz -- mpmath at 60 digits, rounded once (tests/golden/make_special_golden.py).

The device build is the one with the hardware reciprocal seed (__builtin_amdgcn_rcp), the frexp builtins and fma_c's
v_fma_f64 with a scalar constant; tests/test_special_host.py checks the g++ build, in which all three are replaced.  Every
test here runs BOTH builds over the same points and holds both to the bounds special.h states, so a failure shows at
once whether it is the algorithm (both builds) or one of the device paths (device only).

Bounds (special.h; tests/test_special_host.py):
  psi           within 4e-15, relative or absolute
  psi_less_log  |err| <= 4e-15 * max(1, |psi(shape)|, |log rate|)
  log           within 2 ulp of the fixture; log 0 = -inf, log inf = inf, log nan = nan exactly
  exp           relative error <= 4.5e-16 where the result is a normal number; the bits of the correctly rounded value
                for arguments <= -745 (a denormal or 0).  In between (arguments in (-745, -708.4), denormal results) at
                most one denormal step from the fixture: the polynomial is within 4.5e-16 of exp(r), ldexp rounds once,
                so the result is within half a step (and a 1e-16th) of the truth, and so is the fixture
  rcp           |rcp(x) * x - 1| <= 2.3e-16, the product taken exactly (fractions), not rounded to double
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from conftest import load_golden
from _special_host import build_host

pytestmark = pytest.mark.gpu

DBL_MIN = 2.2250738585072014e-308
STEP = 5e-324                       # the denormal spacing
WORST = {}                          # (function, build) -> largest error seen (printed by the last test)
DIFFER = {}                         # function -> (elements whose bits differ between the two builds, elements)
UNITS = {"psi": "abs-or-rel", "psi_less_log": "scaled", "log": "ulp", "exp": "rel", "rcp": "|rcp(x) x - 1|"}
BOUNDS = {"psi": 4e-15, "psi_less_log": 4e-15, "log": 2.0, "exp": 4.5e-16, "rcp": 2.3e-16}


@pytest.fixture(scope="module")
def golden():
    return load_golden("special_edges.npz")


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """{'device': f, 'host': f}, f(name, *arrays) -> float64 array, name one of rcp / log / exp / psi / psi_less_log."""
    from schpf_amd import _lib
    _lib.require_gpu()
    lib = _lib.load()
    which = {"rcp": _lib.SPECIAL_RCP, "log": _lib.SPECIAL_LOG, "exp": _lib.SPECIAL_EXP, "psi": _lib.SPECIAL_PSI,
             "psi_less_log": _lib.SPECIAL_PSI_LESS_LOG}
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def device(name, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
        out = np.full(x.shape[0], np.nan)
        _lib.check(lib.schpf_debug_special(which[name], x.shape[0], p(x), None if y is None else p(y), p(out)))
        return out

    call = build_host(tmp_path_factory.mktemp("special_gpu"))
    return {"device": device, "host": lambda name, *arrays: call("h_" + name, *arrays)}


def both(builds, name, measure, *arrays):
    """measure(got) -> (largest error, message of what else failed or None) for each build: everything is printed and
    recorded before anything is asserted."""
    res, raw = {}, {}
    for build in ("device", "host"):
        with np.errstate(all="ignore"):
            raw[build] = builds[build](name, *arrays)
            res[build] = measure(raw[build])
        WORST[(name, build)] = res[build][0]
        print("%s on the %s: largest error %.3g %s (bound %.3g)%s" % (name, build, res[build][0], UNITS[name],
                                                                      BOUNDS[name], "; " + res[build][1] if res[build][1] else ""))
    d, h = raw["device"], raw["host"]
    DIFFER[name] = (int(((d.view(np.int64) != h.view(np.int64)) & ~(np.isnan(d) & np.isnan(h))).sum()), d.size)
    for build in ("device", "host"):
        err, other = res[build]
        assert err <= BOUNDS[name], "%s, %s build: %.3g %s > %.3g (device %.3g, host %.3g)" % (
            name, build, err, UNITS[name], BOUNDS[name], res["device"][0], res["host"][0])
        assert other is None, "%s, %s build: %s" % (name, build, other)


def test_psi(builds, golden):
    x, want = golden["psi_x"], golden["psi"]

    def measure(got):
        err = np.abs(got - want)
        return float(np.minimum(err, err / np.abs(want)).max()), None
    assert x.min() >= 1e-4 and (x >= 1e8).sum() >= 4 and (x < 1e8).sum() >= 2000      # both branches
    both(builds, "psi", measure, x)


def test_psi_less_log(builds, golden):
    shape, rate, want = golden["pll_shape"], golden["pll_rate"], golden["pll"]
    scale = np.maximum(1.0, np.maximum(np.abs(golden["pll_psi"]), np.abs(golden["pll_log"])))

    def measure(got):
        return float((np.abs(got - want) / scale).max()), None
    assert (shape >= 1e8).sum() >= 4 and rate.min() < 1e-11 and rate.max() > 1e11
    both(builds, "psi_less_log", measure, shape, rate)


def test_log(builds, golden):
    x = np.concatenate([golden["log_x"], golden["log_end_x"]])
    want, n_end = golden["log"], golden["log_end_x"].size

    def measure(got):
        body, ends = got[:-n_end], got[-n_end:]
        ulps = np.abs(body - want) / np.maximum(np.spacing(np.abs(want)), STEP)
        exact = ends[0] == -np.inf and ends[1] == np.inf and np.isnan(ends[2])
        return float(ulps.max()), None if exact else "log of (0, inf, nan) = %s" % (ends,)
    assert (x[:-n_end] < DBL_MIN).sum() >= 3 and (want == 0.0).sum() == 1
    both(builds, "log", measure, x)


def test_exp(builds, golden):
    x, want = golden["exp_x"], golden["exp"]
    normal, tail = want >= DBL_MIN, x <= -745.0
    between = ~normal & ~tail

    def measure(got):
        rel = np.abs(got[normal] - want[normal]) / want[normal]
        other = None
        if not np.array_equal(got[tail].view(np.int64), want[tail].view(np.int64)):
            other = "arguments <= -745: %s, correctly rounded %s" % (got[tail], want[tail])
        elif np.abs(got[between] - want[between]).max() > STEP:
            bad = np.abs(got[between] - want[between]).argmax()
            other = "exp(%r) = %r, correctly rounded %r: more than a denormal step" % (
                x[between][bad], got[between][bad], want[between][bad])
        return float(rel.max()), other
    assert tail.sum() >= 9 and (want[tail] > 0).sum() >= 1 and between.sum() >= 20 and normal.sum() >= 1900
    both(builds, "exp", measure, x)


def test_rcp(builds, golden):
    x = golden["rcp_x"]
    fx = [Fraction(float(v)) for v in x]

    def measure(got):
        if not np.all(np.isfinite(got)):
            return np.inf, "rcp of %r is not finite" % (x[~np.isfinite(got)][0],)
        return float(max(abs(Fraction(float(g)) * f - 1) for g, f in zip(got, fx))), None
    assert x.min() < 1e-299 and x.max() > 1e299
    both(builds, "rcp", measure, x)


def test_entry_point_arguments(builds):
    from schpf_amd import _lib
    lib = _lib.load()
    assert lib.schpf_debug_special(_lib.SPECIAL_LOG, 0, None, None, None) == 0          # n = 0 succeeds
    x, out = np.ones(3), np.zeros(3)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for which in (-1, 5):
        assert lib.schpf_debug_special(which, 3, p(x), p(x), p(out)) != 0
        assert b"SCHPF_SPECIAL_RCP" in lib.schpf_last_error()
    assert lib.schpf_debug_special(_lib.SPECIAL_PSI_LESS_LOG, 3, p(x), None, p(out)) != 0   # the rates are missing
    assert lib.schpf_debug_special(_lib.SPECIAL_RCP, -1, p(x), None, p(out)) != 0
    assert np.array_equal(out, np.zeros(3))
    # 257 elements: a second, partly filled block
    v = np.linspace(1.0, 3.0, 257)
    np.testing.assert_allclose(builds["device"]("rcp", v), 1.0 / v, rtol=3e-16)


def test_zz_report_largest_error():
    """Not a check of its own: one line with the largest error of every function on the device and on the host build
    ("Parity", records it)."""
    line = ", ".join("%s %.3g / %.3g %s" % (name, WORST.get((name, "device"), np.nan), WORST.get((name, "host"), np.nan),
                                            UNITS[name]) for name in ("psi", "psi_less_log", "log", "exp", "rcp"))
    print("special.h largest error, device / host: " + line)
    print("device and host results differ in their bits at: " + ", ".join(
        "%s %d of %d points" % (name, DIFFER[name][0], DIFFER[name][1]) for name in sorted(DIFFER)))
    for (name, build), err in WORST.items():
        assert err <= BOUNDS[name], (name, build, err)
