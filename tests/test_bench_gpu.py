"""bench.py on the GPU: a plain run's line carries the headline and nothing more, --dump-outputs writes the model the
timed steps left (checked against the same iterations run here), --full adds the other measurements."""
import json
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose

from conftest import ROOT

pytestmark = pytest.mark.gpu

CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "loss_after_warmup", "loss_after_steps", "loss_eval_ms", "per_rank", "convergence",
             "cpu_baseline")


def _bench(args):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--config", "c2"] + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("steps,warmup", [(4, 2), (3, 1), (5, 0)])
def test_plain_line_and_dumped_outputs(tmp_path, steps, warmup):
    """A plain run: the contract fields for exactly --steps timed steps and none of --full's measurements.  The dump
    is the model after the warm-up steps, the untimed calls that capture the timed call's graph (one; an odd K two,
    W = 0 one more) and the timed call -- the same iterations, issued one by one here, give the same arrays."""
    line = _bench(["--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)])
    for key in CONTRACT:
        assert key in line
    for key in FULL_ONLY:
        assert key not in line
    assert line["steps"] == steps and line["warmup"] == warmup and line["n_gpus"] == 1
    assert line["unit"] == "iterations/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0 and np.isclose(line["value"], 1e3 / line["ms_per_step"])

    from bench import CONFIGS, init_engine, synthetic_block
    from schpf_amd import DeviceCAVI
    N, G, dens, K = CONFIGS["c2"]
    X = synthetic_block(N, G, dens, seed=42)
    untimed = 1 + steps % 2 + (warmup == 0)
    with DeviceCAVI(N, G, K, dtype=np.float64, device=0) as eng:
        init_engine(eng, X, K, np.float64)
        eng.init_phi_device(12345)
        for _ in range(warmup + (untimed + 1) * steps):
            eng.step()
        for name in ("xi", "theta", "eta", "beta"):
            s, r = eng.get_gamma(name)
            got_s = np.load(str(tmp_path / (name + "_shape.npy")))
            got_r = np.load(str(tmp_path / (name + "_rate.npy")))
            assert got_s.dtype == np.float64 and got_s.shape == s.shape and got_r.shape == r.shape
            assert_allclose(got_s, s, rtol=1e-10, err_msg=name + " shape")
            assert_allclose(got_r, r, rtol=1e-10, err_msg=name + " rate")


def test_full_line():
    """--full: the headline as in a plain run, plus the roofline and the loss evaluations (the CPU baselines, the
    convergence fits and the counter passes left out here by their own options)."""
    line = _bench(["--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-converge", "--no-traffic"])
    for key in CONTRACT:
        assert key in line
    assert line["steps"] == 5 and line["ms_per_step"] > 0
    assert line["roofline"]["launches"] > 0 and line["roofline"]["avg_launch_ms"] > 0
    assert np.isfinite(line["loss_after_steps"]) and line["loss_after_steps"] < line["loss_after_warmup"]
    assert line["cpu_baseline"] is None and "convergence" not in line
