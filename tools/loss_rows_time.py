#!/usr/bin/env python
"""Time the per-row loss (GPU box): python tools/loss_rows_time.py c3 "dtype=f64" "dtype=f32" ...

Settings as in tools/loss_time.py.  Per setting, the median over 30 calls (after 5 untimed) of loss_rows by cell and by
gene -- wall-clock beside the HIP-event time of profile slot 2 (the loss slot) -- and, on the same engine and state, of
the scalar loss; host=1 adds one call of the estimator's host route scHPF.cellmean_negative_pois_llh(X)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from schpf_amd import DeviceCAVI  # noqa: E402


def timed(eng, fn, calls=30, warm=5):
    for _ in range(warm):
        fn()
    eng.profile(True)
    eng.profile_read()
    wall, event = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        event.append(eng.profile_read()["loss_sweep"]["ms"])
    eng.profile(False)
    return {"wall_ms": round(float(np.median(wall)), 4), "event_ms": round(float(np.median(event)), 4),
            "wall_min_max": [round(min(wall), 4), round(max(wall), 4)]}


def run(X, K, setting):
    kv = dict(item.split("=") for item in setting.split(",") if item)
    dtype = np.float32 if kv.pop("dtype", "f64") == "f32" else np.float64
    host = kv.pop("host", "0") == "1"
    for k in list(os.environ):
        if k.startswith("SCHPF_") and k not in ("SCHPF_VERBOSE", "SCHPF_LIB_PATH"):
            del os.environ[k]
    os.environ.update(kv)
    N, G = X.shape
    out = {"setting": setting}
    with DeviceCAVI(N, G, K, dtype=dtype) as eng:
        bench.init_engine(eng, X, K, dtype)
        eng.init_phi_device(1)
        for _ in range(3):
            eng.step()
        out["scalar_loss"] = timed(eng, eng.mean_negative_pois_llh)
        out["rows_by_cell"] = timed(eng, lambda: eng.loss_rows("cell"))
        out["rows_by_gene"] = timed(eng, lambda: eng.loss_rows("gene"))
        if host:
            from schpf_amd import HPF_Gamma, scHPF
            m = scHPF(K, dtype=dtype)
            m.theta, m.beta = HPF_Gamma(*eng.get_gamma("theta")), HPF_Gamma(*eng.get_gamma("beta"))
            t0 = time.perf_counter()
            with np.errstate(divide="ignore", invalid="ignore"):
                m.cellmean_negative_pois_llh(X)
            out["host_route_cellmean_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(out), flush=True)


def main():
    N, G, dens, K = bench.CONFIGS[sys.argv[1]]
    X = bench.synthetic_block(N, G, dens, 42)
    for setting in sys.argv[2:]:
        try:
            run(X, K, setting)
        except Exception as e:
            print(json.dumps({"setting": setting, "error": str(e)}), flush=True)


if __name__ == "__main__":
    main()
