#!/usr/bin/env python
"""Time the ELBO evaluation beside the loss evaluation (GPU box):
    python tools/elbo_time.py c3 "dtype=f64" "dtype=f32" ...      python tools/elbo_time.py c5-shard "dtype=f64"

Settings as in tools/loss_time.py; prints ms per elbo() and per mean_negative_pois_llh() call (wall, 100 calls each
after 10 untimed), both on the state three iterations leave."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from schpf_amd import DeviceCAVI  # noqa: E402


def per_call_ms(eng, fn, n=100):
    for _ in range(10):
        fn()
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    return (time.perf_counter() - t0) / n * 1e3, out


def run(X, K, setting):
    kv = dict(item.split("=") for item in setting.split(",") if item)
    dtype = np.float32 if kv.pop("dtype", "f64") == "f32" else np.float64
    for k in list(os.environ):
        if k.startswith("SCHPF_") and k not in ("SCHPF_VERBOSE", "SCHPF_LIB_PATH"):
            del os.environ[k]
    os.environ.update(kv)
    N, G = X.shape
    with DeviceCAVI(N, G, K, dtype=dtype) as eng:
        bench.init_engine(eng, X, K, dtype)
        eng.init_phi_device(1)
        for _ in range(3):
            eng.step()
        elbo_ms, elbo = per_call_ms(eng, lambda: eng.elbo(1.0, 1.0))
        loss_ms, loss = per_call_ms(eng, eng.mean_negative_pois_llh)
    print(json.dumps({"setting": setting, "elbo_ms": round(elbo_ms, 4), "loss_ms": round(loss_ms, 4),
                      "elbo": elbo, "loss": loss}), flush=True)


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
