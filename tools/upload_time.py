#!/usr/bin/env python
"""Time upload() from the host and from GPU memory (GPU box): python tools/upload_time.py [c3] [dtype=f64]

One process, one engine, the headline matrix (bench.CONFIGS c3: 100k x 20k, 5 %, K = 20).  The median of five upload()
calls (after one untimed) of the same matrix as a SciPy COO, as a GPU sparse COO tensor (int64 indices, as torch makes
them) and as a GPU sparse CSR tensor (int32 indices); upload_info / plan_info must agree between the three.  With
SCHPF_VERBOSE=1 (set here unless exported) the library's own stage times of every call go to stderr.  One JSON line, with
the shader clock the box reports."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SCHPF_VERBOSE", "1")
import bench  # noqa: E402
from schpf_amd import DeviceCAVI  # noqa: E402


def median_upload(eng, X, calls=5):
    import torch
    eng.upload(X, warn=False)
    ms = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.upload(X, warn=False)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ms)), 2), "min_max": [round(min(ms), 2), round(max(ms), 2)]}, \
        (eng.upload_info(), eng.plan_info())


def main():
    import torch
    args = sys.argv[1:]
    name = args[0] if args and "=" not in args[0] else "c3"
    kv = dict(a.split("=") for a in args if "=" in a)
    dtype = np.float32 if kv.get("dtype", "f64") == "f32" else np.float64
    N, G, dens, K = bench.CONFIGS[name]
    X = bench.synthetic_block(N, G, dens, 42)
    ind = torch.tensor(np.stack([X.row, X.col]).astype(np.int64)).cuda()
    val = torch.tensor(X.data).cuda()
    coo = torch.sparse_coo_tensor(ind, val, X.shape, check_invariants=False, is_coalesced=False)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(X.row, minlength=N))]).astype(np.int32)
    csr = torch.sparse_csr_tensor(torch.tensor(indptr).cuda(), ind[1].to(torch.int32), val, size=X.shape)
    out = {"config": name, "shape": [N, G], "nnz": int(X.nnz), "K": K, "dtype": np.dtype(dtype).name,
           "values": str(X.data.dtype)}
    with DeviceCAVI(N, G, K, dtype=dtype) as eng:
        facts = []
        for key, M in (("scipy_coo", X), ("gpu_coo_int64", coo), ("gpu_csr_int32", csr)):
            print("---- %s" % key, file=sys.stderr, flush=True)
            out[key], f = median_upload(eng, M)
            facts.append(f)
        out["same_engine_facts"] = facts[0] == facts[1] == facts[2]
        bench.init_engine(eng, X, K, dtype)      # a few iterations, for the clock the box sustains
        eng.init_phi_device(1)
        eng.steps(10)
        out["sclk_mhz"] = round(eng.profile_clock()[0], 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
