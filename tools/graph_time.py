#!/usr/bin/env python
"""Time the weighted neighbour graphs (GPU box): python tools/graph_time.py [n=100000] [K=20] [k=15] [calls=10]
                                                                         [scipy_calls=3] [out=FILE]

The exact self graph of n x K float64 scores drawn as tests/_knn_reference.py draws them is searched once (schpf_amd.knn,
on the GPU; not timed).  schpf_knn_graph_device is then timed for both methods with HIP events on torch's current stream
-- validation, calibration, sort, scan, fill and the call's device allocations included -- after 3 untimed calls: the
median of `calls`.  Beside it, in the same process and on the host, the vectorised SciPy formulation of
tests/_graph_reference.py (sparse transpose, multiply and add) by the wall clock: the median of `scipy_calls`, the
calibration of the umap weights in NumPy apart from the sparse algebra.  One JSON line, also written to `out`."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _graph_reference import numpy_calibration, scipy_graph  # noqa: E402
from _knn_reference import gamma_scores  # noqa: E402
from knn_time import event_ms  # noqa: E402
import schpf_amd  # noqa: E402
from schpf_amd import _lib  # noqa: E402


def wall_ms(fn, calls):
    """(times, the last call's result)"""
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        result = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ms)), 1), "min_ms": round(min(ms), 1), "max_ms": round(max(ms), 1)}, result


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    n, K, k, calls = int(kv.get("n", 100000)), int(kv.get("K", 20)), int(kv.get("k", 15)), int(kv.get("calls", 10))
    scipy_calls = int(kv.get("scipy_calls", 3))
    _lib.require_gpu()
    lib = _lib.load()
    idx, dist = schpf_amd.knn(torch.tensor(gamma_scores(n, K, np.float64, seed=0), device="cuda:0"), k=k)
    indptr = torch.empty(n + 1, dtype=torch.int64, device="cuda:0")
    cols = torch.empty(2 * n * k, dtype=torch.int32, device="cuda:0")
    data = torch.empty(2 * n * k, dtype=torch.float64, device="cuda:0")
    stream = int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    h_idx, h_dist = idx.cpu().numpy(), dist.cpu().numpy()
    out = {"n": n, "K": K, "k": k, "directed_edges": n * k, "calls": calls, "scipy_calls": scipy_calls,
           "device": torch.cuda.get_device_name(0), "host_threads": len(os.sched_getaffinity(0))}
    for method, code in (("umap", _lib.GRAPH_UMAP), ("jaccard", _lib.GRAPH_JACCARD)):
        def hip():
            _lib.check(lib.schpf_knn_graph_device(0, ctypes.c_void_p(stream), code, n, k, p(idx), p(dist), p(indptr), p(cols),
                                                  p(data), None, None))

        rec = {"schpf_knn_graph_device": event_ms(hip, calls)}
        rec["nnz"] = int(indptr[n])
        if scipy_calls > 0:
            w = None
            if method == "umap":
                rec["numpy_calibration"], calibrated = wall_ms(lambda: numpy_calibration(h_dist), scipy_calls)
                w = calibrated[2]
            rec["scipy_sparse_algebra"], G = wall_ms(lambda: scipy_graph(h_idx, h_dist, method, w=w), scipy_calls)
            host_ms = rec["scipy_sparse_algebra"]["median_ms"] + rec.get("numpy_calibration", {"median_ms": 0.0})["median_ms"]
            rec["scipy_total_ms"] = round(host_ms, 1)
            rec["scipy_over_hip"] = round(host_ms / rec["schpf_knn_graph_device"]["median_ms"], 1)
            hip()
            torch.cuda.synchronize()
            nnz = rec["nnz"]
            from scipy.sparse import csr_matrix
            ours = csr_matrix((data[:nnz].cpu().numpy(), cols[:nnz].cpu().numpy(), indptr.cpu().numpy()), shape=(n, n))
            diff = abs(ours - G)
            rec["max_abs_difference_from_scipy"] = float(diff.max()) if diff.nnz else 0.0
        out[method] = rec
    line = json.dumps(out)
    print(line, flush=True)
    if "out" in kv:
        with open(kv["out"], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
