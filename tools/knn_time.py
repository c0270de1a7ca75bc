#!/usr/bin/env python
"""Time the exact k-NN of cell scores (GPU box): python tools/knn_time.py [n=100000] [K=20] [k=15] [calls=10] [torch=1]
                                                                        [n_query=0] [out=FILE]

The self graph of n x K float64 scores drawn as tests/_knn_reference.py draws them (n_query > 0: that many rows of a
second draw against the n, label transfer).  schpf_knn_device is timed with HIP events on torch's current stream --
table build, validation, selection and its device allocations included -- after 3 untimed calls: the median of `calls`.
torch=1 times, in the same process, the chunked torch formulation in float64 (torch.cdist on 4096 query rows at a time,
then topk) and counts the rows on which both return the same neighbours.  One JSON line, also written to `out`."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _knn_reference import gamma_scores  # noqa: E402
from schpf_amd import _lib  # noqa: E402


def event_ms(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    n, K, k, calls = int(kv.get("n", 100000)), int(kv.get("K", 20)), int(kv.get("k", 15)), int(kv.get("calls", 10))
    n_query = int(kv.get("n_query", 0))
    _lib.require_gpu()
    lib = _lib.load()
    ref = torch.tensor(gamma_scores(n, K, np.float64, seed=0), device="cuda:0")
    query = torch.tensor(gamma_scores(n_query, K, np.float64, seed=1), device="cuda:0") if n_query else ref
    self_first = -1 if n_query else 0
    nq = query.shape[0]
    idx = torch.empty((nq, k), dtype=torch.int32, device="cuda:0")
    d2 = torch.empty((nq, k), dtype=torch.float64, device="cuda:0")
    stream = int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def hip():
        _lib.check(lib.schpf_knn_device(0, ctypes.c_void_p(stream), _lib.F64, nq, n, K, p(query), p(ref), k,
                                        ctypes.c_int64(self_first), p(idx), p(d2)))

    out = {"n_query": nq, "n_ref": n, "K": K, "k": k, "self_graph": not n_query, "calls": calls,
           "device": torch.cuda.get_device_name(0), "schpf_knn_device": event_ms(hip, calls)}
    if kv.get("torch", "1") == "1":
        t_idx = torch.empty((nq, k), dtype=torch.int64, device="cuda:0")

        def chunked():
            for b in range(0, nq, 4096):
                d = torch.cdist(query[b:b + 4096], ref)
                if not n_query:      # a cell is not its own neighbour
                    rows = torch.arange(d.shape[0], device="cuda:0")
                    d[rows, b + rows] = float("inf")
                t_idx[b:b + 4096] = torch.topk(d, k, dim=1, largest=False).indices

        out["torch_cdist_topk"] = event_ms(chunked, calls)
        out["hip_over_torch"] = round(out["schpf_knn_device"]["median_ms"] / out["torch_cdist_topk"]["median_ms"], 3)
        hip()
        torch.cuda.synchronize()
        out["rows_with_equal_neighbours"] = int((t_idx == idx.to(torch.int64)).all(dim=1).sum())
    line = json.dumps(out)
    print(line, flush=True)
    if "out" in kv:
        with open(kv["out"], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
