#!/usr/bin/env python
"""Time the Louvain clustering (GPU box): python tools/louvain_time.py [n=100000,1000000] [K=20] [k=15] [calls=10]
                                                                     [host=1] [networkx_max=100000] [out=FILE]

For every n: the exact self graph of n x K float64 scores drawn as tests/_knn_reference.py draws them is searched and
turned into the Jaccard graph once (schpf_amd.knn, knn_connectivities, on the GPU; not timed).  schpf_louvain_device is
then timed with HIP events around the whole call on torch's current stream -- validation, quantisation, every round's
sorts and reductions, the aggregations and the call's device allocations included -- after 3 untimed calls: the median of
`calls`.  With it the communities, the levels that moved a vertex, the rounds of all levels (the library reports the rounds
in all: per level it is the mean that is recorded) and the modularity.  host=1: beside it, by the wall clock and once,
the library's serial restatement schpf_debug_louvain on the host -- whose labels must be the GPU's -- and, up to
`networkx_max` vertices and where networkx can be imported, networkx's louvain_communities (seed 0) with its modularity.
One JSON line with a record per n, also written to `out`."""
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
from _knn_reference import gamma_scores  # noqa: E402
from knn_time import event_ms  # noqa: E402
import schpf_amd  # noqa: E402
from schpf_amd import _lib  # noqa: E402

I64P = ctypes.POINTER(ctypes.c_int64)


def one_shape(lib, n, K, k, calls, host, networkx_max):
    from scipy.sparse import csr_matrix
    idx, dist = schpf_amd.knn(torch.tensor(gamma_scores(n, K, np.float64, seed=0), device="cuda:0"), k=k)
    G = schpf_amd.knn_connectivities(idx, dist, method="jaccard")
    indptr = G.crow_indices().to(torch.int64).contiguous()
    cols = G.col_indices().to(torch.int32).contiguous()
    data = G.values().contiguous()
    del idx, dist
    labels = torch.empty(n, dtype=torch.int32, device="cuda:0")
    stats = np.zeros(4, np.int64)
    stream = int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def hip():
        _lib.check(lib.schpf_louvain_device(0, ctypes.c_void_p(stream), n, p(indptr), p(cols), p(data), 1.0, p(labels),
                                            stats.ctypes.data_as(I64P)))

    rec = {"n": n, "K": K, "k": k, "graph": "jaccard", "nnz": int(data.numel()), "resolution": 1.0, "calls": calls,
           "schpf_louvain_device": event_ms(hip, calls)}
    h_labels = labels.cpu().numpy()
    h = csr_matrix((data.cpu().numpy(), cols.cpu().numpy(), indptr.cpu().numpy()), shape=(n, n))
    rec.update(communities=int(stats[0]), levels=int(stats[1]), rounds=int(stats[2]),
               mean_rounds_per_level=round(float(stats[2]) / max(1, int(stats[1]) + 1), 1),
               modularity=round(schpf_amd.modularity(h, h_labels), 6))
    if host:
        from _louvain_reference import debug_louvain
        print("n = %d: %s on the GPU; the host restatement runs ..." % (n, rec["schpf_louvain_device"]), file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        want, want_stats = debug_louvain((h.indptr, h.indices, h.data))
        rec["schpf_debug_louvain_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["host_over_hip"] = round(rec["schpf_debug_louvain_host_ms"] / rec["schpf_louvain_device"]["median_ms"], 1)
        rec["labels_equal_host"] = bool(np.array_equal(want, h_labels) and np.array_equal(want_stats, stats))
        try:
            import networkx as nx
        except ImportError:
            nx = None
        if nx is not None and n <= networkx_max:
            N = nx.from_scipy_sparse_array(h)
            t0 = time.perf_counter()
            found = nx.community.louvain_communities(N, weight="weight", resolution=1.0, seed=0)
            rec["networkx_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            theirs = np.empty(n, np.int64)
            for c, members in enumerate(found):
                theirs[list(members)] = c
            rec["networkx_communities"] = len(found)
            rec["networkx_modularity"] = round(schpf_amd.modularity(h, theirs), 6)
            rec["networkx_over_hip"] = round(rec["networkx_ms"] / rec["schpf_louvain_device"]["median_ms"], 1)
        else:
            rec["networkx_ms"] = None       # not importable, or more vertices than networkx_max
    return rec


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    sizes = [int(s) for s in kv.get("n", "100000,1000000").split(",")]
    K, k, calls = int(kv.get("K", 20)), int(kv.get("k", 15)), int(kv.get("calls", 10))
    _lib.require_gpu()
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0), "host_threads": len(os.sched_getaffinity(0)), "shapes": []}
    for n in sizes:
        out["shapes"].append(one_shape(lib, n, K, k, calls, kv.get("host", "1") == "1", int(kv.get("networkx_max", 100000))))
        print(json.dumps(out["shapes"][-1]), flush=True)
    line = json.dumps(out)
    print(line, flush=True)
    if "out" in kv:
        with open(kv["out"], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
