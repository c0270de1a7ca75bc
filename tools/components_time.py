#!/usr/bin/env python
"""Time the connected components and the cluster graph (GPU box):
    python tools/components_time.py [n=100000,1000000] [K=20] [k=15] [calls=10] [host=1] [out=profiles/knn/components_time.json]

For every n: the Jaccard graph of tools/louvain_time.py -- the exact self graph of n x K float64 Gamma scores, searched
and made on the GPU, not timed -- and its Louvain labels.  schpf_components_device is then timed with HIP events around
the whole call on torch's current stream (validation, the rows of the entries, every hook round with its shortcut passes
and its one fetch of the flags, the numbering, the sizes and the call's device allocations included) after 3 untimed
calls: the median of `calls`, once on the whole graph and once `within` the Louvain labels; with them the components, the
hook rounds and the shortcut passes seen.  schpf_cluster_graph_device is timed the same way with the Louvain labels.
host=1: beside them, by the wall clock and once, SciPy's connected_components on the host, whose labelling must be the
GPU's.  One JSON line with a record per n, also written to `out`."""
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


def one_shape(lib, n, K, k, calls, host):
    idx, dist = schpf_amd.knn(torch.tensor(gamma_scores(n, K, np.float64, seed=0), device="cuda:0"), k=k)
    G = schpf_amd.knn_connectivities(idx, dist, method="jaccard")
    indptr = G.crow_indices().to(torch.int64).contiguous()
    cols = G.col_indices().to(torch.int32).contiguous()
    data = G.values().contiguous()
    del idx, dist
    labels = schpf_amd.louvain(G).contiguous()
    groups = int(labels.max()) + 1
    comp = torch.empty(n, dtype=torch.int32, device="cuda:0")
    cells = torch.empty(groups, dtype=torch.int64, device="cuda:0")
    count = torch.empty((groups, groups), dtype=torch.int64, device="cuda:0")
    weight = torch.empty((groups, groups), dtype=torch.int64, device="cuda:0")
    stats = np.zeros(6, np.int64)
    wmax = ctypes.c_double(0.0)
    stream = int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def components(within):
        _lib.check(lib.schpf_components_device(0, ctypes.c_void_p(stream), n, p(indptr), p(cols), within, p(comp),
                                               stats.ctypes.data_as(I64P)))

    def table():
        _lib.check(lib.schpf_cluster_graph_device(0, ctypes.c_void_p(stream), n, p(indptr), p(cols), p(data), p(labels), groups,
                                                  p(cells), p(count), p(weight), ctypes.byref(wmax)))

    rec = {"n": n, "K": K, "k": k, "graph": "jaccard", "nnz": int(data.numel()), "calls": calls, "louvain_communities": groups}
    rec["schpf_components_device"] = event_ms(lambda: components(None), calls)
    whole = comp.cpu().numpy()
    rec.update(components=int(stats[0]), largest=int(stats[1]), hook_rounds=int(stats[4]), shortcut_passes=int(stats[5]))
    rec["schpf_components_device_within"] = event_ms(lambda: components(p(labels)), calls)
    rec.update(components_within=int(stats[0]), hook_rounds_within=int(stats[4]), shortcut_passes_within=int(stats[5]))
    rec["schpf_cluster_graph_device"] = event_ms(table, calls)
    rec["entries_between_clusters"] = int(count.sum() - count.diagonal().sum())
    if host:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components
        h = csr_matrix((data.cpu().numpy(), cols.cpu().numpy(), indptr.cpu().numpy()), shape=(n, n))
        t0 = time.perf_counter()
        found, theirs = connected_components(h, directed=True, connection="weak")
        rec["scipy_connected_components_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["scipy_over_hip"] = round(rec["scipy_connected_components_host_ms"] / rec["schpf_components_device"]["median_ms"], 1)
        rec["labels_equal_scipy"] = bool(found == rec["components"] and np.array_equal(theirs, whole))
    return rec


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    sizes = [int(s) for s in kv.get("n", "100000,1000000").split(",")]
    K, k, calls = int(kv.get("K", 20)), int(kv.get("k", 15)), int(kv.get("calls", 10))
    _lib.require_gpu()
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0), "host_threads": len(os.sched_getaffinity(0)), "shapes": []}
    for n in sizes:
        out["shapes"].append(one_shape(lib, n, K, k, calls, kv.get("host", "1") == "1"))
        print(json.dumps(out["shapes"][-1]), flush=True)
    line = json.dumps(out)
    print(line, flush=True)
    path = kv.get("out", os.path.join(ROOT, "profiles", "knn", "components_time.json"))
    with open(path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
