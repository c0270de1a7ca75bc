#!/usr/bin/env python
"""Time the shortest-path distances (GPU box):
    python tools/geodesic_time.py [n=100000,1000000] [K=20] [k=15] [calls=10] [host=1] [out=profiles/knn/geodesic_time.json]

For every n: the graph of tools/components_time.py before it is weighted -- the exact 15-NN self graph of n x K float64 Gamma
scores, searched on the GPU, not timed -- as the DISTANCE graph `knn_graph` stores it (row i holds its k neighbours with their
Euclidean distances), read undirected.  schpf_geodesic_device is timed with HIP events around the whole call on torch's
current stream (validation, the rows of the entries, every tile with its rounds and its one fetch of the flags per batch, the
transposition and the call's device allocations included) after 3 untimed calls: the median of `calls`, for 1 root, for
ROOT_TILE roots (one full tile) and for 64 roots (64 / ROOT_TILE tiles), every root a set of its own.  With them the rounds
of the last call, the time per round, and what one unfiltered round of a full tile must move at the least -- 16 bytes per
entry, and every vertex's line of distances and its stamp once -- against the HBM peak of 8 TB/s.
host=1: beside them, by the wall clock and once, SciPy's dijkstra(directed=False) on the host for 1 root and for ROOT_TILE
roots, whose bits must be the GPU's.  One JSON line with a record per n, also written to `out`."""
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
from schpf_amd.paths import ROOT_TILE  # noqa: E402

I64P = ctypes.POINTER(ctypes.c_int64)
HBM_BYTES_PER_S = 8e12


def one_shape(lib, n, K, k, calls, host):
    idx, dist = schpf_amd.knn(torch.tensor(gamma_scores(n, K, np.float64, seed=0), device="cuda:0"), k=k)
    indptr = (torch.arange(n + 1, dtype=torch.int64, device="cuda:0") * k).contiguous()
    cols = idx.to(torch.int32).reshape(-1).contiguous()
    data = dist.to(torch.float64).reshape(-1).contiguous()
    del idx, dist
    nnz = int(cols.numel())
    stream = int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rng = np.random.RandomState(1)
    all_roots = rng.choice(n, 64, replace=False).astype(np.int32)
    stats = np.zeros(3, np.int64)
    rec = {"n": n, "K": K, "k": k, "graph": "knn distances, undirected", "nnz": nnz, "calls": calls, "root_tile": ROOT_TILE}
    rec["round_bytes_full_tile"] = 16 * nnz + (8 * ROOT_TILE + 4) * n
    rec["round_us_at_8TBps_full_tile"] = round(rec["round_bytes_full_tile"] / HBM_BYTES_PER_S * 1e6, 1)
    rec["round_bytes_one_root"] = 16 * nnz + 12 * n
    found = {}
    for nsets in (1, ROOT_TILE, 64):
        roots = torch.tensor(all_roots[:nsets], device="cuda:0")
        set_ptr = torch.arange(nsets + 1, dtype=torch.int64, device="cuda:0")
        out = torch.empty((nsets, n), dtype=torch.float64, device="cuda:0")

        def call():
            _lib.check(lib.schpf_geodesic_device(0, ctypes.c_void_p(stream), n, p(indptr), p(cols), p(data), 0, nsets, p(set_ptr),
                                                 p(roots), p(out), stats.ctypes.data_as(I64P)))

        timed = event_ms(call, calls)
        tiles = -(-nsets // ROOT_TILE)
        rec["roots_%d" % nsets] = dict(timed, tiles=tiles, finite=int(stats[0]), rounds=int(stats[1]), lowering_writes=int(stats[2]),
                                       rounds_per_tile=round(int(stats[1]) / tiles, 1),
                                       ms_per_round=round(timed["median_ms"] / max(int(stats[1]), 1), 4),
                                       largest_finite=float(out[torch.isfinite(out)].max()))
        if nsets <= ROOT_TILE:
            found[nsets] = out.cpu().numpy()
        del out
    if host:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import dijkstra
        h = csr_matrix((data.cpu().numpy(), cols.cpu().numpy(), indptr.cpu().numpy()), shape=(n, n))
        for nsets in (1, ROOT_TILE):
            t0 = time.perf_counter()
            theirs = dijkstra(h, directed=False, indices=all_roots[:nsets])
            ms = round((time.perf_counter() - t0) * 1e3, 1)
            rec["scipy_dijkstra_host_ms_roots_%d" % nsets] = ms
            rec["scipy_over_hip_roots_%d" % nsets] = round(ms / rec["roots_%d" % nsets]["median_ms"], 1)
            rec["bits_equal_scipy_roots_%d" % nsets] = bool(np.array_equal(theirs.view(np.int64), found[nsets].view(np.int64)))
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
    path = kv.get("out", os.path.join(ROOT, "profiles", "knn", "geodesic_time.json"))
    with open(path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
