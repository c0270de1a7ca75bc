#!/usr/bin/env python
"""Time the rank sums of the marker-gene test (GPU box):
    python tools/rank_sums_time.py [shapes=100000x20000,1000000x25000] [per_cell=200] [G=20] [calls=10] [slice=200] [host=1]
                                   [out=profiles/markers/rank_sums_time.json]
A shape may carry draws per cell of its own: 1000000x25000@1000.

For every shape N x J: synthetic counts from the tests' maker (tests/_ranksum_reference.py sparse_entries: N * per_cell draws,
skewed gene popularity), made gene-major once on the GPU (not timed), and G labels from a fixed seed.  schpf_rank_sums_device
is then timed with HIP events around the whole call on torch's current stream -- validation, the sort, the scans, the
accumulation and the call's device allocations included -- after 3 untimed calls: the median of `calls`.  host=1: beside it,
by the wall clock and once, on a slice of `slice` genes spread evenly over the matrix: the library's serial restatement
schpf_debug_rank_sums -- whose integers must be the GPU's -- and scipy.stats.mannwhitneyu of group 0 against the rest
(one call per gene; the library's slice answers all G groups).  One JSON line with a record per shape, also written to `out`."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _ranksum_reference import debug_rank_sums, random_labels, sparse_entries  # noqa: E402
from knn_time import event_ms  # noqa: E402
from schpf_amd import _lib  # noqa: E402
from schpf_amd.device_input import gpu_csc  # noqa: E402


def one_shape(lib, N, J, per_cell, G, calls, n_slice, host):
    cells, genes, values = sparse_entries(N, J, per_cell, seed=0)
    X = torch.sparse_coo_tensor(torch.stack([torch.tensor(cells, device="cuda:0").long(), torch.tensor(genes, device="cuda:0").long()]),
                                torch.tensor(values, device="cuda:0"), size=(N, J))
    del cells, genes, values
    indptr, cell_ids, data = gpu_csc(X)
    del X
    h_labels = random_labels(N, G, seed=1)
    labels = torch.tensor(h_labels, device="cuda:0")
    out = [torch.zeros(s, dtype=torch.int64, device="cuda:0") for s in ((G,), (J,), (J,), (G, J), (G, J))]
    stream = int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def hip():
        _lib.check(lib.schpf_rank_sums_device(0, ctypes.c_void_p(stream), N, J, p(indptr), p(cell_ids), p(data), p(labels), G,
                                              *[p(t) for t in out]))

    nnz = int(data.numel())
    rec = {"ncells": N, "ngenes": J, "per_cell": per_cell, "nnz": nnz, "ngroups": G, "calls": calls,
           "longest_gene": int((indptr[1:] - indptr[:-1]).max()), "schpf_rank_sums_device": event_ms(hip, calls)}
    rec["entries_per_second"] = round(nnz / (rec["schpf_rank_sums_device"]["median_ms"] * 1e-3))
    if host:
        print("%d x %d: %s on the GPU; the host slice runs ..." % (N, J, rec["schpf_rank_sums_device"]), file=sys.stderr, flush=True)
        from scipy.stats import mannwhitneyu
        picked = np.linspace(0, J - 1, min(n_slice, J)).astype(np.int64)
        h_indptr = indptr.cpu().numpy()
        parts = [(cell_ids[h_indptr[j]:h_indptr[j + 1]].cpu().numpy(), data[h_indptr[j]:h_indptr[j + 1]].cpu().numpy()) for j in picked]
        s_indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in parts])]).astype(np.int64)
        matrix = (N, len(picked), s_indptr, np.concatenate([c for c, _ in parts]), np.concatenate([v for _, v in parts]))
        t0 = time.perf_counter()
        want = debug_rank_sums(matrix, h_labels, G)
        rec["slice_genes"] = len(picked)
        rec["slice_nnz"] = int(s_indptr[-1])
        rec["schpf_debug_rank_sums_slice_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        mine = [t.cpu().numpy() for t in out]
        rec["slice_equal_host"] = bool(np.array_equal(want[0], mine[0]) and all(np.array_equal(w, m[..., picked])
                                                                              for w, m in zip(want[1:], mine[1:])))
        inside = h_labels == 0
        t0 = time.perf_counter()
        twice_u = np.empty(len(picked))
        for x, (c, v) in enumerate(parts):
            column = np.zeros(N, np.float32)
            column[c] = v
            twice_u[x] = 2 * mannwhitneyu(column[inside], column[~inside], method="asymptotic", use_continuity=False).statistic
        rec["scipy_mannwhitneyu_slice_one_group_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["slice_equal_scipy_u"] = bool(np.array_equal(twice_u, mine[4][0, picked] - mine[0][0] * (mine[0][0] + 1)))
    return rec


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    per_cell, G, calls = int(kv.get("per_cell", 200)), int(kv.get("G", 20)), int(kv.get("calls", 10))
    shapes = [(s.split("@")[0].split("x"), s.split("@")[1] if "@" in s else per_cell)
              for s in kv.get("shapes", "100000x20000,1000000x25000").split(",")]
    _lib.require_gpu()
    lib = _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "host_threads": len(os.sched_getaffinity(0)), "shapes": []}
    for (N, J), draws in shapes:
        result["shapes"].append(one_shape(lib, int(N), int(J), int(draws), G, calls, int(kv.get("slice", 200)), kv.get("host", "1") == "1"))
        print(json.dumps(result["shapes"][-1]), flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    out = kv.get("out", os.path.join(ROOT, "profiles", "markers", "rank_sums_time.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
