#!/usr/bin/env python
"""Time the group statistics of the pseudobulk against two torch formulations of the group sums (GPU box):
    python tools/group_stats_time.py [shape=1000000x25000@200] [groups=20,2000] [calls=10] [torch_calls=3]
                                     [out=profiles/aggregate/group_stats_time.json]
The shape N x J @ draws: synthetic counts from the marker tests' maker (tests/_ranksum_reference.py sparse_entries: N * draws
draws, skewed gene popularity), brought to canonical CSR (int64 indptr, int32 columns, int32 counts) once on the GPU, not
timed.  Labels: G groups of uneven size -- group g is drawn with a weight of 1 / (g + 1), so the largest holds about a
hundred times the cells of the smallest at G = 2 000 -- and every 50th cell in no group.

Per G, each timed with HIP events around the whole call on torch's current stream after untimed warm-up calls, the median:
  * schpf_group_stats_device with all four outputs, and with sumsq = NULL -- validation, the sort of the cells, the slab
    table, the call's device allocations, the zeroing of the outputs and its copies to the host included;
  * the formulation of markers._group_sums: a dense N x (G + 1) float64 one-hot matrix and torch.sparse.mm on the transposed
    matrix.  The sums only; exact, as every sum is an integer below 2^53;
  * torch.index_add_ of the int64 values into a (G + 1) x J table over the coalesced COO, whose row numbers it is given for
    nothing.  The sums only.
First all three sums are asserted equal.  Beside the library's times: the bytes the call must move -- column and count of
every entry, the row pointers and the labels once, the outputs written -- and the time they take at the HBM peak of 8 TB/s
(MI355X).  One JSON line, also written to `out`."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _ranksum_reference import sparse_entries  # noqa: E402
from knn_time import event_ms  # noqa: E402
from schpf_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12      # bytes per second, MI355X


def uneven_labels(N, G, seed=3):
    rng = np.random.RandomState(seed)
    weight = 1.0 / (1.0 + np.arange(G))
    labels = rng.choice(G, N, p=weight / weight.sum()).astype(np.int32)
    labels[::50] = -1
    return labels


def one_count(lib, matrix, rows, cols, data, N, J, nnz, G, calls, torch_calls):
    dev = "cuda:0"
    stream = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    host_labels = uneven_labels(N, G)
    sizes = np.bincount(host_labels[host_labels >= 0], minlength=G)
    labels = torch.from_numpy(host_labels).to(dev)
    n = torch.zeros(G, dtype=torch.int64, device=dev)
    out = torch.zeros((3, G, J), dtype=torch.int64, device=dev)
    rec = {"ngroups": G, "largest_group": int(sizes.max()), "smallest_group": int(sizes.min()), "cells_in_no_group": int((host_labels < 0).sum())}

    def full():
        _lib.check(lib.schpf_group_stats_device(0, stream, *(matrix + (p(labels), G, p(n), p(out[0]), p(out[1]), p(out[2])))))

    def sums_only():
        _lib.check(lib.schpf_group_stats_device(0, stream, *(matrix + (p(labels), G, p(n), p(out[0]), p(out[1]), None))))

    lab = torch.where(labels >= 0, labels, torch.full_like(labels, G)).long()
    kept = {}

    def index_add():
        table = torch.zeros((G + 1) * J, dtype=torch.int64, device=dev)
        kept["sums"] = table.index_add_(0, lab[rows] * J + cols, data.to(torch.int64)).view(G + 1, J)[:G]

    def one_hot():                       # markers._group_sums, as it stands there
        values = data.to(torch.float64)
        onehot = torch.zeros((N, G + 1), dtype=torch.float64, device=dev)
        onehot[torch.arange(N, device=dev), lab] = 1.0
        both = torch.sparse.mm(torch.sparse_coo_tensor(torch.stack([cols, rows]), values, size=(J, N)), onehot)
        kept["sums"] = both.t()[:G]

    # first: all three give equal sums (these calls are also the first warm-up of each)
    full()
    assert bool(torch.equal(n.cpu(), torch.from_numpy(sizes))), "group_cells"
    formulations = []
    for key, fn in (("torch_index_add", index_add), ("torch_one_hot_sparse_mm", one_hot)):
        try:
            fn()
            assert bool(torch.equal(kept["sums"].to(torch.int64), out[1])), key + ": the sums differ"
            rec[key + "_sums_equal"] = True
            formulations.append((key, fn))
        except RuntimeError as e:       # out of memory, or a size torch's sparse kernels do not take
            rec[key] = "failed: " + str(e).splitlines()[0][:200]
        kept.clear()

    for key, fn, tables in (("group_stats", full, 3), ("group_stats_without_sumsq", sums_only, 2)):
        rec[key] = event_ms(fn, calls)
        must_move = 8 * nnz + 8 * (N + 1) + 4 * N + 8 * G + 8 * tables * G * J
        rec[key + "_bytes_must_move"] = must_move
        rec[key + "_ms_at_hbm_peak"] = round(must_move / HBM_PEAK * 1e3, 3)
        rec[key + "_share_of_hbm_peak"] = round(must_move / HBM_PEAK * 1e3 / rec[key]["median_ms"], 4)
    rec["entries_per_second"] = round(nnz / (rec["group_stats"]["median_ms"] * 1e-3))
    print("G = %d: group_stats %s, without sumsq %s" % (G, rec["group_stats"], rec["group_stats_without_sumsq"]), file=sys.stderr, flush=True)
    for key, fn in formulations:
        rec[key] = event_ms(fn, torch_calls, warm=1)
        rec[key + "_over_group_stats"] = round(rec[key]["median_ms"] / rec["group_stats"]["median_ms"], 2)
        rec[key + "_over_group_stats_without_sumsq"] = round(rec[key]["median_ms"] / rec["group_stats_without_sumsq"]["median_ms"], 2)
        kept.clear()
        print("G = %d: %s %s" % (G, key, rec[key]), file=sys.stderr, flush=True)
    return rec


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    shape, draws = kv.get("shape", "1000000x25000@200").split("@")
    N, J, draws = int(shape.split("x")[0]), int(shape.split("x")[1]), int(draws)
    calls, torch_calls = int(kv.get("calls", 10)), int(kv.get("torch_calls", 3))
    out = kv.get("out", os.path.join(ROOT, "profiles", "aggregate", "group_stats_time.json"))
    _lib.require_gpu()
    lib = _lib.load()
    dev = "cuda:0"
    cells, genes, values = sparse_entries(N, J, draws, seed=0)
    X = torch.sparse_coo_tensor(torch.stack([torch.tensor(cells, device=dev).long(), torch.tensor(genes, device=dev).long()]),
                                torch.tensor(values, device=dev), size=(N, J)).coalesce()      # float32: exact counts
    del cells, genes, values
    rows, cols = X.indices()[0].contiguous(), X.indices()[1].contiguous()
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    indices, data = cols.to(torch.int32).contiguous(), X.values().to(torch.int32).contiguous()
    del X
    nnz = int(data.numel())
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    matrix = (N, J, nnz, p(indptr), _lib.IDX_I64, p(indices), _lib.IDX_I32, p(data), _lib.VAL_I32)
    result = {"device": torch.cuda.get_device_name(0), "ncells": N, "ngenes": J, "draws_per_cell": draws, "nnz": nnz,
              "longest_row": int((indptr[1:] - indptr[:-1]).max()), "calls": calls, "torch_calls": torch_calls,
              "hbm_peak_bytes_per_second": HBM_PEAK, "groups": []}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for G in [int(g) for g in kv.get("groups", "20,2000").split(",")]:
        result["groups"].append(one_count(lib, matrix, rows, cols, data, N, J, nnz, G, calls, torch_calls))
        with open(out, "w") as fh:
            fh.write(json.dumps(result) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
