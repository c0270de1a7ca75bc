#!/usr/bin/env python
"""Time the sum of simulated doublets (GPU box):
    python tools/doublets_time.py [shapes=100000x20000@200,100000x20000@1000,1000000x25000@200] [ratio=2] [calls=10]
                                  [torch=1] [torch_calls=3] [append=0] [out=profiles/doublets/doublets_time.json]
A shape N x J @ draws: synthetic counts from the marker tests' maker (tests/_ranksum_reference.py sparse_entries: N * draws
draws, skewed gene popularity), brought to canonical CSR (int64 indptr, int32 columns, int32 counts) once on the GPU, not
timed; n_pairs = ratio * N pairs from schpf_doublet_parents_device, seed 0.

schpf_doublet_rows_device is timed with HIP events around the whole call on torch's current stream -- validation, the
length pass, the scan and the call's device allocations included -- after 3 untimed calls, the median of `calls`: once as
the sizing call (NULL outputs) and once as the filling call.  Beside them:
  * the bytes the sum must move -- both parents read once (column and count of every entry), the result written once, the
    pairs read and the row pointers written -- and the time they take at the HBM peak of 8 TB/s (MI355X); ratio = the
    filling call's time over that time;
  * torch=1: a torch formulation on the same GPU, index_select of both parent sets from the sparse COO matrix, their
    entries concatenated into one COO and coalesce()d; timed the same way over torch_calls calls after one untimed call, its
    values checked against the library's; ratio = its time over the filling call's.
One JSON line with a record per shape, also written to `out` after every shape (append=1: added to the shapes already
there)."""
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


def one_shape(lib, N, J, draws, ratio, calls, with_torch, torch_calls):
    cells, genes, values = sparse_entries(N, J, draws, seed=0)
    X = torch.sparse_coo_tensor(torch.stack([torch.tensor(cells, device="cuda:0").long(), torch.tensor(genes, device="cuda:0").long()]),
                                torch.tensor(values, device="cuda:0"), size=(N, J)).coalesce()      # float32: exact counts
    del cells, genes, values
    rows = X.indices()[0]
    indptr = torch.zeros(N + 1, dtype=torch.int64, device="cuda:0")
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    indices, data = X.indices()[1].to(torch.int32).contiguous(), X.values().to(torch.int32).contiguous()
    nnz, n_pairs = int(data.numel()), int(round(ratio * N))
    stream = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    parents = torch.empty((n_pairs, 2), dtype=torch.int32, device="cuda:0")
    _lib.check(lib.schpf_doublet_parents_device(0, stream, 0, n_pairs, N, ctypes.c_uint64(0), p(parents)))
    out_indptr = torch.zeros(n_pairs + 1, dtype=torch.int64, device="cuda:0")
    args = (0, stream, N, J, nnz, p(indptr), _lib.IDX_I64, p(indices), _lib.IDX_I32, p(data), _lib.VAL_I32, n_pairs, p(parents),
            p(out_indptr))

    def sizing():
        _lib.check(lib.schpf_doublet_rows_device(*(args + (None, None, 0))))

    sizing()
    total = int(out_indptr[-1])
    out_indices = torch.empty(total, dtype=torch.int32, device="cuda:0")
    out_values = torch.empty(total, dtype=torch.int32, device="cuda:0")

    def filling():
        _lib.check(lib.schpf_doublet_rows_device(*(args + (p(out_indices), p(out_values), total))))

    lengths = indptr[1:] - indptr[:-1]
    read = int(lengths[parents[:, 0].long()].sum() + lengths[parents[:, 1].long()].sum())
    must_move = 8 * read + 8 * total + 8 * n_pairs + 8 * (n_pairs + 1)
    rec = {"ncells": N, "ngenes": J, "draws_per_cell": draws, "nnz": nnz, "n_pairs": n_pairs, "out_nnz": total,
           "longest_row": int(lengths.max()), "calls": calls, "sizing_call": event_ms(sizing, calls),
           "filling_call": event_ms(filling, calls), "bytes_must_move": must_move, "hbm_peak_bytes_per_second": HBM_PEAK,
           "ms_at_hbm_peak": round(must_move / HBM_PEAK * 1e3, 3)}
    rec["filling_over_hbm_peak"] = round(rec["filling_call"]["median_ms"] / (must_move / HBM_PEAK * 1e3), 2)
    rec["out_entries_per_second"] = round(total / (rec["filling_call"]["median_ms"] * 1e-3))
    if with_torch:
        print("%d x %d @ %d: %s, %s; torch runs ..." % (N, J, draws, rec["sizing_call"], rec["filling_call"]), file=sys.stderr, flush=True)
        a, b = parents[:, 0].long(), parents[:, 1].long()
        kept = {}

        def formulation():
            A, B = torch.index_select(X, 0, a), torch.index_select(X, 0, b)
            kept["sum"] = torch.sparse_coo_tensor(torch.cat([A._indices(), B._indices()], 1), torch.cat([A._values(), B._values()]),
                                                  size=(n_pairs, J)).coalesce()

        try:
            rec["torch_index_select_coalesce"] = event_ms(formulation, torch_calls, warm=1)
            rec["torch_over_filling"] = round(rec["torch_index_select_coalesce"]["median_ms"] / rec["filling_call"]["median_ms"], 2)
            S = kept["sum"]
            rec["torch_equal"] = bool(S._nnz() == total and torch.equal(S.indices()[1].to(torch.int32), out_indices)
                                      and torch.equal(S.values().to(torch.int32), out_values))
        except RuntimeError as e:       # out of memory, or a size torch's sparse kernels do not take
            rec["torch_index_select_coalesce"] = "failed: " + str(e).splitlines()[0][:200]
    return rec


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    ratio, calls = float(kv.get("ratio", 2)), int(kv.get("calls", 10))
    shapes = [(s.split("@")[0].split("x"), s.split("@")[1]) for s in
              kv.get("shapes", "100000x20000@200,100000x20000@1000,1000000x25000@200").split(",")]
    out = kv.get("out", os.path.join(ROOT, "profiles", "doublets", "doublets_time.json"))
    _lib.require_gpu()
    lib = _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "shapes": []}
    if kv.get("append", "0") == "1" and os.path.exists(out):
        result["shapes"] = json.load(open(out))["shapes"]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for (N, J), draws in shapes:
        result["shapes"].append(one_shape(lib, int(N), int(J), int(draws), ratio, calls, kv.get("torch", "1") == "1",
                                          int(kv.get("torch_calls", 3))))
        print(json.dumps(result["shapes"][-1]), flush=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(result) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
