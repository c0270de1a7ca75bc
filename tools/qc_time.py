#!/usr/bin/env python
"""Time the axis statistics and the submatrix of the cell and gene filtering (GPU box):
    python tools/qc_time.py [shapes=100000x20000@200,100000x20000@1000,1000000x25000@200] [calls=10] [torch=1]
                            [torch_calls=3] [submatrix=1] [append=0] [out=profiles/qc/qc_time.json]
A shape N x J @ draws: synthetic counts from the marker tests' maker (tests/_ranksum_reference.py sparse_entries: N * draws
draws, skewed gene popularity), brought to canonical CSR (int64 indptr, int32 columns, int32 counts) once on the GPU, not
timed.  Two gene sets: the first 13 genes and every 200th gene.  The submatrix drops a random 6 % of the cells and a random
half of the genes.

Each call is timed with HIP events around the whole call on torch's current stream -- validation, scans, the call's device
allocations and its copies to the host included -- after 3 untimed calls, the median of `calls`:
  * schpf_axis_stats_device;
  * schpf_submatrix_device as the sizing call (NULL outputs), as the filling call, and both with the allocation of the
    outputs between them, which is what schpf_amd.submatrix does.
Beside each:
  * the bytes the call must move -- the statistics read column and count of every entry, the row pointers and the flags once
    and write their outputs; the submatrix reads column and value of every entry of the listed rows, the row pointers, the
    list and the mask, and writes the result -- and the time they take at the HBM peak of 8 TB/s (MI355X);
  * torch=1: a torch formulation on the same GPU with equal results, timed the same way over torch_calls calls after one
    untimed call.  Statistics: bincount and index_add_ on int64 over the COO row numbers, which it is given for nothing.
    Submatrix: index_select of the rows from the sparse COO matrix, then a column mask and a renumbering.
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
N_SETS = 2


def at_peak(rec, key, must_move):
    rec[key + "_bytes_must_move"] = must_move
    rec[key + "_ms_at_hbm_peak"] = round(must_move / HBM_PEAK * 1e3, 3)
    rec[key + "_over_hbm_peak"] = round(rec[key]["median_ms"] / (must_move / HBM_PEAK * 1e3), 2)


def one_shape(lib, N, J, draws, calls, with_torch, torch_calls, with_submatrix):
    dev = "cuda:0"
    cells, genes, values = sparse_entries(N, J, draws, seed=0)
    X = torch.sparse_coo_tensor(torch.stack([torch.tensor(cells, device=dev).long(), torch.tensor(genes, device=dev).long()]),
                                torch.tensor(values, device=dev), size=(N, J)).coalesce()      # float32: exact counts
    del cells, genes, values
    rows = X.indices()[0]
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    indices, data = X.indices()[1].to(torch.int32).contiguous(), X.values().to(torch.int32).contiguous()
    nnz = int(data.numel())
    stream = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    matrix = (N, J, nnz, p(indptr), _lib.IDX_I64, p(indices), _lib.IDX_I32, p(data), _lib.VAL_I32)
    rec = {"ncells": N, "ngenes": J, "draws_per_cell": draws, "nnz": nnz, "longest_row": int((indptr[1:] - indptr[:-1]).max()),
           "calls": calls, "hbm_peak_bytes_per_second": HBM_PEAK}

    flags_host = np.zeros(J, np.uint32)
    flags_host[:13] |= 1
    flags_host[::200] |= 2
    flags = torch.from_numpy(flags_host.view(np.int32)).to(dev)
    cell = torch.zeros((2 + N_SETS, N), dtype=torch.int64, device=dev)
    gene = torch.zeros((3, J), dtype=torch.int64, device=dev)

    def stats():
        _lib.check(lib.schpf_axis_stats_device(0, stream, *(matrix + (N_SETS, p(flags), p(cell[0]), p(cell[1]), p(cell[2:]), p(gene[0]),
                                                                       p(gene[1]), p(gene[2])))))

    rec["axis_stats"] = event_ms(stats, calls)
    at_peak(rec, "axis_stats", 8 * nnz + 8 * (N + 1) + 4 * J + 8 * (2 + N_SETS) * N + 24 * J)
    rec["entries_per_second"] = round(nnz / (rec["axis_stats"]["median_ms"] * 1e-3))
    print("%d x %d @ %d: statistics %s" % (N, J, draws, rec["axis_stats"]), file=sys.stderr, flush=True)
    if with_torch:
        cols, kept = indices.long(), {}
        in_set = [((flags >> s) & 1).to(torch.int64) for s in range(N_SETS)]

        def formulation():
            v = data.to(torch.int64)
            pos = v > 0
            zc, zg = (lambda: torch.zeros(N, dtype=torch.int64, device=dev)), (lambda: torch.zeros(J, dtype=torch.int64, device=dev))
            kept["out"] = [torch.bincount(rows[pos], minlength=N), zc().index_add_(0, rows, v),
                           torch.stack([zc().index_add_(0, rows, v * s[cols]) for s in in_set]),
                           torch.bincount(cols[pos], minlength=J), zg().index_add_(0, cols, v), zg().index_add_(0, cols, v * v)]

        try:
            rec["torch_bincount_index_add"] = event_ms(formulation, torch_calls, warm=1)
            rec["torch_over_axis_stats"] = round(rec["torch_bincount_index_add"]["median_ms"] / rec["axis_stats"]["median_ms"], 2)
            rec["torch_stats_equal"] = all(bool(torch.equal(a, b)) for a, b in
                                           zip(kept["out"], (cell[0], cell[1], cell[2:], gene[0], gene[1], gene[2])))
        except RuntimeError as e:
            rec["torch_bincount_index_add"] = "failed: " + str(e).splitlines()[0][:200]
        kept.clear()
    if not with_submatrix:
        return rec

    rng = np.random.RandomState(1)
    picked = torch.from_numpy(np.flatnonzero(rng.random_sample(N) >= 0.06).astype(np.int32)).to(dev)
    keep = torch.from_numpy((rng.random_sample(J) < 0.5).astype(np.uint8)).to(dev)
    n_rows = int(picked.numel())
    out_ngenes, out_indptr = ctypes.c_int64(0), torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    args = (0, stream) + matrix + (n_rows, p(picked), p(keep), ctypes.byref(out_ngenes), p(out_indptr))
    out = {}

    def sizing():
        _lib.check(lib.schpf_submatrix_device(*(args + (None, None, 0))))

    sizing()
    total = int(out_indptr[-1])
    out["indices"] = torch.empty(total, dtype=torch.int32, device=dev)
    out["values"] = torch.empty(total, dtype=torch.int32, device=dev)

    def filling():
        _lib.check(lib.schpf_submatrix_device(*(args + (p(out["indices"]), p(out["values"]), total))))

    def both():
        sizing()
        n = int(out_indptr[-1])
        out["indices"], out["values"] = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        filling()

    lengths = indptr[1:] - indptr[:-1]
    read = int(lengths[picked.long()].sum())
    rec.update({"n_rows": n_rows, "out_ngenes": int(out_ngenes.value), "out_nnz": total, "submatrix_sizing_call": event_ms(sizing, calls),
                "submatrix_filling_call": event_ms(filling, calls), "submatrix": event_ms(both, calls)})
    at_peak(rec, "submatrix", 8 * read + 8 * total + 16 * n_rows + 4 * n_rows + J + 8 * (n_rows + 1))
    print("%d x %d @ %d: submatrix %s" % (N, J, draws, rec["submatrix"]), file=sys.stderr, flush=True)
    if with_torch:
        picked_long, keep_bool = picked.long(), keep.bool()
        colmap = torch.cumsum(keep_bool.to(torch.int64), 0) - 1
        kept = {}

        def formulation():
            A = torch.index_select(X, 0, picked_long)
            idx = A._indices()
            m = keep_bool[idx[1]]
            kept["rows"], kept["cols"], kept["vals"] = idx[0][m], colmap[idx[1][m]], A._values()[m]

        try:
            rec["torch_index_select_mask"] = event_ms(formulation, torch_calls, warm=1)
            rec["torch_over_submatrix"] = round(rec["torch_index_select_mask"]["median_ms"] / rec["submatrix"]["median_ms"], 2)
            S = torch.sparse_coo_tensor(torch.stack([kept["rows"], kept["cols"]]), kept["vals"], size=(n_rows, int(out_ngenes.value))).coalesce()
            crow = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
            crow[1:] = torch.cumsum(torch.bincount(S.indices()[0], minlength=n_rows), 0)
            rec["torch_submatrix_equal"] = bool(S._nnz() == total and torch.equal(crow, out_indptr)
                                                and torch.equal(S.indices()[1].to(torch.int32), out["indices"])
                                                and torch.equal(S.values().to(torch.int32), out["values"]))
        except RuntimeError as e:       # out of memory, or a size torch's sparse kernels do not take
            rec["torch_index_select_mask"] = "failed: " + str(e).splitlines()[0][:200]
    return rec


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    calls = int(kv.get("calls", 10))
    shapes = [(s.split("@")[0].split("x"), s.split("@")[1]) for s in
              kv.get("shapes", "100000x20000@200,100000x20000@1000,1000000x25000@200").split(",")]
    out = kv.get("out", os.path.join(ROOT, "profiles", "qc", "qc_time.json"))
    _lib.require_gpu()
    lib = _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "shapes": []}
    if kv.get("append", "0") == "1" and os.path.exists(out):
        result["shapes"] = json.load(open(out))["shapes"]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for (N, J), draws in shapes:
        result["shapes"].append(one_shape(lib, int(N), int(J), int(draws), calls, kv.get("torch", "1") == "1",
                                          int(kv.get("torch_calls", 3)), kv.get("submatrix", "1") == "1"))
        print(json.dumps(result["shapes"][-1]), flush=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(result) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
