#!/usr/bin/env python
"""Time the transpose of a count matrix to gene-major (GPU box):
    python tools/gene_major_time.py [shapes=100000x20000@200,1000000x25000@200] [calls=10] [G=20]
                                    [out=profiles/gene_major/gene_major_time.json] [only=transpose]
A shape N x J @ draws: synthetic counts from the marker tests' maker (tests/_ranksum_reference.py sparse_entries: N * draws
draws, skewed gene popularity), as a canonical CSR tensor on the GPU with int64 indices and float32 values.

Timed with HIP events on torch's current stream around the whole call -- checks, scratch and output allocations included --
one untimed call, then the median, minimum and maximum of `calls`, all in one job:
  (a) schpf_transpose_device on the CSR tensor's arrays, float32 values out (what `gene_major(X)` runs);
  (b) `parent_gene_major`: what device_input.gpu_csc computed before -- the COO from the CSR, coalesce(), argsort of the
      64-bit keys cols * N + rows, the gathers, bincount and cumsum;
  (c) a library sort on the column alone: torch.sort(cols.to(torch.int32), stable=True), the gathers, bincount and cumsum;
  and end to end, before (the operator on the arrays of (b), the conversion inside the clock) and after: `residual_variance`
  and `rank_sums` (G groups) on the CSR tensor.
(a), (b) and (c) are compared bit for bit.  Recorded beside them: the algorithmic bytes -- 20 per entry with int32 columns and
float32 values: the columns read twice, the values once, 8 bytes written; the run's own index width is recorded too -- their
time at the HBM peak of 8 TB/s and the fraction of that roof (a) reaches.  only=transpose runs (a) alone, for a kernel trace.
One JSON line with a record per shape, also written to `out`."""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _ranksum_reference import random_labels, sparse_entries  # noqa: E402
from knn_time import event_ms  # noqa: E402
from schpf_amd import GeneMajor, _lib, markers, variable_genes  # noqa: E402

HBM_PEAK = 8.0e12      # bytes per second, MI355X


def parent_gene_major(X):
    """device_input.gpu_csc as it was before the transpose."""
    X = X.detach()
    if X.layout == torch.sparse_csr:
        crow = X.crow_indices().to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(X.shape[0], device=X.device), crow[1:] - crow[:-1])
        X = torch.sparse_coo_tensor(torch.stack([rows, X.col_indices().to(torch.int64)]), X.values(), size=tuple(X.shape))
    X = X.coalesce()
    rows, cols, values = X.indices()[0], X.indices()[1], X.values()
    N, J = int(X.shape[0]), int(X.shape[1])
    order = torch.argsort(cols * N + rows)
    indptr = torch.zeros(J + 1, dtype=torch.int64, device=X.device)
    if J:
        indptr[1:] = torch.cumsum(torch.bincount(cols, minlength=J), 0)
    return indptr, rows[order].to(torch.int32).contiguous(), values[order].to(torch.float32).contiguous()


def library_sort(X):
    """A stable sort of the 32-bit columns of a canonical CSR tensor, and the gathers."""
    N, J = int(X.shape[0]), int(X.shape[1])
    crow, cols = X.crow_indices(), X.col_indices()
    rows = torch.repeat_interleave(torch.arange(N, device=X.device, dtype=torch.int32), crow[1:] - crow[:-1])
    order = torch.sort(cols.to(torch.int32), stable=True)[1]
    indptr = torch.zeros(J + 1, dtype=torch.int64, device=X.device)
    indptr[1:] = torch.cumsum(torch.bincount(cols, minlength=J), 0)
    return indptr, rows[order].contiguous(), X.values()[order].to(torch.float32).contiguous()


def one_shape(lib, N, J, draws, calls, G, only):
    dev = "cuda:0"
    cells, genes, values = sparse_entries(N, J, draws, seed=0)
    X = torch.sparse_coo_tensor(torch.stack([torch.tensor(cells, device=dev).long(), torch.tensor(genes, device=dev).long()]),
                                torch.tensor(values, device=dev), size=(N, J)).coalesce()      # float32: exact counts
    del cells, genes, values
    rows, cols, vals = X.indices()[0], X.indices()[1].contiguous(), X.values().contiguous()
    crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    csr = torch.sparse_csr_tensor(crow, cols, vals, size=(N, J))
    del X, rows
    nnz = int(vals.numel())
    stream = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    kept = {}

    def transpose():
        indptr = torch.empty(J + 1, dtype=torch.int64, device=dev)
        cell_ids = torch.empty(nnz, dtype=torch.int32, device=dev)
        data = torch.empty(nnz, dtype=torch.float32, device=dev)
        _lib.check(lib.schpf_transpose_device(0, stream, N, J, nnz, p(crow), _lib.IDX_I64, p(cols), _lib.IDX_I64, p(vals),
                                              _lib.VAL_F32, _lib.VAL_F32, p(indptr), p(cell_ids), p(data), None))
        kept["a"] = (indptr, cell_ids, data)

    index_bytes = cols.element_size()
    rec = {"ncells": N, "ngenes": J, "draws_per_cell": draws, "nnz": nnz, "calls": calls, "hbm_peak_bytes_per_second": HBM_PEAK,
           "a_transpose_device": event_ms(transpose, calls, warm=1)}
    a = rec["a_transpose_device"]
    rec["algorithmic_bytes_int32_columns"] = 20 * nnz
    rec["algorithmic_bytes_this_run"] = (2 * index_bytes + 4 + 8) * nnz
    rec["ms_at_hbm_peak_int32_columns"] = round(20 * nnz / HBM_PEAK * 1e3, 3)
    rec["fraction_of_roof_int32_columns"] = round(20 * nnz / HBM_PEAK * 1e3 / a["median_ms"], 4)
    rec["fraction_of_roof_this_run"] = round(rec["algorithmic_bytes_this_run"] / HBM_PEAK * 1e3 / a["median_ms"], 4)
    rec["entries_per_second"] = round(nnz / (a["median_ms"] * 1e-3))
    print("%d x %d @ %d: (a) %s" % (N, J, draws, a), file=sys.stderr, flush=True)
    if only == "transpose":
        return rec

    def parent():
        kept["b"] = parent_gene_major(csr)

    def sort():
        kept["c"] = library_sort(csr)

    rec["b_parent_gpu_csc"] = event_ms(parent, calls, warm=1)
    rec["c_library_sort"] = event_ms(sort, calls, warm=1)
    rec["a_b_c_equal_bits"] = bool(all(torch.equal(x, y) and torch.equal(x, z) and x.dtype == y.dtype == z.dtype
                                       for x, y, z in zip(kept["a"], kept["b"], kept["c"])))
    rec["a_slowest_under_b_fastest"] = bool(a["max_ms"] < rec["b_parent_gpu_csc"]["min_ms"])
    rec["b_over_a"] = round(rec["b_parent_gpu_csc"]["median_ms"] / a["median_ms"], 2)
    rec["c_over_a"] = round(rec["c_library_sort"]["median_ms"] / a["median_ms"], 2)
    print("%d x %d @ %d: (b) %s (c) %s equal bits %s" % (N, J, draws, rec["b_parent_gpu_csc"], rec["c_library_sort"],
                                                        rec["a_b_c_equal_bits"]), file=sys.stderr, flush=True)
    kept.clear()

    labels = torch.tensor(random_labels(N, G, seed=1), device=dev)
    before = lambda: GeneMajor(*parent_gene_major(csr), shape=(N, J))  # noqa: E731
    rec["residual_variance_before"] = event_ms(lambda: variable_genes.residual_variance(before()), calls, warm=1)
    rec["residual_variance_after"] = event_ms(lambda: variable_genes.residual_variance(csr), calls, warm=1)
    rec["rank_sums_before"] = event_ms(lambda: markers.rank_sums(before(), labels, ngroups=G), calls, warm=1)
    rec["rank_sums_after"] = event_ms(lambda: markers.rank_sums(csr, labels, ngroups=G), calls, warm=1)
    rec["groups"] = G
    print("%d x %d @ %d: residual_variance %s -> %s, rank_sums %s -> %s"
          % (N, J, draws, rec["residual_variance_before"], rec["residual_variance_after"], rec["rank_sums_before"],
             rec["rank_sums_after"]), file=sys.stderr, flush=True)
    return rec


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    shapes = [(s.split("@")[0].split("x"), s.split("@")[1]) for s in kv.get("shapes", "100000x20000@200,1000000x25000@200").split(",")]
    out = kv.get("out", os.path.join(ROOT, "profiles", "gene_major", "gene_major_time.json"))
    _lib.require_gpu()
    lib = _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "shapes": []}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for (N, J), draws in shapes:
        result["shapes"].append(one_shape(lib, int(N), int(J), int(draws), int(kv.get("calls", 10)), int(kv.get("G", 20)),
                                          kv.get("only", "")))
        print(json.dumps(result["shapes"][-1]), flush=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(result) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
