#!/usr/bin/env python
"""Time the Pearson residual sums per gene (GPU box):
    python tools/residual_var_time.py [shapes=1000000x25000@200] [calls=10] [torch=1] [torch_calls=3] [chunk=2048]
                                      [theta=100] [out=profiles/hvg/residual_var_time.json]
A shape N x J @ draws: synthetic counts from the marker tests' maker (tests/_ranksum_reference.py sparse_entries: N * draws
draws, skewed gene popularity), as a coalesced COO tensor and a CSR tensor on the GPU.

Timed with HIP events on torch's current stream, the median of `calls` after one untimed call:
  * schpf_residual_var_device, the whole call -- checks, totals, the sort of the cell totals, both passes, the call's own
    allocations -- on the gene-major arrays, with the default clip sqrt(N);
  * device_input.gpu_csc, the sort to gene-major in torch that residual_variance runs first on a CSR tensor, and
    residual_variance end to end on that tensor.
Recorded beside them: U, the number of distinct cell totals the dense pass walks, and the 12 nnz bytes the sparse pass reads
with their time at the HBM peak of 8 TB/s.
  * torch=1: a torch formulation with equal results on the same GPU, timed the same way over torch_calls calls: the cells in
    chunks of `chunk` rows, a dense float64 chunk, mu, the residuals, the clip, and the two column sums accumulated in
    float64.  Its sums are compared with the call's under the bound of tests/_residual_var_reference.py.
One JSON line with a record per shape, also written to `out`."""
import ctypes
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _ranksum_reference import sparse_entries  # noqa: E402
from _residual_var_reference import tolerance  # noqa: E402
from knn_time import event_ms  # noqa: E402
from schpf_amd import _lib, variable_genes  # noqa: E402
from schpf_amd.device_input import gpu_csc  # noqa: E402

HBM_PEAK = 8.0e12      # bytes per second, MI355X


def one_shape(lib, N, J, draws, calls, with_torch, torch_calls, chunk, theta):
    dev = "cuda:0"
    cells, genes, values = sparse_entries(N, J, draws, seed=0)
    X = torch.sparse_coo_tensor(torch.stack([torch.tensor(cells, device=dev).long(), torch.tensor(genes, device=dev).long()]),
                                torch.tensor(values, device=dev), size=(N, J)).coalesce()      # float32: exact counts
    del cells, genes, values
    rows, cols, vals = X.indices()[0], X.indices()[1], X.values()
    crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    csr = torch.sparse_csr_tensor(crow, cols, vals, size=(N, J))
    indptr, cell_ids, data = gpu_csc(X)
    nnz = int(data.numel())
    inv_theta, clip = (0.0 if math.isinf(theta) else 1.0 / theta), math.sqrt(N)
    stream = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s1, s2 = torch.zeros(J, dtype=torch.float64, device=dev), torch.zeros(J, dtype=torch.float64, device=dev)
    cell_total, gene_total = torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(J, dtype=torch.int64, device=dev)

    def call():
        _lib.check(lib.schpf_residual_var_device(0, stream, N, J, nnz, p(indptr), p(cell_ids), p(data), inv_theta, clip, p(s1), p(s2),
                                                 p(cell_total), p(gene_total)))

    rec = {"ncells": N, "ngenes": J, "draws_per_cell": draws, "nnz": nnz, "theta": theta, "clip": clip, "calls": calls,
           "longest_gene": int((indptr[1:] - indptr[:-1]).max()), "hbm_peak_bytes_per_second": HBM_PEAK,
           "residual_var_device": event_ms(call, calls, warm=1)}
    rec["n_distinct_totals"] = int(torch.unique(cell_total).numel())
    rec["sparse_pass_bytes"] = 12 * nnz
    rec["sparse_pass_ms_at_hbm_peak"] = round(12 * nnz / HBM_PEAK * 1e3, 3)
    rec["entries_per_second"] = round(nnz / (rec["residual_var_device"]["median_ms"] * 1e-3))
    print("%d x %d @ %d: the call %s, U = %d" % (N, J, draws, rec["residual_var_device"], rec["n_distinct_totals"]),
          file=sys.stderr, flush=True)
    rec["gpu_csc_of_a_csr_tensor"] = event_ms(lambda: gpu_csc(csr), 3, warm=1)
    rec["residual_variance_on_a_csr_tensor"] = event_ms(lambda: variable_genes.residual_variance(csr, theta=theta), 3, warm=1)
    print("%d x %d @ %d: to gene-major %s, end to end %s" % (N, J, draws, rec["gpu_csc_of_a_csr_tensor"],
                                                            rec["residual_variance_on_a_csr_tensor"]), file=sys.stderr, flush=True)
    if with_torch:
        kept, bounds = {}, crow.cpu().tolist()      # the chunks' entries, known before the clock starts

        def formulation():
            n = torch.zeros(N, dtype=torch.float64, device=dev).index_add_(0, rows, vals.double())
            s = torch.zeros(J, dtype=torch.float64, device=dev).index_add_(0, cols, vals.double())
            q = s / s.sum()
            t1, t2 = torch.zeros(J, dtype=torch.float64, device=dev), torch.zeros(J, dtype=torch.float64, device=dev)
            for a in range(0, N, chunk):
                b = min(a + chunk, N)
                lo, hi = bounds[a], bounds[b]
                D = torch.zeros((b - a, J), dtype=torch.float64, device=dev)
                D[rows[lo:hi] - a, cols[lo:hi]] = vals[lo:hi].double()
                mu = n[a:b, None] * q[None, :]
                r = (D - mu) / torch.sqrt(mu * (1.0 + mu * inv_theta))
                r = torch.where(mu > 0, r, torch.zeros_like(r)).clamp_(-clip, clip)
                t1 += r.sum(dim=0)
                t2 += (r * r).sum(dim=0)
            kept["sums"] = (t1, t2)

        try:
            rec["torch_dense_chunks"] = dict(event_ms(formulation, torch_calls, warm=1), chunk=chunk)
            rec["torch_over_residual_var_device"] = round(rec["torch_dense_chunks"]["median_ms"] / rec["residual_var_device"]["median_ms"], 2)
            t1, t2 = kept["sums"]
            # the scale of S1's bound is sum |r| <= sqrt(N S2)
            e1 = float(((t1 - s1).abs() / torch.sqrt(N * s2).clamp_min(1e-300)).max())
            e2 = float(((t2 - s2).abs() / s2.clamp_min(1e-300)).max())
            rec.update({"torch_sum_error_over_sqrt_N_sumsq": e1, "torch_sumsq_relative_error": e2, "bound": tolerance(N),
                        "torch_results_equal_within_bound": bool(e1 <= tolerance(N) and e2 <= tolerance(N))})
        except RuntimeError as e:       # out of memory
            rec["torch_dense_chunks"] = "failed: " + str(e).splitlines()[0][:200]
        kept.clear()
    return rec


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    shapes = [(s.split("@")[0].split("x"), s.split("@")[1]) for s in kv.get("shapes", "1000000x25000@200").split(",")]
    out = kv.get("out", os.path.join(ROOT, "profiles", "hvg", "residual_var_time.json"))
    _lib.require_gpu()
    lib = _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "shapes": []}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for (N, J), draws in shapes:
        result["shapes"].append(one_shape(lib, int(N), int(J), int(draws), int(kv.get("calls", 10)), kv.get("torch", "1") == "1",
                                          int(kv.get("torch_calls", 3)), int(kv.get("chunk", 2048)), float(kv.get("theta", 100))))
        print(json.dumps(result["shapes"][-1]), flush=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(result) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
