#!/usr/bin/env python
"""Time the rank sums between pairs of groups (GPU box):
    python tools/pair_rank_sums_time.py [shapes=100000x20000,1000000x25000] [per_cell=200] [G=20] [calls=10] [loop_calls=3]
                                        [few=40] [scaled=100000x20000] [slice=200] [slice_pairs=10] [host=1]
                                        [out=profiles/markers/pair_rank_sums_time.json]

For every shape N x J: the synthetic counts of tools/rank_sums_time.py (tests/_ranksum_reference.py sparse_entries), made
gene-major once on the GPU (not timed), and G labels from a fixed seed.  Timed with HIP events around the whole call on
torch's current stream, after 3 untimed calls, the median of `calls`:
    schpf_pair_rank_sums_device with all G (G - 1) / 2 pairs, and with a "neighbors"-sized list of `few` pairs
    schpf_rank_sums_device on the same matrix, for scale
and, the median of `loop_calls` after one untimed pass, the loop a user can write without the new entry point: for each of
the pairs, `submatrix` of the pair's cells -- of the gene-major matrix, so that nothing has to be transposed -- and
schpf_rank_sums_device with two groups; its u2 = rank2[0] - n_0 (n_0 + 1) must equal the new call's.  A shape listed in
`scaled` is timed again with every cell scaled to the median depth in float32: nearly every entry is then its own value,
the worst case.  host=1: by the wall clock and once, on `slice` genes and `slice_pairs` pairs, the library's serial
restatement -- whose integers must be the GPU's -- and scipy.stats.mannwhitneyu per gene and pair.  One JSON line with a
record per shape, also written to `out`."""
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
from _pair_ranksum_reference import all_pairs, debug_pair_rank_sums  # noqa: E402
from _ranksum_reference import random_labels, sparse_entries  # noqa: E402
from knn_time import event_ms  # noqa: E402
from schpf_amd import _lib  # noqa: E402
from schpf_amd.device_input import gpu_csc  # noqa: E402
from schpf_amd.qc import submatrix  # noqa: E402

p = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731


def few_pairs(G, count):
    """`count` pairs (g, g + d mod G), d = 1, 2, ...: every group with a few neighbours, as a cluster graph gives them."""
    rows = [(g, (g + d) % G) for d in range(1, G) for g in range(G)]
    return np.ascontiguousarray(np.array(rows[:count], np.int32).reshape(-1, 2))


def timings(lib, N, J, G, indptr, cell_ids, data, h_labels, calls, loop_calls, few):
    stream = int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT
    labels = torch.tensor(h_labels, device="cuda:0")
    nnz = int(data.numel())
    rec = {"nnz": nnz, "longest_gene": int((indptr[1:] - indptr[:-1]).max()), "distinct_values": int(torch.unique(data).numel())}
    results = {}
    for name, pairs in (("all_pairs", all_pairs(G)), ("few_pairs", few_pairs(G, few))):
        P = len(pairs)
        d_pairs = torch.tensor(pairs, device="cuda:0")
        out = [torch.zeros(s, dtype=torch.int64, device="cuda:0") for s in ((G,), (G, J), (P, J), (P, J))]

        def hip():
            _lib.check(lib.schpf_pair_rank_sums_device(0, ctypes.c_void_p(stream), N, J, p(indptr), p(cell_ids), p(data), p(labels),
                                                       G, p(d_pairs), P, *[p(t) for t in out]))

        rec[name] = dict(event_ms(hip, calls), npairs=P)
        results[name] = (pairs, out)
    one = [torch.zeros(s, dtype=torch.int64, device="cuda:0") for s in ((G,), (J,), (J,), (G, J), (G, J))]
    rec["schpf_rank_sums_device"] = event_ms(lambda: _lib.check(lib.schpf_rank_sums_device(
        0, ctypes.c_void_p(stream), N, J, p(indptr), p(cell_ids), p(data), p(labels), G, *[p(t) for t in one])), calls)
    del one

    # the loop over the pairs with what the library had before: the gene-major matrix is a CSR matrix of genes x cells
    genes_by_cells = torch.sparse_csr_tensor(indptr, cell_ids.to(torch.int64), data, size=(J, N))
    pairs, out = results["all_pairs"]
    masks = [(h_labels == a) | (h_labels == b) for a, b in pairs]
    loop_u2 = torch.zeros((len(pairs), J), dtype=torch.int64, device="cuda:0")
    two = [torch.zeros(s, dtype=torch.int64, device="cuda:0") for s in ((2,), (J,), (J,), (2, J), (2, J))]

    def loop():
        for row, ((a, b), mask) in enumerate(zip(pairs, masks)):
            sub = submatrix(genes_by_cells, genes=mask)
            n_sub = int(sub.shape[1])
            sub_labels = (labels[torch.from_numpy(mask).to("cuda:0")] == int(b)).to(torch.int32)
            cols = sub.col_indices().to(torch.int32)
            _lib.check(lib.schpf_rank_sums_device(0, ctypes.c_void_p(stream), n_sub, J, p(sub.crow_indices()), p(cols), p(sub.values()),
                                                  p(sub_labels), 2, *[p(t) for t in two]))
            loop_u2[row] = two[4][0] - two[0][0] * (two[0][0] + 1)

    try:
        rec["loop_of_submatrix_and_rank_sums"] = dict(event_ms(loop, loop_calls, warm=1), npairs=len(pairs))
        rec["loop_u2_equal"] = bool(torch.equal(loop_u2, out[2]))
        rec["speedup_over_loop"] = round(rec["loop_of_submatrix_and_rank_sums"]["median_ms"] / rec["all_pairs"]["median_ms"], 2)
    except ValueError as err:                 # the loop's building blocks refuse the matrix
        rec["loop_of_submatrix_and_rank_sums"] = {"refused": str(err)}
    # 16 nnz of keys, 8 nnz of counts and starts, 4 G J of list starts, 16 P of sides; rocPRIM's own comes on top
    rec["scratch_bytes_without_rocprim"] = 24 * nnz + 8 + 4 * (G * J + 1) + 16 * len(pairs) + 8 * (G + 1)
    return rec, results


def one_shape(lib, N, J, per_cell, G, calls, loop_calls, few, scaled, n_slice, slice_pairs, host):
    cells, genes, values = sparse_entries(N, J, per_cell, seed=0)
    X = torch.sparse_coo_tensor(torch.stack([torch.tensor(cells, device="cuda:0").long(), torch.tensor(genes, device="cuda:0").long()]),
                                torch.tensor(values, device="cuda:0"), size=(N, J))
    del cells, genes, values
    indptr, cell_ids, data = gpu_csc(X)
    del X
    h_labels = random_labels(N, G, seed=1)
    rec = {"ncells": N, "ngenes": J, "per_cell": per_cell, "ngroups": G, "calls": calls, "loop_calls": loop_calls}
    counts, results = timings(lib, N, J, G, indptr, cell_ids, data, h_labels, calls, loop_calls, few)
    rec.update(counts)
    print("%d x %d: %s" % (N, J, json.dumps(rec)), file=sys.stderr, flush=True)
    if host:
        from scipy.stats import mannwhitneyu
        pairs, out = results["all_pairs"]
        picked = np.linspace(0, J - 1, min(n_slice, J)).astype(np.int64)
        rows = np.linspace(0, len(pairs) - 1, min(slice_pairs, len(pairs))).astype(np.int64)
        h_indptr = indptr.cpu().numpy()
        parts = [(cell_ids[h_indptr[j]:h_indptr[j + 1]].cpu().numpy(), data[h_indptr[j]:h_indptr[j + 1]].cpu().numpy()) for j in picked]
        s_indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in parts])]).astype(np.int64)
        matrix = (N, len(picked), s_indptr, np.concatenate([c for c, _ in parts]), np.concatenate([v for _, v in parts]))
        t0 = time.perf_counter()
        want = debug_pair_rank_sums(matrix, h_labels, G, pairs[rows])
        rec["slice_genes"], rec["slice_pairs"], rec["slice_nnz"] = len(picked), len(rows), int(s_indptr[-1])
        rec["schpf_debug_pair_rank_sums_slice_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        mine = [t.cpu().numpy() for t in out]
        rec["slice_equal_host"] = bool(np.array_equal(want[0], mine[0]) and np.array_equal(want[1], mine[1][:, picked])
                                       and all(np.array_equal(w, m[rows][:, picked]) for w, m in zip(want[2:], mine[2:])))
        t0 = time.perf_counter()
        twice_u = np.empty((len(rows), len(picked)))
        for x, (c, v) in enumerate(parts):
            column = np.zeros(N, np.float32)
            column[c] = v
            for y, (a, b) in enumerate(pairs[rows]):
                twice_u[y, x] = 2 * mannwhitneyu(column[h_labels == a], column[h_labels == b], method="asymptotic",
                                                 use_continuity=False).statistic
        rec["scipy_mannwhitneyu_slice_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["slice_equal_scipy_u"] = bool(np.array_equal(twice_u, mine[2][rows][:, picked]))
    if scaled:
        depth = torch.zeros(N, dtype=torch.float32, device="cuda:0").index_add_(0, cell_ids.long(), data)
        factor = torch.where(depth > 0, torch.median(depth) / depth, torch.zeros_like(depth))
        rec["scaled_to_median_depth"] = timings(lib, N, J, G, indptr, cell_ids, data * factor[cell_ids.long()], h_labels, calls,
                                                loop_calls, few)[0]
    return rec


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    per_cell, G, calls = int(kv.get("per_cell", 200)), int(kv.get("G", 20)), int(kv.get("calls", 10))
    shapes = [(s.split("@")[0].split("x"), s.split("@")[1] if "@" in s else per_cell)
              for s in kv.get("shapes", "100000x20000,1000000x25000").split(",")]
    scaled = kv.get("scaled", "100000x20000").split(",")
    _lib.require_gpu()
    lib = _lib.load()
    result = {"device": torch.cuda.get_device_name(0), "host_threads": len(os.sched_getaffinity(0)), "shapes": []}
    for (N, J), draws in shapes:
        result["shapes"].append(one_shape(lib, int(N), int(J), int(draws), G, calls, int(kv.get("loop_calls", 3)), int(kv.get("few", 40)),
                                          "%sx%s" % (N, J) in scaled, int(kv.get("slice", 200)), int(kv.get("slice_pairs", 10)),
                                          kv.get("host", "1") == "1"))
        print(json.dumps(result["shapes"][-1]), flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    out = kv.get("out", os.path.join(ROOT, "profiles", "markers", "pair_rank_sums_time.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
