#!/usr/bin/env python
"""A/B of two library builds on the device entries of the stateless operators (GPU box):
    python tools/call_time.py [base=schpf_amd/libschpf_hip_base.so] [rounds=3] [calls=10] [n=100000] [K=20] [k=15]
                              [shape=100000x20000] [per_cell=200] [G=20] [out=profiles/refusals/call_time.json]

Keep the reference build as schpf_amd/libschpf_hip_base.so, build the variant as schpf_amd/libschpf_hip.so, run this.  The
two builds run in processes of their own ($SCHPF_LIB_PATH), in turn, `rounds` times each, on the same card: boxes differ by
more than the builds do, and so can two moments on one box.  Every process makes the inputs of tools/knn_time.py,
graph_time.py, louvain_time.py, components_time.py, geodesic_time.py (8 root sets), rank_sums_time.py and
pair_rank_sums_time.py (all pairs) at their smaller recorded shape and times each device entry on valid input with HIP
events around the whole call -- validation, the fetch of the refusal words and the call's device allocations included --
after 3 untimed calls: the median of `calls`.  Per entry the result holds the medians of every process, each build's fastest
single call, the spread of the reference build between its own repeats (largest - smallest median), and whether the
variant's mean median is within that spread of the reference's.  One JSON line, also written to `out`.  This process never
opens the GPU; it starts nothing more after a child that failed."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(kv):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from _knn_reference import gamma_scores
    from _pair_ranksum_reference import all_pairs
    from _ranksum_reference import random_labels, sparse_entries
    from knn_time import event_ms
    from schpf_amd import _lib
    from schpf_amd.device_input import gpu_csc

    n, K, k, calls = int(kv.get("n", 100000)), int(kv.get("K", 20)), int(kv.get("k", 15)), int(kv.get("calls", 10))
    N, J = (int(s) for s in kv.get("shape", "100000x20000").split("x"))
    per_cell, G = int(kv.get("per_cell", 200)), int(kv.get("G", 20))
    _lib.require_gpu()
    lib = _lib.load()
    I64P = ctypes.POINTER(ctypes.c_int64)
    stream = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream) or _lib.STREAM_DEFAULT)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dev = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda:0")  # noqa: E731
    rec = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SCHPF_LIB_PATH", "")}

    def timed(name, fn):
        rec[name] = event_ms(fn, calls)
        print(name, rec[name], file=sys.stderr, flush=True)

    scores = torch.tensor(gamma_scores(n, K, np.float64, seed=0), device="cuda:0")
    idx, d2 = dev((n, k), torch.int32), dev((n, k), torch.float64)
    timed("schpf_knn_device", lambda: _lib.check(lib.schpf_knn_device(
        0, stream, _lib.F64, n, n, K, p(scores), p(scores), k, ctypes.c_int64(0), p(idx), p(d2))))
    dist = torch.sqrt(d2)
    indptr, cols, data = dev(n + 1, torch.int64), dev(2 * n * k, torch.int32), dev(2 * n * k, torch.float64)
    for method, code in (("umap", _lib.GRAPH_UMAP), ("jaccard", _lib.GRAPH_JACCARD)):   # the Jaccard graph stays
        timed("schpf_knn_graph_device_" + method, lambda: _lib.check(lib.schpf_knn_graph_device(
            0, stream, code, n, k, p(idx), p(dist), p(indptr), p(cols), p(data), None, None)))
    labels, stats = dev(n, torch.int32), np.zeros(6, np.int64)
    timed("schpf_louvain_device", lambda: _lib.check(lib.schpf_louvain_device(
        0, stream, n, p(indptr), p(cols), p(data), 1.0, p(labels), stats.ctypes.data_as(I64P))))
    groups = int(labels.max()) + 1
    comp = dev(n, torch.int32)
    for name, within in (("schpf_components_device", None), ("schpf_components_device_within", p(labels))):
        timed(name, lambda: _lib.check(lib.schpf_components_device(
            0, stream, n, p(indptr), p(cols), within, p(comp), stats.ctypes.data_as(I64P))))
    cells, count, weight, wmax = dev(groups, torch.int64), dev((groups, groups), torch.int64), dev((groups, groups), torch.int64), ctypes.c_double(0.0)
    timed("schpf_cluster_graph_device", lambda: _lib.check(lib.schpf_cluster_graph_device(
        0, stream, n, p(indptr), p(cols), p(data), p(labels), groups, p(cells), p(count), p(weight), ctypes.byref(wmax))))
    # the geodesics walk the directed k-NN lists with their distances, as tools/geodesic_time.py does
    g_indptr = (torch.arange(n + 1, dtype=torch.int64, device="cuda:0") * k).contiguous()
    g_cols, g_data = idx.reshape(-1).contiguous(), dist.reshape(-1).contiguous()
    nsets = 8
    roots = torch.tensor(np.random.RandomState(1).choice(n, 64, replace=False).astype(np.int32)[:nsets], device="cuda:0")
    set_ptr, out = torch.arange(nsets + 1, dtype=torch.int64, device="cuda:0"), dev((nsets, n), torch.float64)
    timed("schpf_geodesic_device_roots_8", lambda: _lib.check(lib.schpf_geodesic_device(
        0, stream, n, p(g_indptr), p(g_cols), p(g_data), 0, nsets, p(set_ptr), p(roots), p(out), stats.ctypes.data_as(I64P))))
    del scores, idx, d2, dist, indptr, cols, data, g_indptr, g_cols, g_data, out

    h_cells, h_genes, h_values = sparse_entries(N, J, per_cell, seed=0)
    X = torch.sparse_coo_tensor(torch.stack([torch.tensor(h_cells, device="cuda:0").long(), torch.tensor(h_genes, device="cuda:0").long()]),
                                torch.tensor(h_values, device="cuda:0"), size=(N, J))
    m_indptr, cell_ids, values = gpu_csc(X)
    del X
    m_labels = torch.tensor(random_labels(N, G, seed=1), device="cuda:0")
    outs = [torch.zeros(s, dtype=torch.int64, device="cuda:0") for s in ((G,), (J,), (J,), (G, J), (G, J))]
    timed("schpf_rank_sums_device", lambda: _lib.check(lib.schpf_rank_sums_device(
        0, stream, N, J, p(m_indptr), p(cell_ids), p(values), p(m_labels), G, *[p(t) for t in outs])))
    pairs = torch.tensor(np.ascontiguousarray(all_pairs(G), np.int32), device="cuda:0")
    P = int(pairs.shape[0])
    outs = [torch.zeros(s, dtype=torch.int64, device="cuda:0") for s in ((G,), (G, J), (P, J), (P, J))]
    timed("schpf_pair_rank_sums_device_all_pairs", lambda: _lib.check(lib.schpf_pair_rank_sums_device(
        0, stream, N, J, p(m_indptr), p(cell_ids), p(values), p(m_labels), G, p(pairs), P, *[p(t) for t in outs])))
    rec["shapes"] = {"n": n, "K": K, "k": k, "louvain_communities": groups, "ncells": N, "ngenes": J, "per_cell": per_cell,
                     "nnz": int(values.numel()), "ngroups": G, "npairs": P, "calls": calls}
    print(json.dumps(rec), flush=True)


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    if kv.get("child") == "1":
        return child(kv)
    base = os.path.abspath(kv.get("base", os.path.join(ROOT, "schpf_amd", "libschpf_hip_base.so")))
    new = os.path.join(ROOT, "schpf_amd", "libschpf_hip.so")
    runs = {"base": [], "new": []}
    for _ in range(int(kv.get("rounds", 3))):
        for which, path in (("base", base), ("new", new)):
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "child=1"] + sys.argv[1:], env=dict(os.environ, SCHPF_LIB_PATH=path),
                                  stdout=subprocess.PIPE, timeout=float(kv.get("timeout", 420)))
            if done.returncode != 0:
                sys.exit("the %s build ended with status %d: nothing more is started" % (which, done.returncode))
            runs[which].append(json.loads(done.stdout.decode().strip().splitlines()[-1]))
    result = {"device": runs["new"][0]["device"], "shapes": runs["new"][0]["shapes"], "entries": {}}
    for name in [key for key in runs["new"][0] if key.startswith("schpf_")]:
        medians = {which: [r[name]["median_ms"] for r in runs[which]] for which in runs}
        mean = {which: sum(v) / len(v) for which, v in medians.items()}
        spread = max(medians["base"]) - min(medians["base"])
        result["entries"][name] = {"base_median_ms": medians["base"], "new_median_ms": medians["new"],
                                   "base_fastest_call_ms": min(r[name]["min_ms"] for r in runs["base"]),
                                   "new_fastest_call_ms": min(r[name]["min_ms"] for r in runs["new"]), "base_spread_ms": round(spread, 3),
                                   "new_minus_base_ms": round(mean["new"] - mean["base"], 3),
                                   "within_base_spread": bool(mean["new"] - mean["base"] <= spread)}
    line = json.dumps(result)
    print(line, flush=True)
    out = kv.get("out", os.path.join(ROOT, "profiles", "refusals", "call_time.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
