#!/usr/bin/env python
"""A/B of two trees of the Python operators, each timed through its public entry (GPU box):
    python tools/wrapper_time.py base=DIR [rounds=3] [calls=10] [host_calls=3] [n=100000] [K=20] [k=15]
                                 [shape=100000x20000] [per_cell=200] [G=20] [out=profiles/call_layer/wrapper_time.json]

`base` is a directory that holds the reference `schpf_amd/` package (say, `git archive` of the parent commit's
schpf_amd/*.py); the variant is this tree's.  Both use this tree's built library ($SCHPF_LIB_PATH), so the Python layer is
the only thing that differs.  The two trees run in processes of their own, in turn, `rounds` times each, on the same card,
as tools/call_time.py runs two library builds.  Every process makes the inputs of the operators' own tools at their smaller
recorded shape (knn_time.py .. geodesic_time.py: n rows, K factors, k neighbours; rank_sums_time.py .. residual_var_time.py:
N x J counts with per_cell draws a cell, G groups) and times every public operator on tensors in GPU memory by the wall
clock, the device idle before the call and after it -- conversions, validation, allocations, the library call and whatever
the wrapper fetches included -- after 3 untimed calls: the median of `calls`.  The entries that take a SciPy matrix through
the host conversions are timed the same way over `host_calls` calls after one.  Per operator the result holds the medians of
every process, the spread of the reference tree between its own repeats (largest - smallest median) and whether the
variant's mean median is within that spread of the reference's.  One JSON line, also written to `out`.  This process never
opens the GPU; it starts nothing more after a child that failed."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(kv):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)                      # the `schpf` package the operators' package imports
    sys.path.insert(0, os.path.abspath(kv["tree"]))
    from _knn_reference import gamma_scores
    from _ranksum_reference import random_labels, sparse_entries
    import schpf_amd
    from scipy.sparse import csr_matrix

    assert os.path.dirname(os.path.dirname(os.path.abspath(schpf_amd.__file__))) == os.path.abspath(kv["tree"])
    n, K, k = int(kv.get("n", 100000)), int(kv.get("K", 20)), int(kv.get("k", 15))
    calls, host_calls = int(kv.get("calls", 10)), int(kv.get("host_calls", 3))
    N, J = (int(s) for s in kv.get("shape", "100000x20000").split("x"))
    per_cell, G = int(kv.get("per_cell", 200)), int(kv.get("G", 20))
    dev = "cuda:0"
    rec = {"device": torch.cuda.get_device_name(0), "tree": os.path.abspath(kv["tree"])}

    def timed(name, fn, count=calls, warm=3):
        for _ in range(warm):
            fn()
        ms = []
        for _ in range(count):
            torch.cuda.synchronize()
            start = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - start) * 1e3)
        rec[name] = {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}
        print(name, rec[name], file=sys.stderr, flush=True)

    scores = torch.tensor(gamma_scores(n, K, np.float64, seed=0), device=dev)
    timed("knn", lambda: schpf_amd.knn(scores, k=k))
    idx, dist = schpf_amd.knn(scores, k=k)
    timed("knn_connectivities_umap", lambda: schpf_amd.knn_connectivities(idx, dist, method="umap"))
    timed("knn_connectivities_jaccard", lambda: schpf_amd.knn_connectivities(idx, method="jaccard"))
    graph = schpf_amd.knn_connectivities(idx, method="jaccard")
    timed("louvain", lambda: schpf_amd.louvain(graph))
    labels = schpf_amd.louvain(graph)
    timed("connected_components", lambda: schpf_amd.connected_components(graph))
    timed("connected_components_within", lambda: schpf_amd.connected_components(graph, within=labels))
    timed("cluster_graph", lambda: schpf_amd.cluster_graph(graph, labels))
    # the geodesics walk the directed k-NN lists with their distances, as tools/geodesic_time.py does
    lists = torch.sparse_csr_tensor(torch.arange(n + 1, dtype=torch.int64, device=dev) * k, idx.reshape(-1).to(torch.int64),
                                    dist.reshape(-1), size=(n, n))
    roots = np.random.RandomState(1).choice(n, 64, replace=False).astype(np.int32)[:8]
    timed("geodesic_distances_roots_8", lambda: schpf_amd.geodesic_distances(lists, roots))
    del scores, idx, dist, graph, labels, lists

    h_cells, h_genes, h_values = sparse_entries(N, J, per_cell, seed=0)
    coo = torch.sparse_coo_tensor(torch.stack([torch.tensor(h_cells, device=dev).long(), torch.tensor(h_genes, device=dev).long()]),
                                  torch.tensor(h_values, device=dev).to(torch.int32), size=(N, J)).coalesce()
    crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(torch.bincount(coo.indices()[0], minlength=N), 0)
    X = torch.sparse_csr_tensor(crow, coo.indices()[1].contiguous(), coo.values().contiguous(), size=(N, J))
    groups = torch.tensor(random_labels(N, G, seed=1), device=dev)
    rng = np.random.RandomState(2)
    keep_cells, keep_genes = torch.tensor(rng.rand(N) >= 0.06, device=dev), rng.rand(J) >= 0.5
    timed("rank_sums", lambda: schpf_amd.rank_sums(X, groups, ngroups=G))
    timed("pair_rank_sums_all_pairs", lambda: schpf_amd.pair_rank_sums(X, groups, ngroups=G))
    timed("residual_variance", lambda: schpf_amd.residual_variance(X))
    timed("qc_metrics", lambda: schpf_amd.qc_metrics(X, gene_sets={"first": np.arange(13), "every_200th": np.arange(0, J, 200)}))
    timed("qc_metrics_coo", lambda: schpf_amd.qc_metrics(coo))
    timed("submatrix", lambda: schpf_amd.submatrix(X, cells=keep_cells, genes=keep_genes))
    timed("group_stats", lambda: schpf_amd.group_stats(X, groups, ngroups=G))
    timed("simulate_doublets", lambda: schpf_amd.simulate_doublets(X, seed=3))
    timed("thin_counts", lambda: schpf_amd.thin_counts(X, 0.2, seed=4))

    # the same matrix in host memory: SciPy's conversions and the copies to the GPU are most of these
    H = csr_matrix((coo.values().cpu().numpy(), (coo.indices()[0].cpu().numpy(), coo.indices()[1].cpu().numpy())), shape=(N, J))
    h_groups = groups.cpu().numpy()
    del coo, X
    for name, fn in (("host_rank_sums", lambda: schpf_amd.rank_sums(H, h_groups, ngroups=G)),
                     ("host_residual_variance", lambda: schpf_amd.residual_variance(H)),
                     ("host_qc_metrics", lambda: schpf_amd.qc_metrics(H)),
                     ("host_group_stats", lambda: schpf_amd.group_stats(H, h_groups, ngroups=G)),
                     ("host_simulate_doublets", lambda: schpf_amd.simulate_doublets(H, seed=3)),
                     ("host_thin_counts", lambda: schpf_amd.thin_counts(H, 0.2, seed=4))):
        timed(name, fn, host_calls, warm=1)
    g_small = schpf_amd.knn_connectivities(*schpf_amd.knn(gamma_scores(n // 10, K, np.float64, seed=0), k=k), method="umap")
    timed("host_louvain_%d" % (n // 10), lambda: schpf_amd.louvain(g_small), host_calls, warm=1)
    timed("host_connected_components_%d" % (n // 10), lambda: schpf_amd.connected_components(g_small), host_calls, warm=1)
    rec["shapes"] = {"n": n, "K": K, "k": k, "ncells": N, "ngenes": J, "per_cell": per_cell, "nnz": int(H.nnz), "ngroups": G,
                     "calls": calls, "host_calls": host_calls}
    print(json.dumps(rec), flush=True)


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    if kv.get("child") == "1":
        return child(kv)
    trees = {"base": os.path.abspath(kv["base"]), "new": ROOT}
    env = dict(os.environ, SCHPF_LIB_PATH=os.path.join(ROOT, "schpf_amd", "libschpf_hip.so"))
    runs = {"base": [], "new": []}
    for _ in range(int(kv.get("rounds", 3))):
        for which in ("base", "new"):
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "child=1", "tree=" + trees[which]] + sys.argv[1:],
                                  env=env, stdout=subprocess.PIPE, timeout=float(kv.get("timeout", 420)))
            if done.returncode != 0:
                sys.exit("the %s tree ended with status %d: nothing more is started" % (which, done.returncode))
            runs[which].append(json.loads(done.stdout.decode().strip().splitlines()[-1]))
    result = {"device": runs["new"][0]["device"], "shapes": runs["new"][0]["shapes"], "operators": {}}
    for name in [key for key in runs["new"][0] if isinstance(runs["new"][0][key], dict) and "median_ms" in runs["new"][0][key]]:
        medians = {which: [r[name]["median_ms"] for r in runs[which]] for which in runs}
        mean = {which: sum(v) / len(v) for which, v in medians.items()}
        spread = max(medians["base"]) - min(medians["base"])
        result["operators"][name] = {"base_median_ms": medians["base"], "new_median_ms": medians["new"],
                                     "base_spread_ms": round(spread, 3), "new_minus_base_ms": round(mean["new"] - mean["base"], 3),
                                     "within_base_spread": bool(mean["new"] - mean["base"] <= spread)}
    line = json.dumps(result)
    print(line, flush=True)
    out = kv.get("out", os.path.join(ROOT, "profiles", "call_layer", "wrapper_time.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
