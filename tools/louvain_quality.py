#!/usr/bin/env python
"""Record the quality yardstick of the Louvain tests (CPU only): python tools/louvain_quality.py [out=tests/golden/louvain_quality.json]

On the two Jaccard 15-NN graphs of tests/test_louvain_host.py (2 000 Gamma-score rows; ten well-separated blobs) the
modularity of networkx's louvain_communities at seeds 0..2 -- the minimum is what the test asks the library to reach, less
a margin -- and beside it what the library's host restatement schpf_debug_louvain reaches, its shortfall, and the margin:
twice the worst shortfall, 5 % at the most.  The test reads the file and imports networkx nowhere."""
import json
import os
import sys

import networkx as nx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _knn_reference import gamma_scores  # noqa: E402
from _louvain_reference import as_csr, blob_scores, debug_louvain, knn_jaccard  # noqa: E402
from schpf_amd import modularity  # noqa: E402

SEEDS = [0, 1, 2]


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    out = kv.get("out", os.path.join(ROOT, "tests", "golden", "louvain_quality.json"))
    makers = {"gamma_scores": lambda: gamma_scores(2000, 20, np.float64, seed=0), "ten_blobs": lambda: blob_scores(2000, seed=0)}
    graphs = {}
    for name, make in sorted(makers.items()):
        graph = knn_jaccard(make(), 15)
        G = as_csr(graph)
        N = nx.from_scipy_sparse_array(G)
        theirs = []
        for seed in SEEDS:
            labels = np.empty(G.shape[0], np.int64)
            for c, members in enumerate(nx.community.louvain_communities(N, weight="weight", resolution=1.0, seed=seed)):
                labels[list(members)] = c
            theirs.append(modularity(G, labels))
        labels, stats = debug_louvain(graph)
        ours = modularity(G, labels)
        graphs[name] = {"networkx_modularity": [round(q, 6) for q in theirs], "networkx_modularity_min": round(min(theirs), 6),
                        "schpf_debug_louvain_modularity": round(ours, 6),
                        "measured_shortfall": round(max(0.0, 1 - ours / round(min(theirs), 6)), 6),
                        "communities": int(stats[0]), "levels": int(stats[1]), "rounds": int(stats[2])}
    worst = max(g["measured_shortfall"] for g in graphs.values())
    record = {"what": "modularity at resolution 1 on the Jaccard 15-NN graphs of 2000 rows (tests/test_louvain_host.py)",
              "networkx": nx.__version__, "seeds": SEEDS, "graphs": graphs,
              "margin": round(min(0.05, 2 * worst), 6), "margin_rule": "twice the worst measured shortfall, 0.05 at the most"}
    with open(out, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
