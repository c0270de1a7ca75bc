"""Louvain clustering, without a GPU: the library's serial restatement schpf_debug_louvain -- which the
kernels are then held to bit for bit (tests/test_louvain_gpu.py) -- is pinned to the definition written out in NumPy / SciPy
(tests/_louvain_reference.py), and the Python layer and the command line are checked with the restatement in the kernels'
place.

Bounds.  Everything is exact: labels and stats are integers, every sum of the definition is an integer sum, and the one
floating-point expression is the same multiply, division and fused multiply-add on both sides (the yardstick's module says
how it gets the fused operation).  The quality test alone has a margin; tests/golden/louvain_quality.json says where it is
from."""
import json
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from _graph_reference import JACCARD, UMAP
from _louvain_reference import (_p, as_csr, blob_scores, clique_ring, debug_louvain, hub, knn_jaccard, numpy_louvain,
                                ring_lattice, score_graph, two_components, with_diagonal, with_empty_rows, with_tiny_weights,
                                with_zero_rows)

GAMMAS = [0.5, 1.0, 2.0]
ONE = (np.array([0, 0], np.int64), np.zeros(0, np.int32), np.zeros(0))
PAIR = (np.array([0, 1, 2], np.int64), np.array([1, 0], np.int32), np.array([0.25, 0.25]))

CASES = {
    "one_vertex": lambda: ONE,
    "pair": lambda: PAIR,
    "scores_65_3_umap": lambda: score_graph(65, 3, UMAP, 1),
    "scores_65_3_jaccard": lambda: score_graph(65, 3, JACCARD, 1),
    "scores_130_15_umap": lambda: score_graph(130, 15, UMAP, 2),
    "scores_130_15_jaccard": lambda: score_graph(130, 15, JACCARD, 2),
    "scores_300_128_jaccard": lambda: score_graph(300, 128, JACCARD, 3),
    "clique_ring": clique_ring,
    "ring_lattice": ring_lattice,
    "hub_400": lambda: hub(400),
    "two_components": two_components,
    "empty_rows": lambda: with_empty_rows(score_graph(130, 15, JACCARD, 2), [0, 7, 64, 129]),
    "zero_rows": lambda: with_zero_rows(score_graph(130, 15, JACCARD, 2), [0, 7, 64, 129]),
    "tiny_weights": lambda: with_tiny_weights(score_graph(130, 15, UMAP, 2)),
    "diagonal": lambda: with_diagonal(score_graph(130, 15, UMAP, 2)),
}


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_equals_the_definition(case, gamma):
    graph = CASES[case]()
    labels, stats = debug_louvain(graph, gamma)
    want_labels, want_stats = numpy_louvain(*graph, gamma=gamma)
    assert_array_equal(stats, want_stats)
    assert_array_equal(labels, want_labels)
    n = len(graph[0]) - 1
    assert labels.dtype == np.int32 and sorted(set(labels.tolist())) == list(range(int(stats[0])))     # contiguous
    assert 0 <= stats[1] <= 32 and stats[1] <= stats[2] <= 32 * 32
    if case in ("one_vertex",):
        assert stats.tolist() == [1, 0, 0, 0]
    if case == "pair":
        assert stats[3] == 2 << 30
    if case == "tiny_weights":
        data = graph[2]
        assert (np.rint(np.ldexp(data / data.max(), 30)) == 0).sum() > 20 and (data > 0).all()
    if n > 60 and case != "ring_lattice":
        assert stats[1] >= 1 and stats[0] < n


def test_a_resolution_that_is_no_power_of_two():
    """The product -gamma * t is rounded away inside the fused operation: the yardstick takes the exact rational."""
    graph = score_graph(65, 3, JACCARD, 1)
    for gamma in (0.7, 1.3):
        labels, stats = debug_louvain(graph, gamma)
        want_labels, want_stats = numpy_louvain(*graph, gamma=gamma)
        assert_array_equal(stats, want_stats)
        assert_array_equal(labels, want_labels)


def test_cliques_in_a_ring_come_back_as_the_cliques():
    graph = clique_ring(cliques=12, size=8, bridge=1e-3)
    labels, stats = debug_louvain(graph)
    assert stats[0] == 12
    assert_array_equal(labels, np.repeat(np.arange(12), 8))     # ascending ids: clique b is community b


def test_components_and_isolated_vertices():
    graph = two_components(60)
    labels, _ = debug_louvain(graph)
    assert not set(labels[:30].tolist()) & set(labels[30:].tolist())
    cut = [0, 7, 64, 129]
    labels, stats = debug_louvain(with_empty_rows(score_graph(130, 15, JACCARD, 2), cut))
    for v in cut:
        assert (labels == labels[v]).sum() == 1
    labels, stats = debug_louvain(with_zero_rows(score_graph(130, 15, JACCARD, 2), cut))
    for v in cut:                                                # entries of no weight: k_i = 0, never eligible, never chosen
        assert (labels == labels[v]).sum() == 1


def test_no_weight_at_all_and_scaling():
    indptr, indices, data = score_graph(65, 3, UMAP, 1)
    labels, stats = debug_louvain((indptr, indices, np.zeros_like(data)))
    assert_array_equal(labels, np.arange(65))
    assert stats.tolist() == [65, 0, 0, 0]
    labels, stats = debug_louvain((np.zeros(66, np.int64), np.zeros(0, np.int32), np.zeros(0)))
    assert_array_equal(labels, np.arange(65))
    assert stats.tolist() == [65, 0, 0, 0]
    want = debug_louvain((indptr, indices, data))
    got = debug_louvain((indptr, indices, data * 3.0))           # data / wmax: the same quotients, or within the rounding
    assert_array_equal(got[0], want[0])                          # of the division -- the same q here
    assert_array_equal(got[1], want[1])
    got = debug_louvain((indptr, indices, data * 4.0))           # a power of two: the same q, always
    assert_array_equal(got[0], want[0])
    assert_array_equal(got[1], want[1])


def test_refusals_leave_the_outputs_untouched():
    import ctypes

    from schpf_amd import _lib
    lib = _lib.load()
    indptr, indices, data = score_graph(65, 3, JACCARD, 1)
    n = 65

    def refused(indptr, indices, data, message, gamma=1.0):
        labels, stats = np.full(n, -7, np.int32), np.full(4, -7, np.int64)
        indptr, indices = np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32)
        assert lib.schpf_debug_louvain(n, _p(indptr), _p(indices), _p(data), gamma, _p(labels),
                                       stats.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) != 0
        assert lib.schpf_last_error().decode() == message
        assert np.all(labels == -7) and np.all(stats == -7)
        with pytest.raises(ValueError):
            debug_louvain((indptr, indices, data), gamma)

    row_of = np.repeat(np.arange(n), np.diff(indptr))
    at = lambda row, j=0: int(indptr[row]) + j  # noqa: E731
    start = "indptr must be 0 at row 0 and must be non-decreasing; offending row %d"
    columns = "columns must be in [0, n) and strictly ascending within a row; offending row %d"
    values = "values must be finite and >= 0; offending row %d"
    bad = indptr.copy()
    bad[0] = 1
    refused(bad, indices, data, start % 0)
    bad = indptr.copy()
    bad[20], bad[40] = bad[19] - 1, bad[39] - 1
    refused(bad, indices, data, start % 19)
    for wrong in (-1, n):
        bad = indices.copy()
        bad[at(50)], bad[at(9, 1)] = n, wrong
        refused(indptr, bad, data, columns % 9)
    bad = indices.copy()
    bad[at(12, 1)] = bad[at(12, 0)]                              # twice: not strictly ascending
    refused(indptr, bad, data, columns % 12)
    bad = indices.copy()
    bad[at(30, 0)], bad[at(30, 1)] = bad[at(30, 1)], bad[at(30, 0)]
    refused(indptr, bad, data, columns % 30)
    for value in (-1e-300, np.inf, np.nan):
        bad = data.copy()
        bad[at(17, 2)], bad[at(60)] = value, np.nan
        refused(indptr, indices, bad, values % 17)
    bad_cols, bad_data = indices.copy(), data.copy()             # structure before values
    bad_cols[at(22, 1)] = bad_cols[at(22, 0)]
    bad_data[at(2)] = -1.0
    refused(indptr, bad_cols, bad_data, columns % 22)
    bad_ptr = indptr.copy()                                      # indptr before columns
    bad_ptr[41] = bad_ptr[40] - 1
    refused(bad_ptr, bad_cols, bad_data, start % 40)
    for gamma in (0.0, -1.0, np.inf, np.nan):
        refused(indptr, indices, data, "gamma must be finite and > 0", gamma=gamma)
    assert row_of[at(17, 2)] == 17
    labels, stats = debug_louvain((np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0)))     # n = 0
    assert len(labels) == 0 and stats.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ the quality
def test_modularity_reaches_networkx_less_the_margin():
    """Jaccard 15-NN graphs of 2 000 rows.  tests/golden/louvain_quality.json holds, per graph, the modularity of networkx's
    louvain_communities (the minimum over its seeds), recorded by tools/louvain_quality.py, and the margin: twice the
    worst shortfall measured with this definition, 5 % at the most."""
    from _knn_reference import gamma_scores
    from schpf_amd import modularity
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "louvain_quality.json")) as fh:
        golden = json.load(fh)
    margin = golden["margin"]
    assert 0 < margin <= 0.05 and margin >= 2 * max(g["measured_shortfall"] for g in golden["graphs"].values())
    makers = {"gamma_scores": lambda: gamma_scores(2000, 20, np.float64, seed=0), "ten_blobs": lambda: blob_scores(2000, seed=0)}
    assert set(makers) == set(golden["graphs"])
    for name, make in sorted(makers.items()):
        graph = knn_jaccard(make(), 15)
        labels, stats = debug_louvain(graph)
        got = modularity(as_csr(graph), labels)
        want = golden["graphs"][name]["networkx_modularity_min"]
        print("%s: modularity %.6f, networkx %.6f, short by %.4f %%, %d communities, %d levels, %d rounds"
              % (name, got, want, 100 * (1 - got / want), stats[0], stats[1], stats[2]))
        assert got >= want * (1 - margin)


def test_modularity_is_the_textbook_number():
    """Two triangles joined by an edge, split at the edge: 2 (6 / 14 - (7 / 14)^2) = 5 / 14; all in one: 0."""
    from scipy.sparse import csr_matrix
    from schpf_amd import modularity
    A = np.zeros((6, 6))
    for u, v in ((0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3)):
        A[u, v] = A[v, u] = 1.0
    assert abs(modularity(csr_matrix(A), [0, 0, 0, 1, 1, 1]) - 5.0 / 14.0) < 1e-15
    assert abs(modularity(A, np.zeros(6, int))) < 1e-15
    assert abs(modularity(csr_matrix(A), [0, 0, 0, 1, 1, 1], resolution=2.0) - (12.0 / 14.0 - 2 * 0.5)) < 1e-15
    assert modularity(csr_matrix((6, 6)), np.arange(6)) == 0.0
    with pytest.raises(ValueError):
        modularity(csr_matrix(A), [0, 1])


# ------------------------------------------------------------------------------------------- the Python layer and the CLI
@pytest.fixture
def neighbors(monkeypatch):
    """schpf_amd.neighbors with the host restatements in the place of schpf_knn, schpf_knn_graph and schpf_louvain."""
    from schpf_amd import neighbors as nb
    from _graph_reference import debug_graph
    from _knn_reference import debug_knn

    def clusters(indptr, indices, data, gamma, device):
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float64
        assert indptr.flags.c_contiguous and indices.flags.c_contiguous and data.flags.c_contiguous
        return debug_louvain((indptr, indices, data), gamma)

    monkeypatch.setattr(nb, "_louvain_host", clusters)
    monkeypatch.setattr(nb, "_graph_host", lambda method, idx, dist, device: debug_graph(idx, dist, method)[:3])
    monkeypatch.setattr(nb, "_search_host", lambda query, ref, k, self_first, device: debug_knn(query, ref, k, self_first))
    return nb


def test_louvain_in_python(neighbors):
    import schpf_amd
    assert schpf_amd.louvain is neighbors.louvain and {"louvain", "modularity"} <= set(schpf_amd.__all__)
    graph = score_graph(130, 15, UMAP, 2)
    G = as_csr(graph)
    want, want_stats = debug_louvain(graph)
    labels = neighbors.louvain(G)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.int32
    assert_array_equal(labels, want)
    labels, stats = neighbors.louvain(G.tocoo(), return_stats=True)          # any SciPy format
    assert_array_equal(labels, want)
    assert stats == dict(zip(("communities", "levels", "rounds", "total_weight"), want_stats.tolist()))
    shuffled = G.copy()                                                        # columns in any order: sorted on a copy
    for i in range(130):
        lo, hi = shuffled.indptr[i], shuffled.indptr[i + 1]
        shuffled.indices[lo:hi] = shuffled.indices[lo:hi][::-1]
        shuffled.data[lo:hi] = shuffled.data[lo:hi][::-1]
    shuffled.has_sorted_indices = False
    keep = shuffled.indices.copy()
    assert_array_equal(neighbors.louvain(shuffled), want)
    assert_array_equal(shuffled.indices, keep)
    assert_array_equal(neighbors.louvain(G, resolution=2.0), debug_louvain(graph, 2.0)[0])
    assert neighbors.modularity(G, want) > 0.3
    with pytest.raises(ValueError, match="resolution must be finite and > 0"):
        neighbors.louvain(G, resolution=0)
    with pytest.raises(ValueError, match="square"):
        neighbors.louvain(G[:10])
    bad = G.copy()
    bad.data[int(bad.indptr[5])] = -1.0
    with pytest.raises(ValueError, match="values must be finite and >= 0; offending row 5$"):
        neighbors.louvain(bad)


def toy_model(n_cells=60, n_genes=60, K=3):
    import schpf_amd
    rng = np.random.RandomState(0)
    gam = lambda shape: schpf_amd.HPF_Gamma(rng.gamma(1.0, 1.0, shape), rng.gamma(1.0, 1.0, shape) + 0.5)  # noqa: E731
    model = schpf_amd.scHPF(K)
    model.xi, model.theta = gam((n_cells,)), gam((n_cells, K))
    model.eta, model.beta = gam((n_genes,)), gam((n_genes, K))
    return model


def test_model_clusters(neighbors):
    model = toy_model()
    labels = model.clusters(k=5)
    graph = model.neighbor_graph(k=5, method="jaccard")[1]
    assert labels.shape == (60,) and labels.dtype == np.int32
    assert_array_equal(labels, neighbors.louvain(graph))
    assert 1 < labels.max() + 1 < 60
    finer = model.clusters(k=5, metric="cosine", method="umap", resolution=4.0)
    assert_array_equal(finer, neighbors.louvain(model.neighbor_graph(k=5, metric="cosine", method="umap")[1], resolution=4.0))


def test_score_clusters_on_the_command_line(neighbors, tmp_path):
    import schpf_amd
    from schpf_amd import cli
    model = toy_model()
    path = str(tmp_path / "model.joblib")
    schpf_amd.save_model(model, path)
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "graph"), "--knn", "5", "--knn-graph", "jaccard"]) == 0
    out = tmp_path / "clusters"
    assert cli.main(["score", "-m", path, "-o", str(out), "--knn", "5", "--knn-graph", "jaccard", "--clusters"]) == 0
    assert set(os.listdir(str(out))) - set(os.listdir(str(tmp_path / "graph"))) == {"clusters.txt"}
    got = np.loadtxt(str(out / "clusters.txt"), dtype=np.int64)
    assert_array_equal(got, model.clusters(k=5))
    args = json.load(open(str(out / "score_commandline_args.json")))
    assert args["clusters"] is True and args["resolution"] == 1.0
    fine = tmp_path / "fine"
    assert cli.main(["score", "-m", path, "-o", str(fine), "--knn", "5", "--knn-graph", "jaccard", "--clusters",
                     "--resolution", "3"]) == 0
    assert_array_equal(np.loadtxt(str(fine / "clusters.txt"), dtype=np.int64), model.clusters(k=5, resolution=3.0))
    # without the option the output set and the arguments file are what they were
    args = json.load(open(str(tmp_path / "graph" / "score_commandline_args.json")))
    assert "clusters" not in args and "resolution" not in args
    with pytest.raises((ValueError, SystemExit)):
        cli.main(["score", "-m", path, "-o", str(tmp_path / "bad"), "--knn", "5", "--clusters"])
    with pytest.raises((ValueError, SystemExit)):
        cli.main(["score", "-m", path, "-o", str(tmp_path / "bad2"), "--clusters"])
