"""Louvain clustering on the GPU.  schpf_louvain and schpf_louvain_device against the library's host
restatement schpf_debug_louvain (tests/test_louvain_host.py pins it to the definition): equal labels and equal stats,
exactly, whatever the shape of the graph.  Then the Python surface: louvain on GPU CSR tensors, scHPF.clusters and
`scHPF score --knn K --knn-graph M --clusters`."""
import ctypes
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from conftest import golden_coo, load_golden
from _graph_reference import JACCARD, UMAP, duplicated_cells, far_neighbour, random_lists, unsorted
from _louvain_reference import (_p, as_csr, clique_ring, debug_louvain, host_louvain, hub, list_graph, ring_lattice, score_graph,
                                with_diagonal, with_empty_rows, with_tiny_weights, with_zero_rows)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
I64P = ctypes.POINTER(ctypes.c_int64)
ONE = (np.array([0, 0], np.int64), np.zeros(0, np.int32), np.zeros(0))
PAIR = (np.array([0, 1, 2], np.int64), np.array([1, 0], np.int32), np.array([0.25, 0.25]))


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def device_louvain(graph, gamma=1.0, stream=None):
    """schpf_louvain_device on torch tensors -> NumPy (labels, stats)."""
    from schpf_amd import _lib
    indptr, indices, data = graph
    n = len(indptr) - 1
    d_indptr = torch.tensor(np.ascontiguousarray(indptr, np.int64), device="cuda:0")
    d_indices = torch.tensor(np.ascontiguousarray(indices, np.int32), device="cuda:0")
    d_data = torch.tensor(np.ascontiguousarray(data, np.float64), device="cuda:0")
    d_labels = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    stats = np.full(4, -7, np.int64)
    torch.cuda.synchronize()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
    _lib.check(_lib.load().schpf_louvain_device(0, ctypes.c_void_p(stream), n, ptr(d_indptr), ptr(d_indices), ptr(d_data),
                                                float(gamma), ptr(d_labels), stats.ctypes.data_as(I64P)))
    return d_labels.cpu().numpy(), stats


def check_both(graph, gamma=1.0, want=None):
    want = debug_louvain(graph, gamma) if want is None else want
    for got in (host_louvain(graph, gamma), device_louvain(graph, gamma)):
        assert_array_equal(got[1], want[1])
        assert_array_equal(got[0], want[0])
    return want


@functools.lru_cache(maxsize=None)
def large_case():
    """The Jaccard and umap graphs of (70001, 15) lists with duplicated cells, far neighbours and unsorted columns, and the
    restatement's answers; computed once."""
    idx, dist = unsorted(*far_neighbour(*duplicated_cells(*random_lists(70001, 15, seed=70001))))
    graphs = {m: list_graph(idx, dist, m) for m in (UMAP, JACCARD)}
    for g in graphs.values():
        for a in g:
            a.setflags(write=False)
    return graphs, {m: debug_louvain(g) for m, g in graphs.items()}


SMALL = {
    "one_vertex": lambda: ONE,
    "pair": lambda: PAIR,
    "scores_65_3_umap": lambda: score_graph(65, 3, UMAP, 1),
    "scores_65_3_jaccard": lambda: score_graph(65, 3, JACCARD, 1),
    "scores_65_15_umap": lambda: score_graph(65, 15, UMAP, 4),
    "scores_65_15_jaccard": lambda: score_graph(65, 15, JACCARD, 4),
    "scores_130_3_umap": lambda: score_graph(130, 3, UMAP, 5),
    "scores_130_3_jaccard": lambda: score_graph(130, 3, JACCARD, 5),
    "scores_130_15_umap": lambda: score_graph(130, 15, UMAP, 2),
    "scores_130_15_jaccard": lambda: score_graph(130, 15, JACCARD, 2),
    "scores_300_128_umap": lambda: score_graph(300, 128, UMAP, 3),
    "scores_300_128_jaccard": lambda: score_graph(300, 128, JACCARD, 3),
    "ring_lattice": ring_lattice,
    "clique_ring": clique_ring,
    "empty_rows": lambda: with_empty_rows(score_graph(130, 15, JACCARD, 2), [0, 7, 64, 129]),
    "zero_rows": lambda: with_zero_rows(score_graph(130, 15, JACCARD, 2), [0, 7, 64, 129]),
    "tiny_weights": lambda: with_tiny_weights(score_graph(130, 15, UMAP, 2)),
    "diagonal": lambda: with_diagonal(score_graph(130, 15, UMAP, 2)),
}


@pytest.mark.parametrize("case", sorted(SMALL))
def test_small_graphs(amd, case):
    """The smallest graphs; ordinary ones across wave and workgroup edges; the densest lists; every score a tie; rows
    without entries and rows of no weight; entries that quantise to 0; a diagonal."""
    graph = SMALL[case]()
    labels, stats = check_both(graph)
    if case == "one_vertex":
        assert stats.tolist() == [1, 0, 0, 0]
    if case == "clique_ring":
        assert_array_equal(labels, np.repeat(np.arange(12), 8))
    if case == "tiny_weights":
        assert (np.rint(np.ldexp(graph[2] / graph[2].max(), 30)) == 0).sum() > 20


@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_resolutions(amd, gamma):
    check_both(score_graph(130, 15, JACCARD, 2), gamma)
    check_both(score_graph(130, 15, UMAP, 2), gamma)
    check_both(clique_ring(), gamma)


@pytest.mark.parametrize("method", [UMAP, JACCARD])
def test_sorts_and_reductions_across_many_blocks(amd, method):
    graphs, want = large_case()
    labels, stats = check_both(graphs[method], want=want[method])
    assert stats[1] >= 2 and stats[0] < 70001 // 10


def test_hub_of_degree_n_minus_1(amd):
    graph = hub(5000)
    assert graph[0][1] == 4999
    check_both(graph)


def test_all_zero_and_no_entries(amd):
    indptr, indices, data = score_graph(65, 3, UMAP, 1)
    for graph in ((indptr, indices, np.zeros_like(data)), (np.zeros(66, np.int64), np.zeros(0, np.int32), np.zeros(0))):
        labels, stats = check_both(graph)
        assert_array_equal(labels, np.arange(65))
        assert stats.tolist() == [65, 0, 0, 0]


def test_louvain_on_gpu_tensors(amd):
    """A sparse CSR tensor on the GPU in, a tensor on the same GPU out, equal to the host path's; on a side stream as well."""
    graphs, want = large_case()
    graph = graphs[JACCARD]
    n = len(graph[0]) - 1
    G = torch.sparse_csr_tensor(torch.tensor(graph[0]), torch.tensor(graph[1]), torch.tensor(graph[2]), size=(n, n)).to("cuda:0")
    keep = G.values().clone()
    labels, stats = amd.louvain(G, return_stats=True)
    assert labels.device == G.device and labels.dtype == torch.int32 and tuple(labels.shape) == (n,)
    assert_array_equal(labels.cpu().numpy(), want[JACCARD][0])
    assert list(stats.values()) == want[JACCARD][1].tolist()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        doubled = torch.sparse_csr_tensor(G.crow_indices(), G.col_indices(), G.values() * 2.0, size=(n, n))   # on this stream
        S = amd.louvain(doubled)
    side.synchronize()
    assert torch.equal(S, labels)
    assert torch.equal(G.values(), keep)
    small = score_graph(130, 15, UMAP, 2)
    H = amd.louvain(as_csr(small), resolution=2.0)                                # SciPy in, NumPy out
    assert isinstance(H, np.ndarray) and H.dtype == np.int32
    assert_array_equal(H, debug_louvain(small, 2.0)[0])
    with pytest.raises(ValueError, match="device=1 was asked for"):
        amd.louvain(G, device=1)


def test_refused_calls_leave_their_outputs(amd):
    from schpf_amd import _lib
    lib = _lib.load()
    indptr, indices, data = score_graph(130, 15, JACCARD, 2)
    n = 130
    at = lambda row, j=0: int(indptr[row]) + j  # noqa: E731
    start = "indptr must be 0 at row 0 and must be non-decreasing; offending row %d$"
    columns = r"columns must be in \[0, n\) and strictly ascending within a row; offending row %d$"
    values = "values must be finite and >= 0; offending row %d$"
    for call in (host_louvain, device_louvain):
        bad = indptr.copy()
        bad[0] = 1
        with pytest.raises(ValueError, match=start % 0):
            call((bad, indices, data))
        bad = indptr.copy()
        bad[71], bad[101] = bad[70] - 1, bad[100] - 1
        with pytest.raises(ValueError, match=start % 70):
            call((bad, indices, data))
        for wrong in (-1, n):
            bad = indices.copy()
            bad[at(100)], bad[at(70, 1)] = n, wrong
            with pytest.raises(ValueError, match=columns % 70):
                call((indptr, bad, data))
        bad = indices.copy()
        bad[at(64, 1)], bad[at(129, 3)] = bad[at(64, 0)], bad[at(129, 2)]
        with pytest.raises(ValueError, match=columns % 64):
            call((indptr, bad, data))
        for value in (-1e-300, np.inf, np.nan):
            bad = data.copy()
            bad[at(66, 2)], bad[at(128)] = value, np.nan
            with pytest.raises(ValueError, match=values % 66):
                call((indptr, indices, bad))
        bad_cols, bad_data = indices.copy(), data.copy()
        bad_cols[at(90, 1)] = bad_cols[at(90, 0)]
        bad_data[at(2)] = -1.0
        with pytest.raises(ValueError, match=columns % 90):
            call((indptr, bad_cols, bad_data))
        with pytest.raises(ValueError, match="gamma must be finite and > 0"):
            call((indptr, indices, data), 0.0)
    # the outputs of a refused call keep what they held
    bad = data.copy()
    bad[at(5)] = np.nan
    labels, stats = np.full(n, -7, np.int32), np.full(4, -7, np.int64)
    assert lib.schpf_louvain(0, n, _p(indptr), _p(indices), _p(bad), 1.0, _p(labels), stats.ctypes.data_as(I64P)) != 0
    assert np.all(labels == -7) and np.all(stats == -7)
    t_indptr, t_indices, t_bad = (torch.tensor(a, device="cuda:0") for a in (indptr, indices, bad))
    t_labels = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.schpf_louvain_device(0, None, n, dp(t_indptr), dp(t_indices), dp(t_bad), 1.0, dp(t_labels),
                                    stats.ctypes.data_as(I64P)) != 0
    assert b"offending row 5" in lib.schpf_last_error()
    assert bool((t_labels == -7).all()) and np.all(stats == -7)
    # n = 0 succeeds: stats 0, nothing else read or written; a device that does not exist does not
    assert lib.schpf_louvain(0, 0, None, None, None, 1.0, None, stats.ctypes.data_as(I64P)) == 0
    assert stats.tolist() == [0, 0, 0, 0]
    stats[:] = -7
    assert lib.schpf_louvain_device(0, None, 0, None, None, None, 1.0, None, stats.ctypes.data_as(I64P)) == 0
    assert stats.tolist() == [0, 0, 0, 0]
    assert lib.schpf_louvain(99, n, _p(indptr), _p(indices), _p(data), 1.0, _p(labels), stats.ctypes.data_as(I64P)) != 0
    assert b"no such HIP device" in lib.schpf_last_error()


def test_fitted_model_end_to_end(amd, tmp_path):
    """Fit the small golden matrix: clusters is neighbor_graph + louvain, and `scHPF score --knn 5 --knn-graph jaccard
    --clusters` writes the same labels."""
    from schpf_amd import cli
    X = golden_coo(load_golden("pbmc_like_data.npz"))
    np.random.seed(0)
    model = amd.scHPF(5, max_iter=12, verbose=False).fit(X)
    N = X.shape[0]
    labels = model.clusters(k=5)
    graph = model.neighbor_graph(k=5, method="jaccard")[1]
    assert labels.shape == (N,) and labels.dtype == np.int32
    want, stats = debug_louvain((graph.indptr, graph.indices, graph.data))
    assert_array_equal(labels, want)
    assert 1 < stats[0] < N and sorted(set(labels.tolist())) == list(range(int(stats[0])))
    assert amd.modularity(graph, labels) > 0.3
    path = str(tmp_path / "model.joblib")
    amd.save_model(model, path)
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "graph"), "--knn", "5", "--knn-graph", "jaccard"]) == 0
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "out"), "--knn", "5", "--knn-graph", "jaccard", "--clusters"]) == 0
    assert set(os.listdir(str(tmp_path / "out"))) - set(os.listdir(str(tmp_path / "graph"))) == {"clusters.txt"}
    assert_array_equal(np.loadtxt(str(tmp_path / "out" / "clusters.txt"), dtype=np.int64), labels)
