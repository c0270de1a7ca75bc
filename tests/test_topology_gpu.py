"""Connected components and the cluster graph on the GPU: schpf_components[_device] and
schpf_cluster_graph[_device] equal the library's serial restatements bit for bit on every input of the host tests (the
rounds of the device, stats[4..5], are outside the contract), on a graph that spans every grid-stride loop, on a side stream
and on torch tensors; the doubling is held to its bound on passes; and the estimator and the command line end to end."""
import ctypes
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from conftest import ROOT, golden_coo, load_golden
from _louvain_reference import as_csr
from _topology_reference import (I64P, cases, debug_cluster_graph, debug_components, host_cluster_graph, host_components,
                                 loop_absorb_small, loop_paga, numpy_cluster_graph, numpy_components, path, two_components)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
CASES = cases()


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def _dev(a, dtype):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype), device="cuda:0")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def device_components(structure, within=None, stream=None):
    """schpf_components_device on torch tensors -> NumPy (comp, stats)."""
    from schpf_amd import _lib
    n = len(structure[0]) - 1
    d_indptr, d_indices, d_within = _dev(structure[0], np.int64), _dev(structure[1], np.int32), _dev(within, np.int32)
    d_comp = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    stats = np.full(6, -7, np.int64)
    torch.cuda.synchronize()
    _lib.check(_lib.load().schpf_components_device(0, ctypes.c_void_p(stream), n, _ptr(d_indptr), _ptr(d_indices), _ptr(d_within),
                                                   _ptr(d_comp), stats.ctypes.data_as(I64P)))
    return d_comp.cpu().numpy(), stats


def device_cluster_graph(graph, labels, G, weights=True, stream=None):
    """schpf_cluster_graph_device on torch tensors -> NumPy (cells, count, weight, wmax)."""
    from schpf_amd import _lib
    n = len(graph[0]) - 1
    d_indptr, d_indices, d_data = _dev(graph[0], np.int64), _dev(graph[1], np.int32), _dev(graph[2], np.float64)
    d_labels = _dev(labels, np.int32)
    cells = torch.full((G,), -7, dtype=torch.int64, device="cuda:0")
    count = torch.full((G, G), -7, dtype=torch.int64, device="cuda:0")
    weight = torch.full((G, G), -7, dtype=torch.int64, device="cuda:0") if weights else None
    wmax = ctypes.c_double(-7.0)
    torch.cuda.synchronize()
    _lib.check(_lib.load().schpf_cluster_graph_device(0, ctypes.c_void_p(stream), n, _ptr(d_indptr), _ptr(d_indices), _ptr(d_data),
                                                      _ptr(d_labels), G, _ptr(cells), _ptr(count), _ptr(weight),
                                                      ctypes.byref(wmax)))
    return cells.cpu().numpy(), count.cpu().numpy(), None if weight is None else weight.cpu().numpy(), wmax.value


def check_components(structure, within=None, want=None):
    want = debug_components(structure, within) if want is None else want
    found = []
    for got in (host_components(structure, within), device_components(structure, within)):
        assert_array_equal(got[1][:4], want[1][:4])
        assert_array_equal(got[0], want[0])
        found.append(got[1])
    return want, found


def check_cluster_graph(graph, labels, G, weights=True):
    want = debug_cluster_graph(graph, labels, G, weights)
    for got in (host_cluster_graph(graph, labels, G, weights), device_cluster_graph(graph, labels, G, weights)):
        for g, w in zip(got, want):
            assert_array_equal(g, w)
    return want


@pytest.mark.parametrize("case", sorted(CASES))
def test_components_equal_the_restatement(amd, case):
    structure, within = CASES[case]
    (comp, stats), found = check_components(structure, within)
    n = len(structure[0]) - 1
    for s in found:
        if len(structure[1]) == 0:
            assert s[4] == 0 and s[5] == 0
        else:
            assert s[4] >= 1 and s[5] >= 0       # the round that raises no flag is counted; no pass follows it
    if case == "two_cliques_through_a_stranger":
        assert comp.tolist() == [0] * 6 + [1] * 6 + [2, 2]
    if case == "hub_5000":
        assert stats[:3].tolist() == [1, n, 0]


@pytest.mark.parametrize("case", ["path_2e18_in_order", "path_4097_shuffled"])
def test_doubling_stays_within_its_bound(amd, case):
    """A path stored in order is one chain of length n after a single hook round.  Doubling halves every depth per pass, so a
    hook round is followed by at most ceil(log2 n) + 1 passes, the one that changes nothing included."""
    structure = path(1 << 18, False) if case == "path_2e18_in_order" else path(4097, True)
    n = len(structure[0]) - 1
    (comp, stats), found = check_components(structure)
    assert stats[:3].tolist() == [1, n, 0] and not comp.any()
    for s in found:
        print(case, "hook rounds", s[4], "shortcut passes", s[5])
        assert s[5] <= s[4] * (math.ceil(math.log2(n)) + 1)


@functools.lru_cache(maxsize=None)
def large_graph():
    """The Jaccard graph of the exact 15-NN self graph of 200 000 Gamma(0.3) score rows with K = 20 -- score_graph at a
    size its dense NumPy search cannot reach, so the search and the graph are the library's own, on the GPU."""
    import schpf_amd
    from _knn_reference import gamma_scores
    idx, dist = schpf_amd.knn(torch.tensor(gamma_scores(200000, 20, np.float64, seed=0), device="cuda:0"), k=15)
    G = schpf_amd.knn_connectivities(idx, dist, method="jaccard")
    graph = (G.crow_indices().cpu().numpy().astype(np.int64), G.col_indices().cpu().numpy().astype(np.int32),
             G.values().cpu().numpy().astype(np.float64))
    for a in graph:
        a.setflags(write=False)
    return graph


def test_graph_across_every_grid_stride_loop(amd):
    graph = large_graph()
    n = len(graph[0]) - 1
    assert n == 200000 and len(graph[1]) > 256 * 4096
    (comp, stats), _ = check_components(graph)
    assert stats[0] >= 1 and stats[1] > n // 2
    within = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(16)).astype(np.int64) % 6 - 1
    (pieces, stats_within), _ = check_components(graph, within.astype(np.int32))
    assert stats_within[0] > stats[0] and stats_within[3] < stats[3] and stats_within[2] >= (within == -1).sum()
    labels = (comp % 3 + 3 * (np.arange(n) % 5 == 0)).astype(np.int32)
    cells, count, weight, wmax = check_cluster_graph(graph, labels, 6)
    assert count.sum() == (graph[1] != np.repeat(np.arange(n), np.diff(graph[0]))).sum() and wmax == graph[2].max()


def test_counters_beyond_one_pass_of_the_grid(amd):
    """300 001 vertices in runs of 25 and of 500 along a path: more than the 1 024 workgroups of the counting kernels cover
    in one pass, wavefronts whose lanes all name one component beside wavefronts that straddle two, a component that changes
    between the passes of a wavefront, and more components -- and groups -- than the 4 096 LDS bins."""
    from _topology_reference import from_pairs
    n = 300001
    i = np.arange(1, n)
    cut = np.where(i % 1000 < 500, i % 25 == 0, i % 500 == 0)
    graph = from_pairs(n, i[~cut] - 1, i[~cut])
    (comp, stats), _ = check_components(graph)
    assert stats[0] == cut.sum() + 1 > 4096 and stats[1] == 500 and stats[2] == 1      # the last vertex is alone
    assert_array_equal(comp, np.concatenate([[0], np.cumsum(cut)]))
    labels = (comp % 5000 - (comp % 11 == 0)).astype(np.int32)                          # -1 among them, G beyond the bins
    cells, count, weight, wmax = check_cluster_graph(graph, labels, 5000)
    assert_array_equal(cells, np.bincount(labels[labels >= 0], minlength=5000))


def test_side_stream(amd):
    structure, within = CASES["plane_3nn_chessboard"]
    want = debug_components(structure, within)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        got = device_components(structure, within, stream=side.cuda_stream)
    assert_array_equal(got[0], want[0])
    assert_array_equal(got[1][:4], want[1][:4])
    graph = two_components()
    labels = (np.arange(60) % 4).astype(np.int32)
    with torch.cuda.stream(side):
        got = device_cluster_graph(graph, labels, 4, stream=side.cuda_stream)
    for g, w in zip(got, debug_cluster_graph(graph, labels, 4)):
        assert_array_equal(g, w)


def test_tensors_in_tensors_out(amd):
    graph, within = CASES["plane_3nn_chessboard"]
    want, want_stats = debug_components(graph, within)
    A = as_csr(graph)
    T = torch.sparse_csr_tensor(torch.tensor(graph[0]), torch.tensor(graph[1].astype(np.int64)), torch.tensor(graph[2]),
                                size=A.shape, device="cuda:0")
    comp, stats = amd.connected_components(T, within=torch.tensor(within, device="cuda:0"), return_stats=True)
    assert comp.is_cuda and comp.dtype == torch.int32
    assert_array_equal(comp.cpu().numpy(), want)
    assert [stats[k] for k in ("components", "largest", "singletons", "edges")] == want_stats[:4].tolist()
    assert_array_equal(amd.connected_components(T, within=within).cpu().numpy(), want)
    assert_array_equal(amd.connected_components(A, within=within), want)
    found = amd.cluster_graph(T, comp)
    table = debug_cluster_graph(graph, want, int(want_stats[0]))
    assert found["count"].is_cuda and found["n_cells"].dtype == torch.int64
    for name, w in zip(("n_cells", "count", "weight"), table):
        assert_array_equal(found[name].cpu().numpy(), w)
    assert found["wmax"] == table[3]
    host = amd.cluster_graph(A, want)
    for name, w in zip(("n_cells", "count", "weight"), table):
        assert_array_equal(host[name], w)
    paga = amd.paga(T, comp)
    np.testing.assert_allclose(paga["connectivities"], loop_paga(table[1], table[0])[0], rtol=1e-15)
    # louvain(connected=True) on a tensor stays on the GPU
    sym = as_csr(two_components())
    S = torch.sparse_csr_tensor(torch.tensor(sym.indptr.astype(np.int64)), torch.tensor(sym.indices.astype(np.int64)),
                                torch.tensor(sym.data), size=sym.shape, device="cuda:0")
    pieces, stats = amd.louvain(S, connected=True, return_stats=True)
    plain = amd.louvain(sym)
    assert pieces.is_cuda and stats["parent"].is_cuda
    assert_array_equal(stats["parent"].cpu().numpy()[pieces.cpu().numpy()], plain)
    assert_array_equal(pieces.cpu().numpy(), numpy_components((sym.indptr, sym.indices), plain)[0])
    assert_array_equal(amd.louvain(sym, connected=True), pieces.cpu().numpy())


@pytest.mark.parametrize("case", ["G1", "Gn", "G2000", "no_data", "directed"])
def test_cluster_graph_equals_the_restatement(amd, case):
    graph = two_components()
    n = 60
    off_diagonal = int((graph[1] != np.repeat(np.arange(n), np.diff(graph[0]))).sum())
    if case == "G1":
        cells, count, weight, wmax = check_cluster_graph(graph, np.zeros(n, np.int32), 1)
        assert count[0, 0] == off_diagonal and cells[0] == n      # labels all 0: every off-diagonal entry
    elif case == "Gn":
        cells, count, weight, wmax = check_cluster_graph(graph, np.arange(n, dtype=np.int32), n)
        assert_array_equal(count, (as_csr(graph).toarray() > 0).astype(np.int64))
    elif case == "G2000":
        big, _ = CASES["random_pairs"]
        labels = (np.random.RandomState(2).randint(0, 1200, len(big[0]) - 1) * 5 % 2000).astype(np.int32)
        labels[::7] = -1
        cells, count, weight, wmax = check_cluster_graph(big, labels, 2000)
        assert (cells == 0).sum() > 700 and cells.sum() == (labels >= 0).sum()
        want = numpy_cluster_graph(big, labels, 2000)
        assert_array_equal(count, want[1])
        assert_array_equal(weight, want[2])
        q = np.rint(np.ldexp(big[2] / big[2].max(), 30)).astype(np.int64)
        rows = np.repeat(np.arange(len(big[0]) - 1), np.diff(big[0]))
        take = (rows != big[1]) & (labels[rows] >= 0) & (labels[big[1]] >= 0)
        assert weight.sum() == q[take].sum()                      # the sum of q by NumPy
    elif case == "no_data":
        labels = (np.arange(n) % 4).astype(np.int32)
        cells, count, weight, wmax = check_cluster_graph((graph[0], graph[1], None), labels, 4)
        assert wmax == 1.0
        assert_array_equal(weight, count << 30)
        assert_array_equal(check_cluster_graph(graph, labels, 4, weights=False)[1], count)
    else:
        directed, within = CASES["plane_3nn_chessboard"]
        labels = np.where(within < 0, -1, within % 9).astype(np.int32)
        cells, count, weight, wmax = check_cluster_graph(directed, labels, 9)
        assert (count != count.T).any()


def test_refusals_on_the_device(amd):
    """The device validates as the restatement does: the same words for the same smallest offender, outputs untouched."""
    from schpf_amd import _lib
    lib = _lib.load()
    indptr, indices, data = two_components()
    n = len(indptr) - 1
    cols = indices.copy()
    cols[[indptr[17], indptr[40]]] = n
    within = np.zeros(n, np.int32)
    within[[5, 44]] = -2
    for structure, w, words in (((indptr, cols), within, "columns must be in [0, n); offending row 17"),
                                ((indptr, indices), within, "components: within must be >= -1; offending vertex 5")):
        for call in (host_components, device_components):
            with pytest.raises(ValueError, match=re.escape(words)):
                call(structure, w)
    vals = data.copy()
    vals[indptr[21]] = np.nan
    labels = (np.arange(n) % 4).astype(np.int32)
    bad_labels = labels.copy()
    bad_labels[[8, 33]] = 4
    for graph, lab, words in (((indptr, cols, vals), bad_labels, "columns must be in [0, n); offending row 17"),
                              ((indptr, indices, vals), bad_labels, "values must be finite and >= 0; offending row 21"),
                              ((indptr, indices, data), bad_labels, "labels must be in [-1, G); offending vertex 8")):
        for call in (host_cluster_graph, device_cluster_graph):
            with pytest.raises(ValueError, match=re.escape(words)):
                call(graph, lab, 4)
    comp = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    stats = np.full(6, -7, np.int64)
    assert lib.schpf_components_device(0, None, n, _ptr(_dev(indptr, np.int64)), _ptr(_dev(cols, np.int32)), None, _ptr(comp),
                                       stats.ctypes.data_as(I64P)) != 0
    assert (comp.cpu().numpy() == -7).all() and (stats == -7).all()


def test_fitted_model_end_to_end(amd, tmp_path):
    """clusters(connected=True, min_size=5) is louvain + components within + absorb_small; cluster_graph() is paga on the
    directed k-NN graph; `scHPF score --clusters --connected --paga` writes the same through a process of its own."""
    X = golden_coo(load_golden("pbmc_like_data.npz"))
    np.random.seed(0)
    model = amd.scHPF(5, max_iter=12, verbose=False).fit(X)
    N = X.shape[0]
    graph = model.neighbor_graph(k=5, method="jaccard")[1]
    arrays = (graph.indptr.astype(np.int64), graph.indices.astype(np.int32), graph.data.astype(np.float64))
    plain = model.clusters(k=5)
    pieces = model.clusters(k=5, connected=True)
    assert_array_equal(pieces, numpy_components(arrays, plain)[0])
    table = numpy_cluster_graph(arrays, pieces, int(pieces.max()) + 1)
    labels = model.clusters(k=5, connected=True, min_size=5)
    assert_array_equal(labels, loop_absorb_small(pieces, table[2], table[0], 5)[0])
    assert labels.shape == (N,)
    assert_array_equal(model.components(k=5), numpy_components(arrays)[0])
    found = model.cluster_graph(k=5, labels=pieces)
    indices, distances = model.neighbors(k=5)
    directed = (np.arange(0, 5 * N + 1, 5, dtype=np.int64), indices.astype(np.int32).ravel(), None)
    want = numpy_cluster_graph(directed, pieces, int(pieces.max()) + 1, weights=False)
    assert_array_equal(found["count"], want[1])
    assert_array_equal(found["n_cells"], want[0])
    conn, expected = loop_paga(want[1], want[0])
    np.testing.assert_allclose(found["connectivities"], conn, rtol=1e-15)
    np.testing.assert_allclose(found["expected"], expected, rtol=1e-15)
    assert_array_equal(model.cluster_graph(k=5, connected=True)["count"], want[1])

    model_path = str(tmp_path / "model.joblib")
    amd.save_model(model, model_path)
    exe = [sys.executable, os.path.join(ROOT, "bin", "scHPF"), "score", "-m", model_path, "--knn", "5", "--knn-graph", "jaccard"]
    subprocess.check_call(exe + ["-o", str(tmp_path / "plain"), "--clusters"], stdout=subprocess.DEVNULL)
    subprocess.check_call(exe + ["-o", str(tmp_path / "out"), "--clusters", "--connected", "--paga"], stdout=subprocess.DEVNULL)
    assert set(os.listdir(str(tmp_path / "out"))) - set(os.listdir(str(tmp_path / "plain"))) == {
        "components.txt", "paga_connectivities.txt", "paga_counts.txt"}
    assert_array_equal(np.loadtxt(str(tmp_path / "plain" / "clusters.txt"), dtype=np.int64), plain)
    assert_array_equal(np.loadtxt(str(tmp_path / "out" / "clusters.txt"), dtype=np.int64), pieces)
    assert_array_equal(np.loadtxt(str(tmp_path / "out" / "components.txt"), dtype=np.int64), numpy_components(arrays)[0])
    assert_array_equal(np.loadtxt(str(tmp_path / "out" / "paga_counts.txt"), dtype=np.int64, ndmin=2), want[1])
    np.testing.assert_allclose(np.loadtxt(str(tmp_path / "out" / "paga_connectivities.txt"), ndmin=2), conn, rtol=1e-15)
    # without --clusters the three options are errors, raised before anything is computed
    from schpf_amd import cli
    for flag in (["--connected"], ["--paga"], ["--min-cluster-size", "3"]):
        with pytest.raises(ValueError, match="belongs to --clusters"):
            cli.main(exe[2:] + ["-o", str(tmp_path / "refused")] + flag)
        assert not os.path.exists(str(tmp_path / "refused" / "cell_score.txt"))
