"""Connected components, the cluster graph and their Python helpers without a GPU: the library's serial
restatements schpf_debug_components and schpf_debug_cluster_graph against SciPy and NumPy, every refusal, and
`absorb_small`, `paga` and `louvain(connected=True)` against their definitions."""
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse.csgraph import connected_components as scipy_components

from _louvain_reference import as_csr, debug_louvain, knn_jaccard
from _topology_reference import (I64P, _cluster_graph, _components, _p, cases, debug_cluster_graph, debug_components,
                                 loop_absorb_small, loop_paga, numpy_cluster_graph, numpy_components, random_pairs, two_components)

CASES = cases()


@pytest.fixture(scope="module")
def lib():
    from schpf_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", sorted(CASES))
def test_components_match_scipy(case):
    structure, within = CASES[case]
    comp, stats = debug_components(structure, within)
    want, want_stats = numpy_components(structure, within)
    assert_array_equal(comp, want)
    assert_array_equal(stats[:4], want_stats)
    n = len(structure[0]) - 1
    if case in ("path_4097_shuffled", "path_4097_in_order", "hub_5000"):
        assert stats[:3].tolist() == [1, n, 0]
    if case in ("no_entries", "diagonal_only", "n1"):
        assert stats[:4].tolist() == [n, 1, n, 0] and comp.tolist() == list(range(n))
    if case == "n0":
        assert stats.tolist() == [0] * 6
    if case == "two_components":
        assert stats[0] == 2 and comp[0] == 0 and comp[-1] == 1
    if case == "plane_3nn_directed":
        assert 1 < stats[0] < n // 100
    if case == "plane_3nn_chessboard":
        assert stats[2] >= n // 50       # every vertex of group -1 is alone
    if case == "two_cliques_through_a_stranger":
        # the two cliques of community 0 are joined only through a vertex of community 1: they split
        assert comp.tolist() == [0] * 6 + [1] * 6 + [2, 2]


@pytest.mark.parametrize("case", ["two_components", "random_pairs", "plane_3nn_directed", "hub_5000", "diagonal_only", "no_entries",
                                  "n0"])
def test_cluster_graph_matches_numpy(case):
    graph = CASES[case][0]
    n = len(graph[0]) - 1
    rng = np.random.RandomState(11)
    for G in (1, 7):
        labels = rng.randint(-1, G, n).astype(np.int32)
        cells, count, weight, wmax = debug_cluster_graph(graph, labels, G)
        want = numpy_cluster_graph(graph, labels, G)
        assert_array_equal(cells, want[0])
        assert_array_equal(count, want[1])
        assert_array_equal(weight, want[2])
        assert wmax == want[3]
        # data = NULL: every entry weighs 2^30; weight = NULL: the counts alone
        ones = debug_cluster_graph((graph[0], graph[1], None), labels, G)
        assert_array_equal(ones[1], want[1])
        assert_array_equal(ones[2], want[1] << 30)
        assert ones[3] == (1.0 if len(graph[1]) else 0.0)
        assert_array_equal(debug_cluster_graph(graph, labels, G, weights=False)[1], want[1])


def test_cluster_graph_of_stored_zeros():
    """Stored zeros count, and with wmax == 0 every entry weighs 2^30."""
    indptr, indices, data = two_components()
    labels = (np.arange(60) % 3).astype(np.int32)
    cells, count, weight, wmax = debug_cluster_graph((indptr, indices, np.zeros_like(data)), labels, 3)
    assert wmax == 0.0 and count.sum() == len(indices)
    assert_array_equal(weight, count << 30)


def _refused(lib, status, words):
    assert status != 0
    assert words in lib.schpf_last_error().decode()


def test_components_refusals_leave_the_outputs(lib):
    fn = lib.schpf_debug_components
    indptr, indices, _ = two_components()
    n = len(indptr) - 1
    within = np.zeros(n, np.int32)

    def refused(structure, w, words):
        status, comp, stats = _components(fn, structure, w)
        _refused(lib, status, words)
        assert (comp == -7).all() and (stats == -7).all()

    bad = indptr.copy()
    bad[0] = 1
    refused((bad, indices), None, "indptr must be 0 at row 0 and must be non-decreasing; offending row 0")
    bad = indptr.copy()
    bad[10] = bad[9] - 1
    refused((bad, indices), None, "indptr must be 0 at row 0 and must be non-decreasing; offending row 9")
    for value in (-1, n):
        cols = indices.copy()
        cols[indptr[17]] = value
        cols[indptr[40]] = value
        refused((indptr, cols), None, "columns must be in [0, n); offending row 17")
        # indptr before columns, columns before within
        bad = indptr.copy()
        bad[30] = bad[29] - 1
        refused((bad, cols), None, "offending row 29")
        w = within.copy()
        w[3] = -2
        refused((indptr, cols), w, "columns must be in [0, n); offending row 17")
    w = within.copy()
    w[[5, 44]] = -2, -9
    refused((indptr, indices), w, "components: within must be >= -1; offending vertex 5")
    # before any read
    stats = np.full(6, -7, np.int64)
    comp = np.full(n, -7, np.int32)
    _refused(lib, fn(-1, _p(indptr), _p(indices), None, _p(comp), stats.ctypes.data_as(I64P)), "n must be in [0, 2^31)")
    _refused(lib, fn(n, None, _p(indices), None, _p(comp), stats.ctypes.data_as(I64P)), "must not be NULL")
    _refused(lib, fn(n, _p(indptr), _p(indices), None, None, stats.ctypes.data_as(I64P)), "must not be NULL")
    _refused(lib, fn(n, _p(indptr), _p(indices), None, _p(comp), None), "stats must not be NULL")
    _refused(lib, fn(n, _p(indptr), None, None, _p(comp), stats.ctypes.data_as(I64P)), "indices must not be NULL")
    huge = np.zeros(3, np.int64)
    huge[1:] = 1 << 32
    _refused(lib, fn(2, _p(huge), _p(indices), None, _p(comp), stats.ctypes.data_as(I64P)), "nnz must be below 2^32")
    assert (comp == -7).all() and (stats == -7).all()


def test_cluster_graph_refusals_leave_the_outputs(lib):
    fn = lib.schpf_debug_cluster_graph
    indptr, indices, data = two_components()
    n = len(indptr) - 1
    labels = (np.arange(n) % 4).astype(np.int32)

    def refused(graph, lab, G, words):
        status, cells, count, weight, wmax = _cluster_graph(fn, graph, lab, G)
        _refused(lib, status, words)
        assert (cells == -7).all() and (count == -7).all() and (weight == -7).all() and wmax == -7.0

    bad = indptr.copy()
    bad[10] = bad[9] - 1
    refused((bad, indices, data), labels, 4, "indptr must be 0 at row 0 and must be non-decreasing; offending row 9")
    cols = indices.copy()
    cols[indptr[17]] = n
    refused((indptr, cols, data), labels, 4, "columns must be in [0, n); offending row 17")
    for value in (-0.5, np.nan, np.inf):
        vals = data.copy()
        vals[indptr[21]] = value
        refused((indptr, indices, vals), labels, 4, "values must be finite and >= 0; offending row 21")
        refused((indptr, cols, vals), labels, 4, "columns must be in [0, n); offending row 17")
        lab = labels.copy()
        lab[2] = 4
        refused((indptr, indices, vals), lab, 4, "values must be finite and >= 0; offending row 21")
    for value in (-2, 4):
        lab = labels.copy()
        lab[[8, 33]] = value
        refused((indptr, indices, data), lab, 4, "cluster_graph: labels must be in [-1, G); offending vertex 8")
    # columns need not ascend: no refusal
    flipped = indices.copy()
    flipped[indptr[1]:indptr[2]] = flipped[indptr[1]:indptr[2]][::-1]
    assert _cluster_graph(fn, (indptr, flipped, data), labels, 4)[0] == 0
    # before any read
    status = _cluster_graph(fn, (indptr, indices, data), labels, 0)[0]
    _refused(lib, status, "ngroups must be at least 1")
    cells, count = np.zeros(1, np.int64), np.zeros(1, np.int64)
    wmax = ctypes.c_double(-7.0)
    _refused(lib, fn(n, _p(indptr), _p(indices), _p(data), _p(labels), 46341, _p(cells), _p(count), None, ctypes.byref(wmax)),
             "ngroups * ngroups must be below 2^31")
    _refused(lib, fn(-1, _p(indptr), _p(indices), _p(data), _p(labels), 1, _p(cells), _p(count), None, ctypes.byref(wmax)),
             "n must be in [0, 2^31)")
    _refused(lib, fn(n, _p(indptr), _p(indices), _p(data), None, 1, _p(cells), _p(count), None, ctypes.byref(wmax)),
             "must not be NULL")
    _refused(lib, fn(n, _p(indptr), _p(indices), _p(data), _p(labels), 1, None, _p(count), None, ctypes.byref(wmax)),
             "must not be NULL")
    assert wmax.value == -7.0


def test_absorb_small_follows_its_definition():
    from schpf_amd import absorb_small
    rng = np.random.RandomState(5)
    for trial in range(20):
        G = int(rng.randint(1, 12))
        table = rng.randint(0, 4, (G, G)) * (rng.rand(G, G) < 0.4)
        sizes = rng.randint(0, 9, G)
        labels = rng.randint(-1, G, 50)
        for min_size in (0, 3, 6, 100):
            got = absorb_small(labels, table, sizes, min_size)
            want = loop_absorb_small(labels, table, sizes, min_size)
            for g, w in zip(got, want):
                assert_array_equal(g, w)
            assert got[2].sum() == sizes.sum() and got[1].sum() == table.sum()
    # a splinter of two hangs on group 0; group 3 is as small but has no outside edge and stays; ties go to the lowest id
    table = np.array([[50, 3, 1, 0], [3, 40, 0, 0], [1, 0, 2, 0], [0, 0, 0, 2]])
    labels, merged, sizes = absorb_small(np.array([0, 1, 2, 3, -1, 2]), table, [30, 30, 2, 2], 5)
    assert labels.tolist() == [0, 1, 0, 2, -1, 0] and sizes.tolist() == [32, 30, 2]
    assert merged.tolist() == [[54, 3, 0], [3, 40, 0], [0, 0, 2]]
    tie = absorb_small(np.array([0, 1, 2]), np.array([[0, 0, 0], [0, 0, 0], [4, 4, 0]]), [9, 9, 1], 2)
    assert tie[0].tolist() == [0, 1, 0]
    untouched = absorb_small(np.array([0, 1, 2]), np.array([[0, 0, 0], [0, 0, 0], [4, 4, 0]]), [9, 9, 1], 0)
    assert untouched[0].tolist() == [0, 1, 2]


def test_paga_tables_follow_their_definition():
    from schpf_amd.topology import paga_tables
    rng = np.random.RandomState(9)
    for trial in range(20):
        G = int(rng.randint(1, 9))
        count = rng.randint(0, 30, (G, G)) * (rng.rand(G, G) < 0.5)
        ns = rng.randint(1, 40, G)
        got = paga_tables(count, ns)
        want = loop_paga(count, ns)
        np.testing.assert_allclose(got[0], want[0], rtol=1e-15, atol=0)
        np.testing.assert_allclose(got[1], want[1], rtol=1e-15, atol=0)
        assert (got[0] == got[0].T).all() and got[0].max(initial=0) <= 1.0 and (np.diagonal(got[0]) == 0).all()
    # group 2 has no outside edge: its row and column are 0.  Groups 0 and 1 are linked but hold no cells: expected == 0
    # and the connectivity is 1
    count = np.array([[4, 2, 0, 0], [1, 6, 0, 0], [0, 0, 9, 0], [0, 0, 0, 3]])
    conn, expected = paga_tables(count, [0, 0, 5, 5])
    assert expected[0, 1] == 0 and conn[0, 1] == conn[1, 0] == 1.0
    assert not conn[2].any() and not conn[:, 2].any() and not expected[2].any()
    assert_array_equal(np.array(loop_paga(count, [0, 0, 5, 5])), np.array([conn, expected]))


class HostLibrary:
    """The library with the two GPU entry points that louvain(connected=True) calls answered by their host restatements."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def schpf_louvain(self, device, *args):
        return self._lib.schpf_debug_louvain(*args)

    def schpf_components(self, device, *args):
        return self._lib.schpf_debug_components(*args)

    def schpf_cluster_graph(self, device, *args):
        return self._lib.schpf_debug_cluster_graph(*args)


@pytest.fixture
def on_the_host(lib, monkeypatch):
    from schpf_amd import _lib
    proxy = HostLibrary(lib)
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)


def test_connected_louvain_returns_connected_clusters(on_the_host):
    """The 15-NN Jaccard graph of 2 000 unclustered Gamma(0.3) score rows: Louvain's communities need not be connected;
    with connected=True every returned cluster is, and `parent` maps it back to the plain labelling."""
    import schpf_amd
    from _knn_reference import gamma_scores
    graph = knn_jaccard(gamma_scores(2000, 20, np.float64, seed=0), 15)
    A = as_csr(graph)
    plain = schpf_amd.louvain(A)
    assert_array_equal(plain, debug_louvain(graph)[0])
    pieces, stats = schpf_amd.louvain(A, connected=True, return_stats=True)
    assert_array_equal(pieces, schpf_amd.louvain(A, connected=True))
    parent = stats["parent"]
    assert stats["clusters"] == len(parent) == pieces.max() + 1 >= stats["communities"]
    assert_array_equal(parent[pieces], plain)
    for c in range(stats["clusters"]):
        members = np.flatnonzero(pieces == c)
        assert scipy_components(A[members][:, members], directed=False)[0] == 1
    # the pieces of a community are its SciPy components, in ascending order of first member
    assert_array_equal(pieces, numpy_components(graph, plain)[0])
    # and the helpers compose on the host as they do on the GPU
    table = schpf_amd.cluster_graph(A, pieces)
    want = numpy_cluster_graph(graph, pieces, stats["clusters"])
    assert_array_equal(table["count"], want[1])
    assert_array_equal(table["weight"], want[2])
    assert_array_equal(table["n_cells"], np.bincount(pieces))
    merged = schpf_amd.absorb_small(pieces, table["weight"], table["n_cells"], 5)
    for got, wanted in zip(merged, loop_absorb_small(pieces, want[2], want[0], 5)):
        assert_array_equal(got, wanted)
    found = schpf_amd.paga(A, pieces)
    assert_array_equal(found["count"], want[1])
    np.testing.assert_allclose(found["connectivities"], loop_paga(want[1], want[0])[0], rtol=1e-15)


def test_connected_components_reads_within(on_the_host):
    import schpf_amd
    graph, within = CASES["plane_3nn_chessboard"]
    A = as_csr(graph)
    comp, stats = schpf_amd.connected_components(A, within=within, return_stats=True)
    want, want_stats = numpy_components(graph, within)
    assert_array_equal(comp, want)
    assert [stats[k] for k in ("components", "largest", "singletons", "edges")] == want_stats.tolist()
    assert_array_equal(schpf_amd.connected_components(A), numpy_components(graph)[0])
    with pytest.raises(ValueError):
        schpf_amd.connected_components(A, within=within[:-1])
    bad = within.copy()
    bad[3] = -2
    with pytest.raises(Exception, match="within must be >= -1; offending vertex 3"):
        schpf_amd.connected_components(A, within=bad)


def test_random_pairs_are_mostly_small_components():
    """20 000 vertices and 11 000 drawn pairs sit below the giant-component threshold: thousands of components, most of
    them single vertices, the largest a small fraction."""
    comp, stats = debug_components(random_pairs())
    assert 8000 < stats[0] < 10000 and stats[2] > 6000 and stats[1] < 6000
