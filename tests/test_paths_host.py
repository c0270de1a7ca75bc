"""Shortest-path distances and what is built on them without a GPU: the library's serial restatement
schpf_debug_geodesic against SciPy's Dijkstra bit for bit, every refusal, and `geodesic_distances`, `pseudotime`,
`farthest_landmarks` and `landmark_isomap` against their definitions with the restatement in the kernels' place."""
import os
import re

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse.csgraph import dijkstra

from conftest import ROOT
from _louvain_reference import as_csr
from _paths_reference import (ROOT_TILE, _geodesic, as_stored, bits, cases, debug_geodesic, expected, grid, loop_farthest_landmarks,
                              loop_landmark_isomap, pack_sets, plane_lengths, scipy_geodesic)
from _topology_reference import I64P, _p, two_components

CASES = cases()


@pytest.fixture(scope="module")
def lib():
    from schpf_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_equals_scipy(case):
    graph, directed, sets = CASES[case]
    dist, stats = debug_geodesic(graph, directed, sets)
    want = expected(case)
    assert_array_equal(bits(dist), bits(want))
    assert stats.tolist() == [int(np.isfinite(want).sum()), 0, 0]
    if case == "grid_30":
        y, x = np.divmod(np.arange(900), 30)
        assert_array_equal(dist[0], x + y)
        assert_array_equal(dist[2], np.minimum(x + y, 58 - x - y))
    if case == "two_components":
        assert np.isinf(dist[0, 30:]).all() and np.isinf(dist[1, :30]).all() and np.isfinite(dist[2]).all()
    if case in ("n1", "no_entries", "plane_3nn_undirected_empty_between"):
        assert np.isinf(dist[1]).all()
    if case == "plane_hops_undirected":
        assert_array_equal(dist[np.isfinite(dist)], np.rint(dist[np.isfinite(dist)]))
    if case == "plane_huge_undirected":
        # a sum that overflows is +inf: fewer finite distances than vertices the roots can reach
        assert np.isfinite(dist[0]).sum() < np.isfinite(expected("plane_3nn_undirected_empty_between")[0]).sum()
    if case == "plane_special_undirected":
        # the zeros, the tiny and the repeated entries are on shortest paths: most distances differ from the plain graph's
        assert (bits(dist) != bits(expected("plane_3nn_undirected_empty_between"))).sum() > 10000


def test_a_set_is_the_minimum_over_its_members():
    """`min_only=True`, which the yardstick uses for the set of a thousand, is the elementwise minimum of the rows."""
    graph = plane_lengths()
    members = CASES["plane_3nn_undirected_a_thousand_members"][2][0][:40]
    rows = dijkstra(as_stored(graph), directed=False, indices=members)
    assert_array_equal(bits(rows.min(axis=0)), bits(dijkstra(as_stored(graph), directed=False, indices=members, min_only=True)))
    assert_array_equal(bits(rows.min(axis=0)), bits(debug_geodesic(graph, False, [members])[0][0]))


def _refused(lib, status, words):
    assert status != 0
    assert words in lib.schpf_last_error().decode()


def test_refusals_leave_the_outputs(lib):
    fn = lib.schpf_debug_geodesic
    indptr, indices, data = two_components()
    n = len(indptr) - 1
    set_ptr, roots = pack_sets([[0], [45, 3], [50]])

    def refused(graph, sp, rt, words):
        status, dist, stats = _geodesic(fn, graph, False, sp, rt)
        _refused(lib, status, words)
        assert (dist == -7).all() and (stats == -7).all()

    bad_ptr = indptr.copy()
    bad_ptr[0] = 1
    refused((bad_ptr, indices, data), set_ptr, roots, "indptr must be 0 at row 0 and must be non-decreasing; offending row 0")
    bad_ptr = indptr.copy()
    bad_ptr[10] = bad_ptr[9] - 1
    bad_ptr[30] = bad_ptr[29] - 1
    refused((bad_ptr, indices, data), set_ptr, roots, "indptr must be 0 at row 0 and must be non-decreasing; offending row 9")
    cols = indices.copy()
    cols[[indptr[17], indptr[40]]] = n, -1
    refused((indptr, cols, data), set_ptr, roots, "columns must be in [0, n); offending row 17")
    refused((bad_ptr, cols, data), set_ptr, roots, "offending row 9")                       # indptr before columns
    bad_sets = set_ptr.copy()
    bad_sets[0] = 1
    bad_roots = roots.copy()
    bad_roots[[1, 3]] = n, -1
    for value in (-0.5, np.nan, np.inf, -np.inf):
        vals = data.copy()
        vals[[indptr[21], indptr[50]]] = value
        refused((indptr, indices, vals), set_ptr, roots, "values must be finite and >= 0; offending row 21")
        refused((indptr, cols, vals), set_ptr, roots, "columns must be in [0, n); offending row 17")     # columns before values
        refused((indptr, indices, vals), bad_sets, bad_roots, "values must be finite and >= 0; offending row 21")
    refused((indptr, indices, data), bad_sets, roots, "geodesic: set_ptr must be 0 at set 0 and must be non-decreasing; offending set 0")
    bad_sets = np.array([0, 3, 2, 4, 3], np.int64)
    refused((indptr, indices, data), bad_sets, np.zeros(4, np.int32),
            "geodesic: set_ptr must be 0 at set 0 and must be non-decreasing; offending set 1")
    refused((indptr, indices, data), bad_sets, bad_roots, "offending set 1")                # set_ptr before roots
    for value in (-1, n):
        bad_roots = roots.copy()
        bad_roots[[1, 3]] = value
        refused((indptr, indices, data), set_ptr, bad_roots, "geodesic: roots must be in [0, n); offending set 1")
    # a stored zero, -0.0 and data == NULL are fine, and so are columns that do not ascend
    vals = data.copy()
    vals[:4] = 0.0, -0.0, 0.0, 5e-324
    assert _geodesic(fn, (indptr, indices[::-1].copy(), vals), False, set_ptr, roots)[0] == 0
    assert _geodesic(fn, (indptr, indices, None), True, set_ptr, roots)[0] == 0

    # before anything is read
    dist = np.full((3, n), -7.0)
    stats = np.full(3, -7, np.int64)
    S = stats.ctypes.data_as(I64P)
    args = dict(n=n, indptr=_p(indptr), indices=_p(indices), data=_p(data), directed=0, nsets=3, set_ptr=_p(set_ptr), roots=_p(roots),
                dist=_p(dist), stats=S)

    def call(**change):
        a = dict(args, **change)
        return fn(a["n"], a["indptr"], a["indices"], a["data"], a["directed"], a["nsets"], a["set_ptr"], a["roots"], a["dist"], a["stats"])

    _refused(lib, call(n=-1), "n must be in [0, 2^31)")
    _refused(lib, call(nsets=-1), "nsets must be in [0, 2^31)")
    _refused(lib, call(stats=None), "stats must not be NULL")
    for name in ("indptr", "set_ptr", "dist"):
        _refused(lib, call(**{name: None}), "indptr, set_ptr and dist must not be NULL")
    _refused(lib, call(indices=None), "indices must not be NULL")
    _refused(lib, call(roots=None), "roots must not be NULL")
    _refused(lib, call(n=2 ** 31 - 1, nsets=2 ** 31 - 1), "the bytes of dist, 8 * nsets * n, must be below 2^63")
    huge = np.zeros(3, np.int64)
    huge[1:] = 1 << 32
    _refused(lib, call(n=2, indptr=_p(huge)), "nnz must be below 2^32")
    assert (dist == -7).all() and (stats == -7).all()
    # n == 0 or nsets == 0: success, stats = 0, nothing else is read
    assert fn(0, None, None, None, 0, 5, None, None, None, S) == 0 and stats.tolist() == [0, 0, 0]
    stats[:] = -7
    assert fn(n, None, None, None, 0, 0, None, None, None, S) == 0 and stats.tolist() == [0, 0, 0]
    assert (dist == -7).all()


def test_root_tile_is_mirrored():
    from schpf_amd import paths
    source = open(os.path.join(ROOT, "schpf_amd", "csrc", "geodesic.hip")).read()
    assert int(re.search(r"constexpr int ROOT_TILE = (\d+);", source).group(1)) == paths.ROOT_TILE == ROOT_TILE


class HostLibrary:
    """The library with the GPU entry point of the distances answered by its host restatement."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def schpf_geodesic(self, device, *args):
        return self._lib.schpf_debug_geodesic(*args)


@pytest.fixture
def on_the_host(lib, monkeypatch):
    from schpf_amd import _lib
    proxy = HostLibrary(lib)
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)


def test_geodesic_distances_reads_every_form_of_roots(on_the_host):
    import schpf_amd
    graph = two_components()
    A = as_csr(graph)
    want = scipy_geodesic(graph, False, [[0], [45], [3, 50]])
    one = schpf_amd.geodesic_distances(A, 0)
    assert one.shape == (1, 60) and one.dtype == np.float64
    assert_array_equal(bits(one[0]), bits(want[0]))
    each = schpf_amd.geodesic_distances(A, np.array([0, 45]))
    assert_array_equal(bits(each), bits(want[:2]))
    assert_array_equal(bits(schpf_amd.geodesic_distances(A, [0, 45])), bits(want[:2]))
    sets, stats = schpf_amd.geodesic_distances(A, [np.array([0]), [45], (3, 50)], return_stats=True)
    assert_array_equal(bits(sets), bits(want))
    assert stats == {"finite": int(np.isfinite(want).sum()), "rounds": 0, "lowering_writes": 0}
    mask = np.zeros(60, bool)
    mask[[3, 50]] = True
    assert_array_equal(bits(schpf_amd.geodesic_distances(A, mask)), bits(want[2:]))
    assert_array_equal(bits(schpf_amd.geodesic_distances(A, [[], [0]])), bits(np.stack([np.full(60, np.inf), want[0]])))
    assert_array_equal(bits(schpf_amd.geodesic_distances(A.toarray(), 0)), bits(want[:1]))
    # directed: SciPy's directed=True on the stored entries
    D = as_csr(plane_lengths())
    assert_array_equal(bits(schpf_amd.geodesic_distances(D, [7, 9], directed=True)), bits(dijkstra(D, directed=True, indices=[7, 9])))
    for bad in (60, -1, np.array([0.5]), np.zeros(59, bool), np.zeros((2, 2), int)):
        with pytest.raises(ValueError):
            schpf_amd.geodesic_distances(A, bad)


def test_pseudotime_scales_and_keeps_inf(on_the_host):
    import schpf_amd
    graph = two_components()
    A = as_csr(graph)
    d = scipy_geodesic(graph, False, [[3, 7]])[0]
    t = schpf_amd.pseudotime(A, [3, 7])
    assert_array_equal(np.isinf(t), np.isinf(d))
    assert np.isinf(t[30:]).all() and np.isfinite(t[:30]).all()
    assert_array_equal(t[:30], d[:30] / d[:30].max())
    assert t[3] == 0 and t[7] == 0 and t[:30].max() == 1.0
    mask = np.zeros(60, bool)
    mask[[3, 7]] = True
    assert_array_equal(schpf_amd.pseudotime(A, mask), t)
    d3 = scipy_geodesic(graph, False, [[3]])[0][:30]
    assert_array_equal(schpf_amd.pseudotime(A, 3)[:30], d3 / d3.max())
    # every length 0: the largest finite distance is 0, reachable rows are 0 and the others stay inf
    zero = as_stored((graph[0], graph[1], np.zeros_like(graph[2])))
    t0 = schpf_amd.pseudotime(zero, 40)
    assert (t0[30:] == 0).all() and np.isinf(t0[:30]).all()


def test_farthest_landmarks_follow_their_definition(on_the_host):
    import schpf_amd
    graph = two_components()
    A = as_csr(graph)
    D = dijkstra(as_stored(graph), directed=False)
    for first, L in ((0, 6), (44, 9), (17, 1)):
        landmarks, dist = schpf_amd.farthest_landmarks(A, L, first=first)
        assert landmarks.dtype == np.int32 and dist.shape == (L, 60)
        assert_array_equal(landmarks, loop_farthest_landmarks(D, L, first))
        assert_array_equal(bits(dist), bits(D[landmarks]))
    landmarks, _ = schpf_amd.farthest_landmarks(A, 2, first=5)
    assert landmarks.tolist() == [5, 30]           # every row of the other component is at inf: the lowest index of them
    # ties to the lowest index: on the grid from a corner, the opposite corner; then the whole anti-diagonal ties at 29 and
    # its lowest index is the corner 29
    G = as_csr(grid())
    found = schpf_amd.farthest_landmarks(G, 5)[0]
    assert found[:3].tolist() == [0, 899, 29]
    assert_array_equal(found, loop_farthest_landmarks(dijkstra(G, directed=False), 5))
    for bad in (0, 61):
        with pytest.raises(ValueError):
            schpf_amd.farthest_landmarks(A, bad)


def test_landmark_isomap_follows_its_definition(on_the_host):
    import schpf_amd
    rng = np.random.RandomState(3)
    x = rng.rand(300, 3)
    x[:, 2] *= 0.1
    from scipy.spatial import cKDTree
    d, idx = cKDTree(x).query(x, 9)
    indptr = np.arange(0, 300 * 8 + 1, 8, dtype=np.int64)
    A = as_stored((indptr, idx[:, 1:].astype(np.int32).ravel(), d[:, 1:].ravel()))
    landmarks, dist = schpf_amd.farthest_landmarks(A, 12)
    assert np.isfinite(dist).all()
    for nc in (1, 2, 3):
        got = schpf_amd.landmark_isomap(dist, landmarks, n_components=nc)
        want = loop_landmark_isomap(dist, landmarks, nc)
        assert got.shape == (300, nc)
        np.testing.assert_allclose(got, want, rtol=1e-9)
        at = got[landmarks]
        assert (at[np.argmax(np.abs(at), axis=0), np.arange(nc)] > 0).all()
    # the landmarks land where classical MDS puts them: their pairwise distances in the full L - 1 dimensions are D
    full = schpf_amd.landmark_isomap(dist, landmarks, n_components=11)[landmarks]
    S = dist[:, landmarks]
    if (np.linalg.eigvalsh(-0.5 * (np.eye(12) - 1 / 12) @ (S * S) @ (np.eye(12) - 1 / 12)) > -1e-9).all():
        np.testing.assert_allclose(np.sqrt(((full[:, None] - full[None]) ** 2).sum(-1)), (S + S.T) / 2, atol=1e-6)


def test_grid_layout_keeps_every_vertex_apart(on_the_host):
    """Two dimensions cannot reproduce Manhattan distances; with every vertex a landmark the 900 points are still pairwise
    distinct and the axis signs follow the rule."""
    import schpf_amd
    G = as_csr(grid())
    dist = schpf_amd.geodesic_distances(G, np.arange(900))
    landmarks = np.arange(900, dtype=np.int32)
    y, x = np.divmod(np.arange(900), 30)
    assert_array_equal(dist, np.abs(x[:, None] - x[None]) + np.abs(y[:, None] - y[None]))
    X = schpf_amd.landmark_isomap(dist, landmarks)
    assert X.shape == (900, 2) and np.isfinite(X).all()
    assert len(np.unique(np.round(X, 9), axis=0)) == 900
    assert (X[np.argmax(np.abs(X), axis=0), np.arange(2)] > 0).all()


def test_landmark_isomap_refuses_a_graph_in_pieces(on_the_host):
    import schpf_amd
    landmarks, dist = schpf_amd.farthest_landmarks(as_csr(two_components()), 4)
    assert np.isinf(dist).any()
    with pytest.raises(ValueError, match="connected_components"):
        schpf_amd.landmark_isomap(dist, landmarks)
    with pytest.raises(ValueError):
        schpf_amd.landmark_isomap(dist[:, :30], landmarks[:3])


def test_cli_refuses_a_pseudotime_without_its_prerequisite(tmp_path):
    """Either option without its prerequisite is an error raised before anything is computed: the model is not even read."""
    from schpf_amd import cli
    base = ["score", "-m", str(tmp_path / "no_such_model.joblib"), "-o", str(tmp_path / "refused")]
    with pytest.raises(ValueError, match="--pseudotime-root belongs to --knn"):
        cli.main(base + ["--pseudotime-root", "0", "3"])
    with pytest.raises(ValueError, match="--pseudotime-root-cluster belongs to --clusters"):
        cli.main(base + ["--knn", "5", "--pseudotime-root-cluster", "1"])
    with pytest.raises(ValueError, match="give one"):
        cli.main(base + ["--knn", "5", "--knn-graph", "jaccard", "--clusters", "--pseudotime-root", "0", "--pseudotime-root-cluster", "1"])
    assert not os.path.exists(str(tmp_path / "refused" / "cell_score.txt"))
    args = cli._parser().parse_args(base + ["--knn", "5", "--pseudotime-root", "0", "3"])
    assert args.pseudotime_root == [0, 3] and args.pseudotime_root_cluster is None
