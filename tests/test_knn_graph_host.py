"""Weighted neighbour graphs, without a GPU: the library's serial restatement schpf_debug_knn_graph -- which
the kernels are then held to bit for bit (tests/test_knn_graph_gpu.py) -- is pinned to the definition written out in
NumPy (tests/_graph_reference.py), and the Python layer and the command line are checked with the restatement in the
kernels' place.

Bounds.  Structure (indptr, indices) and the Jaccard values (a ratio of two small integers, correctly rounded on both
sides) are exact.  rho and sigma are exact: the bisection halves and doubles exactly, so both sides walk the same path as
long as every comparison of psum agrees; the seeds below are ones where it does (a psum within a few ulp of the target or
of its tolerance would need another seed).  The umap values are within rtol 1e-14: t = e / sigma is the same bits on both
sides, the library's exponential is within 2 ulp and np.exp within 1, the union adds two roundings -- about 5 ulp = 1.1e-15
-- and the rest is margin."""
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from _graph_reference import (JACCARD, UMAP, _p, bits, chain_lists, debug_graph, duplicated_cells, far_neighbour, hub_lists,
                              numpy_calibration, numpy_graph, random_lists, ring_lists, scipy_graph, score_lists, unsorted)

BOTH = [UMAP, JACCARD]


CASES = {
    "smallest": lambda: (np.array([[1], [0]], np.int32), np.array([[0.5], [0.5]])),
    "scores_65_3": lambda: score_lists(65, 3, seed=1),
    "scores_130_15": lambda: score_lists(130, 15, seed=2),
    "scores_300_128": lambda: score_lists(300, 128, seed=3),
    "random_200_15": lambda: random_lists(200, 15, seed=4),
    "ring_40_6": lambda: ring_lists(40, 6),
    "chain_41_5": lambda: chain_lists(41, 5),
    "hub_60": lambda: hub_lists(60),
    "duplicated": lambda: duplicated_cells(*score_lists(70, 6, seed=5)),
    "far": lambda: far_neighbour(*score_lists(70, 6, seed=6)),
    "unsorted": lambda: unsorted(*score_lists(70, 9, seed=7)),
}


@pytest.mark.parametrize("method", BOTH)
@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_equals_the_definition(case, method):
    idx, dist = CASES[case]()
    n, k = idx.shape
    indptr, indices, data, rho, sigma = debug_graph(idx, dist, method)
    w_indptr, w_indices, w_data, w_rho, w_sigma, _ = numpy_graph(idx, dist, "umap" if method == UMAP else "jaccard")
    assert_array_equal(indptr, w_indptr)
    assert_array_equal(indices, w_indices)
    if method == JACCARD:
        assert_array_equal(bits(data), bits(w_data))
    else:
        assert_array_equal(bits(rho), bits(w_rho))
        assert_array_equal(bits(sigma), bits(w_sigma))
        assert_allclose(data, w_data, rtol=1e-14, atol=0)
    if case == "ring_40_6":
        assert indptr[n] == n * k
    if case == "chain_41_5":
        assert indptr[n] == 2 * n * k
    if case == "hub_60":
        assert indptr[1] - indptr[0] == n - 1 and indptr[2] - indptr[1] == n - 1
    if case == "far" and method == UMAP:
        assert (data == 0.0).sum() >= 2            # stored, not dropped: the structure depends on idx alone
    if case == "duplicated" and method == UMAP:
        assert rho[3] == 0.0 and rho[10] == 0.0 and rho[5] > 0.0


def as_csr(n, graph):
    from scipy.sparse import csr_matrix
    return csr_matrix((graph[2], graph[1], graph[0]), shape=(n, n))


@pytest.mark.parametrize("method", BOTH)
def test_properties_that_need_no_yardstick(method):
    """(3000, 15) lists with zero rows, far neighbours and unsorted columns.  The matrix equals its transpose bit for bit,
    values lie in [0, 1], no diagonal, columns strictly ascending.  umap: the nearest positive-distance neighbour j of row
    i has directed weight 1, so the union c_ij = fma(-1, b, 1 + b) is 1 up to the rounding of 1 + b: at least 1 - 2^-53,
    at most 1; and where the bisection stopped by its tolerance the row's weights sum to the target within it (np.exp
    against the library's exponential: k * 3 ulp, far below the 1e-9 allowed on top)."""
    idx, dist = unsorted(*far_neighbour(*duplicated_cells(*random_lists(3000, 15, seed=11))))
    n, k = idx.shape
    graph = debug_graph(idx, dist, method)
    indptr, indices, data, rho, sigma = graph
    G = as_csr(n, graph)
    T = G.T.tocsr()
    T.sort_indices()
    assert_array_equal(T.indptr, indptr)
    assert_array_equal(T.indices, indices)
    assert_array_equal(bits(T.data), bits(data))
    assert data.min() >= 0.0 and data.max() <= 1.0
    rows = np.repeat(np.arange(n), np.diff(indptr))
    assert not np.any(rows == indices)
    assert np.all((np.diff(indices.astype(np.int64)) > 0) | (np.diff(rows) > 0))
    assert np.all(np.diff(indptr) >= k) and indptr[0] == 0
    assert_allclose(G.toarray(), scipy_graph(idx, dist, "umap" if method == UMAP else "jaccard").toarray(), rtol=1e-13, atol=0)
    if method == JACCARD:
        return
    positive = np.where(dist > 0, dist, np.inf)
    has = np.isfinite(positive.min(axis=1))
    nearest = idx[np.arange(n), positive.argmin(axis=1)]
    c = np.asarray(G[np.arange(n)[has], nearest[has]]).ravel()
    assert np.all(c >= 1.0 - 2.0 ** -53) and np.all(c <= 1.0)
    w_rho, w_sigma, w, stopped = numpy_calibration(dist)
    assert_array_equal(bits(rho), bits(w_rho))
    assert_array_equal(bits(sigma), bits(w_sigma))
    assert stopped.sum() > n // 2
    assert np.all(np.abs(w.sum(axis=1) - np.log2(k + 1.0))[stopped] < 1e-5 + 1e-9)


def test_refusals_leave_the_outputs_untouched():
    from schpf_amd import _lib
    lib = _lib.load()
    idx, dist = score_lists(30, 4, seed=1)

    def refused(idx, dist, method, message):
        n, k = idx.shape
        out = [np.full(n + 1, -7, np.int64), np.full(2 * n * k, -7, np.int32), np.full(2 * n * k, -7.0), np.full(n, -7.0),
               np.full(n, -7.0)]
        idx = np.ascontiguousarray(idx, np.int32)
        assert lib.schpf_debug_knn_graph(method, n, k, _p(idx), _p(dist), *[_p(a) for a in out]) != 0
        assert lib.schpf_last_error().decode() == message
        assert all(np.all(a == -7) for a in out)
        with pytest.raises(ValueError):
            debug_graph(idx, dist, method)

    lists = "neighbour lists must hold k distinct rows other than the row itself; offending row %d"
    for method in BOTH:
        bad = idx.copy()
        bad[20, 1] = 30
        bad[9, 3] = -1
        refused(bad, dist, method, lists % 9)
        bad = idx.copy()
        bad[12, 2] = 12
        bad[25, 0] = bad[25, 3]
        refused(bad, dist, method, lists % 12)
        bad = idx.copy()
        bad[4, 0] = bad[4, 3]
        refused(bad, dist, method, lists % 4)
    for value in (-1e-300, np.inf, np.nan):
        bad = dist.copy()
        bad[17, 2] = value
        bad[28, 0] = np.nan
        refused(idx, bad, UMAP, "distances must be finite and >= 0; offending row 17")
        debug_graph(idx, bad, JACCARD)             # the distances are not read
    bad_idx, bad_dist = idx.copy(), dist.copy()    # lists are looked at before distances
    bad_idx[22, 0] = bad_idx[22, 1]
    bad_dist[2, 0] = -1.0
    refused(bad_idx, bad_dist, UMAP, lists % 22)
    debug_graph(idx, None, JACCARD)                # dist may be NULL
    with pytest.raises(ValueError, match=r"k must be in \[1, 128\]"):
        debug_graph(np.zeros((300, 129), np.int32), None, JACCARD)
    with pytest.raises(ValueError, match="k must be at most n - 1"):
        debug_graph(np.zeros((4, 4), np.int32), None, JACCARD)
    with pytest.raises(_lib.SchpfHipError, match="dist must not be NULL"):
        debug_graph(idx, None, UMAP)
    with pytest.raises(ValueError, match="method must be"):
        debug_graph(idx, dist, 2)
    out = debug_graph(np.empty((0, 3), np.int32), np.empty((0, 3)), UMAP)     # n = 0 succeeds and writes nothing
    assert out[0][0] == -7 and len(out[1]) == 0


# ------------------------------------------------------------------------------------------- the Python layer and the CLI
@pytest.fixture
def neighbors(monkeypatch):
    """schpf_amd.neighbors with the host restatements in the place of schpf_knn and schpf_knn_graph."""
    from schpf_amd import neighbors as nb
    from _knn_reference import debug_knn

    def graph(method, idx, dist, device):
        assert idx.flags.c_contiguous and idx.dtype == np.int32
        assert dist is None or (dist.flags.c_contiguous and dist.dtype == np.float64)
        return debug_graph(idx, dist, method)[:3]

    monkeypatch.setattr(nb, "_graph_host", graph)
    monkeypatch.setattr(nb, "_search_host", lambda query, ref, k, self_first, device: debug_knn(query, ref, k, self_first))
    return nb


def test_knn_connectivities(neighbors):
    import schpf_amd
    assert schpf_amd.knn_connectivities is neighbors.knn_connectivities and "knn_connectivities" in schpf_amd.__all__
    idx, dist = far_neighbour(*score_lists(70, 6, seed=6))
    n = 70
    G = neighbors.knn_connectivities(idx, dist)
    want = debug_graph(idx, dist, UMAP)
    assert G.format == "csr" and G.shape == (n, n) and G.indptr.dtype == np.int32 and G.dtype == np.float64
    assert (want[2] == 0).sum() >= 2 and G.nnz == len(want[2]) - (want[2] == 0).sum() and np.all(G.data > 0)
    assert_array_equal(G.toarray(), as_csr(n, want).toarray())
    assert (abs(G - G.T)).nnz == 0
    J = neighbors.knn_connectivities(idx.astype(np.int64), method="jaccard")
    want = debug_graph(idx, None, JACCARD)
    assert_array_equal(J.indptr, want[0])
    assert_array_equal(J.indices, want[1])
    assert_array_equal(J.data, want[2])
    assert_array_equal(neighbors.knn_connectivities(idx, dist.astype(np.float32) * 0 + 1, method="jaccard").data, want[2])
    with pytest.raises(ValueError, match="needs the distances"):
        neighbors.knn_connectivities(idx)
    with pytest.raises(ValueError, match="method must be one of umap, jaccard"):
        neighbors.knn_connectivities(idx, dist, method="snn")
    with pytest.raises(ValueError, match="one shape"):
        neighbors.knn_connectivities(idx, dist[:, :2])
    bad = idx.copy()
    bad[5, 0] = 5
    with pytest.raises(ValueError, match="offending row 5$"):
        neighbors.knn_connectivities(bad, dist)
    with pytest.raises(ValueError, match="distances must be finite and >= 0; offending row 0$"):
        neighbors.knn_connectivities(idx, -dist)


def toy_model(n_cells=25, n_genes=60, K=3):
    import schpf_amd
    rng = np.random.RandomState(0)
    gam = lambda shape: schpf_amd.HPF_Gamma(rng.gamma(1.0, 1.0, shape), rng.gamma(1.0, 1.0, shape) + 0.5)  # noqa: E731
    model = schpf_amd.scHPF(K)
    model.xi, model.theta = gam((n_cells,)), gam((n_cells, K))
    model.eta, model.beta = gam((n_genes,)), gam((n_genes, K))
    return model


def test_model_neighbor_graph(neighbors):
    from _knn_reference import debug_knn
    model = toy_model()
    distances, connectivities = model.neighbor_graph(k=4)
    x = model.cell_score()
    idx, d2 = debug_knn(x, x, 4, 0)
    assert distances.shape == connectivities.shape == (25, 25) and distances.format == connectivities.format == "csr"
    assert_array_equal(distances.toarray(), neighbors.knn_graph(idx, np.sqrt(d2), 25).toarray())
    assert_array_equal(connectivities.toarray(), as_csr(25, debug_graph(idx, np.sqrt(d2), UMAP)).toarray())
    _, jac = model.neighbor_graph(k=4, metric="cosine", method="jaccard")
    c_idx, _ = model.neighbors(k=4, metric="cosine")
    assert_array_equal(jac.toarray(), as_csr(25, debug_graph(c_idx, None, JACCARD)).toarray())


def test_score_knn_graph_on_the_command_line(neighbors, tmp_path):
    import json

    import schpf_amd
    from scipy.io import mmread
    from schpf_amd import cli
    model = toy_model()
    path = str(tmp_path / "model.joblib")
    schpf_amd.save_model(model, path)
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "knn"), "--knn", "5"]) == 0
    for method in ("umap", "jaccard"):
        out = tmp_path / method
        assert cli.main(["score", "-m", path, "-o", str(out), "--knn", "5", "--knn-graph", method]) == 0
        assert set(os.listdir(str(out))) - set(os.listdir(str(tmp_path / "knn"))) == {"knn_connectivities.mtx"}
        want = model.neighbor_graph(k=5, method=method)[1]
        got = mmread(str(out / "knn_connectivities.mtx")).tocsr()
        assert_allclose(got.toarray(), want.toarray(), rtol=1e-15, atol=0)
        assert json.load(open(str(out / "score_commandline_args.json")))["knn_graph"] == method
    # without the option the arguments file is what it was
    assert "knn_graph" not in json.load(open(str(tmp_path / "knn" / "score_commandline_args.json")))
    with pytest.raises((ValueError, SystemExit)):
        cli.main(["score", "-m", path, "-o", str(tmp_path / "bad"), "--knn-graph", "umap"])
