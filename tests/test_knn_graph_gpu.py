"""Weighted neighbour graphs on the GPU.  schpf_knn_graph and schpf_knn_graph_device against the library's
host restatement schpf_debug_knn_graph (tests/test_knn_graph_host.py pins it to the definition): equal indptr and indices
and equal bits of data, rho and sigma, for both methods, whatever the shape of the lists.  Then the Python surface:
knn_connectivities on GPU tensors, scHPF.neighbor_graph and `scHPF score --knn K --knn-graph`."""
import ctypes
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from conftest import golden_coo, load_golden
from _graph_reference import (JACCARD, UMAP, _p, bits, chain_lists, debug_graph, duplicated_cells, far_neighbour, host_graph,
                              hub_lists, random_lists, ring_lists, score_lists, unsorted)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
BOTH = [UMAP, JACCARD]


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def device_graph(idx, dist, method, stream=None):
    """schpf_knn_graph_device on torch tensors -> NumPy (indptr, indices, data, rho, sigma), cut to nnz."""
    from schpf_amd import _lib
    n, k = idx.shape
    d_idx = torch.tensor(np.ascontiguousarray(idx, np.int32), device="cuda:0")
    d_dist = torch.tensor(np.ascontiguousarray(dist, np.float64), device="cuda:0") if method == UMAP else None
    d_indptr = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0")
    d_indices = torch.full((2 * n * k,), -7, dtype=torch.int32, device="cuda:0")
    d_data = torch.full((2 * n * k,), -7.0, dtype=torch.float64, device="cuda:0")
    d_rho = torch.full((n,), -7.0, dtype=torch.float64, device="cuda:0")
    d_sigma = torch.full((n,), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)  # noqa: E731
    _lib.check(_lib.load().schpf_knn_graph_device(0, ctypes.c_void_p(stream), method, n, k, ptr(d_idx), ptr(d_dist),
                                                  ptr(d_indptr), ptr(d_indices), ptr(d_data), ptr(d_rho), ptr(d_sigma)))
    indptr = d_indptr.cpu().numpy()
    nnz = int(indptr[n])
    assert bool((d_indices[nnz:] == -7).all()) and bool((d_data[nnz:] == -7.0).all())   # nothing beyond nnz is touched
    umap = method == UMAP
    return (indptr, d_indices[:nnz].cpu().numpy(), d_data[:nnz].cpu().numpy(), d_rho.cpu().numpy() if umap else None,
            d_sigma.cpu().numpy() if umap else None)


def assert_same(got, want):
    assert_array_equal(got[0], want[0])
    assert_array_equal(got[1], want[1])
    assert_array_equal(bits(got[2]), bits(want[2]))
    if want[3] is not None:
        assert_array_equal(bits(got[3]), bits(want[3]))
        assert_array_equal(bits(got[4]), bits(want[4]))


def check_both(idx, dist, method, want=None):
    want = debug_graph(idx, dist, method) if want is None else want
    assert_same(host_graph(idx, dist, method), want)
    assert_same(device_graph(idx, dist, method), want)
    return want


@functools.lru_cache(maxsize=None)
def large_case():
    """(70001, 15) with duplicated cells, far neighbours and unsorted columns, and the restatement's answers; computed once."""
    idx, dist = unsorted(*far_neighbour(*duplicated_cells(*random_lists(70001, 15, seed=70001))))
    want = {m: debug_graph(idx, dist, m) for m in BOTH}
    for a in (idx, dist):
        a.setflags(write=False)
    return idx, dist, want


SMALL = {
    "smallest": lambda: (np.array([[1], [0]], np.int32), np.array([[0.5], [0.5]])),
    "scores_65_3": lambda: score_lists(65, 3, seed=1),
    "scores_130_15": lambda: score_lists(130, 15, seed=2),
    "scores_300_128": lambda: score_lists(300, 128, seed=3),
    "duplicated": lambda: duplicated_cells(*score_lists(70, 6, seed=5)),
    "far": lambda: far_neighbour(*score_lists(70, 6, seed=6)),
    "unsorted": lambda: unsorted(*score_lists(70, 9, seed=7)),
}


@pytest.mark.parametrize("method", BOTH)
@pytest.mark.parametrize("case", sorted(SMALL))
def test_small_lists(amd, case, method):
    """The smallest graph; ordinary lists across wave and workgroup edges; the largest k; rho = 0; an explicit 0 weight;
    columns in any order."""
    idx, dist = SMALL[case]()
    want = check_both(idx, dist, method)
    if case == "far" and method == UMAP:
        assert (want[2] == 0.0).sum() >= 2
    if case == "duplicated" and method == UMAP:
        assert want[3][3] == 0.0 and want[3][10] == 0.0


@pytest.mark.parametrize("method", BOTH)
def test_scans_and_sorts_across_many_blocks(amd, method):
    idx, dist, want = large_case()
    check_both(idx, dist, method, want=want[method])


@pytest.mark.parametrize("method", BOTH)
def test_every_edge_mutual_and_none(amd, method):
    """Ring lattice: nnz = n k.  Directed chain: nnz = 2 n k, the capacity reached exactly."""
    idx, dist = ring_lists(1000, 14)
    assert check_both(idx, dist, method)[0][-1] == 1000 * 14
    idx, dist = chain_lists(1001, 15)
    assert check_both(idx, dist, method)[0][-1] == 2 * 1001 * 15


@pytest.mark.parametrize("method", BOTH)
def test_hub_of_in_degree_n_minus_1(amd, method):
    idx, dist = hub_lists(5000)
    indptr = check_both(idx, dist, method)[0]
    assert indptr[1] == 4999 and indptr[2] - indptr[1] == 4999


def test_knn_connectivities_on_gpu_tensors(amd):
    """GPU tensors in, a sparse CSR tensor on the same GPU out, equal to the host path's; on a side stream as well."""
    idx, dist, want = large_case()
    n = idx.shape[0]
    t_idx, t_dist = torch.tensor(idx, device="cuda:0"), torch.tensor(dist, device="cuda:0")
    keep_i, keep_d = t_idx.clone(), t_dist.clone()
    for method, code in (("umap", UMAP), ("jaccard", JACCARD)):
        G = amd.knn_connectivities(t_idx, t_dist, method=method)
        assert G.layout == torch.sparse_csr and G.device == t_idx.device and tuple(G.shape) == (n, n)
        assert G.values().dtype == torch.float64 and G.col_indices().dtype == torch.int32
        assert_array_equal(G.crow_indices().cpu().numpy(), want[code][0])
        assert_array_equal(G.col_indices().cpu().numpy(), want[code][1])
        assert_array_equal(bits(G.values().cpu().numpy()), bits(want[code][2]))
        side = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(side):
            S = amd.knn_connectivities(t_idx + 0, t_dist * 1.0, method=method)   # enqueued on the same stream
        side.synchronize()
        assert torch.equal(S.values(), G.values()) and torch.equal(S.col_indices(), G.col_indices())
        H = amd.knn_connectivities(idx, dist, method=method)                     # NumPy in, SciPy out
        assert H.format == "csr" and H.indptr.dtype == np.int32
        if method == "umap":
            assert H.nnz == int((want[code][2] != 0).sum()) < len(want[code][2])
        else:
            assert_array_equal(H.data, want[code][2])
    assert torch.equal(t_idx, keep_i) and torch.equal(t_dist, keep_d)
    with pytest.raises(ValueError, match="device=1 was asked for"):
        amd.knn_connectivities(t_idx, t_dist, device=1)


def test_refused_calls_leave_their_outputs(amd):
    from schpf_amd import _lib
    lib = _lib.load()
    idx, dist = score_lists(130, 5, seed=1)
    lists = "neighbour lists must hold k distinct rows other than the row itself; offending row %d$"
    for call in (host_graph, device_graph):
        for method in BOTH:
            bad = idx.copy()
            bad[100, 1] = 130
            bad[70, 3] = -1
            with pytest.raises(ValueError, match=lists % 70):
                call(bad, dist, method)
            bad = idx.copy()
            bad[64, 2] = 64
            bad[129, 0] = bad[129, 3]
            with pytest.raises(ValueError, match=lists % 64):
                call(bad, dist, method)
            bad = idx.copy()
            bad[129, 0] = bad[129, 4]
            with pytest.raises(ValueError, match=lists % 129):
                call(bad, dist, method)
        for value in (-1e-300, np.inf, np.nan):
            bad = dist.copy()
            bad[66, 2] = value
            bad[128, 0] = np.nan
            with pytest.raises(ValueError, match="distances must be finite and >= 0; offending row 66$"):
                call(idx, bad, UMAP)
        bad_idx, bad_dist = idx.copy(), dist.copy()
        bad_idx[90, 0] = bad_idx[90, 1]
        bad_dist[2, 0] = -1.0
        with pytest.raises(ValueError, match=lists % 90):
            call(bad_idx, bad_dist, UMAP)
    # the outputs of a refused call keep what they held
    bad = dist.copy()
    bad[5, 0] = np.nan
    n, k = idx.shape
    out = [np.full(n + 1, -7, np.int64), np.full(2 * n * k, -7, np.int32), np.full(2 * n * k, -7.0), np.full(n, -7.0),
           np.full(n, -7.0)]
    assert lib.schpf_knn_graph(0, UMAP, n, k, _p(idx), _p(bad), *[_p(a) for a in out]) != 0
    assert all(np.all(a == -7) for a in out)
    t_out = [torch.tensor(a, device="cuda:0") for a in out]
    t_idx, t_bad = torch.tensor(idx, device="cuda:0"), torch.tensor(bad, device="cuda:0")
    torch.cuda.synchronize()
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.schpf_knn_graph_device(0, None, UMAP, n, k, dp(t_idx), dp(t_bad), *[dp(t) for t in t_out]) != 0
    assert b"offending row 5" in lib.schpf_last_error()
    assert all(bool((t == -7).all()) for t in t_out)
    # n = 0 succeeds and writes nothing; a device that does not exist does not; NULL rho and sigma are fine
    assert lib.schpf_knn_graph(0, UMAP, 0, 3, None, None, None, None, None, None, None) == 0
    assert lib.schpf_knn_graph_device(0, None, JACCARD, 0, 3, None, None, None, None, None, None, None) == 0
    assert lib.schpf_knn_graph(99, UMAP, n, k, _p(idx), _p(dist), *[_p(a) for a in out]) != 0
    assert b"no such HIP device" in lib.schpf_last_error()
    assert lib.schpf_knn_graph(0, UMAP, n, k, _p(idx), _p(dist), _p(out[0]), _p(out[1]), _p(out[2]), None, None) == 0
    want = debug_graph(idx, dist, UMAP)
    assert_array_equal(out[0], want[0])
    assert_array_equal(bits(out[2][: len(want[2])]), bits(want[2]))
    assert lib.schpf_knn_graph(0, UMAP, n, n, _p(idx), _p(dist), *[_p(a) for a in out]) != 0
    assert b"k must be" in lib.schpf_last_error()


def test_fitted_model_end_to_end(amd, tmp_path):
    """Fit the small golden matrix: neighbor_graph is knn + knn_graph + knn_connectivities, and
    `scHPF score --knn 5 --knn-graph umap` writes the same matrix."""
    from scipy.io import mmread
    from schpf_amd import cli
    X = golden_coo(load_golden("pbmc_like_data.npz"))
    np.random.seed(0)
    model = amd.scHPF(5, max_iter=12, verbose=False).fit(X)
    N = X.shape[0]
    distances, connectivities = model.neighbor_graph(k=5)
    idx, dist = model.neighbors(k=5)
    assert distances.shape == connectivities.shape == (N, N)
    assert_array_equal(distances.toarray(), amd.knn_graph(idx, dist, N).toarray())
    want = debug_graph(idx, dist, UMAP)
    keep = want[2] != 0
    assert_array_equal(connectivities.indices, want[1][keep])
    assert_array_equal(bits(connectivities.data), bits(want[2][keep]))
    assert abs(connectivities - connectivities.T).nnz == 0
    jac = model.neighbor_graph(k=5, method="jaccard")[1]
    assert_array_equal(bits(jac.data), bits(debug_graph(idx, None, JACCARD)[2]))
    path = str(tmp_path / "model.joblib")
    amd.save_model(model, path)
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "knn"), "--knn", "5"]) == 0
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "graph"), "--knn", "5", "--knn-graph", "umap"]) == 0
    assert set(os.listdir(str(tmp_path / "graph"))) - set(os.listdir(str(tmp_path / "knn"))) == {"knn_connectivities.mtx"}
    got = mmread(str(tmp_path / "graph" / "knn_connectivities.mtx")).tocsr()
    np.testing.assert_allclose(got.toarray(), connectivities.toarray(), rtol=1e-15, atol=0)
