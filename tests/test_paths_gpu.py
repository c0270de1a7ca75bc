"""Shortest-path distances on the GPU: schpf_geodesic[_device] equal SciPy's Dijkstra and the library's serial
restatement bit for bit on every input of the host tests (the rounds and the lowering writes of the device, stats[1..2], are
outside the contract), on a side stream, twice over, on torch tensors; the refusals; and the estimator and the command line
end to end."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from conftest import ROOT, golden_coo, load_golden
from _louvain_reference import as_csr
from _paths_reference import bits, cases, debug_geodesic, expected, host_geodesic, pack_sets, plane_lengths, scipy_geodesic
from _topology_reference import I64P, two_components

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


def _device_call(graph, directed, set_ptr, roots, stream=None):
    """schpf_geodesic_device on torch tensors, outputs pre-filled with -7 -> (status, dist, stats) as NumPy."""
    from schpf_amd import _lib
    n, nsets = len(graph[0]) - 1, len(set_ptr) - 1
    d_indptr, d_indices, d_data = _dev(graph[0], np.int64), _dev(graph[1], np.int32), _dev(graph[2], np.float64)
    d_set_ptr, d_roots = _dev(set_ptr, np.int64), _dev(roots, np.int32)
    dist = torch.full((nsets, n), -7.0, dtype=torch.float64, device="cuda:0")
    stats = np.full(3, -7, np.int64)
    torch.cuda.synchronize()
    status = _lib.load().schpf_geodesic_device(0, ctypes.c_void_p(stream), n, _ptr(d_indptr), _ptr(d_indices), _ptr(d_data),
                                               int(directed), nsets, _ptr(d_set_ptr), _ptr(d_roots), _ptr(dist),
                                               stats.ctypes.data_as(I64P))
    return status, dist.cpu().numpy(), stats


def device_geodesic(graph, directed, sets, stream=None):
    from schpf_amd import _lib
    status, dist, stats = _device_call(graph, directed, *pack_sets(sets), stream=stream)
    _lib.check(status)
    return dist, stats


@pytest.mark.parametrize("case", sorted(CASES))
def test_distances_equal_scipy_and_the_restatement(amd, case):
    graph, directed, sets = CASES[case]
    want = expected(case)
    restated, restated_stats = debug_geodesic(graph, directed, sets)
    assert_array_equal(bits(restated), bits(want))
    n_roots = sum(len(set(s)) for s in sets)
    for call in (host_geodesic, device_geodesic):
        dist, stats = call(graph, directed, sets)
        print(case, call.__name__, "finite", stats[0], "rounds", stats[1], "lowering writes", stats[2])
        assert_array_equal(bits(dist), bits(want))
        assert stats[0] == restated_stats[0] == np.isfinite(want).sum()
        if stats[0] > n_roots:            # something is reachable beyond the roots
            assert stats[1] > 0 and stats[2] > 0
        else:
            assert stats[1] >= 0 and stats[2] == 0


def test_ordered_path_finishes(amd):
    """The path of 4 097 stored in order is the depth case: a distance walks one edge per round unless a later thread of
    the same round reads what an earlier one wrote.  No cap beyond n."""
    graph, directed, sets = CASES["path_4097_in_order"]
    dist, stats = device_geodesic(graph, directed, sets)
    print("ordered path of 4097: rounds", stats[1], "lowering writes", stats[2])
    assert_array_equal(bits(dist), bits(expected("path_4097_in_order")))
    assert 0 < stats[1] <= 4097 + 2 * 16       # n, and the rounds of the last batch that found nothing to do
    assert stats[2] >= 4096


def test_twice_the_same_bits(amd):
    graph, directed, sets = CASES["plane_special_undirected"]
    first, second = device_geodesic(graph, directed, sets), device_geodesic(graph, directed, sets)
    assert_array_equal(bits(first[0]), bits(second[0]))
    assert first[1][0] == second[1][0]
    assert_array_equal(bits(first[0]), bits(expected("plane_special_undirected")))


def test_side_stream(amd):
    graph, directed, sets = CASES["plane_3nn_undirected_a_tile_and_one"]
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        dist, stats = device_geodesic(graph, directed, sets, stream=side.cuda_stream)
    assert_array_equal(bits(dist), bits(expected("plane_3nn_undirected_a_tile_and_one")))
    assert graph[0].dtype == np.int64 and stats[0] == np.isfinite(dist).sum()


def test_refusals_on_the_device(amd):
    """The device validates as the restatement does: the same words for the same smallest offender, outputs untouched."""
    from schpf_amd import _lib
    lib = _lib.load()
    indptr, indices, data = two_components()
    indptr, indices, data = indptr.astype(np.int64), indices.astype(np.int32), data.astype(np.float64)
    n = len(indptr) - 1
    set_ptr, roots = pack_sets([[0], [45, 3], [50]])
    cols = indices.copy()
    cols[[indptr[17], indptr[40]]] = n
    vals = data.copy()
    vals[[indptr[21], indptr[50]]] = np.nan
    bad_ptr = indptr.copy()
    bad_ptr[10] = bad_ptr[9] - 1
    bad_sets = np.array([0, 3, 2, 4], np.int64)
    bad_roots = roots.copy()
    bad_roots[[1, 3]] = n, -1
    table = (((bad_ptr, cols, vals), bad_sets, bad_roots, "indptr must be 0 at row 0 and must be non-decreasing; offending row 9"),
             ((indptr, cols, vals), bad_sets, bad_roots, "columns must be in [0, n); offending row 17"),
             ((indptr, indices, vals), bad_sets, bad_roots, "values must be finite and >= 0; offending row 21"),
             ((indptr, indices, data), bad_sets, bad_roots, "geodesic: set_ptr must be 0 at set 0 and must be non-decreasing; offending set 1"),
             ((indptr, indices, data), set_ptr, bad_roots, "geodesic: roots must be in [0, n); offending set 1"))
    for graph, sp, rt, words in table:
        status, dist, stats = _device_call(graph, False, sp, rt)
        assert status != 0 and words in lib.schpf_last_error().decode()
        assert (dist == -7).all() and (stats == -7).all()
        h_dist = np.full((len(sp) - 1, n), -7.0)
        h_stats = np.full(3, -7, np.int64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        status = lib.schpf_geodesic(0, n, p(graph[0]), p(graph[1]), p(graph[2]), 0, len(sp) - 1, p(sp), p(rt), p(h_dist),
                                    h_stats.ctypes.data_as(I64P))
        assert status != 0 and words in lib.schpf_last_error().decode()
        assert (h_dist == -7).all() and (h_stats == -7).all()
        with pytest.raises(ValueError, match=re.escape(words)):
            _lib.check(status)


def test_tensors_in_tensors_out(amd):
    graph = plane_lengths()
    A = as_csr(graph)
    T = torch.sparse_csr_tensor(torch.tensor(graph[0]), torch.tensor(graph[1].astype(np.int64)), torch.tensor(np.array(graph[2])),
                                size=A.shape, device="cuda:0")
    sets = [[11], [], [19999, 5, 5]]
    want = scipy_geodesic(graph, False, sets)
    host, stats = amd.geodesic_distances(A, sets, return_stats=True)
    assert isinstance(host, np.ndarray) and stats["finite"] == np.isfinite(want).sum() and stats["rounds"] > 0
    assert_array_equal(bits(host), bits(want))
    dev = amd.geodesic_distances(T, sets)
    assert dev.is_cuda and dev.device == T.device and dev.dtype == torch.float64 and tuple(dev.shape) == (3, 20000)
    assert_array_equal(bits(dev.cpu().numpy()), bits(host))
    assert_array_equal(bits(amd.geodesic_distances(T, [11, 19999], directed=True).cpu().numpy()),
                       bits(scipy_geodesic(graph, True, [[11], [19999]])))
    t_host, t_dev = amd.pseudotime(A, [11, 19999]), amd.pseudotime(T, [11, 19999])
    assert t_dev.is_cuda
    assert_array_equal(bits(t_dev.cpu().numpy()), bits(t_host))
    reach = np.isfinite(t_host)
    assert t_host[reach].max() == 1.0 and t_host[11] == 0 and not reach.all()
    small = as_csr(two_components())
    S = torch.sparse_csr_tensor(torch.tensor(small.indptr.astype(np.int64)), torch.tensor(small.indices.astype(np.int64)),
                                torch.tensor(small.data), size=small.shape, device="cuda:0")
    marks_host, dist_host = amd.farthest_landmarks(small, 5, first=7)
    marks_dev, dist_dev = amd.farthest_landmarks(S, 5, first=7)
    assert marks_dev.is_cuda and marks_dev.dtype == torch.int32 and marks_host[1] == 30
    assert_array_equal(marks_dev.cpu().numpy(), marks_host)
    assert_array_equal(bits(dist_dev.cpu().numpy()), bits(dist_host))


def _graph_is_connected(model, k):
    from scipy.sparse.csgraph import connected_components
    indices, distances = model.neighbors(k=k)
    n = indices.shape[0]
    rows = np.repeat(np.arange(n), k)
    from scipy.sparse import csr_matrix
    return connected_components(csr_matrix((np.ones(n * k), (rows, indices.ravel())), shape=(n, n)), directed=False)[0] == 1


def test_fitted_model_end_to_end(amd, tmp_path):
    """scHPF.pseudotime is finite exactly on the root's component; scHPF.layout is finite where the graph is in one piece and
    refuses it where it is not; `scHPF score --knn K --pseudotime-root 0` writes one line per cell."""
    X = golden_coo(load_golden("pbmc_like_data.npz"))
    np.random.seed(0)
    model = amd.scHPF(5, max_iter=12, verbose=False).fit(X)
    N = X.shape[0]
    # the smallest k of each kind: one neighbour leaves the graph in pieces, all the others (or the 128 the search allows)
    # make it whole
    candidates = (1, 2, 3, 5, 10, 20, 40, min(N - 1, 128))
    connected = {k: _graph_is_connected(model, k) for k in candidates}
    k_pieces = next(k for k in candidates if not connected[k])
    k_whole = next(k for k in candidates if connected[k])
    ran = set()
    for k in (k_pieces, k_whole):
        comp = model.components(k=k)
        t = model.pseudotime(0, k=k)
        assert t.shape == (N,) and t.dtype == np.float64
        assert_array_equal(np.isfinite(t), comp == comp[0])
        assert t[0] == 0 and t[np.isfinite(t)].max() == 1.0
        if comp.max() > 0:
            ran.add("pieces")
            assert np.isinf(t).any()
            with pytest.raises(ValueError, match="connected_components"):
                model.layout(k=k, n_landmarks=16)
        else:
            ran.add("whole")
            Y = model.layout(k=k, n_landmarks=16)
            assert Y.shape == (N, 2) and np.isfinite(Y).all() and Y.std(axis=0).min() > 0
        mask = np.zeros(N, bool)
        mask[[0, 3]] = True
        assert_array_equal(bits(model.pseudotime(mask, k=k)), bits(model.pseudotime([0, 3], k=k)))
    assert ran == {"pieces", "whole"}

    model_path = str(tmp_path / "model.joblib")
    amd.save_model(model, model_path)
    exe = [sys.executable, os.path.join(ROOT, "bin", "scHPF"), "score", "-m", model_path, "--knn", str(k_whole)]
    subprocess.check_call(exe + ["-o", str(tmp_path / "plain")], stdout=subprocess.DEVNULL)
    subprocess.check_call(exe + ["-o", str(tmp_path / "out"), "--pseudotime-root", "0"], stdout=subprocess.DEVNULL)
    assert set(os.listdir(str(tmp_path / "out"))) - set(os.listdir(str(tmp_path / "plain"))) == {"pseudotime.txt"}
    written = np.loadtxt(str(tmp_path / "out" / "pseudotime.txt"))
    assert written.shape == (N,)
    assert_array_equal(bits(written), bits(model.pseudotime(0, k=k_whole)))
    import json
    plain_args = json.load(open(str(tmp_path / "plain" / "score_commandline_args.json")))
    assert "pseudotime_root" not in plain_args and "pseudotime_root_cluster" not in plain_args
