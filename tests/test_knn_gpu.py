"""Nearest neighbours in factor space on the GPU.  schpf_knn and schpf_knn_device against the library's host
restatement schpf_debug_knn (tests/test_knn_host.py pins it to the definition): equal indices and equal bits of d2,
whatever the shapes, the ties, the order the candidates arrive in and the way the reference axis was cut.  Then the
Python surface: knn on GPU tensors, scHPF.neighbors and `scHPF score --knn`."""
import ctypes
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from conftest import golden_coo, load_golden
from _knn_reference import DTYPES, _p, bits, debug_knn, gamma_scores, host_knn, integer_scores

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
BOTH = [np.float32, np.float64]


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def device_knn(query, ref, k, self_first=-1, stream=None):
    """schpf_knn_device on torch tensors (query is ref: one tensor); results as NumPy arrays, and the tensors."""
    from schpf_amd import _lib
    d_query = torch.tensor(query, device="cuda:0")
    d_ref = d_query if ref is query else torch.tensor(ref, device="cuda:0")
    d_idx = torch.full((query.shape[0], k), -7, dtype=torch.int32, device="cuda:0")
    d_d2 = torch.full((query.shape[0], k), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
    _lib.check(_lib.load().schpf_knn_device(0, ctypes.c_void_p(stream), DTYPES[query.dtype], query.shape[0], ref.shape[0],
                                            query.shape[1], ptr(d_query), ptr(d_ref), k, ctypes.c_int64(self_first),
                                            ptr(d_idx), ptr(d_d2)))
    return d_idx.cpu().numpy(), d_d2.cpu().numpy()


def assert_same(got, want):
    assert_array_equal(got[0], want[0])
    assert_array_equal(bits(got[1]), bits(want[1]))


def check_both(query, ref, k, self_first=-1, want=None):
    want = debug_knn(query, ref, k, self_first) if want is None else want
    assert_same(host_knn(query, ref, k, self_first), want)
    assert_same(device_knn(query, ref, k, self_first), want)
    return want


@functools.lru_cache(maxsize=None)
def random_case(n_query, n_ref, K, k, dtype):
    """Inputs and the host restatement's answer, computed once and shared (read-only) by the tests of a shape."""
    query, ref = gamma_scores(n_query, K, dtype, seed=n_query), gamma_scores(n_ref, K, dtype, seed=7 + n_ref)
    want = debug_knn(query, ref, k)
    for a in (query, ref) + want:
        a.setflags(write=False)
    return query, ref, want


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("n_query,n_ref", [(1, 1), (1, 300), (63, 65), (130, 70)])
def test_small_shapes(amd, n_query, n_ref, dtype):
    """A single pair; one row against five tiles; strips and tiles that stick out by one either way.  K = 50 needs more
    than one staging pass, k = 128 stages 16 factors at a time: K = 20 then takes two passes as well."""
    for K in (1, 5, 20, 50):
        query, ref = gamma_scores(n_query, K, dtype, seed=K), gamma_scores(n_ref, K, dtype, seed=100 + K)
        for k in (1, 15, 128):
            check_both(query, ref, min(k, n_ref))


@pytest.mark.parametrize("split", ["1", "5"])
@pytest.mark.parametrize("dtype", BOTH)
def test_many_tiles(amd, dtype, split, monkeypatch):
    """(257, 5000): 79 tiles, the threshold reject is the common path.  As one segment and as five."""
    monkeypatch.setenv("SCHPF_KNN_SPLIT", split)
    for k in (1, 15, 128):
        query, ref, want = random_case(257, 5000, 20, k, dtype)
        check_both(query, ref, k, want=want)


@pytest.mark.parametrize("split", ["1", "7", ""])
@pytest.mark.parametrize("dtype", BOTH)
def test_long_reference_axis(amd, dtype, split, monkeypatch):
    """(300, 70001), K = 20, k = 30: one segment, seven, and what the rule itself picks."""
    monkeypatch.setenv("SCHPF_KNN_SPLIT", split)
    query, ref, want = random_case(300, 70001, 20, 30, dtype)
    check_both(query, ref, 30, want=want)


@pytest.mark.parametrize("split", ["1", "5"])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("n_query,n_ref,K", [(65, 257, 20), (257, 5000, 5)])
def test_ties(amd, n_query, n_ref, K, dtype, split, monkeypatch):
    """Values in {0, .., 3}: most pairs tie, and equal distances go by index whichever lane, tile or segment held them."""
    monkeypatch.setenv("SCHPF_KNN_SPLIT", split)
    query, ref = integer_scores(n_query, K, dtype, seed=1), integer_scores(n_ref, K, dtype, seed=2)
    want = check_both(query, ref, 128)
    assert (np.diff(want[1], axis=1) == 0).mean() > 0.5


@pytest.mark.parametrize("split", ["1", "3"])
@pytest.mark.parametrize("k", [15, 128])
def test_nearest_rows_arrive_last(amd, k, split, monkeypatch):
    """All queries equal, the references on a line in decreasing distance: every candidate of every tile passes the
    threshold, every merge takes 64 new keys, and the lists are rewritten from end to end each time."""
    monkeypatch.setenv("SCHPF_KNN_SPLIT", split)
    n_ref = 1000
    query = np.zeros((70, 3))
    ref = np.zeros((n_ref, 3))
    ref[:, 1] = np.arange(n_ref, 0, -1) * 0.25
    want = check_both(query, ref, k)
    assert_array_equal(want[0], np.broadcast_to(np.arange(n_ref - 1, n_ref - 1 - k, -1), (70, k)))


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("n", [257, 1000])
def test_self_graph_with_duplicates(amd, n, dtype):
    """query is ref, self_first = 0: a row is never its own neighbour -- by index -- and its duplicates are, at distance 0."""
    x = gamma_scores(n, 20, dtype, seed=n)
    x[5] = x[100] = x[n - 1]          # three copies of one cell
    x[64] = x[63]
    idx, d2 = check_both(x, x, 15, self_first=0)
    assert not np.any(idx == np.arange(n)[:, None])
    assert_array_equal(idx[5, :2], [100, n - 1])
    assert_array_equal(idx[100, :2], [5, n - 1])
    assert_array_equal(idx[n - 1, :2], [5, 100])
    assert idx[63, 0] == 64 and idx[64, 0] == 63
    assert_array_equal(d2[[5, 100, n - 1], :2], np.zeros((3, 2)))
    assert np.all(d2[5, 2:] > 0)
    # nothing removed: every row finds itself first (or its earlier copy)
    idx, d2 = check_both(x, x, 15)
    assert_array_equal(d2[:, 0], np.zeros(n))
    assert idx[100, 0] == 5 and idx[7, 0] == 7
    # a block of the rows against all of them: row q of the block is row 200 + q of the reference
    idx, _ = check_both(np.ascontiguousarray(x[200:230]), x, 15, self_first=200)
    assert not np.any(idx == 200 + np.arange(30)[:, None])


def test_knn_on_gpu_tensors(amd):
    """torch tensors in, torch tensors on the same GPU out, equal to the host path's; the inputs are unchanged; on a
    stream of torch's as on the null stream."""
    query, ref, want = random_case(257, 5000, 20, 15, np.float64)
    t_query, t_ref = torch.tensor(query, device="cuda:0"), torch.tensor(ref, device="cuda:0")
    keep_q, keep_r = t_query.clone(), t_ref.clone()
    idx, dist = amd.knn(t_query, t_ref, k=15)
    assert idx.device == t_query.device and dist.device == t_query.device
    assert idx.dtype == torch.int32 and dist.dtype == torch.float64 and tuple(idx.shape) == (257, 15)
    h_idx, h_dist = amd.knn(query, ref, k=15)
    assert isinstance(h_idx, np.ndarray)
    assert_array_equal(h_idx, want[0])
    assert_array_equal(h_dist, np.sqrt(want[1]))
    assert_array_equal(idx.cpu().numpy(), h_idx)
    assert_array_equal(dist.cpu().numpy(), h_dist)
    assert torch.equal(t_query, keep_q) and torch.equal(t_ref, keep_r)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        s_idx, s_dist = amd.knn(t_query * 1.0, t_ref, k=15)      # the product is enqueued on the same stream
    side.synchronize()
    assert torch.equal(s_idx, idx) and torch.equal(s_dist, dist)
    # the self graph, float32, cosine
    x32 = torch.tensor(gamma_scores(300, 8, np.float32, seed=3) + 0.01, device="cuda:0")
    c_idx, c_dist = amd.knn(x32, k=10, metric="cosine")
    unit = (x32 / torch.linalg.vector_norm(x32, dim=1, keepdim=True)).cpu().numpy()
    assert_same((c_idx.cpu().numpy(), 2 * c_dist.cpu().numpy()), debug_knn(unit, unit, 10, 0))
    assert not bool((c_idx == torch.arange(300, device="cuda:0", dtype=torch.int32)[:, None]).any())
    assert float(c_dist.min()) >= 0 and float(c_dist.max()) <= 1 and c_dist.dtype == torch.float64
    with pytest.raises(ValueError, match="device=1 was asked for"):
        amd.knn(t_query, t_ref, device=1)
    G = amd.knn_graph(idx, dist, 5000)
    assert G.shape == (257, 5000) and G.nnz == 257 * 15


def test_errors_write_nothing(amd):
    from schpf_amd import _lib
    lib = _lib.load()
    query, ref = gamma_scores(70, 4, seed=1), gamma_scores(200, 4, seed=2)
    query[66, 1] = np.inf
    query[3, 2] = np.nan
    ref[1, 0] = np.inf
    for call in (host_knn, device_knn):
        with pytest.raises(ValueError, match="scores must be finite; offending row 3 of query$"):
            call(query, ref, 5)
        with pytest.raises(ValueError, match="scores must be finite; offending row 1 of ref$"):
            call(gamma_scores(70, 4, seed=1), ref, 5)
        with pytest.raises(ValueError, match="offending row 1 of query$"):
            call(ref, ref, 5, 0)
        with pytest.raises(ValueError, match="k must be at most the admissible reference rows"):
            call(ref[:20], ref[:20], 20, 0)
        with pytest.raises(ValueError, match=r"k must be in \[1, 128\]"):
            call(ref, ref, 129)
    # the outputs of a refused call keep what they held
    idx, d2 = np.full((70, 5), -7, np.int32), np.full((70, 5), -7.0)
    assert lib.schpf_knn(0, 1, 70, 200, 4, _p(query), _p(ref), 5, ctypes.c_int64(-1), _p(idx), _p(d2)) != 0
    assert np.all(idx == -7) and np.all(d2 == -7.0)
    t_q, t_r = torch.tensor(query, device="cuda:0"), torch.tensor(ref, device="cuda:0")
    t_idx = torch.full((70, 5), -7, dtype=torch.int32, device="cuda:0")
    t_d2 = torch.full((70, 5), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.schpf_knn_device(0, None, 1, 70, 200, 4, dp(t_q), dp(t_r), 5, ctypes.c_int64(-1), dp(t_idx), dp(t_d2)) != 0
    assert bool((t_idx == -7).all()) and bool((t_d2 == -7.0).all())
    # n_query = 0 succeeds; a device that does not exist does not
    assert lib.schpf_knn(0, 1, 0, 200, 4, None, _p(ref), 5, ctypes.c_int64(-1), None, None) == 0
    assert lib.schpf_knn_device(0, None, 1, 0, 200, 4, None, dp(t_r), 5, ctypes.c_int64(-1), None, None) == 0
    assert lib.schpf_knn(99, 1, 70, 200, 4, _p(ref), _p(ref), 5, ctypes.c_int64(-1), _p(idx), _p(d2)) != 0
    assert b"no such HIP device" in lib.schpf_last_error()
    assert lib.schpf_knn(0, 1, 70, 0, 4, _p(ref), _p(ref), 5, ctypes.c_int64(-1), _p(idx), _p(d2)) != 0
    assert b"n_ref must be at least 1" in lib.schpf_last_error()


def test_fitted_model_end_to_end(amd, tmp_path):
    """Fit the small golden matrix; model.neighbors is knn on the cell scores, and `scHPF score --knn 15` writes it."""
    from schpf_amd import cli
    X = golden_coo(load_golden("pbmc_like_data.npz"))
    np.random.seed(0)
    model = amd.scHPF(5, max_iter=12, verbose=False).fit(X)
    N = X.shape[0]
    idx, dist = model.neighbors(k=15)
    assert idx.shape == (N, 15) and idx.dtype == np.int32 and dist.dtype == np.float64
    want_idx, want_dist = amd.knn(model.cell_score())
    assert_array_equal(idx, want_idx)
    assert_array_equal(dist, want_dist)
    d_idx, d_d2 = debug_knn(model.cell_score(), model.cell_score(), 15, 0)
    assert_array_equal(idx, d_idx)
    assert_array_equal(dist, np.sqrt(d_d2))
    assert not np.any(idx == np.arange(N)[:, None]) and np.all(np.diff(dist, axis=1) >= 0)
    # label transfer: the first cells as a query of their own against the atlas find themselves first
    t_idx, t_dist = model.neighbors(k=3, query=model.cell_score()[:40])
    assert_array_equal(t_dist[:, 0], np.zeros(40))
    path = str(tmp_path / "model.joblib")
    amd.save_model(model, path)
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "plain")]) == 0
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "knn"), "--knn", "15"]) == 0
    plain, with_knn = set(os.listdir(str(tmp_path / "plain"))), set(os.listdir(str(tmp_path / "knn")))
    assert with_knn - plain == {"knn_indices.txt", "knn_distances.txt"}
    f_idx = np.loadtxt(str(tmp_path / "knn" / "knn_indices.txt"), dtype=np.int64)
    f_dist = np.loadtxt(str(tmp_path / "knn" / "knn_distances.txt"))
    assert f_idx.shape == (N, 15) and f_dist.shape == (N, 15)
    assert_array_equal(f_idx, idx)
    assert_array_equal(f_dist, dist)
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "cos"), "--knn", "4", "--knn-metric", "cosine"]) == 0
    assert_array_equal(np.loadtxt(str(tmp_path / "cos" / "knn_indices.txt"), dtype=np.int64),
                       model.neighbors(k=4, metric="cosine")[0])
