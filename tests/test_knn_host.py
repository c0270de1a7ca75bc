"""Nearest neighbours in factor space, without a GPU: the library's serial restatement schpf_debug_knn --
which the kernels are then held to bit for bit (tests/test_knn_gpu.py) -- is pinned to the definition, and the Python
layer's own work (metrics, defaults, the sparse graph) is checked with the restatement in the kernels' place."""
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from _knn_reference import _p, debug_knn, gamma_scores, integer_scores, numpy_d2, numpy_knn


def ascending_in_the_key(idx, d2):
    step_d, step_i = np.diff(d2, axis=1), np.diff(idx.astype(np.int64), axis=1)
    return bool(np.all((step_d > 0) | ((step_d == 0) & (step_i > 0))))


# (n_query, n_ref, K, k, self_first)
INTEGER_CASES = [(1, 1, 1, 1, -1), (2, 2, 1, 1, 0), (33, 129, 5, 15, -1), (65, 257, 20, 128, -1), (40, 40, 3, 39, 0),
                 (10, 50, 2, 7, 20)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_query,n_ref,K,k,self_first", INTEGER_CASES)
def test_integer_inputs_equal_numpy_exactly(n_query, n_ref, K, k, self_first, dtype):
    """Values in {0, .., 3}: d2 is exact in double whatever the order of summation, and most pairs tie -- the order of
    equal distances is the index order, exactly."""
    ref = integer_scores(n_ref, K, dtype, seed=n_ref)
    query = ref if n_query == n_ref else integer_scores(n_query, K, dtype, seed=1000 + n_query)
    idx, d2 = debug_knn(query, ref, k, self_first)
    want_idx, want_d2 = numpy_knn(query, ref, k, self_first)
    assert_array_equal(idx, want_idx)
    assert_array_equal(d2, want_d2)
    if self_first >= 0:
        assert not np.any(idx == self_first + np.arange(n_query)[:, None])
    if n_ref > 100:
        assert (np.diff(d2, axis=1) == 0).mean() > 0.5      # the point: ties


@pytest.mark.parametrize("K", [1, 20, 50])
def test_gamma_inputs_within_the_summation_bound(K):
    """Random doubles, (65, 257), nothing left out.  All K terms are >= 0, so the fused sum and NumPy's differ by at most
    (K + 2) * 2^-52 relative: every returned d2 is that close to NumPy's for the returned index, nothing that was not
    returned is closer than the k-th by more than the bound, and the lists ascend in the key."""
    k = 15
    query, ref = gamma_scores(65, K, seed=K), gamma_scores(257, K, seed=100 + K)
    idx, d2 = debug_knn(query, ref, k)
    bound = (K + 2) * 2.0 ** -52
    all_d2 = numpy_d2(query, ref)
    assert_allclose(d2, np.take_along_axis(all_d2, idx.astype(np.int64), axis=1), rtol=bound, atol=0)
    assert ascending_in_the_key(idx, d2)
    rest = np.ones(all_d2.shape, bool)
    np.put_along_axis(rest, idx.astype(np.int64), False, axis=1)
    assert rest.sum() == 65 * (257 - k)
    smallest_left = np.where(rest, all_d2, np.inf).min(axis=1)
    assert np.all(d2[:, -1] <= smallest_left * (1 + bound))


def test_float32_inputs_are_converted_exactly():
    q32, r32 = gamma_scores(20, 7, np.float32, seed=1), gamma_scores(90, 7, np.float32, seed=2)
    a = debug_knn(q32, r32, 10)
    b = debug_knn(q32.astype(np.float64), r32.astype(np.float64), 10)
    assert_array_equal(a[0], b[0])
    assert_array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


def test_overflowing_distances_sort_by_index():
    """A d2 that overflows is +inf: such pairs tie, and go by index."""
    query = np.array([[1e200, 0.0]])
    ref = np.array([[-1e200, 0.0], [1e200, 1.0], [-1e200, 5.0], [-1e200, 2.0]])
    idx, d2 = debug_knn(query, ref, 4)
    assert_array_equal(idx, [[1, 0, 2, 3]])
    assert_array_equal(d2, [[1.0, np.inf, np.inf, np.inf]])


def test_errors():
    ref = gamma_scores(10, 3)
    with pytest.raises(ValueError, match=r"k must be in \[1, 128\]"):
        debug_knn(ref, ref, 0)
    with pytest.raises(ValueError, match=r"k must be in \[1, 128\]"):
        debug_knn(gamma_scores(4, 3), gamma_scores(300, 3), 129)
    debug_knn(ref, ref, 10)                       # every row, itself included
    debug_knn(ref, ref, 9, self_first=0)
    with pytest.raises(ValueError, match="k must be at most the admissible reference rows"):
        debug_knn(ref, ref, 10, self_first=0)
    with pytest.raises(ValueError, match="n_ref must be at least 1"):
        debug_knn(ref, np.empty((0, 3)), 1)
    idx, d2 = debug_knn(np.empty((0, 3)), ref, 3)         # n_query = 0 succeeds
    assert idx.shape == (0, 3)
    from schpf_amd import _lib
    lib = _lib.load()
    out_i, out_d = np.empty((10, 2), np.int32), np.empty((10, 2))
    assert lib.schpf_debug_knn(1, 10, 10, 3, None, _p(ref), 2, ctypes.c_int64(-1), _p(out_i), _p(out_d)) != 0
    assert b"NULL" in lib.schpf_last_error()
    assert lib.schpf_debug_knn(7, 10, 10, 3, _p(ref), _p(ref), 2, ctypes.c_int64(-1), _p(out_i), _p(out_d)) != 0
    assert lib.schpf_debug_knn(1, 10, 10, 257, _p(ref), _p(ref), 2, ctypes.c_int64(-1), _p(out_i), _p(out_d)) != 0
    assert b"nfactors must be in [1, 256]" in lib.schpf_last_error()


def test_non_finite_inputs_are_refused_by_row():
    query, ref = gamma_scores(8, 4, seed=1), gamma_scores(20, 4, seed=2)
    query[3, 2] = np.nan
    query[6, 0] = np.inf
    ref[1, 1] = np.inf
    with pytest.raises(ValueError, match="scores must be finite; offending row 3 of query$"):
        debug_knn(query, ref, 2)
    with pytest.raises(ValueError, match="scores must be finite; offending row 1 of ref$"):
        debug_knn(gamma_scores(8, 4, seed=1), ref, 2)
    with pytest.raises(ValueError, match="offending row 1 of query$"):
        debug_knn(ref.astype(np.float32), ref.astype(np.float32), 2)


# ---------------------------------------------------------------------------------------------------- the Python layer
@pytest.fixture
def neighbors(monkeypatch):
    """schpf_amd.neighbors with the host restatement in the place of schpf_knn: what is left is the module's own work."""
    from schpf_amd import neighbors as nb
    calls = []

    def search(query, ref, k, self_first, device):
        assert query.flags.c_contiguous and ref.flags.c_contiguous and query.dtype == ref.dtype
        calls.append((query is ref, self_first))
        return debug_knn(query, ref, k, self_first)

    monkeypatch.setattr(nb, "_search_host", search)
    nb.calls = calls
    return nb


def test_exclude_self_defaults(neighbors):
    x, y = gamma_scores(30, 4, seed=1), gamma_scores(12, 4, seed=2)
    idx, dist = neighbors.knn(x, k=5)
    assert neighbors.calls[-1] == (True, 0)                 # the self graph: one table, no cell its own neighbour
    assert idx.dtype == np.int32 and dist.dtype == np.float64 and idx.shape == dist.shape == (30, 5)
    assert not np.any(idx == np.arange(30)[:, None])
    want_idx, want_d2 = debug_knn(x, x, 5, 0)
    assert_array_equal(idx, want_idx)
    assert_array_equal(dist, np.sqrt(want_d2))
    idx, dist = neighbors.knn(y, x, k=5)
    assert neighbors.calls[-1] == (False, -1)               # against a reference: nothing is left out
    assert_array_equal(idx, debug_knn(y, x, 5)[0])
    idx, dist = neighbors.knn(x, k=5, exclude_self=False)
    assert neighbors.calls[-1] == (True, -1)
    assert_array_equal(idx[:, 0], np.arange(30))
    assert_array_equal(dist[:, 0], np.zeros(30))
    neighbors.knn(x[:12], x, k=5, exclude_self=True)
    assert neighbors.calls[-1] == (False, 0)
    # float32 stays float32, anything else becomes float64
    neighbors.knn(x.astype(np.float32), k=3)
    assert_array_equal(neighbors.knn(np.arange(12).reshape(6, 2), k=2)[0], neighbors.knn(np.arange(12.0).reshape(6, 2), k=2)[0])


def test_cosine_is_euclidean_on_unit_rows_halved(neighbors):
    x, y = gamma_scores(40, 6, seed=3) + 0.01, gamma_scores(9, 6, seed=4) + 0.01
    unit = lambda a: a / np.sqrt((a * a).sum(axis=1, keepdims=True))  # noqa: E731
    idx, dist = neighbors.knn(y, x, k=7, metric="cosine")
    e_idx, e_dist = neighbors.knn(unit(y), unit(x), k=7)
    assert_array_equal(idx, e_idx)
    assert_allclose(dist, e_dist ** 2 / 2, rtol=1e-15, atol=0)      # the square root and back: two roundings
    cos = (unit(y) @ unit(x).T)
    assert_allclose(dist, 1 - np.take_along_axis(cos, idx.astype(np.int64), axis=1), atol=1e-14, rtol=0)
    x[17] = 0.0
    with pytest.raises(ValueError, match="zero row"):
        neighbors.knn(y, x, k=7, metric="cosine")
    with pytest.raises(ValueError, match="zero row"):
        neighbors.knn(x, k=7, metric="cosine")
    with pytest.raises(ValueError, match="metric must be one of euclidean, cosine"):
        neighbors.knn(x, k=7, metric="manhattan")
    with pytest.raises(ValueError, match=r"k must be in \[1, 128\]"):
        neighbors.knn(x, k=0)


def test_knn_graph():
    from schpf_amd import knn_graph
    idx = np.array([[2, 0], [3, 1], [0, 4]], np.int32)
    dist = np.array([[0.5, 1.5], [0.0, 2.0], [1.0, 3.0]])
    G = knn_graph(idx, dist, 5)
    assert G.shape == (3, 5) and G.format == "csr" and G.nnz == 6        # the neighbour at distance 0 is stored
    assert_array_equal(G.toarray(), [[1.5, 0, 0.5, 0, 0], [0, 2.0, 0, 0.0, 0], [1.0, 0, 0, 0, 3.0]])
    assert_array_equal(G.indptr, [0, 2, 4, 6])
    assert_array_equal(G[1].indices, [3, 1])
    with pytest.raises(ValueError, match=r"indices must be in \[0, n_ref\)"):
        knn_graph(idx, dist, 4)
    with pytest.raises(ValueError, match="one shape"):
        knn_graph(idx, dist[:, :1], 5)


def test_model_neighbors_and_exports(neighbors):
    import schpf_amd
    assert schpf_amd.knn is neighbors.knn and "knn_graph" in schpf_amd.__all__
    rng = np.random.RandomState(0)
    gam = lambda n: schpf_amd.HPF_Gamma(rng.gamma(1.0, 1.0, n), rng.gamma(1.0, 1.0, n) + 0.5)  # noqa: E731
    atlas, other = schpf_amd.scHPF(3), schpf_amd.scHPF(3)
    atlas.xi, atlas.theta = gam((25,)), gam((25, 3))
    other.xi, other.theta = gam((6,)), gam((6, 3))
    idx, dist = atlas.neighbors(k=4)
    assert neighbors.calls[-1] == (True, 0)
    assert_array_equal(idx, debug_knn(atlas.cell_score(), atlas.cell_score(), 4, 0)[0])
    idx, dist = atlas.neighbors(k=4, query=other)
    assert neighbors.calls[-1] == (False, -1) and idx.shape == (6, 4)
    assert_array_equal(idx, atlas.neighbors(k=4, query=other.cell_score())[0])
    assert_array_equal(idx, debug_knn(other.cell_score(), atlas.cell_score(), 4)[0])
