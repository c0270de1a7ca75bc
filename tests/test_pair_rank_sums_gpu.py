"""Rank sums between pairs of groups on the GPU.  schpf_pair_rank_sums and schpf_pair_rank_sums_device against
the library's host restatement schpf_debug_pair_rank_sums (tests/test_pair_rank_sums_host.py pins it to scipy.stats): all
four int64 arrays equal, exactly, whatever the shape of the matrix and of the list of pairs.  The accumulation works on
chunks of 512 sub-runs (gene, group, value), so the edges are those of the number of distinct values.  Then the Python
surface: pair_rank_sums on GPU COO and CSR tensors, scHPF.pair_markers and `scHPF score ... --markers --marker-pairs`."""
import ctypes
import functools
import os
import re
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from conftest import golden_coo, load_golden
from _pair_ranksum_reference import (BAD_PAIRS, CASES, MESSAGES, NAMES, _p, all_pairs, debug_pair_rank_sums, dense_gene_case,
                                     good_call, host_pair_rank_sums, mixed_pairs, pair_refusals, poisson_counts, random_labels)
from _ranksum_reference import EMPTY_65, ONE, all_distinct_gene, as_csc, as_matrix, one_dense_gene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 512


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def device_pair_rank_sums(matrix, labels, G, pairs, stream=None, fill=-7):
    """schpf_pair_rank_sums_device on torch tensors -> the four NumPy arrays."""
    from schpf_amd import _lib
    N, J, indptr, indices, data = matrix
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    P = len(pairs)
    tensors = [torch.tensor(np.ascontiguousarray(a, t), device="cuda:0")
               for a, t in ((indptr, np.int64), (indices, np.int32), (data, np.float32), (labels, np.int32), (pairs, np.int32))]
    out = [torch.full(s, fill, dtype=torch.int64, device="cuda:0") for s in ((G,), (G, J), (P, J), (P, J))]
    torch.cuda.synchronize()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
    _lib.check(_lib.load().schpf_pair_rank_sums_device(0, ctypes.c_void_p(stream), N, J, *[ptr(t) for t in tensors[:4]], G,
                                                       ptr(tensors[4]), P, *[ptr(t) for t in out]))
    return tuple(t.cpu().numpy() for t in out)


def check_both(case, want=None):
    """Both entry points, their outputs holding -7 before the call: every element is written."""
    matrix, labels, G, pairs = case
    want = debug_pair_rank_sums(matrix, labels, G, pairs) if want is None else want
    for got in (host_pair_rank_sums(matrix, labels, G, pairs, fill=-7), device_pair_rank_sums(matrix, labels, G, pairs)):
        for name, a, b in zip(NAMES, got, want):
            assert_array_equal(a, b, err_msg=name)
    return want


def test_chunk_size_is_mirrored():
    source = open(os.path.join(ROOT, "schpf_amd", "csrc", "pair_rank_sums.hip")).read()
    assert int(re.search(r"constexpr int CHUNK = (\d+);", source).group(1)) == CHUNK


@pytest.mark.parametrize("case", sorted(set(CASES) - {"groups_300_cells_5000"}))
def test_shapes_of_the_rank_sums(amd, case):
    """No entries; wave edges; all values distinct; 300 genes of 0-3 entries in one chunk; one group (no pair); an empty
    group, cells outside every group, all of them outside; stored zeros, -0.0, subnormals, values near the largest float;
    matrices scaled to a target sum.  Every list of pairs holds a repeat and reversed pairs."""
    matrix, labels, G = CASES[case]()
    pairs = mixed_pairs(G) if G > 1 else np.zeros((0, 2), np.int32)
    n, nexpr, u2, ties = check_both((matrix, labels, G, pairs))
    if case == "no_entries":
        assert_array_equal(u2, (n[pairs[:, 0]] * n[pairs[:, 1]])[:, None] * np.ones((1, matrix[1]), np.int64))


def test_300_groups_and_all_their_pairs(amd):
    """44 850 pairs on 3 genes: 89 700 sides, far past the LDS bins of a chunk; every sub-run steps through 299 of them."""
    G = 300
    pairs = all_pairs(G)
    assert len(pairs) == 44850
    check_both((poisson_counts(5000, 3, 6, rate=3.0), random_labels(5000, G, 6), G, pairs))


def test_one_cell_and_an_empty_second_group(amd):
    n, nexpr, u2, ties = check_both((ONE, np.zeros(1, np.int32), 2, [[0, 1], [1, 0]]))
    assert n.tolist() == [1, 0] and nexpr.tolist() == [[1], [0]] and u2.tolist() == [[0], [0]] and ties.tolist() == [[0], [0]]
    check_both((EMPTY_65, random_labels(65, 2, 1), 2, [[0, 1]]))                    # G = 2, P = 1, no entries


@pytest.mark.parametrize("length", [63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1])
def test_lists_at_the_edges_of_waves_and_chunks(amd, length):
    """One gene whose values are all distinct: `length` sub-runs, in two groups, then in one group and an empty one."""
    matrix = all_distinct_gene(length, seed=length)
    check_both((matrix, random_labels(length, 2, length), 2, [[0, 1], [1, 0]]))
    check_both((matrix, np.zeros(length, np.int32), 2, [[1, 0]]))


def test_lists_and_genes_across_chunk_edges(amd):
    """Gene 0 has exactly one chunk of sub-runs, so gene 1 starts on a chunk edge; gene 1 is one value in every cell -- one
    sub-run per group; gene 2's lists lie across the next edges; with four groups every list is cut somewhere."""
    N = CHUNK
    a, b, c = all_distinct_gene(N, 1), one_dense_gene(N), all_distinct_gene(N, 2)
    indptr = np.array([0, N, 2 * N, 3 * N], np.int64)
    matrix = (N, 3, indptr, np.concatenate([m[3] for m in (a, b, c)]), np.concatenate([m[4] for m in (a, b, c)]))
    for G in (2, 4):
        n, nexpr, u2, ties = check_both((matrix, random_labels(N, G, 3), G, mixed_pairs(G)))
        assert (ties[:, 0] == 0).all() and (u2[0, 1] == n[0] * n[1]) and ties[0, 1] == (n[0] + n[1]) ** 3 - (n[0] + n[1])


@functools.lru_cache(maxsize=None)
def large_case():
    """70 001 cells in 20 groups, all 190 pairs: a gene expressed everywhere at one value, a Poisson gene and an all-distinct
    one, and the restatement's answers; computed once."""
    matrix, labels, G = dense_gene_case()
    for a in matrix[2:] + (labels,):
        a.setflags(write=False)
    pairs = all_pairs(G)
    pairs.setflags(write=False)
    return (matrix, labels, G, pairs), debug_pair_rank_sums(matrix, labels, G, pairs)


def test_a_run_across_many_workgroups(amd):
    case, want = large_case()
    n, nexpr, u2, ties = check_both(case, want)
    assert u2[0, 0] == n[0] * n[1] and ties[0, 2] == 0


def test_pairs_repeated_reversed_and_a_group_in_no_pair(amd):
    matrix, labels, G = CASES["empty_group_and_outside"]()
    pairs = np.array([[3, 0], [0, 3], [3, 0], [0, 3], [3, 0]], np.int32)            # group 2 is in no pair, group 1 is empty
    n, nexpr, u2, ties = check_both((matrix, labels, G, pairs))
    assert_array_equal(u2[0], u2[2])
    assert_array_equal(u2[0] + u2[1], np.full(matrix[1], 2 * n[0] * n[3]))
    assert nexpr[2].any()                                                           # ... and is counted all the same
    check_both((matrix, labels, G, np.zeros((0, 2), np.int32)))                     # no pairs at all: n and nexpr
    check_both((matrix, labels, G, [[1, 2]]))                                       # the empty group first


def test_a_side_stream(amd):
    matrix, labels, G = CASES["poisson_130"]()
    pairs = mixed_pairs(G)
    side = torch.cuda.Stream(device="cuda:0")
    got = device_pair_rank_sums(matrix, labels, G, pairs, stream=side.cuda_stream)
    side.synchronize()
    for name, a, b in zip(NAMES, got, debug_pair_rank_sums(matrix, labels, G, pairs)):
        assert_array_equal(a, b, err_msg=name)


def test_refused_calls_leave_their_outputs(amd):
    from schpf_amd import _lib
    lib = _lib.load()
    for message, matrix, labels, G, pairs in pair_refusals():
        if G != 3 or not 0 <= matrix[0] < 1 << 21 or isinstance(pairs, tuple):
            continue                                             # the argument checks: below, without arrays of that size
        for call in (host_pair_rank_sums, device_pair_rank_sums):
            with pytest.raises(ValueError) as err:
                call(matrix, labels, G, pairs)
            assert str(err.value) == message
    # the outputs of a refused call keep what they held
    N, J, indptr, indices, data, labels, G = good_call()
    pairs = all_pairs(G)
    P = len(pairs)
    bad = data.copy()
    bad[int(indptr[5])] = np.nan
    wrong = pairs.copy()
    wrong[1, 1] = wrong[1, 0]
    out = [np.full(s, -7, np.int64) for s in (G, G * J, P * J, P * J)]
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    t_out = [torch.full((s,), -7, dtype=torch.int64, device="cuda:0") for s in (G, G * J, P * J, P * J)]
    for values, lab, rows, message in ((bad, labels, wrong, MESSAGES["values"] % 5), (data, labels, wrong, BAD_PAIRS % 1)):
        assert lib.schpf_pair_rank_sums(0, N, J, _p(indptr), _p(indices), _p(values), _p(lab), G, _p(rows), P,
                                        *[_p(a) for a in out]) != 0
        assert lib.schpf_last_error().decode() == message
        assert all((a == -7).all() for a in out)
        tensors = [torch.tensor(a, device="cuda:0") for a in (indptr, indices, values, lab, rows)]
        torch.cuda.synchronize()
        assert lib.schpf_pair_rank_sums_device(0, None, N, J, *[dp(t) for t in tensors[:4]], G, dp(tensors[4]), P,
                                               *[dp(t) for t in t_out]) != 0
        assert lib.schpf_last_error().decode() == message
        assert all(bool((t == -7).all()) for t in t_out)
    # what is refused before anything is read; so is a device that does not exist
    for kwargs, message in (({"N": 1 << 21}, "ncells must be in [0, 2^21)"), ({"P": (1 << 31) // J + 1}, "npairs * ngenes must be below 2^31"),
                            ({"P": -1}, "npairs must be >= 0")):
        cells, rows = kwargs.get("N", N), kwargs.get("P", P)
        assert lib.schpf_pair_rank_sums(0, cells, J, _p(indptr), _p(indices), _p(data), _p(labels), G, _p(pairs), rows,
                                        *[_p(a) for a in out]) != 0
        assert lib.schpf_last_error().decode() == message
        assert lib.schpf_pair_rank_sums_device(0, None, cells, J, *[dp(t) for t in tensors[:4]], G, dp(tensors[4]), rows,
                                               *[dp(t) for t in t_out]) != 0
        assert lib.schpf_last_error().decode() == message
    assert all((a == -7).all() for a in out) and all(bool((t == -7).all()) for t in t_out)
    assert lib.schpf_pair_rank_sums(99, N, J, _p(indptr), _p(indices), _p(data), _p(labels), G, _p(pairs), P, *[_p(a) for a in out]) != 0
    assert b"no such HIP device" in lib.schpf_last_error()


def test_no_cells_or_no_genes(amd):
    from schpf_amd import _lib
    lib = _lib.load()
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for N, J in ((0, 5), (5, 0)):
        sizes = (3, 3 * J, 2 * J, 2 * J)
        out = [np.full(max(s, 1), -7, np.int64) for s in sizes]
        assert lib.schpf_pair_rank_sums(0, N, J, None, None, None, None, 3, None, 2, *[_p(a) for a in out]) == 0      # reads no input
        assert all(not a[:s].any() for a, s in zip(out, sizes))
        t_out = [torch.full((max(s, 1),), -7, dtype=torch.int64, device="cuda:0") for s in sizes]
        torch.cuda.synchronize()
        assert lib.schpf_pair_rank_sums_device(0, None, N, J, None, None, None, None, 3, None, 2, *[dp(t) for t in t_out]) == 0
        assert all(not bool(t[:s].any()) for t, s in zip(t_out, sizes))
        assert lib.schpf_pair_rank_sums_device(0, None, N, J, None, None, None, None, 3, None, 2, None, None, None, None) == 0


def test_pair_rank_sums_on_gpu_tensors(amd):
    """Sparse COO and CSR tensors on the GPU in, tensors on the same GPU out, equal to the host path's; on a side stream too."""
    (matrix, labels, G, pairs), want = large_case()
    X = as_csc(matrix).tocoo()
    coo = torch.sparse_coo_tensor(torch.tensor(np.stack([X.row, X.col]).astype(np.int64)), torch.tensor(X.data), size=X.shape).to("cuda:0")
    got = amd.pair_rank_sums(coo, labels, ngroups=G)
    for name, b in zip(NAMES + ("pairs",), want + (pairs,)):
        assert got[name].device == coo.device and got[name].dtype == (torch.int32 if name == "pairs" else torch.int64)
        assert_array_equal(got[name].cpu().numpy(), b)
    small, small_labels, small_G = CASES["empty_group_and_outside"]()
    mine = [[3, 0], [0, 2], [3, 0]]
    host = amd.pair_rank_sums(as_csc(small), small_labels, pairs=mine)               # SciPy in, NumPy out
    for name, b in zip(NAMES, debug_pair_rank_sums(small, small_labels, small_G, mine)):
        assert isinstance(host[name], np.ndarray)
        assert_array_equal(host[name], b)
    R = as_csc(small).tocsr()
    side = torch.cuda.Stream(device="cuda:0")
    with warnings.catch_warnings():          # torch announces that its CSR tensors are in beta, once per process
        warnings.filterwarnings("ignore", message="Sparse CSR tensor support is in beta")
        csr = torch.sparse_csr_tensor(torch.tensor(R.indptr), torch.tensor(R.indices), torch.tensor(R.data), size=R.shape).to("cuda:0")
        with torch.cuda.stream(side):
            doubled = torch.sparse_csr_tensor(csr.crow_indices(), csr.col_indices(), csr.values() * 2.0, size=R.shape)   # on this stream
            twice = amd.pair_rank_sums(doubled, torch.tensor(small_labels, device="cuda:0"), pairs=mine)
    side.synchronize()
    for name in NAMES + ("pairs",):                                # twice every value: a monotone map
        assert_array_equal(twice[name].cpu().numpy(), host[name])
    with pytest.raises(ValueError, match="device=1 was asked for"):
        amd.pair_rank_sums(coo, labels, device=1)
    found, plain = amd.rank_genes_pairs(csr, small_labels, pairs=mine), amd.rank_genes_pairs(as_csc(small), small_labels, pairs=mine)
    for name in ("scores", "pvals", "pvals_adj", "pct_a", "pct_b", "mean_a", "mean_b", "logfoldchanges"):   # from integers alone
        assert_array_equal(found[name], plain[name])
    against = amd.rank_genes_groups(as_csc(small), small_labels, reference=0)
    assert_array_equal(against["scores"][3], plain["scores"][0])
    assert np.isnan(against["scores"][0]).all()
    scaled = amd.rank_genes_pairs(csr, small_labels, pairs=mine, target_sum=1e4)     # in float32, on the GPU
    assert np.isfinite(scaled["scores"]).all() and not np.array_equal(scaled["scores"], plain["scores"])


def test_fitted_model_end_to_end(amd, tmp_path):
    """Fit the small golden matrix: pair_markers(pairs="neighbors") tests exactly the pairs of clusters with an edge of the
    k-NN graph between them, its scores are rank_genes_pairs' on those pairs, its integers the restatement's, and `scHPF
    score ... --markers --marker-pairs neighbors` writes the same scores."""
    from scipy.io import mmwrite
    from schpf_amd import cli
    X = golden_coo(load_golden("pbmc_like_data.npz"))
    np.random.seed(0)
    model = amd.scHPF(5, max_iter=12, verbose=False).fit(X)
    N, J = X.shape
    labels = model.clusters(k=5)
    G = int(labels.max()) + 1
    count = np.asarray(model.cluster_graph(k=5, labels=labels)["count"])
    pairs = np.array([[a, b] for a in range(G) for b in range(a + 1, G) if count[a, b] > 0 or count[b, a] > 0], np.int32).reshape(-1, 2)
    found = model.pair_markers(X, k=5)
    assert_array_equal(found["pairs"], pairs)
    assert 0 < len(pairs) <= G * (G - 1) // 2 and found["scores"].shape == (len(pairs), J)
    want = amd.rank_genes_pairs(X, labels, pairs=pairs)
    for name in ("scores", "pvals", "pvals_adj", "logfoldchanges", "pct_a", "pct_b", "mean_a", "mean_b", "n"):
        assert_array_equal(found[name], want[name])
    sums = amd.pair_rank_sums(X, labels, pairs=pairs)
    for name, b in zip(NAMES, debug_pair_rank_sums(as_matrix(X), labels, G, pairs)):
        assert_array_equal(sums[name], b)
    assert np.isfinite(found["scores"]).all() and (found["pvals_adj"] >= found["pvals"]).all() and (found["pvals_adj"] <= 1).all()
    path, matrix = str(tmp_path / "model.joblib"), str(tmp_path / "counts.mtx")
    amd.save_model(model, path)
    mmwrite(matrix, X, field="integer")
    common = ["score", "-m", path, "-i", matrix, "--knn", "5", "--knn-graph", "jaccard", "--clusters", "--markers"]
    assert cli.main(common + ["-o", str(tmp_path / "plain")]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "out"), "--marker-pairs", "neighbors"]) == 0
    assert (set(os.listdir(str(tmp_path / "out"))) - set(os.listdir(str(tmp_path / "plain")))
            == {"pair_marker_pairs.txt", "pair_marker_scores.txt", "pair_marker_pvals_adj.txt"})
    assert_array_equal(np.loadtxt(str(tmp_path / "out" / "pair_marker_pairs.txt"), delimiter="\t", dtype=int, ndmin=2), pairs)
    assert_allclose(np.loadtxt(str(tmp_path / "out" / "pair_marker_scores.txt"), delimiter="\t", ndmin=2), found["scores"].T, rtol=1e-15)
    assert_allclose(np.loadtxt(str(tmp_path / "out" / "pair_marker_pvals_adj.txt"), delimiter="\t", ndmin=2), found["pvals_adj"].T,
                    rtol=1e-15)
