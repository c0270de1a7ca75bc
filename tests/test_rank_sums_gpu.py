"""Wilcoxon rank sums per gene and group on the GPU.  schpf_rank_sums and schpf_rank_sums_device against the
library's host restatement schpf_debug_rank_sums (tests/test_rank_sums_host.py pins it to scipy.stats): all five int64
arrays equal, exactly, whatever the shape of the matrix.  Then the Python surface: rank_sums on GPU COO and CSR tensors,
scHPF.markers and `scHPF score ... --clusters --markers`."""
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from conftest import golden_coo, load_golden
from _ranksum_reference import (CASES, MESSAGES, NAMES, _p, as_csc, as_matrix, debug_rank_sums, dense_gene_case, good_call,
                                host_rank_sums, poisson_counts, random_labels, refusals)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def device_rank_sums(matrix, labels, G, stream=None, fill=-7):
    """schpf_rank_sums_device on torch tensors -> the five NumPy arrays."""
    from schpf_amd import _lib
    N, J, indptr, indices, data = matrix
    tensors = [torch.tensor(np.ascontiguousarray(a, t), device="cuda:0")
               for a, t in ((indptr, np.int64), (indices, np.int32), (data, np.float32), (labels, np.int32))]
    out = [torch.full(s, fill, dtype=torch.int64, device="cuda:0") for s in ((G,), (J,), (J,), (G, J), (G, J))]
    torch.cuda.synchronize()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
    _lib.check(_lib.load().schpf_rank_sums_device(0, ctypes.c_void_p(stream), N, J, *[ptr(t) for t in tensors], G,
                                                  *[ptr(t) for t in out]))
    return tuple(t.cpu().numpy() for t in out)


def check_both(case, want=None):
    matrix, labels, G = case
    want = debug_rank_sums(matrix, labels, G) if want is None else want
    for got in (host_rank_sums(matrix, labels, G), device_rank_sums(matrix, labels, G)):
        for name, a, b in zip(NAMES, got, want):
            assert_array_equal(a, b, err_msg=name)
    return want


@functools.lru_cache(maxsize=None)
def large_case():
    """70 001 cells: a gene expressed everywhere at one value, a Poisson gene and an all-distinct one, and the
    restatement's answers; computed once."""
    case = dense_gene_case()
    for a in case[0][2:] + (case[1],):
        a.setflags(write=False)
    return case, debug_rank_sums(*case)


@pytest.mark.parametrize("case", sorted(CASES))
def test_small_shapes(amd, case):
    """One cell and one gene; no entries; wave edges; all values distinct; 300 genes of 0-3 entries in one chunk; one group
    and 300 of them; an empty group, cells outside every group, all of them outside; stored zeros, -0.0, subnormals,
    values near the largest float; matrices scaled to a target sum."""
    n, zeros, ties, nexpr, rank2 = check_both(CASES[case]())
    if case == "one_cell_one_gene":
        assert rank2.tolist() == [[2]] and nexpr.tolist() == [[1]]


def test_a_run_across_many_workgroups(amd):
    case, want = large_case()
    check_both(case, want)
    N = case[0][0]
    assert want[2][0] == N ** 3 - N and want[2][2] == 0


def test_many_cells_outside_the_bins(amd):
    """5 000 groups: past the 2 048 bins of a workgroup, in the counts and in the sums."""
    matrix = poisson_counts(20000, 3, 51, rate=2.0)
    check_both((matrix, random_labels(20000, 5000, 52, outside=0.1), 5000))


def test_rank_sums_on_gpu_tensors(amd):
    """Sparse COO and CSR tensors on the GPU in, tensors on the same GPU out, equal to the host path's; on a side stream too."""
    (matrix, labels, G), want = large_case()
    X = as_csc(matrix).tocoo()
    coo = torch.sparse_coo_tensor(torch.tensor(np.stack([X.row, X.col]).astype(np.int64)), torch.tensor(X.data), size=X.shape).to("cuda:0")
    keep = coo._values().clone()
    got = amd.rank_sums(coo, labels, ngroups=G)
    for name, b in zip(NAMES, want):
        assert got[name].device == coo.device and got[name].dtype == torch.int64
        assert_array_equal(got[name].cpu().numpy(), b)
    R = as_csc(matrix).tocsr()
    side = torch.cuda.Stream(device="cuda:0")
    with warnings.catch_warnings():          # torch announces that its CSR tensors are in beta, once per process
        warnings.filterwarnings("ignore", message="Sparse CSR tensor support is in beta")
        csr = torch.sparse_csr_tensor(torch.tensor(R.indptr), torch.tensor(R.indices), torch.tensor(R.data), size=R.shape).to("cuda:0")
        with torch.cuda.stream(side):
            doubled = torch.sparse_csr_tensor(csr.crow_indices(), csr.col_indices(), csr.values() * 2.0, size=R.shape)   # on this stream
            twice = amd.rank_sums(doubled, torch.tensor(labels, device="cuda:0"), ngroups=G)
    side.synchronize()
    for name in NAMES:                                           # twice every value: a monotone map
        assert torch.equal(twice[name], got[name])
    assert torch.equal(coo._values(), keep)
    small, small_labels, small_G = CASES["empty_group_and_outside"]()
    S = as_csc(small).tocoo()
    repeated = torch.sparse_coo_tensor(torch.tensor(np.stack([np.tile(S.row, 2), np.tile(S.col, 2)]).astype(np.int64)),
                                       torch.tensor(np.tile(S.data, 2)), size=S.shape).to("cuda:0")            # every entry twice
    summed = amd.rank_sums(repeated, small_labels)
    for name, b in zip(NAMES, debug_rank_sums(small, small_labels, small_G)):
        assert_array_equal(summed[name].cpu().numpy(), b)
    host = amd.rank_sums(as_csc(small), small_labels)                                # SciPy in, NumPy out
    for name in NAMES:
        assert isinstance(host[name], np.ndarray)
        assert_array_equal(host[name], summed[name].cpu().numpy())
    with pytest.raises(ValueError, match="device=1 was asked for"):
        amd.rank_sums(coo, labels, device=1)
    found, want = amd.rank_genes_groups(repeated, small_labels), amd.rank_genes_groups(as_csc(small) * 2, small_labels)
    for name in ("scores", "pvals", "pvals_adj", "pct_in", "pct_out"):                # from the integers alone
        assert_array_equal(found[name], want[name])
    for name in ("mean_in", "mean_out", "logfoldchanges"):                           # double sums in another order
        assert_allclose(found[name], want[name], rtol=1e-12, equal_nan=True)
    from schpf_amd.markers import _scaled
    scaled = _scaled(repeated, 1e4)                                                  # in float32, on the GPU
    totals = torch.sparse.sum(scaled, dim=1).to_dense().cpu().numpy()
    assert scaled.dtype == torch.float32 and scaled.device == repeated.device
    assert_allclose(totals[np.asarray(S.sum(axis=1)).ravel() > 0], 1e4, rtol=1e-5)
    assert_array_equal(amd.rank_genes_groups(repeated, small_labels, target_sum=1e4)["scores"],
                       amd.rank_genes_groups(scaled, small_labels)["scores"])


def test_refused_calls_leave_their_outputs(amd):
    from schpf_amd import _lib
    lib = _lib.load()
    for message, matrix, labels, G in refusals(*good_call()):
        if G != 3 or not 0 <= matrix[0] < 1 << 21:
            continue                                             # the argument checks: below, without arrays of that size
        for call in (host_rank_sums, device_rank_sums):
            with pytest.raises(ValueError) as err:
                call(matrix, labels, G)
            assert str(err.value) == message
    # the outputs of a refused call keep what they held
    N, J, indptr, indices, data, labels, G = good_call()
    bad = data.copy()
    bad[int(indptr[5])] = np.nan
    out = [np.full(s, -7, np.int64) for s in (G, J, J, G * J, G * J)]
    assert lib.schpf_rank_sums(0, N, J, _p(indptr), _p(indices), _p(bad), _p(labels), G, *[_p(a) for a in out]) != 0
    assert lib.schpf_last_error().decode() == MESSAGES["values"] % 5
    assert all((a == -7).all() for a in out)
    tensors = [torch.tensor(a, device="cuda:0") for a in (indptr, indices, bad, labels)]
    t_out = [torch.full((s,), -7, dtype=torch.int64, device="cuda:0") for s in (G, J, J, G * J, G * J)]
    torch.cuda.synchronize()
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.schpf_rank_sums_device(0, None, N, J, *[dp(t) for t in tensors], G, *[dp(t) for t in t_out]) != 0
    assert lib.schpf_last_error().decode() == MESSAGES["values"] % 5
    assert all(bool((t == -7).all()) for t in t_out)
    wrong = labels.copy()
    wrong[11] = G
    tensors[2], tensors[3] = torch.tensor(data, device="cuda:0"), torch.tensor(wrong, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.schpf_rank_sums_device(0, None, N, J, *[dp(t) for t in tensors], G, *[dp(t) for t in t_out]) != 0
    assert lib.schpf_last_error().decode() == MESSAGES["labels"] % 11
    assert all(bool((t == -7).all()) for t in t_out)
    # 2^21 cells are refused by message before anything is read; so is a device that does not exist
    for too_many in (1 << 21, -1):
        assert lib.schpf_rank_sums(0, too_many, J, _p(indptr), _p(indices), _p(data), _p(labels), G, *[_p(a) for a in out]) != 0
        assert lib.schpf_last_error().decode() == "ncells must be in [0, 2^21)"
        assert lib.schpf_rank_sums_device(0, None, too_many, J, *[dp(t) for t in tensors], G, *[dp(t) for t in t_out]) != 0
        assert lib.schpf_last_error().decode() == "ncells must be in [0, 2^21)"
    assert all((a == -7).all() for a in out) and all(bool((t == -7).all()) for t in t_out)
    assert lib.schpf_rank_sums(99, N, J, _p(indptr), _p(indices), _p(data), _p(labels), G, *[_p(a) for a in out]) != 0
    assert b"no such HIP device" in lib.schpf_last_error()


def test_no_cells_or_no_genes(amd):
    from schpf_amd import _lib
    lib = _lib.load()
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for N, J in ((0, 5), (5, 0)):
        out = [np.full(max(s, 1), -7, np.int64) for s in (3, J, J, 3 * J, 3 * J)]
        assert lib.schpf_rank_sums(0, N, J, None, None, None, None, 3, *[_p(a) for a in out]) == 0          # reads no input
        assert not out[0].any() and all(not a[:s].any() for a, s in zip(out[1:], (J, J, 3 * J, 3 * J)))
        t_out = [torch.full((max(s, 1),), -7, dtype=torch.int64, device="cuda:0") for s in (3, J, J, 3 * J, 3 * J)]
        torch.cuda.synchronize()
        assert lib.schpf_rank_sums_device(0, None, N, J, None, None, None, None, 3, *[dp(t) for t in t_out]) == 0
        assert not bool(t_out[0].any()) and all(not bool(t[:s].any()) for t, s in zip(t_out[1:], (J, J, 3 * J, 3 * J)))
        assert lib.schpf_rank_sums_device(0, None, N, J, None, None, None, None, 3, None, None, None, None, None) == 0


def test_fitted_model_end_to_end(amd, tmp_path):
    """Fit the small golden matrix: markers is clusters + rank_genes_groups, its integers are the restatement's, and `scHPF
    score -i X --knn 5 --knn-graph jaccard --clusters --markers` writes the same scores."""
    from scipy.io import mmwrite
    from schpf_amd import cli
    X = golden_coo(load_golden("pbmc_like_data.npz"))
    np.random.seed(0)
    model = amd.scHPF(5, max_iter=12, verbose=False).fit(X)
    N, J = X.shape
    labels = model.clusters(k=5)
    found = model.markers(X, k=5)
    G = int(labels.max()) + 1
    assert found["scores"].shape == (G, J) and found["n"].sum() == N
    sums = amd.rank_sums(X, labels)
    for name, b in zip(NAMES, debug_rank_sums(as_matrix(X), labels, G)):
        assert_array_equal(sums[name], b)
    assert_array_equal(found["n"], sums["n"])
    assert np.isfinite(found["scores"]).all() and (found["pvals_adj"] >= found["pvals"]).all() and (found["pvals_adj"] <= 1).all()
    assert (found["scores"].max(axis=1) > 3).any()               # the clusters of a fitted model are marked by some gene
    path, matrix = str(tmp_path / "model.joblib"), str(tmp_path / "counts.mtx")
    amd.save_model(model, path)
    mmwrite(matrix, X, field="integer")
    common = ["score", "-m", path, "-i", matrix, "--knn", "5", "--knn-graph", "jaccard", "--clusters"]
    assert cli.main(common + ["-o", str(tmp_path / "plain")]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "out"), "--markers"]) == 0
    assert (set(os.listdir(str(tmp_path / "out"))) - set(os.listdir(str(tmp_path / "plain")))
            == {"marker_scores.txt", "marker_pvals_adj.txt"})
    assert_allclose(np.loadtxt(str(tmp_path / "out" / "marker_scores.txt"), delimiter="\t", ndmin=2), found["scores"].T, rtol=1e-15)
    assert_allclose(np.loadtxt(str(tmp_path / "out" / "marker_pvals_adj.txt"), delimiter="\t", ndmin=2), found["pvals_adj"].T,
                    rtol=1e-15)
