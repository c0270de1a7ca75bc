"""Cell and gene filtering on the GPU: both GPU entry points of the axis statistics and of the submatrix
against the host restatement, bit for bit, in every storage and on a side stream; the refusals; the contention case of the
gene side; the Python surface on tensors in GPU memory; a fit of the filtered tensor; `scHPF qc` through a subprocess."""
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse import csr_matrix

from conftest import ROOT, golden_coo, load_golden
from _qc_reference import (FILL, MESSAGES, NGENES, NROWS, call_stats, call_submatrix, debug_stats, debug_submatrix,
                           device_stats, device_submatrix, kernel_matrix, odd_values, row_lists, same, spoiled, stats_out,
                           wide_matrix, VALUE_KINDS)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


@pytest.fixture(scope="module")
def case(amd):
    X, flags = kernel_matrix()
    want = debug_stats(X, flags, 32)
    for a in want:
        a.setflags(write=False)
    return X, flags, want


@pytest.mark.parametrize("n_sets", [0, 1, 32])
def test_the_statistics_equal_the_restatement(case, n_sets):
    X, flags, want = case
    want = list(want)
    want[2] = want[2][:n_sets]
    given = flags if n_sets else None
    same(call_stats("schpf_axis_stats", X, given, n_sets, device=0), want)
    same(device_stats(X, given, n_sets), want)


def test_the_statistics_of_wide_rows(amd):
    """Rows whose share of a window is long: the gene side gives each a whole wavefront, not 16 lanes."""
    X, flags = wide_matrix()
    want = debug_stats(X, flags, 2)
    same(device_stats(X, flags, 2), want)
    same(device_stats(X, flags, 2, indptr_dtype=np.int32, idx_dtype=np.int64, val_dtype=np.float32), want)
    same(call_stats("schpf_axis_stats", X, flags, 2, device=0), want)


def test_the_statistics_in_every_storage(case):
    import torch
    X, flags, want = case
    want = list(want)
    want[2] = want[2][:3]
    side = torch.cuda.Stream()
    for indptr_dtype, idx_dtype in ((np.int32, np.int32), (np.int64, np.int64), (np.int32, np.int64)):
        for val_dtype in VALUE_KINDS:
            same(device_stats(X, flags, 3, indptr_dtype=indptr_dtype, idx_dtype=idx_dtype, val_dtype=val_dtype, stream=side), want)
    for val_dtype in VALUE_KINDS:
        same(call_stats("schpf_axis_stats", X, flags, 3, device=0, val_dtype=val_dtype), want)


@pytest.mark.parametrize("name,rows,keep", row_lists(), ids=[r[0] for r in row_lists()])
def test_the_submatrix_equals_the_restatement(case, name, rows, keep):
    X = case[0]
    want = debug_submatrix(X, rows, keep)
    same(call_submatrix("schpf_submatrix", X, rows, keep, device=0), want)
    same(device_submatrix(X, rows, keep), want)


def test_the_submatrix_in_every_storage(case):
    import torch
    X = case[0]
    _, rows, keep = row_lists()[3]
    side = torch.cuda.Stream()
    for val_dtype in VALUE_KINDS:
        want = debug_submatrix(X, rows, keep, val_dtype=val_dtype)
        same(call_submatrix("schpf_submatrix", X, rows, keep, device=0, val_dtype=val_dtype), want)
        for indptr_dtype, idx_dtype in ((np.int32, np.int32), (np.int64, np.int64)):
            same(device_submatrix(X, rows, keep, indptr_dtype=indptr_dtype, idx_dtype=idx_dtype, val_dtype=val_dtype, stream=side), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_value_bytes_survive_on_the_device(dtype):
    """Unsorted rows, duplicate columns, -0.0, a NaN with a payload: nothing is interpreted, the stored order stays."""
    X = csr_matrix((5, 5), dtype=dtype)
    X.indptr, X.indices, X.data = np.array([0, 4, 4, 8, 8, 8], np.int64), np.array([4, 1, 1, 3, 0, 4, 2, 4], np.int32), odd_values(dtype)
    keep, rows = np.array([1, 1, 0, 1, 7], np.uint8), [2, 0, 2, 1]
    want = debug_submatrix(X, rows, keep)
    same(device_submatrix(X, rows, keep), want)
    same(call_submatrix("schpf_submatrix", X, rows, keep, device=0), want)


def test_the_sizing_call_and_the_capacity(case):
    X = case[0]
    _, rows, keep = row_lists()[3]
    want = debug_submatrix(X, rows, keep)
    for got in (device_submatrix(X, rows, keep, fill=False), call_submatrix("schpf_submatrix", X, rows, keep, device=0, fill=False)):
        assert got[0] == want[0] and got[2] is None and got[3] is None
        assert_array_equal(got[1], want[1])
    message = MESSAGES["capacity"] % (want[1][-1], want[1][-1] - 1)
    with pytest.raises(ValueError) as err:
        device_submatrix(X, rows, keep, short=1)
    assert err.value.args[0] == message
    assert err.value.args[1][0] == FILL and all((a == FILL).all() for a in err.value.args[1][1:])      # nothing written
    with pytest.raises(ValueError) as err:
        call_submatrix("schpf_submatrix", X, rows, keep, device=0, short=1)
    assert str(err.value) == message


@pytest.mark.parametrize("kind", ["indptr", "indptr_end", "index", "order", "value"])
def test_the_statistics_refuse_by_message_and_write_nothing(case, kind):
    X, message = spoiled(kind)
    with pytest.raises(ValueError) as err:
        device_stats(X, case[1], 2)
    assert err.value.args[0] == message
    assert all((a == FILL).all() for a in err.value.args[1])
    out = stats_out(NROWS, NGENES, 2)
    with pytest.raises(ValueError) as err:
        call_stats("schpf_axis_stats", X, case[1], 2, device=0, val_dtype=np.float64, out=out)
    assert str(err.value) == message
    assert all((a == FILL).all() for a in out)


def test_the_overflow_boundary_on_the_device():
    for ncells, fits in ((32768, False), (32767, True)):
        X = csr_matrix((np.full(1, 2 ** 24, np.int32), np.zeros(1, np.int32), np.concatenate([[0], np.ones(ncells, np.int64)])),
                       shape=(ncells, 1))
        if fits:
            same(device_stats(X), debug_stats(X))
        else:
            with pytest.raises(ValueError) as err:
                device_stats(X)
            assert err.value.args[0] == MESSAGES["overflow"] % (2 ** 24, ncells)
            assert all((a == FILL).all() for a in err.value.args[1])


@pytest.mark.parametrize("kind", ["indptr", "indptr_end", "index", "rows"])
def test_the_submatrix_refuses_by_message_and_writes_nothing(kind):
    rows = [3, 5, NROWS, 4, -1]
    if kind == "rows":
        X, message = kernel_matrix()[0], MESSAGES["rows"] % 2
    else:
        X, message = spoiled(kind)
    with pytest.raises(ValueError) as err:
        device_submatrix(X, rows, None)
    assert err.value.args[0] == message
    assert err.value.args[1][0] == FILL and (err.value.args[1][1] == FILL).all()
    with pytest.raises(ValueError) as err:
        call_submatrix("schpf_submatrix", X, rows, None, device=0)
    assert str(err.value) == message


def test_empty_inputs_on_the_device(case):
    X, flags, _ = case
    empty = csr_matrix((NROWS, NGENES), dtype=np.int32)
    keep = np.arange(NGENES) % 3 == 0
    same(device_stats(empty, flags, 2), debug_stats(empty, flags, 2))
    same(call_stats("schpf_axis_stats", empty, flags, 2, device=0), debug_stats(empty, flags, 2))
    for M, rows in ((X, []), (empty, [3, 3, 0]), (X, None)):
        same(device_submatrix(M, rows, keep), debug_submatrix(M, rows, keep))
        same(call_submatrix("schpf_submatrix", M, rows, keep, device=0), debug_submatrix(M, rows, keep))
    with pytest.raises(ValueError) as err:                              # rows are still checked
        device_submatrix(empty, [3, NROWS], keep)
    assert err.value.args[0] == MESSAGES["rows"] % 1


def test_the_contention_case():
    """70 001 cells x 3 genes: one gene expressed everywhere at one value, one Poisson, one empty; set bits on the first two.
    Every entry of the gene side lands in two bins per workgroup, and the final atomics carry everything."""
    N = 70001
    rng = np.random.RandomState(5)
    poisson = rng.poisson(0.7, N).astype(np.int32)            # stored as it is: zeros among the entries
    stored = rng.random_sample(N) < 0.9
    cols = np.stack([np.zeros(N, np.int32), np.ones(N, np.int32)], axis=1)
    vals = np.stack([np.full(N, 3, np.int32), poisson], axis=1)
    mask = np.stack([np.ones(N, bool), stored], axis=1)
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    X = csr_matrix((vals[mask], cols[mask], indptr), shape=(N, 3))
    flags = np.array([1, 3, 0], np.uint32)
    want = debug_stats(X, flags, 2)
    assert want[3][0] == N and want[4][0] == 3 * N and want[5][0] == 9 * N and want[3][2] == 0 and 0 < want[3][1] < stored.sum()
    assert_array_equal(want[2][0], want[1])
    same(device_stats(X, flags, 2), want)
    same(call_stats("schpf_axis_stats", X, flags, 2, device=0), want)


def as_tensor(X, layout, device="cuda:0"):
    import torch
    X = X.tocsr()
    if layout == "csr":
        return torch.sparse_csr_tensor(torch.tensor(X.indptr, dtype=torch.int64), torch.tensor(X.indices, dtype=torch.int64),
                                       torch.tensor(X.data), size=X.shape).to(device)
    C = X.tocoo()
    return torch.sparse_coo_tensor(torch.tensor(np.stack([C.row, C.col]), dtype=torch.int64), torch.tensor(C.data), size=X.shape).to(device)


@pytest.mark.parametrize("layout", ["csr", "coo"])
def test_the_python_surface_on_gpu_tensors(amd, case, layout):
    import torch
    X, flags, want = case
    Xg = as_tensor(X, layout)
    mito = (flags & 1).astype(bool)
    host = amd.qc_metrics(X, gene_sets={"mito": mito})
    found = amd.qc_metrics(Xg, gene_sets={"mito": mito})
    for key, w in zip(("cell_n_genes", "cell_total", "gene_n_cells", "gene_total", "gene_sumsq"), (want[0], want[1]) + tuple(want[3:])):
        assert found[key].is_cuda and found[key].dtype == torch.int64 and host[key].dtype == np.int64
        assert_array_equal(found[key].cpu().numpy(), w)
        assert_array_equal(host[key], w)
    assert found["cell_set_total"]["mito"].is_cuda
    assert_array_equal(found["cell_set_total"]["mito"].cpu().numpy(), want[2][0])
    assert_array_equal(host["cell_set_total"]["mito"], want[2][0])
    assert_array_equal(found["gene_mean"], host["gene_mean"])
    assert_array_equal(found["gene_var"], host["gene_var"])
    assert_array_equal(amd.scHPF.qc(Xg)["gene_n_cells"].cpu().numpy(), want[3])

    cells = np.arange(NROWS) % 7 != 0
    picks = [5, 5, 139, 0]
    for rows, genes in ((cells, mito), (picks, np.flatnonzero(mito)), (torch.tensor(cells).cuda(), None),
                        (torch.tensor(picks, dtype=torch.int32).cuda(), mito), (None, None)):
        S = amd.submatrix(Xg, cells=rows, genes=genes)
        assert S.is_cuda and S.layout == torch.sparse_csr and S.values().dtype == torch.int32
        H = amd.submatrix(X, cells=rows.cpu().numpy() if torch.is_tensor(rows) else rows, genes=genes)
        assert isinstance(H, csr_matrix) and H.dtype == X.dtype and tuple(S.shape) == H.shape
        ref = X[np.arange(NROWS) if rows is None else (rows.cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows))]
        ref = ref if genes is None else ref[:, mito]
        for got in (H, csr_matrix((S.values().cpu().numpy(), S.col_indices().cpu().numpy(), S.crow_indices().cpu().numpy()), shape=H.shape)):
            assert_array_equal(got.indptr, ref.indptr)
            assert_array_equal(got.indices, ref.indices)
            assert_array_equal(got.data, ref.data)

    F, cell_keep, gene_keep, _ = amd.filter_counts(Xg, min_cells=3, min_genes=10, min_counts=200, max_set_fraction={"mito": 0.6},
                                                   gene_sets={"mito": mito})
    Fh, cell_keep_h, gene_keep_h, _ = amd.filter_counts(X, min_cells=3, min_genes=10, min_counts=200, max_set_fraction={"mito": 0.6},
                                                        gene_sets={"mito": mito})
    assert F.is_cuda and cell_keep.is_cuda and gene_keep.is_cuda and cell_keep.dtype == torch.bool
    assert_array_equal(cell_keep.cpu().numpy(), cell_keep_h)
    assert_array_equal(gene_keep.cpu().numpy(), gene_keep_h)
    assert_array_equal(gene_keep_h, want[3] >= 3)
    assert 0 < cell_keep_h.sum() < NROWS
    assert_array_equal(F.crow_indices().cpu().numpy(), Fh.indptr)
    assert_array_equal(F.col_indices().cpu().numpy(), Fh.indices)
    assert_array_equal(F.values().cpu().numpy(), Fh.data)
    assert (Fh != X[cell_keep_h][:, gene_keep_h]).nnz == 0
    with pytest.raises(ValueError, match="X is on GPU 0, device=1 was asked for"):
        amd.qc_metrics(Xg, device=1)


def test_a_fit_of_the_filtered_tensor_equals_a_fit_of_the_scipy_slice(amd):
    """Drop every seventh cell, then the genes seen in fewer than 3 of the cells that are left, on the GPU; fit the tensor
    that comes back as it is.  The SciPy slice under the same seed gives the same model."""
    g = load_golden("fit_data_k5_s0_f64.npz")
    X = golden_coo(g).tocsr()
    Xg = as_tensor(X, "coo")
    cells = np.arange(X.shape[0]) % 7 != 0
    F, cell_keep, gene_keep, found = amd.filter_counts(amd.submatrix(Xg, cells=cells), min_cells=3)
    Xs = X[cells]
    genes = np.asarray((Xs > 0).sum(axis=0)).ravel() >= 3
    assert cell_keep.all() and 0 < genes.sum() < X.shape[1]
    assert_array_equal(gene_keep.cpu().numpy(), genes)
    S = Xs[:, genes].tocoo()
    assert F.is_cuda and tuple(F.shape) == S.shape
    models = []
    for M, kw in ((F, {}), (S, {"init": "device"})):
        np.random.seed(0)
        models.append(amd.scHPF(5, max_iter=5, min_iter=5, check_freq=1, verbose=False).fit(M, **kw))
    a, b = models
    assert (a.bp, a.dp) == (b.bp, b.dp)
    assert a.loss == b.loss and len(a.loss) > 0
    assert_array_equal(a.theta.e_x, b.theta.e_x)
    assert_array_equal(a.beta.e_x, b.beta.e_x)


def test_qc_write_filtered_on_the_command_line(amd, case, tmp_path):
    from scipy.io import mmread, mmwrite
    X, flags, want = case
    matrix = str(tmp_path / "counts.mtx")
    mmwrite(matrix, X.tocoo(), field="integer")
    exe = [sys.executable, os.path.join(ROOT, "bin", "scHPF")]
    out = tmp_path / "out"
    subprocess.check_call(exe + ["qc", "-i", matrix, "-o", str(out), "--min-cells", "3", "--min-genes", "10", "--write-filtered"],
                          stdout=subprocess.DEVNULL)
    assert sorted(os.listdir(str(out))) == ["cell_qc.txt", "filtered.mtx", "gene_qc.txt", "kept_cells.txt", "kept_genes.txt",
                                            "qc_commandline_args.json"]
    cells, genes = want[0] >= 10, want[3] >= 3
    assert_array_equal(np.loadtxt(str(out / "kept_cells.txt"), dtype=np.int64), np.flatnonzero(cells))
    assert_array_equal(np.loadtxt(str(out / "kept_genes.txt"), dtype=np.int64), np.flatnonzero(genes))
    assert_array_equal(np.loadtxt(str(out / "cell_qc.txt"), skiprows=1, dtype=np.int64), np.stack([want[0], want[1]], axis=1))
    F, S = mmread(str(out / "filtered.mtx")).tocsr(), X[cells][:, genes]
    F.sort_indices()
    assert F.shape == S.shape
    assert_array_equal(F.indptr, S.indptr)
    assert_array_equal(F.indices, S.indices)
    assert_array_equal(F.data, S.data)
