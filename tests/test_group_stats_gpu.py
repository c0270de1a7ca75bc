"""Pseudobulk on the GPU: both GPU entry points of the group statistics against the host restatement, bit for
bit, on every label set, in every storage and on a side stream; the contention case; the refusals; the Python surface on
tensors in GPU memory; `scHPF.pseudobulk` on a fitted model; `scHPF score --pseudobulk` through a subprocess."""
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse import coo_matrix, csr_matrix

from conftest import ROOT, golden_coo, load_golden
from _aggregate_reference import (MESSAGES, N, NGENES, NROWS, VALUE_KINDS, call_group_stats, check_the_cases, debug_group_stats,
                                  device_group_stats, equal, label_sets, labels_out, overflowing, small_matrix, spoiled, stacked_matrix,
                                  stacked_wide_matrix, untouched)
from _qc_reference import kernel_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def _cases(X):
    cases = []
    for name, labels, G in label_sets(X.shape[0]):
        want = debug_group_stats(X, labels, G)
        for a in want:
            a.setflags(write=False)
        cases.append((name, labels, G, want))
    return X, cases


@pytest.fixture(scope="module")
def stacked(amd):
    check_the_cases()
    return _cases(stacked_matrix())


@pytest.fixture(scope="module")
def wide(amd):
    return _cases(stacked_wide_matrix())


def test_the_kernel_matrix_on_every_label_set(stacked):
    X, cases = stacked
    for name, labels, G, want in cases:
        equal(device_group_stats(X, labels, G), want)
        equal(call_group_stats("schpf_group_stats", X, labels, G, device=0), want)


def test_the_wide_matrix_on_every_label_set(wide):
    X, cases = wide
    for name, labels, G, want in cases:
        equal(device_group_stats(X, labels, G), want)
        equal(call_group_stats("schpf_group_stats", X, labels, G, device=0), want)


def test_every_cell_its_own_group(amd):
    X = small_matrix()
    labels = np.arange(NROWS, dtype=np.int32)
    want = debug_group_stats(X, labels, NROWS)
    assert_array_equal(want[2], X.toarray())
    equal(device_group_stats(X, labels, NROWS), want)
    equal(call_group_stats("schpf_group_stats", X, labels, NROWS, device=0), want)


def test_every_storage_and_a_side_stream(stacked):
    import torch
    X, cases = stacked
    name, labels, G, want = cases[1]
    side = torch.cuda.Stream()
    for indptr_dtype, idx_dtype in ((np.int32, np.int32), (np.int64, np.int64), (np.int32, np.int64)):
        for val_dtype in VALUE_KINDS:
            equal(device_group_stats(X, labels, G, indptr_dtype=indptr_dtype, idx_dtype=idx_dtype, val_dtype=val_dtype, stream=side), want)
    for val_dtype in VALUE_KINDS:
        equal(call_group_stats("schpf_group_stats", X, labels, G, device=0, val_dtype=val_dtype), want)
    without = list(want[:3]) + [None]
    equal(device_group_stats(X, labels, G, sumsq=False), without)
    equal(call_group_stats("schpf_group_stats", X, labels, G, device=0, sumsq=False), without)


def test_the_contention_case(amd):
    """20 001 cells that all store the same three columns, in one group: every lane of a workgroup meets the others in three
    bins, and the final atomics of ten slabs meet in three places."""
    ncells = 20001
    rng = np.random.RandomState(5)
    vals = np.stack([np.full(ncells, 3, np.int32), rng.poisson(0.7, ncells).astype(np.int32), rng.randint(1, 100, ncells).astype(np.int32)], axis=1)
    cols = np.tile(np.array([0, 1, 4], np.int32), ncells)
    X = csr_matrix((vals.ravel(), cols, np.arange(ncells + 1, dtype=np.int64) * 3), shape=(ncells, 5))
    labels = np.zeros(ncells, np.int32)
    want = debug_group_stats(X, labels, 1)
    assert want[1][0, 0] == ncells and want[2][0, 0] == 3 * ncells and want[3][0, 0] == 9 * ncells and 0 < want[1][0, 1] < ncells
    equal(device_group_stats(X, labels, 1), want)
    equal(call_group_stats("schpf_group_stats", X, labels, 1, device=0), want)


@pytest.mark.parametrize("kind", ["indptr", "indptr_end", "index", "order", "value", "below", "above"])
def test_refusals_by_message_with_nothing_written(amd, kind):
    X, labels, G, message = spoiled(kind)
    with pytest.raises(ValueError) as err:
        device_group_stats(X, labels, G)
    assert err.value.args[0] == message and untouched(err.value.args[1])
    out = labels_out(G, NGENES)
    with pytest.raises(ValueError) as err:
        call_group_stats("schpf_group_stats", X, labels, G, device=0, out=out)
    assert str(err.value) == message and untouched(out)


def test_the_overflow_rule_the_product_and_no_entries(amd):
    from schpf_amd import _lib
    X, labels, G, message = overflowing()
    with pytest.raises(ValueError) as err:
        device_group_stats(X, labels, G)
    assert err.value.args[0] == message and untouched(err.value.args[1])
    out = labels_out(G, 1)
    with pytest.raises(ValueError) as err:
        call_group_stats("schpf_group_stats", X, labels, G, device=0, out=out)
    assert str(err.value) == message and untouched(out)
    equal(device_group_stats(X, labels, G, sumsq=False), debug_group_stats(X, labels, G, sumsq=False))      # not asked for: not checked
    one = np.zeros(1, np.int64)
    lab = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert _lib.load().schpf_group_stats(0, 1, 2 ** 15, 0, None, None, None, 0, p(lab), 2 ** 16, p(one), p(one), p(one), p(one)) != 0
    assert _lib.load().schpf_last_error().decode() == MESSAGES["product"]
    # nnz = 0: the matrix is not read, the labels are checked and the cells counted
    empty = csr_matrix((NROWS, NGENES), dtype=np.int32)
    labels = (np.arange(NROWS) % 4 - 1).astype(np.int32)
    want = debug_group_stats(empty, labels, 5)
    equal(device_group_stats(empty, labels, 5), want)
    equal(call_group_stats("schpf_group_stats", empty, labels, 5, device=0), want)
    labels[17] = 5
    with pytest.raises(ValueError) as err:
        device_group_stats(empty, labels, 5)
    assert err.value.args[0] == MESSAGES["labels"] % 17 and untouched(err.value.args[1])
    nobody = np.full(NROWS, -1, np.int32)                      # no cell in a group: no slab
    X = kernel_matrix()[0]
    equal(device_group_stats(X, nobody, 2), debug_group_stats(X, nobody, 2))


def as_tensor(X, layout, device="cuda:0"):
    import torch
    if layout == "csr":
        X = X.tocsr()
        return torch.sparse_csr_tensor(torch.tensor(X.indptr, dtype=torch.int64), torch.tensor(X.indices, dtype=torch.int64),
                                       torch.tensor(X.data), size=X.shape).to(device)
    C = X.tocoo()
    return torch.sparse_coo_tensor(torch.tensor(np.stack([C.row, C.col]), dtype=torch.int64), torch.tensor(C.data), size=X.shape).to(device)


@pytest.mark.parametrize("layout", ["csr", "coo"])
def test_the_python_surface_on_gpu_tensors(amd, layout):
    import torch
    X = kernel_matrix()[0]
    labels = (np.arange(NROWS) % 5 - 1).astype(np.int64)
    want = debug_group_stats(X, labels, 4)
    host = amd.group_stats(X, labels)
    found = amd.group_stats(as_tensor(X, layout), torch.tensor(labels).cuda() if layout == "csr" else labels)
    for key, w in zip(("n", "nexpr", "total", "sumsq"), want):
        assert found[key].is_cuda and found[key].dtype == torch.int64 and host[key].dtype == np.int64
        assert_array_equal(found[key].cpu().numpy(), w)
        assert_array_equal(host[key], w)
    assert list(amd.group_stats(as_tensor(X, layout), labels, ngroups=6, sumsq=False)) == ["n", "nexpr", "total"]
    bulk_host, bulk = amd.pseudobulk(X, labels, min_cells=2), amd.pseudobulk(as_tensor(X, layout), labels, min_cells=2)
    assert bulk["groups"] == bulk_host["groups"] == [(0,), (1,), (2,), (3,)]
    assert bulk["counts"].is_cuda and bulk["n_cells"].is_cuda
    assert_array_equal(bulk["counts"].cpu().numpy(), want[2])
    assert_array_equal(bulk_host["counts"], want[2])
    for key in ("pct", "mean", "var"):
        assert_array_equal(bulk[key], bulk_host[key])
    if layout == "coo":                                        # duplicates in a COO tensor are summed
        half = X.copy()
        half.data = np.minimum(half.data, 2 ** 23)
        C = half.tocoo()
        twice = coo_matrix((np.tile(C.data, 2), (np.tile(C.row, 2), np.tile(C.col, 2))), shape=X.shape)
        Tg = torch.sparse_coo_tensor(torch.tensor(np.stack([twice.row, twice.col]), dtype=torch.int64), torch.tensor(twice.data),
                                     size=X.shape).cuda()
        assert not Tg.is_coalesced()
        assert_array_equal(amd.group_stats(Tg, labels)["total"].cpu().numpy(), 2 * debug_group_stats(half, labels, 4)[2])
    with pytest.raises(ValueError, match="X is on GPU 0, device=1 was asked for"):
        amd.group_stats(as_tensor(X, layout), labels, device=1)
    with pytest.raises(ValueError, match=r"labels must be in \[-1, ngroups\); offending cell 3$"):
        amd.group_stats(as_tensor(X, layout), np.where(np.arange(NROWS) == 3, 4, labels), ngroups=4)


def test_a_fitted_model_and_the_command_line(amd, tmp_path):
    """Fit the small golden matrix: `scHPF.pseudobulk(X)` sums every labelled cell once, and `scHPF score -i X --knn 5
    --knn-graph jaccard --clusters --pseudobulk --sample-ids FILE` writes the sample x cluster table."""
    from scipy.io import mmwrite
    X = golden_coo(load_golden("pbmc_like_data.npz"))
    np.random.seed(0)
    model = amd.scHPF(5, max_iter=12, verbose=False).fit(X)
    ncells, J = X.shape
    labels = model.clusters(k=5)
    found = model.pseudobulk(X, k=5)
    assert found["groups"] == [(c,) for c in range(int(labels.max()) + 1)]
    assert found["counts"].shape == (len(found["groups"]), J) and found["n_cells"].sum() == ncells
    assert_array_equal(found["counts"].sum(axis=0), np.asarray(X.tocsr().sum(axis=0)).ravel())
    assert_array_equal(found["counts"], debug_group_stats(X.tocsr(), labels, len(found["groups"]))[2])

    path, matrix, ids = str(tmp_path / "model.joblib"), str(tmp_path / "counts.mtx"), str(tmp_path / "samples.txt")
    amd.save_model(model, path)
    mmwrite(matrix, X, field="integer")
    samples = np.array(["donor%d" % (i % 3) for i in range(ncells)])
    with open(ids, "w") as fh:
        fh.write("".join(s + "\n" for s in samples))
    out = tmp_path / "out"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "bin", "scHPF"), "score", "-m", path, "-i", matrix, "-o", str(out), "-p", "run",
                           "--knn", "5", "--knn-graph", "jaccard", "--clusters", "--pseudobulk", "--sample-ids", ids],
                          stdout=subprocess.DEVNULL, timeout=240)
    counts = np.loadtxt(str(out / "run.pseudobulk_counts.txt"), delimiter="\t", dtype=np.int64, ndmin=2)
    pct = np.loadtxt(str(out / "run.pseudobulk_pct.txt"), delimiter="\t", ndmin=2)
    groups = [line.rstrip("\n").split("\t") for line in open(str(out / "run.pseudobulk_groups.txt"))]
    written = np.loadtxt(str(out / "run.clusters.txt"), dtype=np.int64)
    want = amd.pseudobulk(X, (samples, written))
    assert [(s, int(c)) for s, c, n in groups] == want["groups"] and [int(n) for s, c, n in groups] == list(want["n_cells"])
    assert counts.shape == pct.shape == (len(groups), J)
    assert counts.sum() == X.sum()
    assert_array_equal(counts, want["counts"])
    assert ((pct >= 0) & (pct <= 1)).all()
