"""Pearson residual variance per gene, without a GPU: the yardstick (tests/_residual_var_reference.py, the
definition on a dense matrix in NumPy float64) against the split into distinct cell totals the kernels use, the library's
serial restatement schpf_debug_residual_var against the yardstick, its refusals with their words, and the Python layer and
the command line with the restatement in the kernels' place.

Bounds.  |S1 - S1_ref| <= tol sum|r| and |S2 - S2_ref| <= tol S2_ref with tol = max(1e-12, 4 N 2^-53) -- a sum of n doubles
is within (n - 1) eps sum|terms| of exact in any order, each term carries a few ulps, and the yardstick rounds too.  A
ranking is asserted only where the yardstick's variance has a relative gap above 1e-6 at the cut: the sums agree to 1e-11
at these sizes, so the selected set and the ranks above the cut cannot differ."""
import json
import os
import re

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from conftest import golden_coo, load_golden
from _residual_var_reference import (BAD_VALUES, CASE_NAMES, CLIPS, THETAS, batch_reference, call, case, counts, cut_gap,
                                     dense_reference, errors, expected, refusals, refused, split_reference, tolerance)

DEBUG = "schpf_debug_residual_var"


def test_the_generator_plants_its_cases():
    X, (N, J, indptr, indices, data) = case("257x129")
    assert not X[:, 0].any() and not X[3].any()                      # a gene and a cell without counts
    assert (X[:, 1] > 0).sum() == N - 1 and indptr[2] - indptr[1] == N  # a gene in every cell; its segment has every cell
    assert (data == 0).sum() > 100                                  # stored zeros
    n, s = X.sum(axis=1), X.sum(axis=0)
    mu = n[N - 1] * s[J - 1] / s.sum()
    assert (X[N - 1, J - 1] - mu) / np.sqrt(mu + mu * mu / 100.0) > np.sqrt(N)   # the outlier is clipped by the default
    assert len(np.unique(case("equal_totals")[0].sum(axis=1))) == 1
    assert len(np.unique(case("distinct_totals")[0].sum(axis=1))) == 2000


@pytest.mark.parametrize("name", ["257x129", "70001x67", "equal_totals", "distinct_totals"])
def test_the_split_is_the_definition(name):
    X = case(name)[0]
    for theta in THETAS:
        for clip in CLIPS:
            S1, S2, U = split_reference(X, theta, clip)
            e1, e2 = errors(S1, S2, expected(name, theta, clip))
            print("%s theta=%s clip=%s U=%d: S1 %.3g S2 %.3g" % (name, theta, clip, U, e1, e2))
            assert e1 <= tolerance(X.shape[0]) and e2 <= tolerance(X.shape[0])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_against_the_yardstick(name):
    X, matrix = case(name)
    N = X.shape[0]
    for theta in THETAS:
        for clip in CLIPS:
            s1, s2, cell_total, gene_total = call(DEBUG, matrix, theta, clip)
            assert_array_equal(cell_total, X.sum(axis=1))
            assert_array_equal(gene_total, X.sum(axis=0))
            e1, e2 = errors(s1, s2, expected(name, theta, clip))
            print("%s theta=%s clip=%s: S1 %.3g S2 %.3g" % (name, theta, clip, e1, e2))
            assert e1 <= tolerance(N) and e2 <= tolerance(N)
    if name == "257x129":
        assert s1[0] == 0.0 and s2[0] == 0.0                          # the gene without counts
        assert (np.abs(s1) <= 2.0 * N).all() and (s2 <= 4.0 * N).all()  # clip = 2 bounds every residual


def test_refusals_leave_the_outputs_untouched():
    seen = set()
    for message, change in refusals():
        status, said, out = refused(DEBUG, change)
        assert status != 0 and said == message, (message, said)
        assert all((a == -7).all() for a in out)
        seen.add(message.split(";")[0])
    assert len(seen) == 9
    status, said, out = refused(DEBUG, {})
    assert status == 0 and not any((a == -7).any() for a in out)
    status, said, out = refused(DEBUG, {"clip": np.inf, "inv_theta": 0.0, "cell_total": None, "gene_total": None})
    assert status == 0 and (out[2] == -7).all() and (out[3] == -7).all() and not (out[0] == -7).any()   # NULL is skipped


def test_nothing_to_do_succeeds():
    from schpf_amd import _lib
    lib = _lib.load()
    N, J = 7, 5
    empty = (N, J, np.zeros(J + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    for a in call(DEBUG, empty):                                     # nnz = 0: zeros
        assert not a.any()
    for n, j in ((0, 5), (5, 0), (0, 0)):
        out = call(DEBUG, (n, j, np.zeros(j + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)), clip=1.0)
        assert all(not a.any() for a in out)
    assert lib.schpf_debug_residual_var(0, 0, 0, None, None, None, 0.0, 1.0, None, None, None, None) == 0
    zeros = (3, 2, np.array([0, 2, 3], np.int64), np.array([0, 2, 1], np.int32), np.zeros(3, np.float32))   # T = 0
    assert all(not a.any() for a in call(DEBUG, zeros))


# ------------------------------------------------------------------------------------------- the Python layer and the CLI
HOSTED = ("schpf_residual_var", "schpf_axis_stats", "schpf_submatrix")


class HostLibrary:
    """The library with the GPU entry points of HOSTED answered by their host restatements: the same arguments without the
    device."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in HOSTED:
            debug = getattr(self._lib, "schpf_debug_" + name[len("schpf_"):])
            return lambda device, *args: debug(*args)
        return getattr(self._lib, name)


@pytest.fixture
def hvg(monkeypatch):
    """schpf_amd.variable_genes with the host restatements in the kernels' place."""
    from schpf_amd import _lib, variable_genes
    proxy = HostLibrary(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    return variable_genes


def check_sums(found, want, N):
    e1, e2 = errors(found["residual_sum"], found["residual_sumsq"], want)
    assert e1 <= tolerance(N) and e2 <= tolerance(N)
    assert_allclose(found["residual_var"], found["residual_sumsq"] / N - (found["residual_sum"] / N) ** 2, rtol=0, atol=0)


def test_residual_variance_in_python(hvg):
    import schpf
    import schpf_amd
    from scipy.sparse import csc_matrix
    assert schpf_amd.residual_variance is hvg.residual_variance and schpf_amd.highly_variable_genes is hvg.highly_variable_genes
    assert schpf.residual_variance is hvg.residual_variance and schpf.highly_variable_genes is hvg.highly_variable_genes
    assert {"residual_variance", "highly_variable_genes"} <= set(schpf_amd.__all__)
    X = case("257x129")[0]
    N, J = X.shape
    C = csc_matrix(X)
    for M in (C, C.tocsr(), C.tocoo(), np.asarray(X)):
        found = hvg.residual_variance(M)
        assert list(found) == list(hvg.NAMES)
        check_sums(found, expected("257x129", 100.0, None), N)       # the default clip: the planted outlier is clipped
        assert_array_equal(found["cell_total"], X.sum(axis=1))
        assert_array_equal(found["gene_total"], X.sum(axis=0))
        assert found["n_distinct_totals"] == len(np.unique(X.sum(axis=1)))
        assert found["residual_sum"].dtype == found["residual_var"].dtype == np.float64 and found["gene_total"].dtype == np.int64
    unclipped = hvg.residual_variance(C, clip=np.inf)["residual_sumsq"][J - 1]
    assert unclipped > found["residual_sumsq"][J - 1] + 1000.0       # ... and without a clip it is not
    check_sums(hvg.residual_variance(C, theta=np.inf), expected("257x129", np.inf, None), N)
    check_sums(hvg.residual_variance(C, clip=2.0), expected("257x129", 100.0, 2.0), N)   # below sqrt(theta): zeros are clipped too
    check_sums(hvg.residual_variance(C, theta=np.inf, clip=2.0), expected("257x129", np.inf, 2.0), N)
    doubled = C.tocoo()
    doubled = type(doubled)((np.concatenate([doubled.data, doubled.data]), (np.concatenate([doubled.row, doubled.row]),
                                                                            np.concatenate([doubled.col, doubled.col]))), shape=X.shape)
    assert_array_equal(hvg.residual_variance(doubled)["gene_total"], 2 * X.sum(axis=0))   # duplicates are summed
    for wrong in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="theta"):
            hvg.residual_variance(C, theta=wrong)
        with pytest.raises(ValueError, match="clip"):
            hvg.residual_variance(C, clip=wrong)
    bad = C.astype(np.float64)
    assert bad.indptr[7] > bad.indptr[6]
    bad.data[int(bad.indptr[6])] = 1.5
    with pytest.raises(ValueError, match=re.escape(BAD_VALUES % 6) + "$"):
        hvg.residual_variance(bad)
    assert not hvg.residual_variance(csc_matrix((0, 4)))["residual_var"].any()


@pytest.mark.parametrize("fraction", [10, 4, 2])
def test_highly_variable_genes(hvg, fraction):
    from scipy.sparse import csr_matrix
    from schpf_amd import scHPF, qc
    X = case("257x129")[0]
    N, J = X.shape
    n_top = J // fraction
    S1, S2, absr, var, order = expected("257x129", 100.0, None)
    gap = cut_gap(var, order, n_top)
    print("J/%d: relative gap at the cut %.3g" % (fraction, gap))
    assert gap > 1e-6
    found = scHPF.variable_genes(csr_matrix(X), n_top_genes=n_top)
    assert set(found) == {"highly_variable", "rank", "residual_var", "means"}
    assert found["highly_variable"].dtype == np.bool_ and found["highly_variable"].sum() == n_top
    assert_array_equal(np.flatnonzero(found["highly_variable"]), np.sort(order[:n_top]))
    assert_array_equal(found["rank"][order[:n_top]], np.arange(n_top))
    assert sorted(found["rank"]) == list(range(J))
    # the bound of the sums carried through S2 / N - (S1 / N)^2
    assert (np.abs(found["residual_var"] - var) <= tolerance(N) * (S2 / N + 2 * np.abs(S1) * absr / N ** 2)).all()
    assert_allclose(found["means"], X.mean(axis=0), rtol=1e-15)
    picked = qc.submatrix(csr_matrix(X), genes=found["highly_variable"])       # the mask goes straight into submatrix
    assert picked.shape == (N, n_top) and (picked != csr_matrix(X)[:, np.sort(order[:n_top])]).nnz == 0


def test_ties_are_settled_by_the_gene_index(hvg):
    X = np.tile(counts(40, 5, 9), (1, 2))                            # genes j and j + 5 are the same
    found = hvg.highly_variable_genes(X, n_top_genes=3)
    assert_array_equal(found["rank"][:5] + 1, found["rank"][5:])
    assert hvg.highly_variable_genes(X, n_top_genes=0)["highly_variable"].sum() == 0
    assert hvg.highly_variable_genes(X, n_top_genes=99)["highly_variable"].all()


def test_highly_variable_genes_in_batches(hvg):
    from scipy.sparse import csr_matrix
    X = case("257x129")[0]
    N, J = X.shape
    batch = np.array(["b", "a", "c"])[np.arange(N) * 7 % 3]
    n_top = J // 4
    for label in np.unique(batch):                                    # every batch's own cut has its gap
        _, _, _, var_b, order_b = dense_reference(X[batch == label])
        assert cut_gap(var_b, order_b, n_top) > 1e-6
    order, n_batches, median, var = batch_reference(X, batch, n_top)
    found = hvg.highly_variable_genes(csr_matrix(X), n_top_genes=n_top, batch=batch)
    assert set(found) == {"highly_variable", "rank", "residual_var", "means", "n_batches", "median_rank"}
    assert_array_equal(found["n_batches"], n_batches)
    assert_array_equal(found["median_rank"][n_batches > 0], median[n_batches > 0])
    assert np.isnan(found["median_rank"][n_batches == 0]).all()
    assert_array_equal(found["rank"][order], np.arange(J))
    assert_array_equal(np.flatnonzero(found["highly_variable"]), np.sort(order[:n_top]))
    assert_allclose(found["residual_var"], var, rtol=1e-9)
    assert_allclose(found["means"], X.mean(axis=0), rtol=1e-15)
    assert 0 < (n_batches == 3).sum() < n_top                        # the rule has something to decide
    with pytest.raises(ValueError, match="one label per cell"):
        hvg.highly_variable_genes(X, batch=batch[:-1])


def test_qc_selects_genes_on_the_command_line(hvg, tmp_path):
    from scipy.io import mmread, mmwrite
    from schpf_amd import cli
    X = golden_coo(load_golden("pbmc_like_data.npz")).tocsr()
    matrix = str(tmp_path / "counts.mtx")
    mmwrite(matrix, X.tocoo(), field="integer")
    D = np.asarray(X.todense())
    genes = (D > 0).sum(axis=0) >= 5
    kept = np.flatnonzero(genes)
    n_top = len(kept) // 4
    for theta, extra in ((100.0, []), (np.inf, ["--hvg-theta", "inf"])):
        _, _, _, var, order = dense_reference(D[:, genes], theta)
        assert cut_gap(var, order, n_top) > 1e-6
        out = tmp_path / ("out%d" % len(extra))
        assert cli.main(["qc", "-i", matrix, "-o", str(out), "--min-cells", "5", "--n-top-genes", str(n_top), "--write-filtered"]
                        + extra) == 0
        assert sorted(os.listdir(str(out))) == ["cell_qc.txt", "filtered.mtx", "gene_hvg.txt", "gene_qc.txt", "kept_cells.txt",
                                                "kept_genes.txt", "qc_commandline_args.json"]
        table = np.loadtxt(str(out / "gene_hvg.txt"), skiprows=1)
        assert open(str(out / "gene_hvg.txt")).readline().split() == ["residual_var", "rank", "highly_variable"]
        assert table.shape == (X.shape[1], 3)
        assert np.isnan(table[~genes, 0]).all() and (table[~genes, 1] == -1).all() and not table[~genes, 2].any()
        assert_allclose(table[genes, 0], var, rtol=1e-9)
        assert_array_equal(table[kept[order[:n_top]], 1], np.arange(n_top))
        chosen = np.sort(kept[order[:n_top]])
        assert_array_equal(np.flatnonzero(table[:, 2]), chosen)
        assert_array_equal(np.loadtxt(str(out / "kept_genes.txt"), dtype=np.int64), chosen)
        F = mmread(str(out / "filtered.mtx")).tocsr()
        assert F.shape == (X.shape[0], n_top) and (F != X[:, chosen]).nnz == 0
        args = json.load(open(str(out / "qc_commandline_args.json")))
        assert args["n_top_genes"] == n_top and args["hvg_theta"] == theta
    # without the option the outputs and the arguments file are what they were
    plain = tmp_path / "plain"
    assert cli.main(["qc", "-i", matrix, "-o", str(plain), "--min-cells", "5"]) == 0
    assert sorted(os.listdir(str(plain))) == ["cell_qc.txt", "gene_qc.txt", "qc_commandline_args.json"]
    args = json.load(open(str(plain / "qc_commandline_args.json")))
    assert "n_top_genes" not in args and "hvg_theta" not in args
    with pytest.raises(ValueError, match="--hvg-theta belongs to --n-top-genes"):
        cli.main(["qc", "-i", matrix, "-o", str(plain), "--hvg-theta", "10"])
