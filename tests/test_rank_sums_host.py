"""Wilcoxon rank sums per gene and group, without a GPU: the library's serial restatement
schpf_debug_rank_sums -- which the kernels are then held to bit for bit (tests/test_rank_sums_gpu.py) -- is pinned to the
definition written with scipy.stats.rankdata (tests/_ranksum_reference.py) and to scipy.stats.mannwhitneyu, and the Python
layer and the command line are checked with the restatement in the kernels' place.

Bounds.  The five arrays are integers and are compared exactly; U of mannwhitneyu is a multiple of 1/2 below 2^53 and is
compared exactly as well.  The p-values are held to rtol 1e-10: 8e-16 was measured, the margin covers erfc in the far tail on
other libm builds.  The z-score without tie correction is compared with its closed form to 1e-13 relative: two roundings
of sqrt and a division."""
import functools
import json
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.stats import mannwhitneyu

from _ranksum_reference import (CASES, NAMES, _p, all_distinct_gene, as_csc, as_matrix, debug_rank_sums, dense_gene_case, dense_of,
                                good_call, poisson_counts, random_labels, reference_rank_sums, refusals)


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_equals_the_definition(case):
    matrix, labels, G = CASES[case]()
    got, want = debug_rank_sums(matrix, labels, G), reference_rank_sums(matrix, labels, G)
    for name, a, b in zip(NAMES, got, want):
        assert a.dtype == np.int64
        assert_array_equal(a, b, err_msg=name)
    N, J = matrix[0], matrix[1]
    n, zeros, ties, nexpr, rank2 = got
    assert n.sum() == (np.asarray(labels) >= 0).sum()
    assert ((0 <= zeros) & (zeros <= N)).all() and (nexpr.sum(axis=0) <= N - zeros).all()
    if case == "one_cell_one_gene":
        assert [a.tolist() for a in got] == [[1], [0], [0], [[1]], [[2]]]
    if case == "no_entries":
        assert (zeros == N).all() and (ties == N ** 3 - N).all() and not nexpr.any() and (rank2 == n[:, None] * (N + 1)).all()
    if case == "empty_group_and_outside":
        assert n[1] == 0 and not nexpr[1].any() and not rank2[1].any() and (np.asarray(labels) == -1).any()
    if case == "all_outside":
        assert not n.any() and not nexpr.any() and not rank2.any() and zeros.min() < N
    if case == "stored_zeros_and_subnormals":
        data = matrix[4]
        assert (data == 0).any() and np.signbit(data[data == 0]).any() and ((data > 0) & (data < 1e-38)).any()
    if (np.asarray(labels) >= 0).all():           # every cell in a group: the ranks 1 .. N, twice
        assert (rank2.sum(axis=0) == N * (N + 1)).all()


def test_a_run_of_70001_and_all_distinct():
    matrix, labels, G = dense_gene_case()
    got, want = debug_rank_sums(matrix, labels, G), reference_rank_sums(matrix, labels, G)
    for name, a, b in zip(NAMES, got, want):
        assert_array_equal(a, b, err_msg=name)
    N = matrix[0]
    assert got[1][0] == 0 and got[2][0] == N ** 3 - N and (got[4][:, 0] == got[0] * (N + 1)).all()    # all tie: the mean rank
    assert got[1][2] == 0 and got[2][2] == 0                                                        # no tie at all


@functools.lru_cache(maxsize=None)
def cross_check():
    """N = 301, 40 genes, 5 groups with one empty, label -1 present, an all-zero, an all-equal and an all-distinct column."""
    N, J, G = 301, 40, 5
    D = dense_of(poisson_counts(N, J, 21, rate=1.5))
    D[:, 3] = 0.0
    D[:, 4] = 2.0
    D[:, 5] = dense_of(all_distinct_gene(N, 22))[:, 0]
    labels = random_labels(N, G, 23, outside=0.1)
    labels[labels == 2] = 4
    assert (labels == -1).any() and not (labels == 2).any()
    D.setflags(write=False)
    labels.setflags(write=False)
    return D, labels, G


def test_twice_u_of_mannwhitneyu_exactly():
    D, labels, G = cross_check()
    n, zeros, ties, nexpr, rank2 = debug_rank_sums(as_matrix(D), labels, G)
    for g in range(G):
        if n[g] == 0:
            continue
        for j in range(D.shape[1]):
            u = mannwhitneyu(D[labels == g, j], D[labels != g, j], method="asymptotic", use_continuity=False).statistic
            assert rank2[g, j] - n[g] * (n[g] + 1) == 2 * u


@pytest.fixture
def markers(monkeypatch):
    """schpf_amd.markers with the host restatement in the place of schpf_rank_sums."""
    from schpf_amd import markers as mk

    def hook(ncells, ngenes, indptr, indices, data, labels, ngroups, device):
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32 and labels.dtype == np.int32
        assert all(a.flags.c_contiguous for a in (indptr, indices, data, labels))
        return debug_rank_sums((ncells, ngenes, indptr, indices, data), labels, ngroups)

    monkeypatch.setattr(mk, "_rank_sums_host", hook)
    return mk


def test_pvalues_against_mannwhitneyu(markers):
    from scipy.sparse import csr_matrix
    D, labels, G = cross_check()
    found = markers.rank_genes_groups(csr_matrix(D), labels)
    assert set(found) == set(markers.STATISTICS) | {"n"}
    worst = 0.0
    for g in range(G):
        if found["n"][g] == 0:
            assert np.isnan(found["scores"][g]).all() and np.isnan(found["pvals"][g]).all() and np.isnan(found["pvals_adj"][g]).all()
            continue
        for j in range(D.shape[1]):
            if j in (3, 4):       # every cell ties: no variance.  scipy divides by it, here the score is 0
                assert found["scores"][g, j] == 0.0 and found["pvals"][g, j] == 1.0
                continue
            p = mannwhitneyu(D[labels == g, j], D[labels != g, j], method="asymptotic", use_continuity=False).pvalue
            worst = max(worst, abs(found["pvals"][g, j] / p - 1))
            assert_allclose(found["pvals"][g, j], p, rtol=1e-10, atol=0)
    print("largest relative difference to mannwhitneyu: %.3g" % worst)
    for name in markers.STATISTICS:
        assert found[name].shape == (G, D.shape[1]) and found[name].dtype == np.float64
    inside = labels == 0
    assert_allclose(found["mean_in"][0], D[inside].mean(axis=0, dtype=np.float64), rtol=1e-12)
    assert_allclose(found["mean_out"][0], D[~inside].mean(axis=0, dtype=np.float64), rtol=1e-12)
    assert_allclose(found["pct_in"][0], (D[inside] > 0).mean(axis=0), rtol=1e-15)
    assert_allclose(found["pct_out"][0], (D[~inside] > 0).mean(axis=0), rtol=1e-15)
    assert_allclose(found["logfoldchanges"], np.log2((found["mean_in"] + 1e-9) / (found["mean_out"] + 1e-9)), rtol=1e-15, equal_nan=True)
    assert_array_equal(found["pvals_adj"][0], markers.benjamini_hochberg(found["pvals"][0]))


def test_without_tie_correction_is_the_closed_form(markers):
    from scipy.sparse import csc_matrix
    D, labels, G = cross_check()
    N = D.shape[0]
    found = markers.rank_genes_groups(csc_matrix(D), labels, tie_correct=False)
    n, zeros, ties, nexpr, rank2 = debug_rank_sums(as_matrix(D), labels, G)
    for g in (0, 1, 3, 4):
        want = (rank2[g] / 2.0 - n[g] * (N + 1) / 2.0) / np.sqrt(n[g] * (N - n[g]) * (N + 1) / 12.0)
        assert_allclose(found["scores"][g], want, rtol=1e-13, atol=0)
    assert np.isnan(found["scores"][2]).all()
    everyone = markers.rank_genes_groups(csc_matrix(D), np.zeros(N, int))          # a group that holds all the cells
    assert np.isnan(everyone["scores"]).all() and everyone["n"].tolist() == [N]


def test_benjamini_hochberg_by_hand():
    from schpf_amd.markers import benjamini_hochberg
    p = np.array([0.01, 0.04, 0.03, 0.005, 0.5])
    # sorted 0.005 0.01 0.03 0.04 0.5, times 5 / rank: 0.025 0.025 0.05 0.05 0.5, already monotone
    assert_allclose(benjamini_hochberg(p), [0.025, 0.05, 0.05, 0.025, 0.5], rtol=1e-15)
    # 0.02 0.03 0.031 -> 0.06 0.045 0.031: made monotone from the largest down
    assert_allclose(benjamini_hochberg([0.03, 0.02, 0.031]), [0.031, 0.031, 0.031], rtol=1e-15)
    assert_allclose(benjamini_hochberg([[0.9, 0.8], [0.001, 1.0]]), [[0.9, 0.9], [0.002, 1.0]], rtol=1e-15)
    assert np.isnan(benjamini_hochberg([np.nan, np.nan])).all() and benjamini_hochberg(np.zeros((3, 0))).shape == (3, 0)


def test_monotone_maps_change_nothing():
    matrix, labels, G = CASES["empty_group_and_outside"]()
    want = debug_rank_sums(matrix, labels, G)
    N, J, indptr, indices, data = matrix
    for mapped in (data * 3.0, np.sqrt(data), np.expm1(data), data * 1e-38, data * 1e37):
        mapped = mapped.astype(np.float32)
        assert (np.diff(np.unique(mapped)) > 0).all() and len(np.unique(mapped)) == len(np.unique(data))
        for a, b in zip(debug_rank_sums((N, J, indptr, indices, mapped), labels, G), want):
            assert_array_equal(a, b)


def test_relabelling_permutes_the_rows():
    matrix, labels, G = CASES["empty_group_and_outside"]()
    want = debug_rank_sums(matrix, labels, G)
    perm = np.array([2, 0, 3, 1])
    moved = np.where(labels >= 0, perm[np.maximum(labels, 0)], -1).astype(np.int32)
    got = debug_rank_sums(matrix, moved, G)
    assert_array_equal(got[0][perm], want[0])
    assert_array_equal(got[1], want[1])
    assert_array_equal(got[2], want[2])
    assert_array_equal(got[3][perm], want[3])
    assert_array_equal(got[4][perm], want[4])
    wider = debug_rank_sums(matrix, labels, G + 2)                                 # more groups: empty rows behind
    assert_array_equal(wider[4][:G], want[4])
    assert not wider[4][G:].any() and not wider[0][G:].any()


def test_refusals_leave_the_outputs_untouched():
    from schpf_amd import _lib
    lib = _lib.load()
    for message, matrix, labels, G in refusals(*good_call()):
        N, J, indptr, indices, data = matrix
        size = 3 if not 0 < G < 100 else G                      # outputs of the good call's size: a refused call reads no G
        out = [np.full(s, -7, np.int64) for s in (size, J, J, size * J, size * J)]
        assert lib.schpf_debug_rank_sums(N, J, _p(indptr), _p(indices), _p(data), _p(labels), G, *[_p(a) for a in out]) != 0
        assert lib.schpf_last_error().decode() == message
        assert all((a == -7).all() for a in out)
        if size == G and 0 <= N < 1 << 21:                       # through the checked call: a ValueError
            with pytest.raises(ValueError, match=message.split(";")[0].replace("[", r"\[").replace(")", r"\)")):
                debug_rank_sums(matrix, labels, G)


def test_no_cells_or_no_genes():
    from schpf_amd import _lib
    lib = _lib.load()
    for N, J in ((0, 5), (5, 0), (0, 0)):
        out = [np.full(max(s, 1), -7, np.int64) for s in (3, J, J, 3 * J, 3 * J)]
        assert lib.schpf_debug_rank_sums(N, J, None, None, None, None, 3, *[_p(a) for a in out]) == 0        # reads no input
        assert not out[0].any() and all(not a[:s].any() for a, s in zip(out[1:], (J, J, 3 * J, 3 * J)))
        assert lib.schpf_debug_rank_sums(N, J, None, None, None, None, 3, None, None, None, None, None) == 0


# ------------------------------------------------------------------------------------------- the Python layer and the CLI
def test_rank_sums_in_python(markers):
    import schpf_amd
    assert schpf_amd.rank_sums is markers.rank_sums and schpf_amd.rank_genes_groups is markers.rank_genes_groups
    assert {"rank_sums", "rank_genes_groups"} <= set(schpf_amd.__all__)
    matrix, labels, G = CASES["empty_group_and_outside"]()
    want = debug_rank_sums(matrix, labels, G)
    C = as_csc(matrix)
    for X in (C, C.tocsr(), C.tocoo()):
        got = markers.rank_sums(X, labels)
        assert list(got) == list(NAMES)
        for name, b in zip(NAMES, want):
            assert isinstance(got[name], np.ndarray) and got[name].dtype == np.int64
            assert_array_equal(got[name], b)
    doubled = C.tocoo()                                          # duplicates are summed, cells in any order: on a copy
    from scipy.sparse import coo_matrix
    twice = coo_matrix((np.concatenate([doubled.data, doubled.data])[::-1], (np.concatenate([doubled.row, doubled.row])[::-1],
                                                                          np.concatenate([doubled.col, doubled.col])[::-1])),
                       shape=C.shape)
    keep = twice.data.copy()
    got = markers.rank_sums(twice, labels.astype(np.int64), ngroups=G)
    for name, b in zip(NAMES, want):                             # twice every value: a monotone map
        assert_array_equal(got[name], b)
    assert_array_equal(twice.data, keep)
    assert twice.nnz == 2 * C.nnz
    wider = markers.rank_sums(C, labels, ngroups=6)
    assert wider["rank2"].shape == (6, 40) and not wider["rank2"][4:].any()
    bad = C.copy()
    bad.data[int(bad.indptr[5])] = -1.0
    with pytest.raises(ValueError, match="values must be finite and >= 0; offending gene 5$"):
        markers.rank_sums(bad, labels)
    wrong = labels.copy()
    wrong[9] = -2
    with pytest.raises(ValueError, match=r"labels must be in \[-1, ngroups\); offending cell 9$"):
        markers.rank_sums(C, wrong)
    with pytest.raises(ValueError, match="one label per cell"):
        markers.rank_sums(C, labels[:10])
    with pytest.raises(ValueError, match=r"ncells must be in \[0, 2\^21\)"):
        from scipy.sparse import csc_matrix
        markers.rank_sums(csc_matrix((1 << 21, 1), dtype=np.float32), np.zeros(1 << 21, np.int32))


def test_target_sum(markers):
    matrix, labels, G = CASES["empty_group_and_outside"]()
    C = as_csc(matrix)
    depth = np.asarray(C.sum(axis=1)).ravel()
    for target in (1e4, "median"):
        scaled = markers._scaled(C, target)
        want_total = np.median(depth) if target == "median" else target
        assert scaled.dtype == np.float32
        assert_allclose(np.asarray(scaled.sum(axis=1)).ravel()[depth > 0], want_total, rtol=1e-5)
        found = markers.rank_genes_groups(C, labels, target_sum=target)
        plain = markers.rank_genes_groups(scaled, labels)
        for name in markers.STATISTICS:
            assert_array_equal(found[name], plain[name])
    assert not np.array_equal(found["scores"], markers.rank_genes_groups(C, labels)["scores"])


def toy_model(n_cells=60, n_genes=60, K=3):
    import schpf_amd
    rng = np.random.RandomState(0)
    gam = lambda shape: schpf_amd.HPF_Gamma(rng.gamma(1.0, 1.0, shape), rng.gamma(1.0, 1.0, shape) + 0.5)  # noqa: E731
    model = schpf_amd.scHPF(K)
    model.xi, model.theta = gam((n_cells,)), gam((n_cells, K))
    model.eta, model.beta = gam((n_genes,)), gam((n_genes, K))
    return model


@pytest.fixture
def neighbors(monkeypatch):
    """schpf_amd.neighbors with the host restatements in the place of schpf_knn, schpf_knn_graph and schpf_louvain."""
    from schpf_amd import neighbors as nb
    from _graph_reference import debug_graph
    from _knn_reference import debug_knn
    from _louvain_reference import debug_louvain
    monkeypatch.setattr(nb, "_louvain_host", lambda indptr, indices, data, gamma, device: debug_louvain((indptr, indices, data), gamma))
    monkeypatch.setattr(nb, "_graph_host", lambda method, idx, dist, device: debug_graph(idx, dist, method)[:3])
    monkeypatch.setattr(nb, "_search_host", lambda query, ref, k, self_first, device: debug_knn(query, ref, k, self_first))
    return nb


def test_model_markers(markers, neighbors):
    model = toy_model()
    X = as_csc(poisson_counts(60, 60, 41, rate=1.0)).tocoo()
    found = model.markers(X, k=5)
    labels = model.clusters(k=5)
    want = markers.rank_genes_groups(X, labels)
    for name in markers.STATISTICS + ("n",):
        assert_array_equal(found[name], want[name])
    assert found["scores"].shape == (labels.max() + 1, 60)
    mine = np.arange(60) % 2
    assert_array_equal(model.markers(X, labels=mine, tie_correct=False)["scores"],
                       markers.rank_genes_groups(X, mine, tie_correct=False)["scores"])


def test_score_markers_on_the_command_line(markers, neighbors, tmp_path, monkeypatch):
    import schpf_amd
    from scipy.io import mmwrite
    from schpf_amd import cli, loss
    model = toy_model()
    path, matrix, genefile = str(tmp_path / "model.joblib"), str(tmp_path / "counts.mtx"), str(tmp_path / "genes.txt")
    schpf_amd.save_model(model, path)
    X = as_csc(poisson_counts(60, 60, 41, rate=1.0)).tocoo()
    mmwrite(matrix, X, field="integer")
    with open(genefile, "w") as fh:
        fh.write("".join("ENS%03d\tgene%d\n" % (j, j) for j in range(60)))
    # the per-row losses of -i need the GPU: not what this test is about
    for name in ("cellmean_negative_pois_llh", "genemean_negative_pois_llh"):
        monkeypatch.setattr(loss, name, lambda data, theta=None, beta=None: np.zeros(60))
    common = ["score", "-m", path, "-i", matrix, "-g", genefile, "--knn", "5", "--knn-graph", "jaccard", "--clusters"]
    assert cli.main(common + ["-o", str(tmp_path / "plain")]) == 0
    out = tmp_path / "marked"
    assert cli.main(common + ["-o", str(out), "--markers"]) == 0
    assert (set(os.listdir(str(out))) - set(os.listdir(str(tmp_path / "plain")))
            == {"marker_scores.txt", "marker_pvals_adj.txt", "ranked_markers.txt"})
    labels = model.clusters(k=5)
    want = markers.rank_genes_groups(X, labels)
    scores = np.loadtxt(str(out / "marker_scores.txt"), delimiter="\t", ndmin=2)
    assert scores.shape == (60, labels.max() + 1)
    assert_allclose(scores, want["scores"].T, rtol=1e-15)
    assert_allclose(np.loadtxt(str(out / "marker_pvals_adj.txt"), delimiter="\t", ndmin=2), want["pvals_adj"].T, rtol=1e-15)
    ranked = np.loadtxt(str(out / "ranked_markers.txt"), delimiter="\t", dtype=str, ndmin=2)
    assert ranked.shape == scores.shape
    assert ranked[0, 0] == "gene%d" % np.argsort(want["scores"][0])[::-1][0]
    assert json.load(open(str(out / "score_commandline_args.json")))["markers"] is True
    # without the option the output set and the arguments file are what they were
    assert "markers" not in json.load(open(str(tmp_path / "plain" / "score_commandline_args.json")))
    assert cli.main(common[:5] + ["-o", str(tmp_path / "bare"), "--knn", "5", "--knn-graph", "jaccard", "--clusters", "--markers"]) == 0
    assert "ranked_markers.txt" not in os.listdir(str(tmp_path / "bare"))          # no gene names, no ranked names
    with pytest.raises((ValueError, SystemExit)):                                  # without -i
        cli.main(["score", "-m", path, "-o", str(tmp_path / "bad"), "--knn", "5", "--knn-graph", "jaccard", "--clusters",
                  "--markers"])
    with pytest.raises((ValueError, SystemExit)):                                  # without --clusters
        cli.main(["score", "-m", path, "-i", matrix, "-o", str(tmp_path / "bad2"), "--knn", "5", "--knn-graph", "jaccard",
                  "--markers"])
