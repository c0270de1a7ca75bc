"""Rank sums between pairs of groups, without a GPU: the library's serial restatement
schpf_debug_pair_rank_sums -- which the kernels are then held to bit for bit (tests/test_pair_rank_sums_gpu.py) -- is pinned
to the definition written with scipy.stats.rankdata on the cells of a ∪ b (tests/_pair_ranksum_reference.py), to
scipy.stats.mannwhitneyu and to schpf_debug_rank_sums for two groups, and the Python layer and the command line are checked
with the restatements in the kernels' place.

Bounds.  The four arrays are integers and are compared exactly; U of mannwhitneyu is a multiple of 1/2 below 2^53 and is
compared exactly as well.  The p-values are held to rtol 1e-10, the bound and the reasoning of test_rank_sums_host.py (the
same formula: 8e-16 was measured there; the margin covers erfc in the far tail on other libm builds).  The z-score without
tie correction is compared with its closed form to 1e-13 relative: two roundings of sqrt and a division."""
import functools
import json
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.stats import mannwhitneyu

from _pair_ranksum_reference import (BAD_PAIRS, CASES, NAMES, _p, all_pairs, debug_pair_rank_sums, dense_of, mixed_pairs,
                                     pair_refusals, poisson_counts, random_labels, reference_pair_rank_sums)
from _ranksum_reference import all_distinct_gene, as_csc, as_matrix, debug_rank_sums, good_call


@functools.lru_cache(maxsize=None)
def cross_check():
    """301 cells, 40 genes, 5 groups with group 2 empty and -1 present; gene 3 all zero, gene 4 all equal, gene 5 all
    distinct.  (dense matrix, labels, G), read-only."""
    D = dense_of(poisson_counts(301, 40, 7)).copy()
    D[:, 3], D[:, 4], D[:, 5] = 0.0, 2.0, all_distinct_gene(301, 3)[4]
    labels = random_labels(301, 5, seed=5, outside=0.15)
    labels[labels == 2] = 4
    D.setflags(write=False)
    labels.setflags(write=False)
    return D, labels, 5


def test_restatement_equals_the_definition_and_scipy():
    D, labels, G = cross_check()
    assert (labels == -1).any() and not (labels == 2).any()
    pairs = mixed_pairs(G)
    matrix = as_matrix(D)
    got, want = debug_pair_rank_sums(matrix, labels, G, pairs), reference_pair_rank_sums(matrix, labels, G, pairs)
    for name, a, b in zip(NAMES, got, want):
        assert a.dtype == np.int64
        assert_array_equal(a, b, err_msg=name)
    n, nexpr, u2, ties = got
    for p, (a, b) in enumerate(pairs):
        if n[a] == 0 or n[b] == 0:
            assert not u2[p].any()                                # an empty group
            continue
        for j in range(D.shape[1]):
            u = mannwhitneyu(D[labels == a, j], D[labels == b, j], method="asymptotic", use_continuity=False).statistic
            assert u2[p, j] == 2 * u
    row = {(int(a), int(b)): p for p, (a, b) in enumerate(pairs[:len(all_pairs(G))])}
    P = len(all_pairs(G))
    assert_array_equal(u2[P], u2[0])                              # the repeat of pair 0
    assert_array_equal(ties[P], ties[0])
    for extra, (b, a) in enumerate(pairs[P + 1:], start=P + 1):  # the reversed pairs
        assert_array_equal(u2[extra], 2 * n[a] * n[b] - u2[row[(int(a), int(b))]])
        assert_array_equal(ties[extra], ties[row[(int(a), int(b))]])
    assert ties[0, 5] == 0 and u2[0, 3] == n[0] * n[1]            # all distinct: no ties; all zero: every cell ties
    n_all = n[0] + n[1]
    assert ties[0, 3] == n_all ** 3 - n_all == ties[0, 4]


@pytest.mark.parametrize("case", ["one_cell_one_gene", "no_entries", "short_genes_300", "stored_zeros_and_subnormals",
                                  "near_float_max", "scaled_to_median", "all_outside"])
def test_restatement_on_the_shapes_of_the_rank_sums(case):
    matrix, labels, G = CASES[case]()
    pairs = mixed_pairs(G) if G > 1 else np.zeros((0, 2), np.int32)
    if case == "one_cell_one_gene":
        G, pairs = 2, np.array([[0, 1], [1, 0]], np.int32)        # the second group is empty
    for name, a, b in zip(NAMES, debug_pair_rank_sums(matrix, labels, G, pairs), reference_pair_rank_sums(matrix, labels, G, pairs)):
        assert_array_equal(a, b, err_msg=name)


def test_two_groups_are_the_rank_sums_of_section_19():
    """G = 2 and no cell outside: the pair is all the cells, so u2 = rank2[0] - n_0 (n_0 + 1) and the ties are the ties."""
    matrix = poisson_counts(301, 40, 7)
    labels = random_labels(301, 2, seed=3)
    n, zeros, ties, nexpr, rank2 = debug_rank_sums(matrix, labels, 2)
    pn, pnexpr, u2, pties = debug_pair_rank_sums(matrix, labels, 2, [[0, 1]])
    assert_array_equal(pn, n)
    assert_array_equal(pnexpr, nexpr)
    assert_array_equal(u2[0], rank2[0] - n[0] * (n[0] + 1))
    assert_array_equal(pties[0], ties)


def test_refusals_leave_the_outputs_untouched():
    from schpf_amd import _lib
    lib = _lib.load()
    seen = set()
    for message, matrix, labels, G, pairs in pair_refusals():
        N, J, indptr, indices, data = matrix
        size = 3 if not 0 < G < 100 else G                       # outputs of the good call's size: a refused call reads no G
        if isinstance(pairs, tuple):                             # a count of pairs alone: refused before pairs is read
            P, pairs = pairs[0], all_pairs(3)
        else:
            P = len(pairs)
        rows = max(min(P, 8), 1)
        out = [np.full(s, -7, np.int64) for s in (size, size * J, rows * J, rows * J)]
        assert lib.schpf_debug_pair_rank_sums(N, J, _p(indptr), _p(indices), _p(data), _p(labels), G, _p(pairs), P,
                                              *[_p(a) for a in out]) != 0
        assert lib.schpf_last_error().decode() == message
        assert all((a == -7).all() for a in out)
        seen.add(message.split(";")[0])
    assert len(seen) == 10          # ncells, ngroups, G * J, npairs twice; indptr, cell ids, values, labels; pairs
    with pytest.raises(ValueError, match=r"offending pair 1$"):
        debug_pair_rank_sums(as_matrix(dense_of(poisson_counts(20, 3, 1))), np.zeros(20, np.int32), 2, [[0, 1], [1, 1]])


def test_nothing_to_do_succeeds():
    from schpf_amd import _lib
    lib = _lib.load()
    pairs = all_pairs(3)
    for N, J in ((0, 5), (5, 0), (0, 0)):
        out = [np.full(max(s, 1), -7, np.int64) for s in (3, 3 * J, 3 * J, 3 * J)]
        assert lib.schpf_debug_pair_rank_sums(N, J, None, None, None, None, 3, None, 3, *[_p(a) for a in out]) == 0   # reads no input
        assert not out[0].any() and all(not a[:3 * J].any() for a in out[1:])
        assert lib.schpf_debug_pair_rank_sums(N, J, None, None, None, None, 3, _p(pairs), 3, None, None, None, None) == 0
    N, J, indptr, indices, data, labels, G = good_call()         # no pairs: n and nexpr are those of the rank sums
    n, nexpr, u2, ties = debug_pair_rank_sums((N, J, indptr, indices, data), labels, G, np.zeros((0, 2), np.int32), fill=-7)
    want = debug_rank_sums((N, J, indptr, indices, data), labels, G)
    assert_array_equal(n, want[0])
    assert_array_equal(nexpr, want[3])
    assert u2.shape == ties.shape == (0, J)
    out = [np.full(s, -7, np.int64) for s in (G, G * J)]
    assert lib.schpf_debug_pair_rank_sums(N, J, _p(indptr), _p(indices), _p(data), _p(labels), G, None, 0, *[_p(a) for a in out],
                                          None, None) == 0
    assert_array_equal(out[0], want[0])


# ------------------------------------------------------------------------------------------- the Python layer and the CLI
HOSTED = ("schpf_rank_sums", "schpf_pair_rank_sums", "schpf_group_stats", "schpf_cluster_graph", "schpf_knn", "schpf_knn_graph",
          "schpf_louvain")


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
def markers(monkeypatch):
    """schpf_amd.markers with the host restatements in the kernels' place."""
    from schpf_amd import _lib, markers as mk
    proxy = HostLibrary(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    return mk


def test_pair_rank_sums_in_python(markers):
    import schpf
    import schpf_amd
    assert schpf_amd.pair_rank_sums is markers.pair_rank_sums and schpf_amd.rank_genes_pairs is markers.rank_genes_pairs
    assert schpf.pair_rank_sums is markers.pair_rank_sums and schpf.rank_genes_pairs is markers.rank_genes_pairs
    assert {"pair_rank_sums", "rank_genes_pairs"} <= set(schpf_amd.__all__)
    D, labels, G = cross_check()
    matrix = as_matrix(D)
    C = as_csc(matrix)
    want = debug_pair_rank_sums(matrix, labels, G, all_pairs(G))
    for X in (C, C.tocsr(), C.tocoo(), D):
        got = markers.pair_rank_sums(X, labels)
        assert list(got) == list(NAMES) + ["pairs"]
        assert got["pairs"].dtype == np.int32
        assert_array_equal(got["pairs"], all_pairs(G))
        for name, b in zip(NAMES, want):
            assert isinstance(got[name], np.ndarray) and got[name].dtype == np.int64
            assert_array_equal(got[name], b)
    mine = [[4, 0], [0, 4], [4, 0]]
    got = markers.pair_rank_sums(C, labels.astype(np.int64), pairs=mine, ngroups=7)
    assert got["nexpr"].shape == (7, 40) and got["u2"].shape == (3, 40) and got["pairs"].tolist() == mine
    assert_array_equal(got["u2"][0], got["u2"][2])
    assert_array_equal(got["u2"][0] + got["u2"][1], np.full(40, 2 * got["n"][0] * got["n"][4]))
    assert markers.pair_rank_sums(C, labels, pairs=[])["u2"].shape == (0, 40)
    for wrong, row in (([[0, 1], [1, 1]], 1), ([[0, 5]], 0), ([[-1, 2]], 0)):
        with pytest.raises(ValueError, match=(BAD_PAIRS % row).replace("[", r"\[").replace(")", r"\)") + "$"):
            markers.pair_rank_sums(C, labels, pairs=wrong)
    with pytest.raises(ValueError, match="rows"):
        markers.pair_rank_sums(C, labels, pairs=[0, 1, 2])
    with pytest.raises(ValueError, match='"all"'):
        markers.pair_rank_sums(C, labels, pairs="neighbours")
    bad = C.copy()
    bad.data[int(bad.indptr[5])] = -1.0
    with pytest.raises(ValueError, match="values must be finite and >= 0; offending gene 5$"):
        markers.pair_rank_sums(bad, labels)


def test_pvalues_against_mannwhitneyu(markers):
    from scipy.sparse import csr_matrix
    D, labels, G = cross_check()
    found = markers.rank_genes_pairs(csr_matrix(D), labels)
    pairs = all_pairs(G)
    assert set(found) == set(markers.PAIR_STATISTICS) | {"n", "pairs"}
    assert_array_equal(found["pairs"], pairs)
    worst = 0.0
    for p, (a, b) in enumerate(pairs):
        if 2 in (a, b):                                           # an empty group
            assert all(np.isnan(found[name][p]).all() for name in ("scores", "pvals", "pvals_adj"))
            continue
        for j in range(D.shape[1]):
            if j in (3, 4):       # every cell ties: no variance.  scipy divides by it, here the score is 0
                assert found["scores"][p, j] == 0.0 and found["pvals"][p, j] == 1.0
                continue
            want = mannwhitneyu(D[labels == a, j], D[labels == b, j], method="asymptotic", use_continuity=False).pvalue
            worst = max(worst, abs(found["pvals"][p, j] / want - 1))
            assert_allclose(found["pvals"][p, j], want, rtol=1e-10, atol=0)
    print("largest relative difference to mannwhitneyu: %.3g" % worst)
    for name in markers.PAIR_STATISTICS:
        assert found[name].shape == (len(pairs), D.shape[1]) and found[name].dtype == np.float64
    p = 2                                                         # (0, 3)
    assert pairs[p].tolist() == [0, 3]
    assert_allclose(found["mean_a"][p], D[labels == 0].mean(axis=0, dtype=np.float64), rtol=1e-12)
    assert_allclose(found["mean_b"][p], D[labels == 3].mean(axis=0, dtype=np.float64), rtol=1e-12)
    assert_allclose(found["pct_a"][p], (D[labels == 0] > 0).mean(axis=0), rtol=1e-15)
    assert_allclose(found["pct_b"][p], (D[labels == 3] > 0).mean(axis=0), rtol=1e-15)
    assert_allclose(found["logfoldchanges"], np.log2((found["mean_a"] + 1e-9) / (found["mean_b"] + 1e-9)), rtol=1e-15, equal_nan=True)
    for p in range(len(pairs)):                                   # Benjamini-Hochberg within a pair
        assert_array_equal(found["pvals_adj"][p], markers.benjamini_hochberg(found["pvals"][p]))


def test_derived_numbers(markers):
    from scipy.sparse import csc_matrix
    D, labels, G = cross_check()
    C = csc_matrix(D)
    n, nexpr, u2, ties = debug_pair_rank_sums(as_matrix(D), labels, G, all_pairs(G))
    plain = markers.rank_genes_pairs(C, labels, tie_correct=False)
    for p, (a, b) in enumerate(all_pairs(G)):
        if 2 in (a, b):
            continue
        both = n[a] + n[b]
        want = (u2[p] / 2.0 - n[a] * n[b] / 2.0) / np.sqrt(n[a] * n[b] * (both + 1) / 12.0)
        assert_allclose(plain["scores"][p], want, rtol=1e-13, atol=0)
    # reference=r: the pairs (g, r) as (G, J), NaN in row r (and in the row of the empty group)
    r = 3
    against = markers.rank_genes_groups(C, labels, reference=r)
    others = [g for g in range(G) if g != r]
    want = markers.rank_genes_pairs(C, labels, pairs=[[g, r] for g in others])
    assert set(against) == set(markers.PAIR_STATISTICS) | {"n"}
    for name in markers.PAIR_STATISTICS:
        assert against[name].shape == (G, D.shape[1])
        assert np.isnan(against[name][r]).all()
        assert_array_equal(against[name][others], want[name])
    assert np.isnan(against["scores"][2]).all() and np.isfinite(against["scores"][[0, 1, 4]]).all()
    assert_array_equal(against["n"], n)
    with pytest.raises(ValueError, match="reference must be a group"):
        markers.rank_genes_groups(C, labels, reference=G)
    plain_groups = markers.rank_genes_groups(C, labels)         # reference=None: one against the rest, as before
    assert set(plain_groups) == set(markers.STATISTICS) | {"n"}
    # a matrix scaled to a target sum: ranked as float32, the means from a float64 product
    scaled = markers._scaled(C, 1e4)
    found = markers.rank_genes_pairs(C, labels, target_sum=1e4)
    sums = markers.pair_rank_sums(scaled, labels)
    first = sums["pairs"][:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        assert_allclose(found["pct_a"], sums["nexpr"][first] / sums["n"][first][:, None], rtol=1e-15, equal_nan=True)
    assert not np.array_equal(found["scores"], markers.rank_genes_pairs(C, labels)["scores"])
    assert_allclose(found["mean_a"][2], np.asarray(scaled.todense(), dtype=np.float64)[labels == 0].mean(axis=0), rtol=1e-12)


def toy_model(n_cells=60, n_genes=60, K=3):
    import schpf_amd
    rng = np.random.RandomState(0)
    gam = lambda shape: schpf_amd.HPF_Gamma(rng.gamma(1.0, 1.0, shape), rng.gamma(1.0, 1.0, shape) + 0.5)  # noqa: E731
    model = schpf_amd.scHPF(K)
    model.xi, model.theta = gam((n_cells,)), gam((n_cells, K))
    model.eta, model.beta = gam((n_genes,)), gam((n_genes, K))
    return model


def neighbour_pairs(model, labels, k):
    count = np.asarray(model.cluster_graph(k=k, labels=labels)["count"])
    G = count.shape[0]
    return np.array([[a, b] for a in range(G) for b in range(a + 1, G) if count[a, b] > 0 or count[b, a] > 0], np.int32).reshape(-1, 2)


def test_model_pair_markers(markers):
    model = toy_model()
    X = as_csc(poisson_counts(60, 60, 41, rate=1.0)).tocoo()
    labels = (np.arange(60) * 7 % 60) // 12                       # 5 clusters of my own
    found = model.pair_markers(X, labels=labels, k=5)
    pairs = neighbour_pairs(model, labels, 5)
    assert len(pairs) > 0
    assert_array_equal(found["pairs"], pairs)
    want = markers.rank_genes_pairs(X, labels, pairs=pairs)
    for name in markers.PAIR_STATISTICS + ("n",):
        assert_array_equal(found[name], want[name])
    everything = model.pair_markers(X, labels=labels, pairs="all", tie_correct=False)
    assert_array_equal(everything["scores"], markers.rank_genes_pairs(X, labels, tie_correct=False)["scores"])
    assert model.pair_markers(X, labels=labels, pairs=[[1, 0]])["scores"].shape == (1, 60)
    clustered = model.pair_markers(X, k=5)                        # labels=None: the clusters of `markers`
    mine = model.clusters(k=5)
    assert_array_equal(clustered["pairs"], neighbour_pairs(model, mine, 5))
    assert_array_equal(clustered["scores"], markers.rank_genes_pairs(X, mine, pairs=clustered["pairs"])["scores"])


def test_score_pair_markers_on_the_command_line(markers, tmp_path, monkeypatch):
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
    common = ["score", "-m", path, "-i", matrix, "-g", genefile, "--knn", "5", "--knn-graph", "jaccard", "--clusters", "--markers"]
    assert cli.main(common + ["-o", str(tmp_path / "plain")]) == 0
    labels = model.clusters(k=5)
    new = {"pair_marker_pairs.txt", "pair_marker_scores.txt", "pair_marker_pvals_adj.txt", "ranked_pair_markers.txt"}
    for which in ("all", "neighbors"):
        out = tmp_path / which
        assert cli.main(common + ["-o", str(out), "--marker-pairs", which]) == 0
        assert set(os.listdir(str(out))) - set(os.listdir(str(tmp_path / "plain"))) == new
        pairs = all_pairs(int(labels.max()) + 1) if which == "all" else neighbour_pairs(model, labels, 5)
        want = markers.rank_genes_pairs(X, labels, pairs=pairs)
        assert_array_equal(np.loadtxt(str(out / "pair_marker_pairs.txt"), delimiter="\t", dtype=int, ndmin=2), pairs)
        scores = np.loadtxt(str(out / "pair_marker_scores.txt"), delimiter="\t", ndmin=2)
        assert scores.shape == (60, len(pairs)) and len(pairs) > 0
        assert_allclose(scores, want["scores"].T, rtol=1e-15)
        assert_allclose(np.loadtxt(str(out / "pair_marker_pvals_adj.txt"), delimiter="\t", ndmin=2), want["pvals_adj"].T, rtol=1e-15)
        ranked = np.loadtxt(str(out / "ranked_pair_markers.txt"), delimiter="\t", dtype=str, ndmin=2)
        assert ranked.shape == scores.shape
        assert ranked[0, 0] == "gene%d" % np.argsort(want["scores"][0])[::-1][0]
        assert json.load(open(str(out / "score_commandline_args.json")))["marker_pairs"] == which
    # without the option the output set and the arguments file are what they were
    assert "marker_pairs" not in json.load(open(str(tmp_path / "plain" / "score_commandline_args.json")))
    assert cli.main(common[:5] + common[7:] + ["-o", str(tmp_path / "bare"), "--marker-pairs", "all"]) == 0
    assert "ranked_pair_markers.txt" not in os.listdir(str(tmp_path / "bare"))     # no gene names, no ranked names
    with pytest.raises((ValueError, SystemExit)):                                  # without --markers
        cli.main(common[:-1] + ["-o", str(tmp_path / "bad"), "--marker-pairs", "all"])
    with pytest.raises((ValueError, SystemExit)):                                  # without --clusters
        cli.main(["score", "-m", path, "-i", matrix, "-o", str(tmp_path / "bad2"), "--knn", "5", "--knn-graph", "jaccard",
                  "--marker-pairs", "all"])
