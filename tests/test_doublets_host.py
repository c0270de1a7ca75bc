"""Simulated doublets without a GPU: the draw of the parents and the host restatement of the pair sum
against the definition restated in NumPy (tests/_doublet_reference.py), the refusals with their messages, Scrublet's score
on values worked out by hand, and the arguments of `scHPF score --doublets`."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from _doublet_reference import (LONG, LONGER, MESSAGES, PIECE, _p, debug_rows, draw_parents, host_parents, kernel_matrix,
                                pair_sums, scrublet, spoiled)

SEEDS = (0, 0x1234567887654321)


@pytest.fixture(scope="module")
def case():
    X, parents = kernel_matrix()
    want = pair_sums(X, parents)
    for a in want:
        a.setflags(write=False)
    return X, parents, want


@pytest.mark.parametrize("ncells", [1, 2, 3, 257, 2 ** 31 - 1])
def test_parents_equal_the_numpy_draw(ncells):
    for seed in SEEDS:
        # from row 0, and across the rows 2^32 - 3 .. 2^32 + 4: the counter's second word takes over
        for first, n_sim in ((0, 300), (2 ** 32 - 3, 8)):
            got = host_parents(first, n_sim, ncells, seed)
            assert_array_equal(got, draw_parents(first, n_sim, ncells, seed))
            assert got.min() >= 0 and got.max() < ncells
            assert_array_equal(got[5:], host_parents(first + 5, n_sim - 5, ncells, seed))      # depends on (seed, N, s) alone
            if ncells == 1:
                assert not got.any()
    if ncells == 257:
        a, b = host_parents(0, 300, ncells, 0), host_parents(0, 300, ncells, 1)
        assert (a != b).any() and (a[:, 0] != a[:, 1]).any() and len(np.unique(a)) > 100


def test_parents_do_not_share_the_thinning_stream():
    """Counter word 3 is 1: thinning's block (s, 0, 0, 0) of the same seed gives other words."""
    from _thin_reference import philox
    w = philox(7, 0, 0, 0, 5, 0)
    got = host_parents(7, 1, 2 ** 31 - 1, 5)[0]
    assert got[0] != (int(w[0][0]) * (2 ** 31 - 1)) >> 32


def test_parents_refusals():
    from schpf_amd import _lib
    lib = _lib.load()
    out = np.zeros((4, 2), np.int32)
    for args, message in (((-1, 4, 5), "first must be >= 0"), ((0, -1, 5), r"n_sim must be in [0, 2^31)"),
                          ((0, 4, 0), "ncells must be in (0, 2^31)"), ((0, 4, 2 ** 31), "ncells must be in (0, 2^31)")):
        assert lib.schpf_doublet_parents(*(args + (ctypes.c_uint64(0), _p(out)))) != 0
        assert lib.schpf_last_error().decode() == message
    assert lib.schpf_doublet_parents(0, 4, 5, ctypes.c_uint64(0), None) != 0
    assert lib.schpf_doublet_parents(0, 0, 5, ctypes.c_uint64(0), None) == 0


def test_the_restatement_equals_the_definition(case):
    X, parents, want = case
    lengths = np.diff(X.indptr)
    assert X.shape == (80, 700) and list(lengths[:6]) == [0, 0, 1, 63, 64, 65]
    assert lengths[13] == LONG > 2 * PIECE and lengths[14] == LONGER > 2 * PIECE and LONGER % PIECE
    assert (X.data == 0).sum() > 10 and want[2].max() == 2 ** 25 and (want[2] == 0).sum() > 10
    for dtype in (np.int32, np.int64, np.float32, np.float64):
        got = debug_rows(X, parents, val_dtype=dtype)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype
            assert_array_equal(g, w)
    for n_pairs in (1, 65):
        got = debug_rows(X, parents[:n_pairs])
        assert_array_equal(got[0], want[0][:n_pairs + 1])
        assert_array_equal(got[1], want[1][:want[0][n_pairs]])
        assert_array_equal(got[2], want[2][:want[0][n_pairs]])
    # the pairs the matrix was made for
    dense = X.toarray()
    out = np.zeros((len(parents), 700), np.int64)
    for s in range(len(parents)):
        out[s, want[1][want[0][s]:want[0][s + 1]]] = want[2][want[0][s]:want[0][s + 1]]
    assert_array_equal(out, dense[parents[:, 0]].astype(np.int64) + dense[parents[:, 1]])
    assert np.diff(want[0])[0] == 0 and np.diff(want[0])[1] > LONG and np.diff(want[0])[7] == 700


def test_sizing_call_and_capacity(case):
    X, parents, want = case
    assert_array_equal(debug_rows(X, parents, fill=False)[0], want[0])
    with pytest.raises(ValueError, match="capacity must be at least the %d entries of the result, got %d"
                       % (want[0][-1], want[0][-1] - 1)):
        debug_rows(X, parents, short=1)


def test_empty_inputs():
    from schpf_amd import _lib
    from scipy.sparse import csr_matrix
    lib = _lib.load()
    X, parents, = kernel_matrix()
    # no pairs, no entries: nothing is read, out_indptr is zeros where it is given
    assert lib.schpf_debug_doublet_rows(80, 700, 5, None, None, None, 0, 0, None, None, None, None, 0) == 0
    out = np.full(4, -7, np.int64)
    assert lib.schpf_debug_doublet_rows(80, 700, 0, None, None, None, 0, 3, None, _p(out), None, None, 0) == 0
    assert not out.any()
    got = debug_rows(csr_matrix((80, 700), dtype=np.int32), parents)
    assert not got[0].any() and got[1].size == 0
    assert lib.schpf_debug_doublet_rows(80, 700, 5, None, None, None, 0, 3, None, _p(out), None, None, 0) != 0
    assert b"must not be NULL" in lib.schpf_last_error()
    assert lib.schpf_debug_doublet_rows(80, 700, 5, None, None, None, 9, 0, None, None, None, None, 0) != 0
    assert b"unknown index or value kind" in lib.schpf_last_error()
    assert lib.schpf_debug_doublet_rows(2 ** 31, 700, 0, None, None, None, 0, 0, None, None, None, None, 0) != 0
    assert lib.schpf_last_error().decode() == "ncells must be in [0, 2^31)"


@pytest.mark.parametrize("kind", ["indptr", "indptr_end", "index", "order", "value", "parent"])
def test_refusals_name_the_smallest_offender(kind):
    X, parents, message = spoiled(kind)
    with pytest.raises(ValueError) as err:
        debug_rows(X, parents, fill=False)
    assert str(err.value) == message
    with pytest.raises(ValueError) as err:
        debug_rows(X, parents, val_dtype=np.float64, fill=False)
    assert str(err.value) == message


def test_refusals_come_in_order():
    """indptr, index, order, value, parent: a matrix with all of them names the first; float values must be integral."""
    X, parents, _ = spoiled("parent")
    for kind in ("value", "order", "index"):
        e = int(X.indptr[13]) + 1
        if kind == "value":
            X.data[e] = -3
        elif kind == "order":
            X.indices[e] = X.indices[e - 1]
        else:
            X.indices[e + 1] = 700
        with pytest.raises(ValueError, match=MESSAGES[kind].split("%")[0].replace("[", r"\[").replace("^", r"\^").replace("]", r"\]")):
            debug_rows(X, parents, fill=False)
    X, parents = kernel_matrix()
    half = X.astype(np.float64)
    half.data[9] = 0.5
    with pytest.raises(ValueError, match="offending entry 9$"):
        debug_rows(half, parents, fill=False)


def test_scrublet_score_on_hand_computed_values():
    """rho = 0.06, r = 2, k_adj = 30: q = 1/32, 1/2, 31/32 for k_sim = 0, 15, 30; the score in exact fractions."""
    from schpf_amd.doublets import scrublet_score
    rho, r, k_adj = Fraction(6, 100), Fraction(2), 30
    score, se = scrublet_score(np.array([0, 15, 30]), k_adj, 2.0)
    for i, k_sim in enumerate((0, 15, 30)):
        q = Fraction(k_sim + 1, k_adj + 2)
        d = 1 - rho - q * (1 - rho - rho / r)
        assert_allclose(score[i], float(q * rho / r / d), rtol=1e-15, atol=0)
        se_q = math.sqrt(float(q * (1 - q) / (k_adj + 3)))
        want = float(q * rho / r / d / d) * math.sqrt((se_q / float(q) * 0.94) ** 2 + (0.02 / 0.06 * float(1 - q)) ** 2)
        assert_allclose(se[i], want, rtol=1e-14, atol=0)
    # q = 1/2: d = 0.94 - 0.455 = 0.485, score = 0.015 / 0.485 = 3 / 97
    assert_allclose(score[1], 3.0 / 97.0, rtol=1e-15, atol=0)
    assert score[0] < 0.06 / 2 < score[1] < score[2] < 1.0          # a cell among doublets only scores high, never 1
    # the reference of the GPU test is held to the same values
    ref_score, ref_se = scrublet(np.array([0, 15, 30]), k_adj, 2.0)
    assert_allclose(ref_score, score, rtol=1e-15, atol=0)
    assert_allclose(ref_se, se, rtol=1e-14, atol=0)
    # another ratio and rate
    score, _ = scrublet_score(np.array([10]), 20, 1.0, expected_rate=0.1, rate_sd=0.05)
    q = Fraction(11, 22)
    assert_allclose(score[0], float(q * Fraction(1, 10) / (1 - Fraction(1, 10) - q * (1 - Fraction(2, 10)))), rtol=1e-15, atol=0)


def test_the_brute_force_neighbours_use_the_library_key():
    """The NumPy yardstick of k_sim (an emulated fma, a stable sort) gives the distances of schpf_debug_knn bit for bit, on
    scores as a fit leaves them and on scores full of ties."""
    from _doublet_reference import fma, knn_counts
    from _knn_reference import debug_knn, gamma_scores, integer_scores
    assert fma(np.array([1.0 + 2.0 ** -30]), np.array([1.0 + 2.0 ** -30]), np.array([-1.0]))[0] == 2.0 ** -29 + 2.0 ** -60
    assert fma(np.array([3.0]), np.array([1.0 / 3.0]), np.array([-1.0]))[0] == -2.0 ** -54
    for x in (gamma_scores(301, 5, seed=2), integer_scores(200, 3, np.float64, 1)):
        counts, order, d2 = knn_counts(x, 17, 250)
        idx, want = debug_knn(x, x, 17, self_first=0)
        assert_array_equal(d2.view(np.uint64), want.view(np.uint64))
        assert_array_equal(order, idx)
        assert_array_equal(counts, (idx >= 250).sum(axis=1))


def toy_model(n_cells=60, n_genes=60, K=3):
    import schpf_amd
    rng = np.random.RandomState(0)
    gam = lambda shape: schpf_amd.HPF_Gamma(rng.gamma(1.0, 1.0, shape), rng.gamma(1.0, 1.0, shape) + 0.5)  # noqa: E731
    model = schpf_amd.scHPF(K)
    model.xi, model.theta = gam((n_cells,)), gam((n_cells, K))
    model.eta, model.beta = gam((n_genes,)), gam((n_genes, K))
    return model


def test_score_doublets_argument_errors(tmp_path):
    import json
    import schpf_amd
    from schpf_amd import cli
    path = str(tmp_path / "model.joblib")
    schpf_amd.save_model(toy_model(), path)
    with pytest.raises(ValueError, match=r"--doublets needs the count matrix \(-i\)"):
        cli.main(["score", "-m", path, "-o", str(tmp_path / "a"), "--doublets"])
    for flag, value in (("--doublet-ratio", "3"), ("--doublet-rate", "0.1"), ("--doublet-k", "5"), ("--doublet-seed", "2")):
        with pytest.raises(ValueError, match="%s belongs to --doublets" % flag):
            cli.main(["score", "-m", path, "-o", str(tmp_path / "b"), flag, value])
    # a run without the option: the arguments file holds what it held before there was one
    assert cli.main(["score", "-m", path, "-o", str(tmp_path / "plain")]) == 0
    args = json.load(open(str(tmp_path / "plain" / "score_commandline_args.json")))
    assert sorted(args) == ["cmd", "genefile", "model", "name_col", "outdir", "prefix"]


def test_simulate_doublets_checks_its_arguments():
    """What Python refuses before the library is asked (the library itself needs a GPU from here on)."""
    from schpf_amd import doublets
    with pytest.raises(ValueError, match=r"seed must be in \[0, 2\^64\)"):
        doublets._seed(-1)
    with pytest.raises(ValueError, match=r"parents must be an \(n_sim, 2\) array"):
        doublets._check_parents((4, 3), 10)
    assert doublets._n_sim(None, 2.0, 101) == 202 and doublets._n_sim(7, 2.0, 101) == 7
    with pytest.raises(ValueError, match=r"n_sim must be in \[0, 2\^31\)"):
        doublets._n_sim(-1, 2.0, 5)
