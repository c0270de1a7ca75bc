"""Pseudobulk without a GPU: the host restatement of the group statistics against the definition restated in
NumPy (tests/_aggregate_reference.py) and against the axis statistics, the refusals with their messages, and `group_codes`,
`pseudobulk` and the arguments of `scHPF score --pseudobulk` with the restatement in the kernels' place."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.sparse import coo_matrix, csr_matrix

from _aggregate_reference import (FILL, MESSAGES, N, NGENES, NROWS, SMALL_COLUMNS, _p, check_the_cases, debug_group_stats, equal, label_sets,
                                  labels_out, numpy_stats, overflowing, small_matrix, spoiled, stacked_matrix, stacked_wide_matrix, untouched)
from _qc_reference import debug_stats, kernel_matrix


@pytest.fixture(scope="module")
def stacked():
    X = stacked_matrix()
    return X, label_sets(N)


def test_the_cases_exist():
    check_the_cases()


def test_the_hook_equals_numpy_on_every_label_set(stacked):
    X, sets = stacked
    for name, labels, G in sets:
        equal(debug_group_stats(X, labels, G), numpy_stats(X, labels, G))
    W = stacked_wide_matrix()
    for name, labels, G in label_sets(W.shape[0]):
        equal(debug_group_stats(W, labels, G), numpy_stats(W, labels, G))


def test_one_group_of_all_cells_is_the_gene_side_of_the_axis_statistics(stacked):
    X = stacked[0]
    n, nexpr, total, sumsq = debug_group_stats(X, np.zeros(N, np.int32), 1)
    axis = debug_stats(X)
    assert n[0] == N
    for got, want in zip((nexpr, total, sumsq), axis[3:]):
        assert_array_equal(got[0], want)


def test_every_cell_its_own_group_is_the_dense_matrix():
    X = small_matrix()
    assert X.shape == (NROWS, SMALL_COLUMNS)
    n, nexpr, total, sumsq = debug_group_stats(X, np.arange(NROWS, dtype=np.int32), NROWS)
    D = X.toarray().astype(np.int64)
    assert_array_equal(total, D)
    assert_array_equal(nexpr, (D > 0).astype(np.int64))
    assert_array_equal(sumsq, D * D)
    assert_array_equal(n, np.ones(NROWS, np.int64))
    equal([n, nexpr, total, sumsq], numpy_stats(X, np.arange(NROWS), NROWS))


def test_without_the_squares_the_others_are_the_same(stacked):
    X, sets = stacked
    name, labels, G = sets[1]
    with_squares, without = debug_group_stats(X, labels, G), debug_group_stats(X, labels, G, sumsq=False)
    assert without[3] is None
    equal(without[:3], with_squares[:3])


@pytest.mark.parametrize("kind", ["indptr", "indptr_end", "index", "order", "value", "below", "above"])
def test_refusals_by_message_with_nothing_written(kind):
    X, labels, G, message = spoiled(kind)
    for dtype in (np.int32, np.float64):
        out = labels_out(G, NGENES)
        with pytest.raises(ValueError) as err:
            debug_group_stats(X, labels, G, val_dtype=dtype, out=out)
        assert str(err.value) == message
        assert untouched(out)


def test_the_overflow_rule_and_the_product():
    from schpf_amd import _lib
    lib = _lib.load()
    X, labels, G, message = overflowing()
    out = labels_out(1, 1)
    with pytest.raises(ValueError) as err:
        debug_group_stats(X, labels, G, out=out)
    assert str(err.value) == message and untouched(out)
    got = debug_group_stats(X, labels, G, sumsq=False)          # not asked for: not checked
    assert got[0][0] == 32768 and got[1][0, 0] == 1 and got[2][0, 0] == 2 ** 24
    got = debug_group_stats(X[:32767], labels[:32767], G)
    assert got[3][0, 0] == 2 ** 48
    one = np.full(1, FILL, np.int64)
    assert lib.schpf_debug_group_stats(1, 2 ** 15, 0, None, None, None, 0, _p(np.zeros(1, np.int32)), 2 ** 16, *[_p(one)] * 4) != 0
    assert lib.schpf_last_error().decode() == MESSAGES["product"] and one[0] == FILL


def test_the_refusals_come_in_order():
    """indptr, index, order, value, labels, overflow: an input with all that follow names the first."""
    X, labels, G, _ = spoiled("value")
    labels[3] = 7
    with pytest.raises(ValueError) as err:
        debug_group_stats(X, labels, G)
    assert str(err.value).startswith(MESSAGES["value"].split("%")[0])
    X, labels, G, _ = overflowing()
    labels[9] = -2
    with pytest.raises(ValueError) as err:
        debug_group_stats(X, labels, G)
    assert str(err.value) == MESSAGES["labels"] % 9


def test_edge_sizes_and_arguments():
    from schpf_amd import _lib
    lib = _lib.load()
    # nnz = 0: the matrix is not read, the labels are checked and the cells counted
    empty = csr_matrix((NROWS, NGENES), dtype=np.int32)
    labels = (np.arange(NROWS) % 4 - 1).astype(np.int32)
    n, nexpr, total, sumsq = debug_group_stats(empty, labels, 5)
    assert list(n) == [35, 35, 35, 0, 0] and not nexpr.any() and not total.any() and not sumsq.any()
    out = labels_out(5, NGENES)
    labels[17] = 5
    with pytest.raises(ValueError) as err:
        debug_group_stats(empty, labels, 5, out=out)
    assert str(err.value) == MESSAGES["labels"] % 17 and untouched(out)
    # no cells, no genes
    n = np.full(2, FILL, np.int64)
    assert lib.schpf_debug_group_stats(0, 0, 0, None, None, None, 0, None, 2, _p(n), None, None, None) == 0
    assert not n.any()
    one = np.zeros(1, np.int64)
    lab = np.zeros(1, np.int32)
    for args, message in (((2 ** 31, 1, 0), "ncells must be in [0, 2^31)"), ((1, -1, 0), "ngenes must be in [0, 2^31)"),
                          ((1, 1, 2 ** 31), "nnz must be in [0, 2^31)")):
        assert lib.schpf_debug_group_stats(*(args + (None, None, None, 0, _p(lab), 1) + (_p(one),) * 4)) != 0
        assert lib.schpf_last_error().decode() == message
    for G in (0, -1, 2 ** 31):
        assert lib.schpf_debug_group_stats(1, 1, 0, None, None, None, 0, _p(lab), G, *[_p(one)] * 4) != 0
        assert lib.schpf_last_error().decode() == "ngroups must be in [1, 2^31)"
    assert lib.schpf_debug_group_stats(1, 1, 0, None, None, None, 0, None, 1, *[_p(one)] * 4) != 0
    assert lib.schpf_last_error().decode() == "labels must not be NULL"
    assert lib.schpf_debug_group_stats(1, 1, 0, None, None, None, 0, _p(lab), 1, None, _p(one), _p(one), None) != 0
    assert lib.schpf_last_error().decode() == "group_cells must not be NULL"
    assert lib.schpf_debug_group_stats(1, 1, 0, None, None, None, 0, _p(lab), 1, _p(one), None, _p(one), None) != 0
    assert lib.schpf_last_error().decode() == "nexpr and total must not be NULL"
    assert lib.schpf_debug_group_stats(1, 1, 1, None, None, None, 0, _p(lab), 1, *[_p(one)] * 4) != 0
    assert lib.schpf_last_error().decode() == "indptr, indices and val must not be NULL"
    assert lib.schpf_debug_group_stats(1, 1, 0, None, None, None, 9, _p(lab), 1, *[_p(one)] * 4) != 0
    assert lib.schpf_last_error().decode() == "unknown index or value kind"


# ---- the Python layer, with the restatement in the kernels' place ----

def test_group_codes():
    from schpf_amd import group_codes
    sample = np.array(["s2", "s1", "s2", "", "s10", "s1", "s2", None], dtype=object)
    cluster = np.array([1, 0, 1, 0, 2, -1, 0, 2])
    codes, table = group_codes(sample, cluster)
    assert codes.dtype == np.int32
    assert table == [("s1", 0), ("s10", 2), ("s2", 0), ("s2", 1)]           # strings order as strings: "s10" < "s2"
    assert_array_equal(codes, [3, 0, 3, -1, 1, -1, 2, -1])
    codes, table = group_codes(cluster)
    assert table == [(0,), (1,), (2,)]
    assert_array_equal(codes, [1, 0, 1, 0, 2, -1, 0, 2])
    codes, table = group_codes(np.array([10, 2, 10, 2]), np.array([5, 7, 3, 7]))
    assert table == [(2, 7), (10, 3), (10, 5)]                              # integers order by value: 2 < 10
    assert_array_equal(codes, [2, 0, 1, 0])
    codes, table = group_codes(["b", "a", "b"])
    assert table == [("a",), ("b",)] and list(codes) == [1, 0, 1]
    codes, table = group_codes(np.array([-1, -1]))
    assert table == [] and list(codes) == [-1, -1]
    with pytest.raises(ValueError, match="one value per cell"):
        group_codes(np.zeros(3, int), np.zeros(4, int))
    with pytest.raises(ValueError, match="integers or strings"):
        group_codes(np.zeros(3))


@pytest.fixture
def aggregate(monkeypatch):
    """schpf_amd.aggregate with the host restatement in the place of schpf_group_stats."""
    from schpf_amd import aggregate as module

    def stats(ncells, ngenes, indptr, indices, vals, labels, ngroups, sumsq, device):
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and labels.dtype == np.int32
        X = csr_matrix((ncells, ngenes), dtype=vals.dtype)
        X.indptr, X.indices, X.data = indptr, indices, vals
        return debug_group_stats(X, labels, ngroups, sumsq=sumsq)

    monkeypatch.setattr(module, "_group_stats_host", stats)
    return module


def test_group_stats_in_python(aggregate):
    import schpf_amd
    assert schpf_amd.group_stats is aggregate.group_stats
    X = kernel_matrix()[0]
    labels = (np.arange(NROWS) % 5 - 1).astype(np.int64)
    want = numpy_stats(X, labels, 4)
    coo = X.tocoo()
    found = aggregate.group_stats(coo, labels)
    assert list(found) == ["n", "nexpr", "total", "sumsq"]
    equal([found[k] for k in found], want)
    found = aggregate.group_stats(X.toarray(), list(labels), ngroups=6, sumsq=False)       # dense, more groups than labels
    assert list(found) == ["n", "nexpr", "total"] and found["total"].shape == (6, NGENES)
    assert_array_equal(found["total"][:4], want[2])
    assert not found["total"][4:].any()
    half = X.copy()
    half.data = np.minimum(half.data, 2 ** 23)
    half = half.tocoo()
    twice = coo_matrix((np.tile(half.data, 2), (np.tile(half.row, 2), np.tile(half.col, 2))), shape=X.shape)    # duplicates are summed
    assert_array_equal(aggregate.group_stats(twice, labels)["total"], 2 * numpy_stats(half.tocsr(), labels, 4)[2])
    with pytest.raises(ValueError, match="one label per cell"):
        aggregate.group_stats(X, labels[:-1])
    with pytest.raises(ValueError, match=r"ngroups \* ngenes must be below 2\^31"):
        aggregate.group_stats(X, labels, ngroups=2 ** 20)
    with pytest.raises(ValueError, match=r"labels must be in \[-1, ngroups\); offending cell 3$"):
        aggregate.group_stats(X, np.where(np.arange(NROWS) == 3, 2 ** 32, labels), ngroups=4)


def test_pseudobulk_in_python(aggregate):
    X = kernel_matrix()[0]
    D = X.toarray().astype(np.float64)
    rng = np.random.RandomState(2)
    sample = np.array(["b", "a", "c"])[rng.randint(0, 3, NROWS)]
    cluster = rng.randint(0, 3, NROWS)
    cluster[5], sample[5] = 9, "z"                    # the 300-entry row: a group of exactly one cell
    cluster[::11] = -1
    found = aggregate.pseudobulk(X, (sample, cluster))
    groups = found["groups"]
    assert groups == sorted(set((s, c) for s, c in zip(sample, cluster) if c >= 0)) and ("z", 9) in groups
    assert found["counts"].dtype == np.int64 and found["counts"].shape == (len(groups), NGENES)
    for g, (s, c) in enumerate(groups):
        cells = (sample == s) & (cluster == c)
        assert found["n_cells"][g] == cells.sum()
        assert_array_equal(found["counts"][g], D[cells].sum(axis=0).astype(np.int64))
        assert_allclose(found["mean"][g], D[cells].mean(axis=0), rtol=1e-12)
        assert_allclose(found["pct"][g], (D[cells] > 0).mean(axis=0), rtol=1e-15)
        if cells.sum() > 1:
            assert_allclose(found["var"][g], D[cells].var(axis=0, ddof=1), rtol=1e-9)
        else:
            assert (s, c) == ("z", 9) and not found["var"][g].any()     # as qc does for one cell
    sizes = np.asarray(found["n_cells"])
    cut = int(np.median(sizes))
    fewer = aggregate.pseudobulk(X, (sample, cluster), min_cells=cut)
    keep = np.flatnonzero(sizes >= cut)
    assert 0 < len(keep) < len(groups) and fewer["groups"] == [groups[g] for g in keep]
    for key in ("n_cells", "counts", "pct", "mean", "var"):
        assert_array_equal(fewer[key], found[key][keep])
    alone = aggregate.pseudobulk(X, cluster)
    assert alone["groups"] == [(c,) for c in sorted(set(cluster[cluster >= 0]))]
    with pytest.raises(ValueError, match="one value per cell"):
        aggregate.pseudobulk(X, cluster[:-1])


def test_the_estimator_takes_labels(aggregate):
    import schpf_amd
    X = kernel_matrix()[0]
    labels = np.arange(NROWS) % 3
    found = schpf_amd.scHPF(3).pseudobulk(X, by=labels)
    assert_array_equal(found["counts"], numpy_stats(X, labels, 3)[2])
    with pytest.raises(TypeError, match="resolution belong to the clusters"):
        schpf_amd.scHPF(3).pseudobulk(X, by=labels, resolution=2.0)


def test_score_pseudobulk_argument_errors(tmp_path):
    import schpf_amd
    from schpf_amd import cli
    path, matrix, ids = str(tmp_path / "model.joblib"), str(tmp_path / "counts.mtx"), str(tmp_path / "ids.txt")
    rng = np.random.RandomState(0)
    gam = lambda shape: schpf_amd.HPF_Gamma(rng.gamma(1.0, 1.0, shape), rng.gamma(1.0, 1.0, shape) + 0.5)  # noqa: E731
    model = schpf_amd.scHPF(3)
    model.xi, model.theta, model.eta, model.beta = gam((60,)), gam((60, 3)), gam((60,)), gam((60, 3))
    schpf_amd.save_model(model, path)
    from scipy.io import mmwrite
    mmwrite(matrix, csr_matrix(np.random.RandomState(0).poisson(0.3, (60, 60))).tocoo(), field="integer")
    with open(ids, "w") as fh:
        fh.write("a\n" * 59)
    with pytest.raises(ValueError, match="--pseudobulk needs groups: the clusters .* --sample-ids FILE, or both"):
        cli.main(["score", "-m", path, "-i", matrix, "-o", str(tmp_path / "a"), "--pseudobulk"])
    with pytest.raises(ValueError, match=r"--pseudobulk needs the count matrix \(-i\)"):
        cli.main(["score", "-m", path, "-o", str(tmp_path / "a"), "--pseudobulk", "--sample-ids", ids])
    with pytest.raises(ValueError, match="--sample-ids belongs to --pseudobulk"):
        cli.main(["score", "-m", path, "-o", str(tmp_path / "a"), "--sample-ids", ids])
    with pytest.raises(ValueError, match="ids.txt holds 59 sample ids, the matrix has 60 cells"):
        cli.main(["score", "-m", path, "-i", matrix, "-o", str(tmp_path / "a"), "--pseudobulk", "--sample-ids", ids])
