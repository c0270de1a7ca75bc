"""Cell and gene filtering without a GPU: the host restatements of the axis statistics and of the submatrix
against the definitions restated as loops (tests/_qc_reference.py) and against SciPy where SciPy defines the same thing,
the refusals with their messages, the edge sizes, and the Python layer and `scHPF qc` with the restatements in the
kernels' place."""
import ctypes
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.sparse import csr_matrix

from _qc_reference import (BINS, EMPTY, EVERY, FILL, LONG, MESSAGES, NGENES, NROWS, PIECE, _p, bits, call_stats, call_submatrix,
                           debug_stats, debug_submatrix, kernel_matrix, loop_stats, loop_submatrix, odd_values, row_lists, same, spoiled,
                           stats_out, wide_matrix, VALUE_KINDS)

GOLD = os.path.join(os.path.dirname(__file__), "golden")

@pytest.fixture(scope="module")
def case():
    X, flags = kernel_matrix()
    want = loop_stats(X, flags, 32)
    for a in want:
        a.setflags(write=False)
    return X, flags, want


def test_the_kernel_matrix_is_the_one_described(case):
    X, flags, want = case
    lengths = np.diff(X.indptr)
    assert X.shape == (NROWS, NGENES) and NGENES > BINS + 1 and list(lengths[:6]) == [0, 1, 63, 64, 65, LONG] and LONG > 4 * PIECE
    assert X.has_canonical_format and X.data.max() == 2 ** 24 and (X.data == 0).sum() > 10
    assert want[3][EVERY] == NROWS - 1 and want[3][EMPTY] == 0 and want[3][0] > 0 and want[3][NGENES - 1] > 0
    assert want[3][BINS - 1] > 0 and want[3][BINS] > 0 and want[5].max() >= 2 ** 48
    assert (want[0] < lengths).sum() == 2                      # stored zeros are not counted


@pytest.mark.parametrize("n_sets", [0, 1, 32])
def test_the_statistics_equal_the_loops(case, n_sets):
    X, flags, want = case
    want = list(want)
    want[2] = want[2][:n_sets]
    for dtype in VALUE_KINDS:
        same(debug_stats(X, flags if n_sets else None, n_sets, val_dtype=dtype), want)


def test_the_statistics_of_wide_rows_equal_the_loops():
    X, flags = wide_matrix()
    same(debug_stats(X, flags, 2), [a[:2] if a.ndim == 2 else a for a in loop_stats(X, flags, 2)])


def test_the_statistics_equal_scipy(case):
    X, flags, want = case
    D = X.astype(np.int64)
    assert_array_equal(want[0], np.asarray((D > 0).sum(axis=1)).ravel())
    assert_array_equal(want[1], np.asarray(D.sum(axis=1)).ravel())
    assert_array_equal(want[3], np.asarray((D > 0).sum(axis=0)).ravel())
    assert_array_equal(want[4], np.asarray(D.sum(axis=0)).ravel())
    assert_array_equal(want[5], np.asarray(D.multiply(D).sum(axis=0)).ravel())
    for s in (0, 31):
        in_set = ((flags >> np.uint32(s)) & np.uint32(1)).astype(np.int64)
        assert_array_equal(want[2][s], D @ in_set)


@pytest.mark.parametrize("name,rows,keep", row_lists(), ids=[r[0] for r in row_lists()])
def test_the_submatrix_equals_the_loop_and_scipy(case, name, rows, keep):
    X = case[0]
    want = loop_submatrix(X, rows, keep)
    for dtype in VALUE_KINDS:
        got = debug_submatrix(X, rows, keep, val_dtype=dtype)
        same(got, want[:3] + (want[3].astype(dtype),))
    S = X[np.arange(NROWS) if rows is None else np.array(rows)]
    S = S[:, np.ones(NGENES, bool) if keep is None else keep]
    assert S.shape == (len(want[1]) - 1, want[0])
    assert_array_equal(S.indptr, want[1])
    assert_array_equal(S.indices, want[2])
    assert_array_equal(S.data, want[3])


def test_the_sizing_call_and_the_capacity(case):
    X = case[0]
    _, rows, keep = row_lists()[3][:3]
    want = loop_submatrix(X, rows, keep)
    got = debug_submatrix(X, rows, keep, fill=False)
    assert got[0] == want[0] and got[2] is None
    assert_array_equal(got[1], want[1])
    with pytest.raises(ValueError) as err:
        debug_submatrix(X, rows, keep, short=1)
    assert str(err.value) == MESSAGES["capacity"] % (want[1][-1], want[1][-1] - 1)


@pytest.mark.parametrize("dtype", VALUE_KINDS)
def test_values_survive_bit_for_bit_and_rows_keep_their_order(dtype):
    """A matrix the statistics would refuse: unsorted rows, duplicate columns, values of any kind."""
    vals = odd_values(dtype)
    indices = np.array([4, 1, 1, 3, 0, 4, 2, 4], np.int32)         # row 0: 4 1 1 3, row 1 empty, row 2: 0 4 2 4
    X = csr_matrix((5, 5), dtype=dtype)
    X.indptr, X.indices, X.data = np.array([0, 4, 4, 8, 8, 8], np.int64), indices, vals
    keep = np.array([1, 1, 0, 1, 7], np.uint8)                     # any byte but 0 keeps
    rows = [2, 0, 2, 1]
    got = debug_submatrix(X, rows, keep)
    want = loop_submatrix(X, rows, keep)
    same(got, want)
    assert got[0] == 4 and list(got[1]) == [0, 3, 7, 10, 10]
    assert list(got[2]) == [0, 3, 3, 3, 1, 1, 2, 0, 3, 3]          # column 4 is now 3, column 3 is 2: stored order kept
    assert (bits(got[3]) == bits(vals[[4, 5, 7, 0, 1, 2, 3, 4, 5, 7]])).all()


@pytest.mark.parametrize("kind", ["indptr", "indptr_end", "index", "order", "value"])
def test_the_statistics_refuse_by_message_and_write_nothing(case, kind):
    X, message = spoiled(kind)
    for dtype in (np.int32, np.float64):
        out = stats_out(NROWS, NGENES, 2)
        with pytest.raises(ValueError) as err:
            debug_stats(X, case[1], 2, val_dtype=dtype, out=out)
        assert str(err.value) == message
        assert all((a == FILL).all() for a in out)


def test_the_statistics_refuse_in_order():
    """indptr, index, order, value, overflow: a matrix with all that follow names the first; float values must be integral."""
    X, flags = kernel_matrix()
    huge = csr_matrix((np.full(1, 2 ** 24, np.int32), np.zeros(1, np.int32), np.concatenate([[0], np.ones(2 ** 15, np.int64)])),
                      shape=(2 ** 15, 1))
    with pytest.raises(ValueError, match="may overflow"):
        debug_stats(huge)
    huge.data[0] += 1
    with pytest.raises(ValueError, match="offending entry 0$"):
        debug_stats(huge)
    e = int(X.indptr[5]) + 1
    for kind, damage in (("value", lambda: X.data.__setitem__(e, -3)), ("order", lambda: X.indices.__setitem__(e, X.indices[e - 1])),
                         ("index", lambda: X.indices.__setitem__(e + 1, NGENES))):
        damage()
        with pytest.raises(ValueError) as err:
            debug_stats(X, flags, 1)
        assert str(err.value).startswith(MESSAGES[kind].split("%")[0])
    X, _ = kernel_matrix()
    half = X.astype(np.float64)
    half.data[9] = 0.5
    with pytest.raises(ValueError, match="offending entry 9$"):
        debug_stats(half)


def test_the_overflow_boundary():
    """vmax^2 * ncells >= 2^63 is refused: 2^48 * 32768 = 2^63, and 2^48 * 32767 is the largest sum that fits."""
    for ncells, fits in ((32768, False), (32767, True)):
        X = csr_matrix((np.full(1, 2 ** 24, np.int32), np.zeros(1, np.int32), np.concatenate([[0], np.ones(ncells, np.int64)])),
                       shape=(ncells, 1))
        out = stats_out(ncells, 1, 0)
        if fits:
            got = debug_stats(X, out=out)
            assert got[5][0] == 2 ** 48 and got[4][0] == 2 ** 24 and got[3][0] == 1 and got[0][0] == 1 and not got[0][1:].any()
        else:
            with pytest.raises(ValueError) as err:
                debug_stats(X, out=out)
            assert str(err.value) == MESSAGES["overflow"] % (2 ** 24, ncells)
            assert all((a == FILL).all() for a in out)


@pytest.mark.parametrize("kind", ["indptr", "indptr_end", "index", "rows"])
def test_the_submatrix_refuses_by_message_and_writes_nothing(kind):
    rows = [3, 5, NROWS, 4, -1]
    if kind == "rows":
        X, message = kernel_matrix()[0], MESSAGES["rows"] % 2
    else:
        X, message = spoiled(kind)              # the bad rows come after the matrix
    out = [ctypes.c_int64(FILL), np.full(len(rows) + 1, FILL, np.int64)]
    with pytest.raises(ValueError) as err:
        debug_submatrix(X, rows, None, out=out)
    assert str(err.value) == message
    assert out[0].value == FILL and (out[1] == FILL).all()
    # the submatrix asks for no order and no counts
    X, _ = spoiled("order")
    same(debug_submatrix(X, [5, 90], None), loop_submatrix(X, [5, 90], None))
    X, _ = spoiled("value")
    same(debug_submatrix(X, [5, 90], None), loop_submatrix(X, [5, 90], None))


def test_a_refused_capacity_writes_nothing(case):
    from schpf_amd import _lib
    X = case[0]
    lib = _lib.load()
    indptr, indices, val = X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data
    kept, out_indptr = ctypes.c_int64(FILL), np.full(NROWS + 1, FILL, np.int64)
    out_indices, out_values = np.full(X.nnz, FILL, np.int32), np.full(X.nnz, FILL, np.int32)
    assert lib.schpf_debug_submatrix(NROWS, NGENES, X.nnz, _p(indptr), _p(indices), _p(val), 0, NROWS, None, None, ctypes.byref(kept),
                                     _p(out_indptr), _p(out_indices), _p(out_values), X.nnz - 1) != 0
    assert lib.schpf_last_error().decode() == MESSAGES["capacity"] % (X.nnz, X.nnz - 1)
    assert kept.value == FILL and (out_indptr == FILL).all() and (out_indices == FILL).all() and (out_values == FILL).all()


def test_edge_sizes_and_arguments(case):
    from schpf_amd import _lib
    lib = _lib.load()
    X, flags, want = case
    # nnz = 0: the matrix is not read, the outputs are zeros
    empty = csr_matrix((NROWS, NGENES), dtype=np.int32)
    assert all(not a.any() for a in debug_stats(empty, flags, 3))
    out = stats_out(4, 3, 0)
    assert lib.schpf_debug_axis_stats(4, 3, 0, None, None, None, 0, 0, None, *[_p(a) for a in out]) == 0
    assert all(not a.any() for a in out)
    # N = 0, J = 0: nothing to write
    assert lib.schpf_debug_axis_stats(0, 0, 0, None, None, None, 0, 0, None, None, None, None, None, None, None) == 0
    assert all(not a.any() for a in debug_stats(csr_matrix((0, 5), dtype=np.int32), flags[:5], 2))
    assert all(not a.any() for a in debug_stats(csr_matrix((5, 0), dtype=np.int32)))
    # a matrix that stores something but has no room for it
    with pytest.raises(ValueError, match="offending row 0$"):
        call_stats("schpf_debug_axis_stats", X, shape=(0, NGENES))
    with pytest.raises(ValueError, match="out of range at entry 0$"):
        call_stats("schpf_debug_axis_stats", X[1:2], shape=(1, 0))
    for args, message in (((2 ** 31, 1, 0), "ncells must be in [0, 2^31)"), ((1, -1, 0), "ngenes must be in [0, 2^31)"),
                          ((1, 1, 2 ** 31), "nnz must be in [0, 2^31)")):
        assert lib.schpf_debug_axis_stats(*(args + (None, None, None, 0, 0, None, None, None, None, None, None, None))) != 0
        assert lib.schpf_last_error().decode() == message
    one = np.zeros(1, np.int64)
    for n_sets in (-1, 33):
        assert lib.schpf_debug_axis_stats(1, 1, 0, None, None, None, 0, n_sets, _p(one), *[_p(one)] * 6) != 0
        assert lib.schpf_last_error().decode() == "n_sets must be in [0, 32]"
    assert lib.schpf_debug_axis_stats(1, 1, 0, None, None, None, 0, 1, None, *[_p(one)] * 6) != 0
    assert b"gene_flags must not be NULL" in lib.schpf_last_error()
    assert lib.schpf_debug_axis_stats(1, 1, 0, None, None, None, 9, 0, None, *[_p(one)] * 6) != 0
    assert b"unknown index or value kind" in lib.schpf_last_error()
    assert lib.schpf_debug_axis_stats(1, 1, 1, None, None, None, 0, 0, None, *[_p(one)] * 6) != 0
    assert b"must not be NULL" in lib.schpf_last_error()

    # the submatrix: no rows, no entries, no genes
    keep = np.arange(NGENES) % 3 == 0
    got = debug_submatrix(X, [], keep)
    assert got[0] == keep.sum() and list(got[1]) == [0] and got[2].size == 0
    got = debug_submatrix(empty, [3, 3, 0], keep)
    assert got[0] == keep.sum() and list(got[1]) == [0, 0, 0, 0]
    with pytest.raises(ValueError) as err:                              # rows are still checked
        debug_submatrix(empty, [3, NROWS], keep)
    assert str(err.value) == MESSAGES["rows"] % 1
    same(debug_submatrix(X, None, np.zeros(NGENES, bool)), (0, np.zeros(NROWS + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32)))
    same(debug_submatrix(X), (NGENES, X.indptr.astype(np.int64), X.indices, X.data))        # rows = NULL, gene_keep = NULL
    got = debug_submatrix(csr_matrix((0, 4), dtype=np.int32), None, np.array([1, 0, 1, 1]))
    assert got[0] == 3 and list(got[1]) == [0]
    got = debug_submatrix(csr_matrix((3, 0), dtype=np.int32))
    assert got[0] == 0 and list(got[1]) == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="n_rows must be ncells where rows is NULL"):
        debug_submatrix(X, None, None, n_rows=3)
    kept, ptr = ctypes.c_int64(0), np.zeros(2, np.int64)
    for args, message in (((2 ** 31, 1, 0, None, None, None, 0, 0, None, None), "ncells must be in [0, 2^31)"),
                          ((1, 1, 0, None, None, None, 0, -1, _p(ptr), None), "n_rows must be in [0, 2^31)"),
                          ((1, 1, 0, None, None, None, 9, 1, None, None), "unknown index or value kind")):
        assert lib.schpf_debug_submatrix(*(args + (ctypes.byref(kept), _p(ptr), None, None, 0))) != 0
        assert lib.schpf_last_error().decode() == message
    assert lib.schpf_debug_submatrix(1, 1, 0, None, None, None, 0, 1, None, None, None, _p(ptr), None, None, 0) != 0
    assert b"out_ngenes and out_indptr must not be NULL" in lib.schpf_last_error()
    assert lib.schpf_debug_submatrix(1, 1, 0, None, None, None, 0, 1, None, None, ctypes.byref(kept), _p(ptr), _p(ptr), None, 0) != 0
    assert b"both be given or both be NULL" in lib.schpf_last_error()


# ---- the Python layer, with the restatements in the kernels' place ----

@pytest.fixture
def qc(monkeypatch):
    """schpf_amd.qc with the host restatements in the place of schpf_axis_stats and schpf_submatrix."""
    from schpf_amd import qc as module

    def stats(ncells, ngenes, indptr, indices, vals, n_sets, flags, device):
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and flags.dtype == np.uint32
        X = csr_matrix((ncells, ngenes), dtype=vals.dtype)
        X.indptr, X.indices, X.data = indptr, indices, vals
        return [a if a.flags.writeable else a.copy() for a in debug_stats(X, flags, n_sets)]

    def sub(ncells, ngenes, indptr, indices, vals, rows, keep, device):
        assert rows is None or rows.dtype == np.int32
        assert keep is None or keep.dtype == np.uint8
        X = csr_matrix((ncells, ngenes), dtype=vals.dtype)
        X.indptr, X.indices, X.data = indptr, indices, vals
        return debug_submatrix(X, rows, keep)

    monkeypatch.setattr(module, "_axis_stats_host", stats)
    monkeypatch.setattr(module, "_submatrix_host", sub)
    return module


def test_qc_metrics_and_submatrix_in_python(case, qc):
    import schpf_amd
    X, flags, want = case
    mito, ribo = (flags & 1).astype(bool), np.flatnonzero(flags & 2)
    found = qc.qc_metrics(X.tocoo(), gene_sets={"mito": mito, "ribo": ribo})
    for key, w in zip(("cell_n_genes", "cell_total", "gene_n_cells", "gene_total", "gene_sumsq"), (want[0], want[1]) + tuple(want[3:])):
        assert found[key].dtype == np.int64
        assert_array_equal(found[key], w)
    assert list(found["cell_set_total"]) == ["mito", "ribo"]
    assert_array_equal(found["cell_set_total"]["mito"], want[2][0])
    assert_array_equal(found["cell_set_total"]["ribo"], want[2][1])
    D = X.toarray().astype(np.float64)
    assert_allclose(found["gene_mean"], D.mean(axis=0), rtol=1e-12)
    assert_allclose(found["gene_var"], D.var(axis=0, ddof=1), rtol=1e-9)
    assert_array_equal(schpf_amd.scHPF.qc(X)["gene_n_cells"], want[3])
    with pytest.raises(ValueError, match="at most 32 gene sets"):
        qc.qc_metrics(X, gene_sets={str(s): mito for s in range(33)})
    with pytest.raises(ValueError, match=r"gene set 'a' indices must be in \[0, %d\)" % NGENES):
        qc.qc_metrics(X, gene_sets={"a": [NGENES]})

    cells = np.arange(NROWS) % 7 != 0
    S = qc.submatrix(X, cells=cells, genes=mito)
    assert isinstance(S, csr_matrix) and S.dtype == X.dtype and (S != X[cells][:, mito]).nnz == 0
    picks = [5, 5, 139, 0]
    S = qc.submatrix(X.astype(np.float32), cells=picks, genes=np.flatnonzero(mito))
    assert S.dtype == np.float32 and (S != X[picks][:, mito]).nnz == 0
    assert (qc.submatrix(X) != X).nnz == 0
    assert qc.submatrix(X.astype(np.int16), cells=picks).dtype == np.int16
    with pytest.raises(ValueError, match="strictly ascending"):
        qc.submatrix(X, genes=[3, 2])
    with pytest.raises(ValueError, match=r"rows must be in \[0, ncells\); offending position 1"):
        qc.submatrix(X, cells=[0, 2 ** 32])
    with pytest.raises(ValueError, match="boolean cell mask must have shape"):
        qc.submatrix(X, cells=np.ones(3, bool))


def test_filter_counts_in_python(case, qc):
    X, flags, want = case
    mito = (flags & 1).astype(bool)
    F, cell_keep, gene_keep, found = qc.filter_counts(X, min_cells=3, min_genes=10, min_counts=200, max_counts=10 ** 6,
                                                      max_set_fraction={"mito": 0.6}, gene_sets={"mito": mito})
    assert_array_equal(gene_keep, want[3] >= 3)
    cells = (want[0] >= 10) & (want[1] >= 200) & (want[1] <= 10 ** 6) & (want[2][0] <= 0.6 * want[1])
    assert_array_equal(cell_keep, cells)
    assert 0 < cells.sum() < NROWS and 0 < gene_keep.sum() < NGENES
    assert (F != X[cells][:, gene_keep]).nnz == 0
    assert_array_equal(found["gene_n_cells"], want[3])          # the statistics of X, not of F: one pass
    F, cell_keep, gene_keep, _ = qc.filter_counts(X)
    assert cell_keep.all() and gene_keep.all() and (F != X).nnz == 0
    with pytest.raises(ValueError, match="names the gene set 'ribo'"):
        qc.filter_counts(X, max_set_fraction={"ribo": 0.1}, gene_sets={"mito": mito})


def test_min_cells_is_the_rule_of_min_cells_expressing_mask(qc):
    from schpf_amd import preprocessing as prep
    gold = np.load(os.path.join(GOLD, "prep_data.npz"))
    umis, _ = prep.load_txt(os.path.join(GOLD, "PJ030merge.c300t400_g0t500.matrix.txt"), verbose=False)
    for threshold, key in ((3, "mask_min3"), (0.1, "mask_frac")):
        gene_keep = qc.filter_counts(umis, min_cells=threshold)[2]
        assert_array_equal(gene_keep, gold[key])
        assert_array_equal(gene_keep, prep.min_cells_expressing_mask(umis, threshold, verbose=False))
    zeros = umis.tocsr().copy()
    zeros.data[::2] = 0                                         # stored zeros are no expression, in both
    assert_array_equal(qc.filter_counts(zeros, min_cells=2)[2], prep.min_cells_expressing_mask(zeros, 2, verbose=False))


def test_qc_on_the_command_line(case, qc, tmp_path):
    import json
    from scipy.io import mmread, mmwrite
    from schpf_amd import cli
    X, flags, want = case
    matrix, mito = str(tmp_path / "counts.mtx"), str(tmp_path / "mito.txt")
    mmwrite(matrix, X.tocoo(), field="integer")                # Matrix Market drops nothing: stored zeros are written
    np.savetxt(mito, np.flatnonzero(flags & 1), fmt="%d")
    out = tmp_path / "out"
    assert cli.main(["qc", "-i", matrix, "-o", str(out), "--gene-set", "mito=" + mito]) == 0
    assert sorted(os.listdir(str(out))) == ["cell_qc.txt", "gene_qc.txt", "qc_commandline_args.json"]
    cell = np.loadtxt(str(out / "cell_qc.txt"), skiprows=1, dtype=np.int64)
    assert open(str(out / "cell_qc.txt")).readline().split() == ["n_genes", "total", "mito"]
    assert_array_equal(cell, np.stack([want[0], want[1], want[2][0]], axis=1))
    gene = np.loadtxt(str(out / "gene_qc.txt"), skiprows=1)
    assert_array_equal(gene[:, :3].astype(np.int64), np.stack(want[3:], axis=1))
    assert_allclose(gene[:, 3], want[4] / NROWS, rtol=1e-15)
    out = tmp_path / "filtered"
    assert cli.main(["qc", "-i", matrix, "-o", str(out), "-p", "run", "--min-cells", "3", "--min-genes", "10", "--min-counts", "200",
                     "--max-counts", "1000000", "--write-filtered"]) == 0
    cells, genes = (want[0] >= 10) & (want[1] >= 200) & (want[1] <= 10 ** 6), want[3] >= 3
    assert_array_equal(np.loadtxt(str(out / "run.kept_cells.txt"), dtype=np.int64), np.flatnonzero(cells))
    assert_array_equal(np.loadtxt(str(out / "run.kept_genes.txt"), dtype=np.int64), np.flatnonzero(genes))
    F = mmread(str(out / "run.filtered.mtx")).tocsr()
    assert F.shape == (cells.sum(), genes.sum()) and (F != X[cells][:, genes]).nnz == 0
    assert json.load(open(str(out / "run.qc_commandline_args.json")))["min_cells"] == 3
    with pytest.raises(ValueError, match="--gene-set takes NAME=FILE"):
        cli.main(["qc", "-i", matrix, "-o", str(out), "--gene-set", "mito"])
