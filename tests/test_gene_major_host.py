"""The exact sparse transpose to gene-major, without a GPU: SciPy's tocsc() (tests/_gene_major_reference.py)
against the definition restated in NumPy, the library's serial restatement schpf_debug_transpose against the yardstick bit
for bit, its refusals with their words and their precedence, the empty inputs, and the Python layer on host inputs with the
restatements in the kernels' place."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from _gene_major_reference import (CASE_NAMES, DEBUG, MIDDLE, VAL_DTYPES, S, W, argument_refusals, assert_same, call, case,
                                   expected, matrix_refusals, outputs, restated, same_bits, untouched)


def test_the_generator_plants_its_cases():
    N, J, indptr, indices, data = case("(S+1)x(2W+1)")
    assert (N, J) == (S + 1, 2 * W + 1)
    per_column = np.bincount(indices, minlength=J)
    assert indptr[8] == indptr[7] and per_column[100] == 0 and per_column[200] == N - 1
    assert all(per_column[c] > 0 for c in (0, W - 1, W, 2 * W - 1, 2 * W))
    assert 0.005 < len(data) / float(N * J) < 0.02
    for name in ("64x3 dense", "65x3 dense", "1x(W+1)"):
        n, j, ptr, _, _ = case(name)
        assert ptr[-1] == n * j                                       # every mask bit of a group is set
    assert np.isnan(case(MIDDLE)[4][2]) and np.signbit(case(MIDDLE)[4][1]) and (case(MIDDLE)[4] == 0).sum() > 100


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_yardstick_is_the_definition(name):
    assert_same(expected(name), restated(case(name)), name)
    out_indptr, out_cells, _, source = expected(name)
    N, J, indptr, indices, data = case(name)
    assert out_indptr[0] == 0 and out_indptr[-1] == len(data)
    assert_array_equal(np.repeat(np.arange(J), np.diff(out_indptr)), indices[source])     # gene j holds column j's entries
    assert all((np.diff(out_cells[a:b]) > 0).all() for a, b in zip(out_indptr[:-1], out_indptr[1:]))   # the cells ascend


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_against_the_yardstick(name):
    for out_dtype in (None, np.float32):
        status, said, out = call(DEBUG, case(name), out_dtype)
        assert status == 0, said
        assert_same(out, expected(name), name)                        # float32 values: both choices move the bytes
    status, said, out = call(DEBUG, case(name), source=False)          # out_source == NULL is skipped
    assert status == 0 and out[3] is None
    assert_same(out[:3], expected(name)[:3], name)


@pytest.mark.parametrize("dtype", VAL_DTYPES)
def test_every_value_kind(dtype):
    status, said, out = call(DEBUG, case(MIDDLE, dtype))
    assert status == 0, said
    assert out[2].dtype == np.dtype(dtype)
    assert_same(out, expected(MIDDLE, dtype), str(dtype))             # the bytes as they are: -0.0, a NaN's payload, the extremes
    plain = case(MIDDLE, dtype, False)
    status, said, out = call(DEBUG, plain, np.float32)
    assert status == 0, said
    want = expected(MIDDLE, dtype, False)
    assert_same(out, want[:2] + (want[2].astype(np.float32), want[3]), "%s as float32" % dtype)


def test_refusals_in_their_order_leave_the_outputs_untouched():
    good = case(MIDDLE)
    for message, change in argument_refusals():
        status, said, out = call(DEBUG, good, **change)
        assert status != 0 and said == message, (message, said)
        assert untouched(out)
    for message, matrix in matrix_refusals(good):
        status, said, out = call(DEBUG, matrix)
        assert status != 0 and said == message, (message, said)
        assert untouched(out)
    status, said, out = call(DEBUG, good)
    assert status == 0 and not any((a == -7).all() for a in out)


def test_nothing_to_do_succeeds():
    from schpf_amd import _lib
    lib = _lib.load()
    for N, J in ((7, 5), (0, 5), (5, 0), (0, 0)):
        empty = (N, J, np.zeros(N + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
        status, said, out = call(DEBUG, empty)
        assert status == 0 and not out[0].any() and len(out[0]) == J + 1
    # ncells == 0 or ngenes == 0 with entries announced: nothing is read, the pointers may be NULL
    for N, J in ((0, 5), (5, 0)):
        out = outputs(J, 3, np.float32)
        assert lib.schpf_debug_transpose(N, J, 3, None, None, None, 2, 2, out[0].ctypes.data, None, None, None) == 0
        assert not out[0].any() and untouched(out[1:])


# ----------------------------------------------------------------------------------------------------- the Python layer
HOSTED = ("schpf_rank_sums", "schpf_pair_rank_sums", "schpf_residual_var")


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
def hosted(monkeypatch):
    from schpf_amd import _lib
    proxy = HostLibrary(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)


def counts():
    """The middle case as a SciPy CSR of counts (no NaN: the operators downstream refuse one)."""
    from scipy.sparse import csr_matrix
    N, J, indptr, indices, data = case(MIDDLE, np.float32, False)
    return csr_matrix((data, indices, indptr), shape=(N, J)), expected(MIDDLE, np.float32, False)


def test_gene_major_of_host_inputs():
    import schpf
    import schpf_amd
    from schpf_amd import GeneMajor, gene_major, scHPF
    from schpf_amd.gene_major import gene_major as defined
    assert gene_major is defined and schpf.gene_major is defined and schpf.GeneMajor is GeneMajor
    assert {"gene_major", "GeneMajor"} <= set(schpf_amd.__all__)
    X, want = counts()
    for given in (X, X.tocsc(), X.tocoo(), X.toarray()):
        G = scHPF.gene_major(given)
        assert isinstance(G, GeneMajor) and G.shape == X.shape and not G.on_gpu and G.device is None
        assert_array_equal(G.tensor().toarray(), X.toarray().T)
        assert G.nnz == (np.count_nonzero(X.toarray()) if isinstance(given, np.ndarray) else X.nnz)   # a dense input stores no zero
    G = gene_major(X)
    assert_same((G.indptr, G.cells, G.values), want[:3], "gene_major")         # stored zeros survive a SciPy input
    assert G.values.dtype == np.float32 and G.cells.dtype == np.int32 and G.indptr.dtype == np.int64
    assert gene_major(G) is G
    doubled = X.tocoo()
    doubled = type(doubled)((np.concatenate([doubled.data, doubled.data]), (np.concatenate([doubled.row, doubled.row]),
                                                                            np.concatenate([doubled.col, doubled.col]))), shape=X.shape)
    D = gene_major(doubled)
    assert_same((D.indptr, D.cells, D.values), (want[0], want[1], 2 * want[2]), "duplicates are summed")
    kept = gene_major(X.astype(np.int64), values="same")
    assert kept.values.dtype == np.int64 and same_bits(kept.values, want[2].astype(np.int64)) and same_bits(kept.cells, want[1])
    assert same_bits(kept.float32()[2], want[2])
    with pytest.raises(ValueError, match="values must be"):
        gene_major(X, values="float64")
    T = G.tensor()                                                    # the transpose as a matrix
    assert T.shape == (X.shape[1], X.shape[0]) and T.format == "csr"
    assert_array_equal(T.toarray(), X.toarray().T)
    assert same_bits(T.indptr.astype(np.int64), want[0]) and same_bits(T.data, want[2])


def test_the_operators_take_a_gene_major(hosted):
    from schpf_amd import gene_major, highly_variable_genes, pair_rank_sums, rank_sums, residual_variance
    X, _ = counts()
    G = gene_major(X)
    labels = np.arange(X.shape[0]) % 3
    for found, again in ((rank_sums(X, labels), rank_sums(G, labels)), (pair_rank_sums(X, labels), pair_rank_sums(G, labels)),
                         (residual_variance(X), residual_variance(G)),
                         (highly_variable_genes(X, n_top_genes=20), highly_variable_genes(G, n_top_genes=20))):
        assert list(found) == list(again)
        for key in found:
            assert same_bits(np.asarray(found[key]), np.asarray(again[key])), key


def test_the_functions_that_need_X_say_so(hosted):
    from schpf_amd import gene_major, highly_variable_genes, rank_genes_groups, rank_genes_pairs
    X, _ = counts()
    G = gene_major(X)
    labels = np.arange(X.shape[0]) % 3
    for call_it in (lambda: rank_genes_groups(G, labels), lambda: rank_genes_groups(G, labels, reference=0),
                    lambda: rank_genes_pairs(G, labels), lambda: highly_variable_genes(G, batch=labels)):
        with pytest.raises(TypeError, match="needs the cell-major count matrix X"):
            call_it()
