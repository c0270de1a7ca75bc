"""The exact sparse transpose to gene-major on the GPU: schpf_transpose and schpf_transpose_device against
SciPy's tocsc() (tests/_gene_major_reference.py), bit for bit, on the cases that sit on the edges of the kernels' cut --
W columns per window, S rows per slab, groups of 64 M rows, as csrc/transpose.hip fixes them and the reference module names
them -- then the refusals, and the Python layer on tensors in GPU memory: `gpu_csc` against the formulation it replaces,
restated here in torch, and the operators on a `GeneMajor`."""
import ctypes

import numpy as np
import pytest

from _gene_major_reference import (BAD_ORDER, CASE_NAMES, FILL, HOST, MIDDLE, VAL_DTYPES, argument_refusals, assert_same, call,
                                   case, expected, kind_of, matrix_refusals, same_bits, untouched)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def device_call(matrix, out_dtype=None, source=True, index_dtypes=(np.int64, np.int32), stream=None, **change):
    """One call of schpf_transpose_device on tensors -> (status, message, the four outputs fetched to NumPy)."""
    from schpf_amd import _lib
    lib = _lib.load()
    N, J, indptr, indices, data = matrix
    out_dtype = np.dtype(out_dtype or data.dtype)
    nnz = len(data)
    d_in = [torch.from_numpy(a).to(DEV) for a in (indptr.astype(index_dtypes[0]), indices.astype(index_dtypes[1]), np.array(data))]
    out = [torch.full((J + 1,), FILL, dtype=torch.int64, device=DEV), torch.full((nnz,), FILL, dtype=torch.int32, device=DEV),
           torch.from_numpy(np.full(nnz, FILL, out_dtype)).to(DEV),
           torch.full((nnz,), FILL, dtype=torch.int64, device=DEV) if source else None]
    args = {"ncells": N, "ngenes": J, "nnz": nnz, "indptr": _ptr(d_in[0]), "indptr_kind": int(index_dtypes[0] == np.int64),
            "indices": _ptr(d_in[1]), "idx_kind": int(index_dtypes[1] == np.int64), "val": _ptr(d_in[2]), "val_kind": kind_of(data.dtype),
            "out_val_kind": kind_of(out_dtype), "out_indptr": _ptr(out[0]), "out_cells": _ptr(out[1]), "out_values": _ptr(out[2]),
            "out_source": _ptr(out[3])}
    args.update(change)
    torch.cuda.synchronize()
    # NULL: a stream of the call's own; "null": the device's null stream (SCHPF_STREAM_DEFAULT); else a torch stream
    handle = None if stream is None else ctypes.c_void_p(_lib.STREAM_DEFAULT if stream == "null" else stream.cuda_stream)
    status = lib.schpf_transpose_device(0, handle, *args.values())
    return status, lib.schpf_last_error().decode() if status else "", [None if t is None else t.cpu().numpy() for t in out]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_both_entries_against_the_yardstick(name):
    want = expected(name)
    status, said, out = call(HOST, case(name))
    assert status == 0, said
    assert_same(out, want, "host pointers, " + name)
    status, said, out = device_call(case(name))
    assert status == 0, said
    assert_same(out, want, "device pointers, " + name)


@pytest.mark.parametrize("val", VAL_DTYPES)
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("ptr", [np.int32, np.int64])
def test_every_triple_of_kinds(ptr, idx, val):
    status, said, out = device_call(case(MIDDLE, val), index_dtypes=(ptr, idx))
    assert status == 0, said
    assert_same(out, expected(MIDDLE, val), "moved")                  # -0.0, a NaN's payload and the extremes survive
    want = expected(MIDDLE, val, False)
    status, said, out = device_call(case(MIDDLE, val, False), np.float32, index_dtypes=(ptr, idx))
    assert status == 0, said
    assert_same(out, want[:2] + (want[2].astype(np.float32), want[3]), "as float32")


@pytest.mark.parametrize("val", VAL_DTYPES)
def test_float32_values_through_host_pointers(val):
    want = expected(MIDDLE, val, False)
    status, said, out = call(HOST, case(MIDDLE, val, False), np.float32)
    assert status == 0, said
    assert_same(out, want[:2] + (want[2].astype(np.float32), want[3]), "as float32")


def test_equal_bits_on_every_route():
    name = "(S+1)x(2W+1)"
    want = expected(name)
    first = device_call(case(name))[2]
    again = device_call(case(name))[2]
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        on_side = device_call(case(name), stream=side)[2]
    on_null = device_call(case(name), stream="null")[2]
    for out in (first, again, on_side, on_null, call(HOST, case(name))[2]):
        assert_same(out, want, name)
    status, said, out = device_call(case(name), source=False)         # out_source == NULL is skipped
    assert status == 0 and out[3] is None
    assert_same(out[:3], want[:3], name)
    status, said, out = call(HOST, case(name), source=False)
    assert status == 0 and out[3] is None
    assert_same(out[:3], want[:3], name)


def test_refusals_on_both_entries_leave_the_outputs_untouched():
    good = case(MIDDLE)
    for message, change in argument_refusals():
        status, said, out = call(HOST, good, **change)
        assert status != 0 and said == message, (message, said)
        assert untouched(out)
        status, said, out = device_call(good, **change)
        assert status != 0 and said == message, (message, said)
        assert untouched(out)
    for message, matrix in matrix_refusals(good):
        for status, said, out in (call(HOST, matrix), device_call(matrix)):
            assert status != 0 and said == message, (message, said)
            assert untouched(out)


def test_nothing_to_do_succeeds():
    for N, J in ((7, 5), (0, 5), (5, 0), (0, 0)):
        empty = (N, J, np.zeros(N + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
        for status, said, out in (call(HOST, empty), device_call(empty)):
            assert status == 0, said
            assert not out[0].any() and len(out[0]) == J + 1


# ------------------------------------------------------------------------------------------------ tensors in GPU memory
def parent_gene_major(X):
    """What device_input.gpu_csc computed before the transpose: the coalesced COO, a full sort of the 64-bit keys
    cols * N + rows, the gathers, and the genes' pointer by bincount and cumsum."""
    X = X.detach()
    if X.layout == torch.sparse_csr:
        crow = X.crow_indices().to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(X.shape[0], device=X.device), crow[1:] - crow[:-1])
        X = torch.sparse_coo_tensor(torch.stack([rows, X.col_indices().to(torch.int64)]), X.values(), size=tuple(X.shape))
    X = X.coalesce()
    rows, cols, values = X.indices()[0], X.indices()[1], X.values()
    N, J = int(X.shape[0]), int(X.shape[1])
    order = torch.argsort(cols * N + rows)
    indptr = torch.zeros(J + 1, dtype=torch.int64, device=X.device)
    if J:
        indptr[1:] = torch.cumsum(torch.bincount(cols, minlength=J), 0)
    return indptr, rows[order].to(torch.int32).contiguous(), values[order].to(torch.float32).contiguous()


def tensors(dtype=np.float32, index=torch.int64):
    """The middle case on the GPU three ways: a canonical CSR tensor; a CSR tensor whose rows are reversed and that stores
    every entry of its first rows twice; an uncoalesced COO tensor of the same entries in a shuffled order."""
    N, J, indptr, indices, data = case(MIDDLE, dtype, False)
    crow, col, val = (torch.from_numpy(np.array(a)).to(DEV) for a in (indptr, indices.astype(np.int64), data))
    canonical = torch.sparse_csr_tensor(crow.to(index), col.to(index), val, size=(N, J))
    rows = np.repeat(np.arange(N), np.diff(indptr))
    twice = rows < 9
    r2, c2, v2 = np.concatenate([rows, rows[twice]]), np.concatenate([indices, indices[twice]]), np.concatenate([data, data[twice]])
    order = np.lexsort((-c2.astype(np.int64), r2))                    # by row, the columns descending
    ptr2 = np.zeros(N + 1, np.int64)
    ptr2[1:] = np.cumsum(np.bincount(r2, minlength=N))
    unsorted = torch.sparse_csr_tensor(torch.from_numpy(ptr2).to(DEV).to(index), torch.from_numpy(c2[order].astype(np.int64)).to(DEV).to(index),
                                       torch.from_numpy(v2[order]).to(DEV), size=(N, J))
    shuffle = np.random.default_rng(0).permutation(len(r2))
    coo = torch.sparse_coo_tensor(torch.from_numpy(np.stack([r2[shuffle], c2[shuffle].astype(np.int64)])).to(DEV),
                                  torch.from_numpy(v2[shuffle]).to(DEV), size=(N, J))
    return canonical, unsorted, coo


def equal_tensors(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and same_bits(g.cpu().numpy(), w.cpu().numpy()) for g, w in zip(got, want))


@pytest.mark.parametrize("dtype", VAL_DTYPES)
@pytest.mark.parametrize("index", [torch.int32, torch.int64])
def test_gpu_csc_returns_the_bits_it_always_did(dtype, index):
    from schpf_amd.device_input import gpu_csc
    for X in tensors(dtype, index):
        got = gpu_csc(X)
        assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.float32] and all(t.is_cuda for t in got)
        assert equal_tensors(got, parent_gene_major(X))
    canonical = tensors(dtype, index)[0]
    want = expected(MIDDLE, dtype, False)
    assert_same([t.cpu().numpy() for t in gpu_csc(canonical)], (want[0], want[1], want[2].astype(np.float32)), "gpu_csc")


def test_the_library_refuses_rows_that_do_not_ascend():
    X = tensors()[1]
    N, J = X.shape
    matrix = (N, J, X.crow_indices().cpu().numpy(), X.col_indices().cpu().numpy().astype(np.int32), X.values().cpu().numpy())
    for status, said, out in (call(HOST, matrix), device_call(matrix)):
        assert status != 0 and said == BAD_ORDER % 0 and untouched(out)


def test_a_canonical_csr_tensor_meets_no_sort(monkeypatch):
    from schpf_amd import GeneMajor, gene_major
    from schpf_amd.device_input import gpu_csc
    canonical, unsorted, coo = tensors()
    want = parent_gene_major(canonical)

    def never(*args, **kwargs):
        raise AssertionError("a sort or a coalesce on the way to gene-major")

    for owner, name in ((torch, "argsort"), (torch, "sort"), (torch.Tensor, "argsort"), (torch.Tensor, "sort"), (torch.Tensor, "coalesce")):
        monkeypatch.setattr(owner, name, never)
    with pytest.raises(AssertionError):
        coo.coalesce()
    assert equal_tensors(gpu_csc(canonical), want)
    G = gene_major(canonical)
    assert isinstance(G, GeneMajor) and G.on_gpu and G.shape == tuple(canonical.shape) and G.nnz == int(want[2].numel())
    assert equal_tensors((G.indptr, G.cells, G.values), want)
    with pytest.raises(AssertionError):                               # only rows that do not ascend are coalesced
        gene_major(unsorted)


def test_gene_major_on_the_gpu():
    from schpf_amd import gene_major, scHPF
    canonical = tensors(np.int64)[0]
    want = expected(MIDDLE, np.int64, False)
    kept = scHPF.gene_major(canonical, values="same")
    assert kept.values.dtype == torch.int64 and same_bits(kept.values.cpu().numpy(), want[2])
    T = gene_major(canonical).tensor()                                # the transpose as a matrix
    assert T.layout == torch.sparse_csr and tuple(T.shape) == (canonical.shape[1], canonical.shape[0])
    assert torch.equal(T.to_dense(), canonical.to_dense().to(torch.float32).t())
    with pytest.raises(ValueError, match="device=1 was asked for"):
        gene_major(canonical, device=1)
    with pytest.raises(TypeError):
        gene_major(canonical.to_dense())


def test_the_operators_take_a_gene_major():
    from schpf_amd import gene_major, highly_variable_genes, pair_rank_sums, rank_sums, residual_variance
    X = tensors()[0]
    G = gene_major(X)
    labels = np.arange(X.shape[0]) % 3
    for found, again in ((rank_sums(X, labels), rank_sums(G, labels)), (pair_rank_sums(X, labels), pair_rank_sums(G, labels)),
                         (residual_variance(X), residual_variance(G)),
                         (highly_variable_genes(X, n_top_genes=20), highly_variable_genes(G, n_top_genes=20))):
        assert list(found) == list(again)
        for key in found:
            a, b = found[key], again[key]
            if torch.is_tensor(a):
                assert b.is_cuda and a.dtype == b.dtype and same_bits(a.cpu().numpy(), b.cpu().numpy()), key
            else:
                assert a == b, key
