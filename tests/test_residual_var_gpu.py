"""Pearson residual variance per gene on the GPU.  schpf_residual_var and schpf_residual_var_device against
the yardstick of tests/_residual_var_reference.py (the definition on a dense matrix in NumPy float64) at the shapes where
the two passes can go wrong: grid and tile edges, segments longer than one piece of 4096 entries, one distinct cell total
and as many as there are cells.  Then equal bits between the entry points, between calls and between streams, a
renumbering of the cells, the optional outputs, the refusals, and the Python surface on GPU tensors.

Bound (derived, not tuned): |S1 - S1_ref| <= tol sum|r|, |S2 - S2_ref| <= tol S2_ref, tol = max(1e-12, 4 N 2^-53): a sum of n
doubles in any order is within (n - 1) eps sum|terms| of exact, every term carries a few ulps of rcp and sqrt, and the
yardstick rounds as well.  Every case prints its largest error."""
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from _residual_var_reference import (CASE_NAMES, CLIPS, THETAS, call, case, clip_of, cut_gap, dense_reference, errors, expected,
                                     gene_major, inverse, refusals, refused, tolerance)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def device_call(matrix, theta=100.0, clip=None, stream=None, fill=-7, totals=True):
    """schpf_residual_var_device on torch tensors -> (sum, sumsq, cell_total, gene_total) in NumPy."""
    from schpf_amd import _lib
    N, J, indptr, indices, data = matrix
    tensors = [torch.tensor(np.ascontiguousarray(a), device="cuda:0") for a in (indptr, indices, data)]
    out = [torch.full((J,), fill, dtype=torch.float64, device="cuda:0"), torch.full((J,), fill, dtype=torch.float64, device="cuda:0"),
           torch.full((N,), fill, dtype=torch.int64, device="cuda:0"), torch.full((J,), fill, dtype=torch.int64, device="cuda:0")]
    torch.cuda.synchronize()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
    outs = [ptr(t) for t in out] if totals else [ptr(out[0]), ptr(out[1]), None, None]
    _lib.check(_lib.load().schpf_residual_var_device(0, ctypes.c_void_p(stream), N, J, len(data), *[ptr(t) for t in tensors],
                                                     inverse(theta), clip_of(clip, N), *outs))
    return [t.cpu().numpy() for t in out]


def same_bits(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_parity_with_the_yardstick(amd, name):
    X, matrix = case(name)
    N = X.shape[0]
    for theta in THETAS:
        for clip in CLIPS:
            staged = call("schpf_residual_var", matrix, theta, clip, device=0)
            direct = device_call(matrix, theta, clip)
            for a, b in zip(staged, direct):
                assert same_bits(a, b)                                # host pointers and device pointers: equal bits
            s1, s2, cell_total, gene_total = direct
            assert_array_equal(cell_total, X.sum(axis=1))
            assert_array_equal(gene_total, X.sum(axis=0))
            e1, e2 = errors(s1, s2, expected(name, theta, clip))
            print("%s theta=%s clip=%s: S1 %.3g S2 %.3g (bound %.3g)" % (name, theta, clip, e1, e2, tolerance(N)))
            assert e1 <= tolerance(N) and e2 <= tolerance(N)


def test_division_above_the_domain_of_the_fast_reciprocal(amd):
    """1 / theta = 1e280 is above 2^900: the kernels divide instead of calling fast_rcp."""
    X, matrix = case("130x70")
    want = dense_reference(X, 1e-280, None)
    s1, s2, _, _ = device_call(matrix, 1e-280, None)
    e1, e2 = errors(s1, s2, want)
    print("theta=1e-280: S1 %.3g S2 %.3g" % (e1, e2))
    assert e1 <= tolerance(130) and e2 <= tolerance(130)
    assert (s2[X.sum(axis=0) > 0] > 0).all() and np.isfinite(s1).all()   # tiny residuals, neither flushed nor overflowed


def test_two_calls_and_two_streams_give_the_same_bits(amd):
    matrix = case("70001x67")[1]
    first = device_call(matrix)
    side = torch.cuda.Stream()
    for again in (device_call(matrix), device_call(matrix, stream=side.cuda_stream)):
        for a, b in zip(first, again):
            assert same_bits(a, b)


@pytest.mark.parametrize("name", ["257x129", "70001x67"])
def test_renumbering_the_cells(amd, name):
    X, _ = case(name)
    N = X.shape[0]
    perm = np.random.default_rng(3).permutation(N)
    s1, s2, cell_total, gene_total = device_call(gene_major(X[perm], stored_zeros=300, seed=8))
    assert_array_equal(cell_total, X.sum(axis=1)[perm])
    assert_array_equal(gene_total, X.sum(axis=0))
    e1, e2 = errors(s1, s2, expected(name, 100.0, None))              # the definition does not know the cells' numbers
    print("%s renumbered: S1 %.3g S2 %.3g" % (name, e1, e2))
    assert e1 <= tolerance(N) and e2 <= tolerance(N)
    silent = ~(X > 0).any(axis=0)                                     # a gene without entries is the dense part alone
    plain = device_call(case(name)[1])
    assert silent.any() and same_bits(s1[silent], plain[0][silent]) and same_bits(s2[silent], plain[1][silent])


def test_optional_outputs_may_be_null(amd):
    matrix = case("63x65")[1]
    full = device_call(matrix)
    s1, s2, cell_total, gene_total = device_call(matrix, totals=False)
    assert same_bits(s1, full[0]) and same_bits(s2, full[1])
    assert (cell_total == -7).all() and (gene_total == -7).all()


def test_refusals_leave_the_outputs_untouched(amd):
    from schpf_amd import _lib
    for message, change in refusals():
        status, said, out = refused("schpf_residual_var", change, device=0)
        assert status != 0 and said == message, (message, said)
        assert all((a == -7).all() for a in out)
    # the device entry: the same arrays in device memory
    from _residual_var_reference import NAMES, good_call, outputs
    N, J, indptr, indices, data = good_call()
    lib = _lib.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)  # noqa: E731
    for message, change in refusals():
        args = {"ncells": N, "ngenes": J, "nnz": len(data), "indptr": indptr, "indices": indices, "data": data, "inv_theta": 0.01,
                "clip": float(np.sqrt(N))}
        out = dict(zip(NAMES, [torch.tensor(a, device="cuda:0") for a in outputs(N, J)]))
        args.update(out)
        args.update(change)
        for key in ("indptr", "indices", "data"):
            if args[key] is not None:
                args[key] = torch.tensor(args[key], device="cuda:0")
        torch.cuda.synchronize()
        status = lib.schpf_residual_var_device(0, None, args["ncells"], args["ngenes"], args["nnz"],
                                               *[ptr(args[k]) for k in ("indptr", "indices", "data")], args["inv_theta"], args["clip"],
                                               *[ptr(args[k]) for k in NAMES])
        assert status != 0 and lib.schpf_last_error().decode() == message
        assert all(bool((t == -7).all()) for t in out.values())
    status, said, out = refused("schpf_residual_var", {}, device=99)  # no such device: an error, not an abort
    assert status != 0 and all((a == -7).all() for a in out)


def test_nothing_to_do_succeeds(amd):
    empty = (7, 5, np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    for entry in (lambda m: call("schpf_residual_var", m, clip=1.0, device=0), lambda m: device_call(m, clip=1.0)):
        assert all(not a.any() for a in entry(empty))
        for n, j in ((0, 5), (5, 0), (0, 0)):
            assert all(not a.any() for a in entry((n, j, np.zeros(j + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))))


def test_residual_variance_on_gpu_tensors(amd):
    from scipy.sparse import csr_matrix
    X = case("257x129")[0]
    N, J = X.shape
    want = expected("257x129", 100.0, None)
    C = csr_matrix(X)
    csr = torch.sparse_csr_tensor(torch.tensor(C.indptr, dtype=torch.int64), torch.tensor(C.indices, dtype=torch.int64),
                                  torch.tensor(C.data, dtype=torch.float32), size=X.shape).to("cuda:0")
    coo = C.tocoo()
    half = coo.data // 2                                              # every entry twice: x = half + (x - half)
    twice = torch.sparse_coo_tensor(torch.tensor(np.stack([np.concatenate([coo.row, coo.row]), np.concatenate([coo.col, coo.col])])),
                                    torch.tensor(np.concatenate([half, coo.data - half]), dtype=torch.float32), size=X.shape).to("cuda:0")
    results = [amd.residual_variance(csr), amd.residual_variance(twice)]
    for found in results:
        for name in ("residual_sum", "residual_sumsq", "residual_var", "gene_total", "cell_total"):
            assert found[name].device == csr.device
        e1, e2 = errors(found["residual_sum"].cpu().numpy(), found["residual_sumsq"].cpu().numpy(), want)
        assert e1 <= tolerance(N) and e2 <= tolerance(N)
        assert_array_equal(found["cell_total"].cpu().numpy(), X.sum(axis=1))
        assert found["n_distinct_totals"] == len(np.unique(X.sum(axis=1)))
    assert same_bits(results[0]["residual_sumsq"].cpu().numpy(), results[1]["residual_sumsq"].cpu().numpy())
    host = amd.residual_variance(C)                                    # SciPy in, NumPy out, the same bits
    assert isinstance(host["residual_sum"], np.ndarray) and same_bits(host["residual_sum"], results[0]["residual_sum"].cpu().numpy())
    with pytest.raises(ValueError, match="device=1"):
        amd.residual_variance(csr, device=1)


@pytest.mark.parametrize("fraction", [10, 4, 2])
def test_highly_variable_genes_end_to_end(amd, fraction):
    from scipy.sparse import csr_matrix
    X = case("257x129")[0]
    N, J = X.shape
    n_top = J // fraction
    _, _, _, var, order = expected("257x129", 100.0, None)
    assert cut_gap(var, order, n_top) > 1e-6
    C = csr_matrix(X)
    csr = torch.sparse_csr_tensor(torch.tensor(C.indptr, dtype=torch.int64), torch.tensor(C.indices, dtype=torch.int64),
                                  torch.tensor(C.data, dtype=torch.float32), size=X.shape).to("cuda:0")
    for M in (csr, C):
        found = amd.scHPF.variable_genes(M, n_top_genes=n_top)
        mask, rank = (found[k].cpu().numpy() if M is csr else found[k] for k in ("highly_variable", "rank"))
        assert_array_equal(np.flatnonzero(mask), np.sort(order[:n_top]))
        assert_array_equal(rank[order[:n_top]], np.arange(n_top))
        picked = amd.submatrix(M, genes=found["highly_variable"])
        assert tuple(picked.shape) == (N, n_top)
    batch = np.arange(N) * 7 % 3
    from _residual_var_reference import batch_reference
    want_order, n_batches, _, _ = batch_reference(X, batch, n_top)
    for label in range(3):
        _, _, _, var_b, order_b = dense_reference(X[batch == label])
        assert cut_gap(var_b, order_b, n_top) > 1e-6
    found = amd.highly_variable_genes(csr, n_top_genes=n_top, batch=batch)
    assert found["rank"].device == csr.device
    assert_array_equal(found["n_batches"].cpu().numpy(), n_batches)
    assert_array_equal(found["rank"].cpu().numpy()[want_order], np.arange(J))
