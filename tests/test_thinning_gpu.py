"""Count thinning on the GPU.  The kernels use integer arithmetic only, so every comparison with the
library's host restatement (schpf_debug_thin_counts; tests/test_thinning_host.py pins it to the definition) is for equal
bits -- whatever the storage of the matrix and wherever it lives.  Then the Python surface: thin_counts, the held-out
loss, run_trials(thin=...) and the command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.sparse import coo_matrix
from scipy.special import gammaln

from conftest import GOLDEN, ROOT
from _thin_reference import KINDS, debug_thin, matrix_with_heavy_tail, _p

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
FRAC, SEED = 0.3, 0x1234567887654321


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


@pytest.fixture(scope="module")
def case():
    """The matrix of the host tests (light entries, then the heavy ones) and its split by the host restatement."""
    row, col, val = matrix_with_heavy_tail()
    train, test, stats = debug_thin(row, col, val, FRAC, SEED)
    for a in (row, col, val, train, test):
        a.setflags(write=False)
    return row, col, val, train, test, stats


def host_call(row, col, val, frac=FRAC, seed=SEED):
    from schpf_amd import _lib
    row, col = np.ascontiguousarray(row, np.int32), np.ascontiguousarray(col, np.int32)
    val = np.ascontiguousarray(val)
    train, test = np.full(len(val), -7, np.int32), np.full(len(val), -7, np.int32)
    stats = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().schpf_thin_counts(0, len(val), _p(row), _p(col), _p(val), KINDS[val.dtype], frac,
                                             ctypes.c_uint64(seed), _p(train), _p(test), stats))
    return train, test, [int(s) for s in stats]


def device_call(row, col, val, idx=np.int32, frac=FRAC, seed=SEED, stream=None):
    """schpf_thin_counts_device on torch tensors of the given index dtype and val's dtype; results as NumPy arrays."""
    from schpf_amd import _lib
    n = len(val)
    d_row = torch.tensor(np.asarray(row, idx), device="cuda:0")
    d_col = torch.tensor(np.asarray(col, idx), device="cuda:0")
    d_val = torch.tensor(np.asarray(val), device="cuda:0")
    d_train = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    d_test = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    stats = (ctypes.c_int64 * 4)(9, 9, 9, 9)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
    kind = _lib.IDX_I64 if np.dtype(idx) == np.int64 else _lib.IDX_I32
    _lib.check(_lib.load().schpf_thin_counts_device(0, ctypes.c_void_p(stream), n, ptr(d_row), ptr(d_col), kind,
                                                    ptr(d_val), KINDS[np.asarray(val).dtype], frac,
                                                    ctypes.c_uint64(seed), ptr(d_train), ptr(d_test), stats))
    return d_train.cpu().numpy(), d_test.cpu().numpy(), [int(s) for s in stats]


def test_both_entry_points_equal_the_host_restatement(amd, case):
    row, col, val, train, test, stats = case
    assert stats[3] > 0 and stats[2] > 0 and (val > 256).sum() == 5
    for got in (host_call(row, col, val), device_call(row, col, val)):
        assert_array_equal(got[1], test)
        assert_array_equal(got[0], train)
        assert got[2] == stats


def test_the_host_entry_point_in_several_slabs(amd, case, monkeypatch):
    """Slabs of 1 000 entries: six trips through the device, the heavy entries in the last one."""
    row, col, val, train, test, stats = case
    monkeypatch.setenv("SCHPF_THIN_SLAB", "1000")
    got = host_call(row, col, val)
    assert_array_equal(got[1], test)
    assert_array_equal(got[0], train)
    assert got[2] == stats
    bad = val.astype(np.float64)
    bad[4321] = bad[2100] = 0.5
    with pytest.raises(ValueError, match="offending entry 2100$"):
        host_call(row, col, bad)
    bad_row = row.copy()
    bad_row[3003] = -2              # a later slab than the bad value: an index error still goes first
    with pytest.raises(ValueError, match="COO index out of range at entry 3003$"):
        host_call(bad_row, col, bad)


@pytest.mark.parametrize("n", [1, 65])
def test_small_shapes(amd, n):
    """A single entry (a grid of one partial wavefront) and a wavefront plus one lane."""
    row, col = np.arange(n, dtype=np.int32) * 3, np.arange(n, dtype=np.int32)[::-1].copy()
    val = (np.arange(n, dtype=np.int32) * 7 + 300 * (n == 1)) % 301 + 9      # n = 1: one heavy entry (x = 309)
    want = debug_thin(row, col, val, FRAC, SEED)
    for got in (host_call(row, col, val), device_call(row, col, val)):
        assert_array_equal(got[0], want[0])
        assert_array_equal(got[1], want[1])
        assert got[2] == want[2]


def test_every_storage_gives_one_result(amd, case):
    row, col, val, train, test, stats = case
    # index and value types, on the caller's (null) stream as well
    for idx, vdtype, stream in ((np.int64, np.float64, None), (np.int32, np.int32, None), (np.int64, np.float32, 1),
                                (np.int32, np.int64, None)):
        got = device_call(row, col, val.astype(vdtype), idx=idx, stream=stream)
        assert_array_equal(got[1], test)
        assert_array_equal(got[0], train)
        assert got[2] == stats
    thin = lambda X: amd.thin_counts(X, FRAC, seed=SEED)  # noqa: E731
    # SciPy
    S_train, S_test = thin(coo_matrix((val, (row, col)), shape=(257, 1031)))
    assert_array_equal(S_test.data, test)
    assert S_test.data.dtype == val.dtype and S_train.data.dtype == val.dtype
    assert_array_equal(S_test.row, row)
    assert_array_equal(S_test.col, col)
    assert_array_equal(S_train.data, train[train > 0])
    assert_array_equal(S_train.row, row[train > 0])
    # a torch COO tensor in permuted order
    perm = np.random.RandomState(1).permutation(len(val))
    index = torch.tensor(np.stack([row[perm], col[perm]]).astype(np.int64), device="cuda:0")
    T_train, T_test = thin(torch.sparse_coo_tensor(index, torch.tensor(val[perm].astype(np.float32), device="cuda:0"),
                                                   (257, 1031)))
    assert T_test._values().dtype == torch.float32
    assert_array_equal(T_test._values().cpu().numpy(), test[perm])
    assert_array_equal(T_test._indices().cpu().numpy(), index.cpu().numpy())
    assert_array_equal(T_train._values().cpu().numpy(), train[perm][train[perm] > 0])
    # a torch CSR tensor (entries sorted by row, then column), int32 and int64 indices
    order = np.lexsort((col, row))
    S = coo_matrix((val[order], (row[order], col[order])), shape=(257, 1031)).tocsr()
    assert_array_equal(S.data, val[order])       # tocsr kept the stored zeros and the order
    for idt in (torch.int32, torch.int64):
        C = torch.sparse_csr_tensor(torch.tensor(S.indptr).to(idt), torch.tensor(S.indices).to(idt),
                                    torch.tensor(S.data.astype(np.int64)), size=(257, 1031)).to("cuda:0")
        C_train, C_test = thin(C)
        assert C_test._values().dtype == torch.int64
        assert_array_equal(C_test._values().cpu().numpy(), test[order])
        assert_array_equal(C_test._indices().cpu().numpy(), np.stack([row[order], col[order]]))
        assert_array_equal(C_train._values().cpu().numpy(), train[order][train[order] > 0])


def test_thin_counts_on_a_gpu_tensor(amd, case):
    row, col, val, train, test, stats = case
    index = torch.tensor(np.stack([row, col]).astype(np.int64), device="cuda:0")
    X = torch.sparse_coo_tensor(index, torch.tensor(val.astype(np.int64), device="cuda:0"), (257, 1031))
    X_train, X_test = amd.thin_counts(X, FRAC, seed=SEED)
    for t in (X_train, X_test):
        assert t.device == X.device and t.layout == torch.sparse_coo and tuple(t.shape) == (257, 1031)
    total, want = (X_train + X_test).coalesce(), X.coalesce()
    assert torch.equal(total.indices(), want.indices()) and torch.equal(total.values(), want.values())
    assert X_test._nnz() == len(val) and int((X_test._values() == 0).sum()) == int((test == 0).sum()) > 0
    assert torch.equal(X_test._indices(), index)
    assert X_train._nnz() == stats[0] and bool((X_train._values() > 0).all())
    with pytest.raises(ValueError, match="device=1 was asked for"):
        amd.thin_counts(X, FRAC, device=1)


def test_empty_input(amd):
    from schpf_amd import _lib
    lib = _lib.load()
    stats = (ctypes.c_int64 * 4)(9, 9, 9, 9)
    assert lib.schpf_thin_counts_device(0, None, 0, None, None, 0, None, 0, 0.5, 0, None, None, stats) == 0
    assert list(stats) == [0, 0, 0, 0]
    stats = (ctypes.c_int64 * 4)(9, 9, 9, 9)
    assert lib.schpf_thin_counts(0, 0, None, None, None, 0, 0.5, 0, None, None, stats) == 0
    assert list(stats) == [0, 0, 0, 0]
    E_train, E_test = amd.thin_counts(coo_matrix((4, 5), dtype=np.int32), 0.5)
    assert E_train.nnz == 0 and E_test.nnz == 0 and E_test.shape == (4, 5)
    G_train, G_test = amd.thin_counts(torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.int64),
                                                              torch.zeros(0), (4, 5)).to("cuda:0"), 0.5)
    assert G_train._nnz() == 0 and G_test._nnz() == 0 and G_test.device.type == "cuda"
    assert lib.schpf_thin_counts_device(99, None, 0, None, None, 0, None, 0, 0.5, 0, None, None, stats) != 0
    assert b"no such HIP device" in lib.schpf_last_error()


def test_validation_on_the_device(amd, case):
    """A bad value in the middle of the array: refused with the smallest offending entry (the outputs of a refused call
    are unspecified and not looked at)."""
    row, col, val = case[:3]
    for bad_value in (2.5, -1.0, 2.0 ** 24 + 1, np.nan):
        bad = val.astype(np.float64)
        bad[3100] = bad[2500] = bad_value
        with pytest.raises(ValueError, match=r"thinning needs integer counts in \[0, 2\^24\]; offending entry 2500$"):
            device_call(row, col, bad)
    bad = val.astype(np.float64)
    bad[100] = 0.5
    wide = row.astype(np.int64)
    wide[700] = 2 ** 31              # an int64 beyond int32
    wide[4000] = -1
    with pytest.raises(ValueError, match="COO index out of range at entry 700$"):
        device_call(wide, col, bad, idx=np.int64)
    with pytest.raises(ValueError, match=r"frac must be in \(0, 1\)"):
        device_call(row, col, val, frac=1.0)


def planted(ncells=300, ngenes=120, K=3, seed=4):
    rng = np.random.RandomState(seed)
    theta = rng.gamma(0.5, 2.0, (ncells, K))
    beta = rng.gamma(0.5, 1.5, (ngenes, K))
    X = coo_matrix(rng.poisson(theta @ beta.T))
    X.eliminate_zeros()
    return X.astype(np.int32).tocoo()


def numpy_thinned_loss(X_test, model, frac):
    s = frac / (1.0 - frac)
    r = (model.theta.e_x[X_test.row] * model.beta.e_x[X_test.col]).sum(axis=1)
    x = X_test.data.astype(np.float64)
    return np.mean(-(x * np.log(s * r) - s * r - gammaln(x + 1.0)))


def test_run_trials_on_thinned_counts(amd):
    from schpf_amd import loss
    X = planted()
    np.random.seed(0)
    best, rest = amd.run_trials(X, 3, ntrials=2, thin=0.2, max_iter=40, verbose=False, return_all=True)
    X_train, X_test = amd.thin_counts(X, 0.2)          # run_trials' split: thin_seed = 0
    assert X_test.nnz == X.nnz and (X_test.data == 0).any()
    assert_array_equal((X_train + X_test).toarray(), X.toarray())
    assert best.theta.dims == (300, 3) and len(rest) == 1
    assert best.loss[-1] <= rest[0].loss[-1]            # selected by the loss it recorded: the held-out one
    for model in (best, rest[0]):
        got = loss.thinned_mean_negative_pois_llh(X_test, theta=model.theta, beta=model.beta, frac=0.2)
        want = numpy_thinned_loss(X_test, model, 0.2)
        print("thinned loss %.15g, numpy %.15g, rel %.3g" % (got, want, abs(got - want) / abs(want)))
        assert_allclose(got, want, rtol=1e-12, atol=0)
        # the same through the engine, for X_test in GPU memory
        G_test = torch.sparse_coo_tensor(torch.tensor(np.stack([X_test.row, X_test.col]).astype(np.int64)),
                                         torch.tensor(X_test.data), X_test.shape).to("cuda:0")
        assert_allclose(loss.thinned_mean_negative_pois_llh(G_test, theta=model.theta, beta=model.beta, frac=0.2), want,
                        rtol=1e-12, atol=0)
    # a run whose last check is its last iteration records the held-out loss of the model it returns
    np.random.seed(1)
    short = amd.run_trials(X, 3, ntrials=1, thin=0.2, max_iter=11, verbose=False)
    assert_allclose(short.loss[-1], numpy_thinned_loss(X_test, short, 0.2), rtol=1e-12, atol=0)
    # the model was fitted to the train counts: the training loss on X_train is what a plain fit of X_train records
    np.random.seed(1)
    plain = amd.run_trials(X_train, 3, ntrials=1, max_iter=11, verbose=False)
    assert plain.theta == short.theta and plain.beta == short.beta


def test_thin_none_changes_nothing(amd):
    X = planted()
    np.random.seed(5)
    a = amd.run_trials(X, 3, ntrials=2, max_iter=40, verbose=False)
    np.random.seed(5)
    b = amd.run_trials(X, 3, ntrials=2, max_iter=40, verbose=False, thin=None)
    assert a.theta == b.theta and a.beta == b.beta and a.xi == b.xi and a.eta == b.eta
    assert a.loss == b.loss
    # the pool takes the same argument: the loss it records (here at the last iteration) is the held-out one
    np.random.seed(5)
    c, = amd.run_trials_pool(X, 3, ntrials=2, max_iter=11, verbose=False, thin=0.2, thin_seed=8)
    X_test = amd.thin_counts(X, 0.2, seed=8)[1]
    assert_allclose(c.loss[-1], numpy_thinned_loss(X_test, c, 0.2), rtol=1e-12, atol=0)


def test_train_thin_from_the_shell(tmp_path):
    """`scHPF train --thin 0.2` on the golden PJ030 matrix (a genes x cells text file: loaded like `prep` loads it and
    handed over as the .mtx `train` reads): both split files are written and add up to the input."""
    from scipy.io import mmread, mmwrite
    from schpf_amd.preprocessing import load_txt
    X, _ = load_txt(os.path.join(GOLDEN, "PJ030merge.c300t400_g0t500.matrix.txt"), verbose=False)
    mtx = tmp_path / "pj.mtx"
    mmwrite(str(mtx), X, field="integer")
    exe = [sys.executable, os.path.join(ROOT, "bin", "scHPF")]
    subprocess.check_call(exe + ["train", "-i", str(mtx), "-o", str(tmp_path / "m"), "-p", "pj", "-k", "3", "-M", "20",
                                 "--thin", "0.2", "--thin-seed", "3", "--quiet"])
    out = tmp_path / "m"
    assert (out / "pj.scHPF_K3_b0_1trials.joblib").exists()
    train, test = mmread(str(out / "pj.thin_train.mtx")), mmread(str(out / "pj.thin_test.mtx"))
    assert train.shape == X.shape and test.shape == X.shape
    assert_array_equal((train + test).toarray(), X.toarray())
    assert 0 < test.sum() < train.sum()
    want_train, want_test = __import__("schpf_amd").thin_counts(X, 0.2, seed=3)
    assert_array_equal(test.toarray(), want_test.toarray())
    import json
    args = json.load(open(str(out / "pj.train_commandline_args.json")))
    assert args["thin"] == 0.2 and args["thin_seed"] == 3
