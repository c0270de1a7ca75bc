"""Simulated doublets and doublet scores on the GPU.  The pair sum is integer work: every comparison with
the library's host restatement (schpf_debug_doublet_rows; tests/test_doublets_host.py pins it to the definition) is for
equal bits -- whatever the storage of the matrix and wherever it lives.  Then the Python surface: simulate_doublets,
doublet_scores on a planted matrix with injected doublets, and the command line."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.sparse import coo_matrix, csr_matrix

from conftest import GOLDEN, ROOT
from _doublet_reference import (LONG, PIECE, _p, call_rows, debug_rows, draw_parents, host_parents, kernel_matrix, knn_counts,
                                scrublet, spoiled)
from _thin_reference import KINDS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
SEED = 0x1234567887654321


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


@pytest.fixture(scope="module")
def case():
    """The kernel matrix (one row of LONG = 300 entries: a wavefront takes PIECE = 64 per pass), its pairs, and their sums by
    the host restatement."""
    X, parents = kernel_matrix()
    assert np.diff(X.indptr)[13] == LONG > 2 * PIECE
    want = debug_rows(X, parents)
    for a in want + (parents,):
        a.setflags(write=False)
    return X, parents, want


def device_rows(X, parents, idx=np.int32, indptr=np.int64, val=None, stream=None, fill=True, short=0):
    """schpf_doublet_rows_device on torch tensors of the given dtypes; results as NumPy arrays, (-7 where nothing was
    written)."""
    from schpf_amd import _lib
    lib = _lib.load()
    data = np.asarray(X.data if val is None else X.data.astype(val))
    parents = np.ascontiguousarray(parents, np.int32).reshape(-1, 2)
    n_pairs = parents.shape[0]
    d_indptr = torch.tensor(np.asarray(X.indptr, indptr), device="cuda:0")
    d_indices = torch.tensor(np.asarray(X.indices, idx), device="cuda:0")
    d_val = torch.tensor(data, device="cuda:0")
    d_parents = torch.tensor(parents, device="cuda:0")
    d_out = torch.full((n_pairs + 1,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
    kind = lambda d: _lib.IDX_I64 if np.dtype(d) == np.int64 else _lib.IDX_I32  # noqa: E731
    args = (0, ctypes.c_void_p(stream), X.shape[0], X.shape[1], len(data), ptr(d_indptr), kind(indptr), ptr(d_indices), kind(idx),
            ptr(d_val), KINDS[data.dtype], n_pairs, ptr(d_parents))
    _lib.check(lib.schpf_doublet_rows_device(*(args + (ptr(d_out), None, None, 0))))
    out_indptr = d_out.cpu().numpy()
    if not fill:
        return out_indptr, None, None
    total = int(out_indptr[-1])
    d_again = torch.full((n_pairs + 1,), -7, dtype=torch.int64, device="cuda:0")
    d_oi = torch.full((max(total, 1),), -7, dtype=torch.int32, device="cuda:0")
    d_ov = torch.full((max(total, 1),), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(lib.schpf_doublet_rows_device(*(args + (ptr(d_again), ptr(d_oi), ptr(d_ov), total - short))))
    assert_array_equal(d_again.cpu().numpy(), out_indptr)
    return out_indptr, d_oi.cpu().numpy()[:total], d_ov.cpu().numpy()[:total]


def same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype
        assert_array_equal(g, w)


@pytest.mark.parametrize("n_pairs", [1, 65, None])
def test_both_entry_points_equal_the_host_restatement(amd, case, n_pairs):
    X, parents, want = case
    if n_pairs is not None:
        parents = parents[:n_pairs]
        want = (want[0][:n_pairs + 1], want[1][:want[0][n_pairs]], want[2][:want[0][n_pairs]])
    same(device_rows(X, parents), want)
    same(call_rows("schpf_doublet_rows", X, parents, device=0), want)
    # the sizing call alone
    assert_array_equal(device_rows(X, parents, fill=False)[0], want[0])
    assert_array_equal(call_rows("schpf_doublet_rows", X, parents, device=0, fill=False)[0], want[0])


@pytest.mark.parametrize("idx,indptr,val,stream", [(np.int64, np.int64, np.float64, None), (np.int32, np.int32, np.int32, None),
                                                   (np.int64, np.int32, np.float32, 1), (np.int32, np.int64, np.int64, None)])
def test_every_storage_gives_one_result(amd, case, idx, indptr, val, stream):
    X, parents, want = case
    same(device_rows(X, parents, idx=idx, indptr=indptr, val=val, stream=stream), want)


def test_on_a_stream_of_the_callers(amd, case):
    X, parents, want = case
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        same(device_rows(X, parents, stream=int(s.cuda_stream)), want)
    s.synchronize()


def test_capacity_one_short_is_refused(amd, case):
    X, parents, want = case
    message = "capacity must be at least the %d entries of the result, got %d" % (want[0][-1], want[0][-1] - 1)
    with pytest.raises(ValueError, match=message):
        device_rows(X, parents, short=1)
    with pytest.raises(ValueError, match=message):
        call_rows("schpf_doublet_rows", X, parents, device=0, short=1)


@pytest.mark.parametrize("n_sim", [1, 65, 1000])
def test_parents_from_the_kernel_equal_the_host_draw(amd, n_sim):
    from schpf_amd import _lib
    lib = _lib.load()
    for ncells, first in ((257, 0), (2 ** 31 - 1, 2 ** 32 - 3), (1, 5)):
        out = torch.full((n_sim, 2), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        _lib.check(lib.schpf_doublet_parents_device(0, None, first, n_sim, ncells, ctypes.c_uint64(SEED),
                                                    ctypes.c_void_p(out.data_ptr())))
        assert_array_equal(out.cpu().numpy(), host_parents(first, n_sim, ncells, SEED))
    assert_array_equal(host_parents(0, n_sim, 257, SEED), draw_parents(0, n_sim, 257, SEED))


def test_empty_inputs_and_a_bad_device(amd, case):
    from schpf_amd import _lib
    lib = _lib.load()
    X, parents, want = case
    assert lib.schpf_doublet_rows_device(0, None, 80, 700, 5, None, 0, None, 0, None, 0, 0, None, None, None, None, 0) == 0
    assert lib.schpf_doublet_rows(0, 80, 700, 5, None, None, None, 0, 0, None, None, None, None, 0) == 0
    assert lib.schpf_doublet_parents_device(0, None, 0, 0, 5, ctypes.c_uint64(0), None) == 0
    # no entries: every row of the result is empty, no input pointer is looked at
    d_out = torch.full((4,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.schpf_doublet_rows_device(0, None, 80, 700, 0, None, 0, None, 0, None, 0, 3, None,
                                         ctypes.c_void_p(d_out.data_ptr()), None, None, 0) == 0
    assert not d_out.cpu().numpy().any()
    out = np.full(4, -7, np.int64)
    assert lib.schpf_doublet_rows(0, 80, 700, 0, None, None, None, 0, 3, None, _p(out), None, None, 0) == 0
    assert not out.any()
    E, none = amd.simulate_doublets(csr_matrix((4, 5), dtype=np.int32), n_sim=3)
    assert E.shape == (3, 5) and E.nnz == 0 and none.shape == (3, 2)
    G, _ = amd.simulate_doublets(torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0), (4, 5)).to("cuda:0"),
                                 n_sim=3)
    assert tuple(G.shape) == (3, 5) and G.values().numel() == 0 and G.device.type == "cuda"
    Z, none = amd.simulate_doublets(X, n_sim=0)
    assert Z.shape == (0, 700) and none.shape == (0, 2)
    assert lib.schpf_doublet_rows_device(99, None, 80, 700, 0, None, 0, None, 0, None, 0, 0, None, None, None, None, 0) != 0
    assert b"no such HIP device" in lib.schpf_last_error()
    assert lib.schpf_doublet_parents_device(99, None, 0, 0, 5, ctypes.c_uint64(0), None) != 0
    assert b"no such HIP device" in lib.schpf_last_error()
    with pytest.raises(ValueError, match="device=1 was asked for"):
        amd.simulate_doublets(torch.sparse_csr_tensor(torch.tensor(X.indptr), torch.tensor(X.indices), torch.tensor(X.data),
                                                      size=X.shape).to("cuda:0"), device=1)


@pytest.mark.parametrize("kind", ["indptr", "indptr_end", "index", "order", "value", "parent"])
def test_validation_on_the_device(amd, kind):
    """Two offenders of a kind, the smaller one set behind the larger: the smaller one is named, by both entry points and
    for both index widths."""
    X, parents, message = spoiled(kind)
    with pytest.raises(ValueError) as err:
        device_rows(X, parents, fill=False)
    assert str(err.value) == message
    with pytest.raises(ValueError) as err:
        call_rows("schpf_doublet_rows", X, parents, device=0, fill=False)
    assert str(err.value) == message
    with pytest.raises(ValueError) as err:
        device_rows(X, parents, idx=np.int64, indptr=np.int64, val=np.float64, fill=False)
    assert str(err.value) == message


def test_validation_of_wide_indices_and_fractions(amd):
    X, parents = kernel_matrix()
    wide = X.copy()
    wide.indices = wide.indices.astype(np.int64)
    wide.indices[123] = 2 ** 32 + 5              # in range once cut to 32 bits
    with pytest.raises(ValueError, match="column index out of range at entry 123$"):
        device_rows(wide, parents, idx=np.int64, fill=False)
    half = X.astype(np.float32)
    half.data[2000] = half.data[700] = 2.5
    with pytest.raises(ValueError, match="offending entry 700$"):
        device_rows(half, parents, fill=False)


def dense_sum(X, parents):
    D = X.toarray().astype(np.int64)
    return D[parents[:, 0]] + D[parents[:, 1]]


def test_simulate_doublets_from_every_source(amd, case):
    X, parents, want = case
    # SciPy CSR, the pairs drawn
    S, drawn = amd.simulate_doublets(X, seed=SEED)
    assert isinstance(S, csr_matrix) and S.shape == (160, 700) and S.dtype == X.dtype and drawn.dtype == np.int32
    assert_array_equal(drawn, draw_parents(0, 160, 80, SEED))
    assert_array_equal(S.toarray(), dense_sum(X, drawn))
    assert S.has_sorted_indices
    assert_array_equal(amd.simulate_doublets(X, n_sim=7, seed=SEED)[1], drawn[:7])
    # a torch COO in permuted order, float32: brought to CSR on the GPU, the result there, dtype kept
    C = X.tocoo()
    perm = np.random.RandomState(1).permutation(C.nnz)
    index = torch.tensor(np.stack([C.row[perm], C.col[perm]]).astype(np.int64), device="cuda:0")
    T, t_drawn = amd.simulate_doublets(torch.sparse_coo_tensor(index, torch.tensor(C.data[perm].astype(np.float32), device="cuda:0"),
                                                               (80, 700)), seed=SEED)
    assert T.layout == torch.sparse_csr and T.device.type == "cuda" and T.values().dtype == torch.float32
    assert t_drawn.device.type == "cuda" and t_drawn.dtype == torch.int32
    assert_array_equal(t_drawn.cpu().numpy(), drawn)
    assert_array_equal(T.crow_indices().cpu().numpy(), S.indptr)
    assert_array_equal(T.col_indices().cpu().numpy(), S.indices)
    assert_array_equal(T.values().cpu().numpy(), S.data.astype(np.float32))
    # a torch CSR, int32 and int64 indices, the pairs given: used as they are
    for idt in (torch.int32, torch.int64):
        G = torch.sparse_csr_tensor(torch.tensor(X.indptr).to(idt), torch.tensor(X.indices).to(idt),
                                    torch.tensor(X.data.astype(np.int64)), size=(80, 700)).to("cuda:0")
        R, given = amd.simulate_doublets(G, parents=parents)
        assert R.values().dtype == torch.int64 and tuple(R.shape) == (len(parents), 700)
        assert_array_equal(given.cpu().numpy(), parents)
        assert_array_equal(R.crow_indices().cpu().numpy(), want[0])
        assert_array_equal(R.col_indices().cpu().numpy(), want[1])
        assert_array_equal(R.values().cpu().numpy(), want[2])
    H, given = amd.simulate_doublets(X, parents=parents)
    assert_array_equal(given, parents)
    same((H.indptr.astype(np.int64), H.indices, H.data), want)
    with pytest.raises(ValueError, match=r"parents must be in \[0, ncells\); offending pair 2$"):
        amd.simulate_doublets(X, parents=np.array([[0, 1], [2, 3], [80, 0]]))


def planted_with_doublets(n_each=185, n_doublets=30, ngenes=150, seed=7):
    """Two populations with their own genes, then n_doublets rows that are the sum of one cell of each: (X, injected)."""
    rng = np.random.RandomState(seed)
    K = 3
    beta = rng.gamma(0.4, 1.0, (ngenes, K))
    beta[:ngenes // 2, 1] *= 0.05
    beta[ngenes // 2:, 0] *= 0.05
    theta = rng.gamma(2.0, 1.0, (2 * n_each, K))
    theta[:n_each, 1] *= 0.02
    theta[n_each:, 0] *= 0.02
    singles = rng.poisson(theta @ beta.T)
    a, b = rng.randint(0, n_each, n_doublets), rng.randint(n_each, 2 * n_each, n_doublets)
    X = coo_matrix(np.concatenate([singles, singles[a] + singles[b]]).astype(np.int32))
    X.eliminate_zeros()
    injected = np.zeros(X.shape[0], bool)
    injected[2 * n_each:] = True
    return X.tocoo(), injected


def auc(scores, positive):
    order = np.argsort(scores, kind="stable")
    ranks = np.empty(len(scores))
    ranks[order] = np.arange(1, len(scores) + 1)
    n_pos, n_neg = positive.sum(), (~positive).sum()
    return (ranks[positive].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg)


def test_doublet_scores_of_a_planted_matrix(amd, monkeypatch):
    from schpf_amd import neighbors
    X, injected = planted_with_doublets()
    assert X.shape == (400, 150) and injected.sum() == 30
    np.random.seed(0)
    model = amd.scHPF(3, max_iter=30, verbose=False).fit(X)
    seen = {}
    knn = neighbors.knn

    def recording(query, *args, **kwargs):      # the embedding the neighbours are taken of
        seen["embedded"] = np.array(query)
        return knn(query, *args, **kwargs)

    monkeypatch.setattr(neighbors, "knn", recording)
    np.random.seed(1)
    found = model.doublets(X, seed=3, threshold=0.2, verbose=False)
    n_obs, n_sim = 400, 800
    embedded = seen["embedded"]
    assert embedded.shape == (n_obs + n_sim, 3)
    assert found["k_adj"] == 30 and found["parents"].shape == (n_sim, 2)          # k = round(0.5 sqrt(400)) = 10, r = 2
    assert_array_equal(found["parents"], draw_parents(0, n_sim, n_obs, 3))
    # the integers: a NumPy brute force on the same embedding, under the key of DESIGN.md 16
    counts = knn_counts(embedded, 30, n_obs)[0]
    assert_array_equal(found["k_sim"], counts[:n_obs])
    assert_array_equal(found["k_sim_sim"], counts[n_obs:])
    # the scores: host float64 arithmetic on both sides
    score, se = scrublet(counts, 30, 2.0)
    assert_allclose(found["scores"], score[:n_obs], rtol=1e-12, atol=0)
    assert_allclose(found["se"], se[:n_obs], rtol=1e-12, atol=0)
    assert_allclose(found["scores_sim"], score[n_obs:], rtol=1e-12, atol=0)
    assert_array_equal(found["calls"], found["scores"] > 0.2)
    assert found["detectable_fraction"] == np.mean(found["scores_sim"] > 0.2)
    print("doublet scores: mean of the injected rows %.4f, of the others %.4f, AUC %.4f, detectable fraction %.3f"
          % (found["scores"][injected].mean(), found["scores"][~injected].mean(), auc(found["scores"], injected),
             found["detectable_fraction"]))
    assert found["scores"][injected].mean() > found["scores"][~injected].mean()
    # the same matrix from GPU memory: the same pairs and, the projection being the device-initialised one, a score per row
    G = torch.sparse_coo_tensor(torch.tensor(np.stack([X.row, X.col]).astype(np.int64)), torch.tensor(X.data), X.shape).to("cuda:0")
    on_gpu = amd.doublet_scores(model, G, seed=3, verbose=False)
    assert_array_equal(on_gpu["parents"], found["parents"])
    assert on_gpu["scores"].shape == (n_obs,) and on_gpu["k_adj"] == 30
    assert on_gpu["scores"][injected].mean() > on_gpu["scores"][~injected].mean()


def test_score_doublets_from_the_shell(amd, tmp_path):
    """`scHPF score -i X --doublets` on the golden PJ030 matrix: both files, one row per cell and per simulated row; a run
    without the option writes the arguments file it wrote before there was one."""
    from scipy.io import mmwrite
    from schpf_amd.preprocessing import load_txt
    X, _ = load_txt(os.path.join(GOLDEN, "PJ030merge.c300t400_g0t500.matrix.txt"), verbose=False)
    mtx, path = tmp_path / "pj.mtx", str(tmp_path / "model.joblib")
    mmwrite(str(mtx), X, field="integer")
    np.random.seed(0)
    amd.save_model(amd.scHPF(3, max_iter=15, verbose=False).fit(X), path)
    exe = [sys.executable, os.path.join(ROOT, "bin", "scHPF")]
    subprocess.check_call(exe + ["score", "-m", path, "-i", str(mtx), "-o", str(tmp_path / "d"), "--doublets", "--doublet-seed", "5",
                                 "--doublet-ratio", "1.5"], stdout=subprocess.DEVNULL)
    n_obs = X.shape[0]
    n_sim = int(round(1.5 * n_obs))
    scores = np.loadtxt(str(tmp_path / "d" / "doublet_scores.txt"), ndmin=2)
    sim = np.loadtxt(str(tmp_path / "d" / "doublet_scores_sim.txt"), ndmin=2)
    assert scores.shape == (n_obs, 3) and sim.shape == (n_sim, 4)
    assert (scores[:, 0] > 0).all() and (scores[:, 0] < 1).all() and (scores[:, 2] == np.round(scores[:, 2])).all()
    assert_array_equal(sim[:, 2:], draw_parents(0, n_sim, n_obs, 5))
    args = json.load(open(str(tmp_path / "d" / "score_commandline_args.json")))
    assert args["doublets"] is True and args["doublet_seed"] == 5 and args["doublet_ratio"] == 1.5 and args["doublet_rate"] == 0.06
    subprocess.check_call(exe + ["score", "-m", path, "-i", str(mtx), "-o", str(tmp_path / "plain")], stdout=subprocess.DEVNULL)
    plain = json.load(open(str(tmp_path / "plain" / "score_commandline_args.json")))
    assert sorted(plain) == ["cmd", "genefile", "input", "model", "name_col", "outdir", "prefix"]
    assert set(os.listdir(str(tmp_path / "d"))) - set(os.listdir(str(tmp_path / "plain"))) == {"doublet_scores.txt",
                                                                                              "doublet_scores_sim.txt"}
