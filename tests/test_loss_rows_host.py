"""CPU-side checks of the per-row loss: the C ABI exports and binds schpf_loss_rows, nothing computes
without a GPU, the float64 yardstick of the GPU tests reproduces the reference's own per-cell vector, and
`scHPF score -i` writes its two extra files (the device call replaced by the yardstick)."""
import ctypes
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose

from conftest import GOLDEN, load_golden, golden_coo
from schpf_amd import _lib
import _loss_rows_reference as ref


def test_library_exports_and_binds_loss_rows():
    lib = _lib.load()
    assert hasattr(lib, "schpf_loss_rows"), "libschpf_hip.so does not export schpf_loss_rows"
    dblp, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    assert _lib.SIGNATURES["schpf_loss_rows"] == [ctypes.c_void_p, ctypes.c_int, dblp, dblp, i64p]
    assert list(lib.schpf_loss_rows.argtypes) == [ctypes.c_void_p, ctypes.c_int, dblp, dblp, i64p]
    assert (_lib.BY_CELL, _lib.BY_GENE) == (0, 1)
    # a NULL context is refused with a message, not dereferenced
    out, cnt = (ctypes.c_double * 1)(), (ctypes.c_int64 * 1)()
    assert lib.schpf_loss_rows(None, 0, out, out, cnt) != 0
    assert b"NULL" in lib.schpf_last_error()


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_loss_rows_needs_a_gpu(ops):
    """Without a GPU the per-row loss raises like every computing call: no engine, hence no loss_rows."""
    from schpf_amd import DeviceCAVI, HPF_Gamma, loss
    with pytest.raises(_lib.SchpfHipError):
        DeviceCAVI(10, 10, 2).loss_rows("cell")
    theta = HPF_Gamma(ops["theta_shape"], ops["theta_rate"])
    beta = HPF_Gamma(ops["beta_shape"], ops["beta_rate"])
    for fn in (loss.cellmean_negative_pois_llh, loss.genemean_negative_pois_llh):
        with pytest.raises(_lib.SchpfHipError):
            fn(golden_coo(ops), theta=theta, beta=beta)


def test_yardstick_reproduces_the_reference_cellmean(ops):
    """tests/golden/ops_*.npz `cellmean_neg_llh` was written by the reference's scHPF.cellmean_negative_pois_llh: the
    yardstick the GPU tests compare against must give it, at test_ops_gpu.py's tolerance for that vector."""
    dt = ops["theta_shape"].dtype
    X = golden_coo(ops)
    theta, beta = (ops["theta_shape"], ops["theta_rate"]), (ops["beta_shape"], ops["beta_rate"])
    got = ref.rowmean_negative(X, theta, beta, "cell")
    assert_allclose(got, ops["cellmean_neg_llh"], rtol=1e-5 if dt == np.float32 else 1e-7)
    # both axes account for every stored entry, and their totals are the scalar loss's
    c, g = ref.loss_rows(X, theta, beta, "cell"), ref.loss_rows(X, theta, beta, "gene")
    assert c["count"].sum() == g["count"].sum() == X.nnz
    assert_allclose(c["llh"].sum(), g["llh"].sum(), rtol=1e-12)
    assert_allclose(-(c["llh"].sum() - c["gl"].sum()) / X.nnz, float(ops["mean_neg_llh"]),
                    rtol=1e-6 if dt == np.float32 else 1e-9)


def test_yardstick_counts_zeros_and_duplicates_and_leaves_empty_rows_nan():
    from scipy.sparse import coo_matrix
    X = coo_matrix((np.array([2.0, 0.0, 3.0, 3.0, 0.5]), (np.array([0, 0, 2, 2, 2]), np.array([1, 2, 1, 1, 0]))),
                   shape=(4, 3))
    th = (np.full((4, 2), 2.0), np.ones((4, 2)))
    be = (np.full((3, 2), 0.5), np.ones((3, 2)))            # r = 2 everywhere
    t = ref.loss_rows(X, th, be, "cell")
    assert t["count"].tolist() == [2, 0, 3, 0]
    assert_allclose(t["llh"][0], 2 * np.log(2.0) - 2.0 - 2.0)   # the stored zero adds -r
    assert_allclose(t["llh"][2], 6.5 * np.log(2.0) - 6.0)
    m = ref.rowmean_negative(X, th, be, "cell")
    assert np.isnan(m).tolist() == [False, True, False, True]
    assert ref.loss_rows(X, th, be, "gene")["count"].tolist() == [1, 3, 1]


def test_rowmean_helper_is_quiet_nan_for_empty_rows():
    import warnings
    from schpf_amd.engine import rowmean_negative
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = rowmean_negative(np.array([-3.0, 0.0]), np.array([1.0, 0.0]), np.array([2, 0]))
    assert out.dtype == np.float64 and out[0] == 2.0 and np.isnan(out[1])


def test_threaded_shards_concatenate_cells_and_sum_genes():
    """ThreadedShards.loss_rows over stand-in engines: cells in the original order, genes summed."""
    from schpf_amd.sharded import ThreadedShards

    class Shard(object):
        def __init__(self, k):
            self.k = k

        def loss_rows(self, by):
            n = 2 + self.k if by == "cell" else 3
            return (np.full(n, -1.0 - self.k), np.full(n, 0.5 * (1 + self.k)), np.full(n, 1 + self.k, np.int64))

        def close(self):
            pass

    from concurrent.futures import ThreadPoolExecutor
    sh = ThreadedShards.__new__(ThreadedShards)
    sh.engines, sh.world, sh._pool = [Shard(0), Shard(1)], 2, ThreadPoolExecutor(max_workers=2)
    try:
        llh, gl, cnt = sh.loss_rows("cell")
        assert llh.tolist() == [-1.0, -1.0, -2.0, -2.0, -2.0] and cnt.tolist() == [1, 1, 2, 2, 2]
        llh, gl, cnt = sh.loss_rows("gene")
        assert llh.tolist() == [-3.0] * 3 and gl.tolist() == [1.5] * 3 and cnt.tolist() == [3] * 3
        assert cnt.dtype == np.int64
        assert_allclose(sh.genemean_negative_pois_llh(), [1.5] * 3)
        with pytest.raises(ValueError):
            sh.loss_rows("factor")
    finally:
        sh.close()


def test_score_with_input_writes_cell_and_gene_loss(tmp_path, monkeypatch):
    """`scHPF score -i X` adds cell_loss.txt / gene_loss.txt; without -i the file set is what it was."""
    import joblib
    from scipy.io import mmwrite
    from scipy.sparse import coo_matrix
    from schpf_amd import cli, loss
    model = os.path.join(GOLDEN, "ref_model_f64.joblib")
    m = joblib.load(model)
    N, G = m.theta.vi_shape.shape[0], m.beta.vi_shape.shape[0]
    rng = np.random.RandomState(3)
    nnz = 4 * N
    X = coo_matrix((rng.randint(1, 5, nnz), (rng.randint(0, N, nnz), rng.randint(0, G, nnz))), shape=(N, G))
    X.sum_duplicates()
    mmwrite(str(tmp_path / "x.mtx"), X.tocoo(), field="integer")

    def on_host(by):   # the device evaluation, played by the yardstick
        def fn(X, *, theta, beta, device=None, **kwargs):
            return ref.rowmean_negative(X.tocoo(), (theta.vi_shape, theta.vi_rate), (beta.vi_shape, beta.vi_rate), by)
        return fn
    monkeypatch.setattr(loss, "cellmean_negative_pois_llh", on_host("cell"))
    monkeypatch.setattr(loss, "genemean_negative_pois_llh", on_host("gene"))

    assert cli.main(["score", "-m", model, "-o", str(tmp_path / "plain")]) == 0
    assert cli.main(["score", "-m", model, "-o", str(tmp_path / "with"), "-i", str(tmp_path / "x.mtx")]) == 0
    plain, with_x = set(os.listdir(str(tmp_path / "plain"))), set(os.listdir(str(tmp_path / "with")))
    assert plain == {"cell_score.txt", "gene_score.txt", "mean_cellscore_fraction.txt", "maximum_overlaps.txt",
                     "score_commandline_args.json"}
    assert with_x == plain | {"cell_loss.txt", "gene_loss.txt"}
    import json
    assert "input" not in json.load(open(str(tmp_path / "plain" / "score_commandline_args.json")))
    cl, gl = np.loadtxt(str(tmp_path / "with" / "cell_loss.txt")), np.loadtxt(str(tmp_path / "with" / "gene_loss.txt"))
    assert cl.shape == (N,) and gl.shape == (G,)
    assert_allclose(cl, on_host("cell")(X, theta=m.theta, beta=m.beta), equal_nan=True)
    with pytest.raises(ValueError):
        mmwrite(str(tmp_path / "bad.mtx"), coo_matrix(np.ones((2, 3), int)), field="integer")
        cli.main(["score", "-m", model, "-o", str(tmp_path / "bad"), "-i", str(tmp_path / "bad.mtx")])
