"""Host-side pieces of bench.py that run without a GPU: the synthetic generator (generator A),
the row split of the N > 1 bench -- every rank draws the N = 1 matrix and keeps its block of the product's
nnz-balanced partition -- and the writer behind --dump-outputs."""
import os

import numpy as np
import pytest
from scipy.sparse import coo_matrix

from conftest import synthetic_counts


@pytest.mark.parametrize("shape", [(300, 1000, 0.03, 42), (1000, 500, 0.05, 3), (7, 3, 0.5, 1), (2000, 1500, 0.08, 9)])
def test_bench_generator_equals_the_fixture_recipe(shape):
    """bench.synthetic_block sums duplicates by sorting packed keys; it must return, entry for entry, what the
    reference's fixture recipe (draws, then coo_matrix.sum_duplicates) returns."""
    from bench import synthetic_block
    n, g, dens, seed = shape
    A = synthetic_block(n, g, dens, seed)
    B = synthetic_counts(n, g, dens, seed=seed)
    assert A.shape == B.shape and A.nnz == B.nnz
    assert A.row.dtype == np.int32 and A.col.dtype == np.int32 and A.data.dtype == np.int32
    assert np.array_equal(A.row, B.row) and np.array_equal(A.col, B.col) and np.array_equal(A.data, B.data)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_rank_blocks_tile_the_unsharded_matrix(world):
    from bench import synthetic_block
    from schpf_amd.sharded import row_partition, take_rows
    X = synthetic_block(5000, 800, 0.04, 42)
    bounds = row_partition(X, world)
    assert bounds[0] == 0 and bounds[-1] == X.shape[0] and np.all(np.diff(bounds) >= 0)
    parts = [take_rows(X, int(bounds[r]), int(bounds[r + 1])) for r in range(world)]
    assert sum(p[0].nnz for p in parts) == X.nnz
    back = coo_matrix((np.concatenate([p[0].data for p in parts]),
                       (np.concatenate([p[0].row + int(bounds[r]) for r, p in enumerate(parts)]),
                        np.concatenate([p[0].col for p in parts]))), shape=X.shape)
    assert (back != X).nnz == 0
    nnz = np.array([p[0].nnz for p in parts])
    assert nnz.max() - nnz.min() <= 2 * np.bincount(X.row, minlength=X.shape[0]).max()


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_per_rank_draw_gives_the_blocks_of_the_whole_matrix(world):
    """bench.py --gpus N --config c5: no rank draws the whole matrix (synthetic_slabs_of_rank).  Ranks are played by
    threads, the all-reduce by a barrier: every rank ends up with exactly its block of the product's row partition
    of the whole-matrix draw, the global nnz and marginals, having drawn about 1 / world of it."""
    import threading
    from bench import synthetic_slabs, synthetic_slabs_of_rank
    from schpf_amd.sharded import row_partition, take_rows
    N, G, dens, slab = 20000, 3000, 0.02, 500
    X = synthetic_slabs(N, G, dens, seed=42, slab_rows=slab)
    bounds_want = row_partition(X, world)
    barrier = threading.Barrier(world)
    box, out, errors = {}, {}, []

    def all_reduce_of(rank):
        def all_reduce(a):
            box[rank] = a
            barrier.wait()
            total = sum(box[r] for r in range(world))
            barrier.wait()
            return total
        return all_reduce

    def run(rank):
        try:
            out[rank] = synthetic_slabs_of_rank(N, G, dens, 42, world, rank, all_reduce_of(rank), slab_rows=slab, threads=1)
        except Exception as e:      # noqa: BLE001
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    for rank in range(world):
        Xl, bounds, facts = out[rank]
        want, _ = take_rows(X, int(bounds_want[rank]), int(bounds_want[rank + 1]))
        assert np.array_equal(bounds, bounds_want)
        assert Xl.shape == want.shape
        assert np.array_equal(Xl.row, want.row) and np.array_equal(Xl.col, want.col) and np.array_equal(Xl.data, want.data)
        assert facts["nnz_total"] == X.nnz
        assert np.array_equal(facts["row_sums"], np.asarray(X.sum(1)).ravel())
        assert np.array_equal(facts["col_sums"], np.asarray(X.sum(0)).ravel())
        # 1 / world of the draws and at most three boundary slabs more
        assert facts["draws"] <= facts["draws_whole_matrix"] * (1.0 / world + 3.0 / facts["slabs_total"]) + 1


class _FakeEngine:
    """What dump_outputs reads of a DeviceCAVI: get_gamma(name) -> (shape, rate) in the model dtype."""

    def __init__(self, N, G, K, dtype, seed=5):
        rng = np.random.RandomState(seed)
        dims = {"xi": (N,), "theta": (N, K), "eta": (G,), "beta": (G, K)}
        self.state = {n: (rng.gamma(2.0, 1.0, d).astype(dtype), rng.gamma(3.0, 1.0, d).astype(dtype))
                      for n, d in dims.items()}

    def get_gamma(self, name):
        s, r = self.state[name]
        return s.copy(), r.copy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dump_outputs_writes_the_whole_model(tmp_path, dtype):
    """bench.py --dump-outputs: below the size limit every array, bit for bit, in the model dtype."""
    import bench
    eng = _FakeEngine(300, 200, 7, dtype)
    bench.dump_outputs(eng, str(tmp_path))
    names = [f[:-4] for f in os.listdir(str(tmp_path))]
    assert sorted(names) == sorted(n + p for n in ("xi", "theta", "eta", "beta") for p in ("_shape", "_rate"))
    for n, (s, r) in eng.state.items():
        for part, want in (("_shape", s), ("_rate", r)):
            got = np.load(str(tmp_path / (n + part + ".npy")))
            assert got.dtype == dtype and np.array_equal(got, want)


def test_dump_outputs_samples_rows_beyond_the_limit(tmp_path, monkeypatch):
    """Above the limit: one fixed, seeded sample of rows per side, the same from run to run, within the limit in
    all (row indices included), with the indices written beside it."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    eng = _FakeEngine(3000, 1000, 9, np.float64)
    bench.dump_outputs(eng, str(tmp_path / "a"))
    bench.dump_outputs(eng, str(tmp_path / "b"))
    names = [f[:-4] for f in os.listdir(str(tmp_path / "a"))]
    assert "cell_rows" in names and "gene_rows" in names
    total = 0
    for name in names:
        a, b = np.load(str(tmp_path / "a" / (name + ".npy"))), np.load(str(tmp_path / "b" / (name + ".npy")))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        total += a.nbytes
    assert total <= 200_000
    for side, (n, names_of_side) in {"cell": (3000, ("xi", "theta")), "gene": (1000, ("eta", "beta"))}.items():
        rows = np.load(str(tmp_path / "a" / (side + "_rows.npy")))
        assert 0 < rows.size < n and np.all(np.diff(rows) > 0) and rows[-1] < n
        keep = rows.astype(np.int64)
        for name in names_of_side:
            s, r = eng.state[name]
            assert np.array_equal(np.load(str(tmp_path / "a" / (name + "_shape.npy"))), s[keep])
            assert np.array_equal(np.load(str(tmp_path / "a" / (name + "_rate.npy"))), r[keep])


def test_bench_options():
    """The options every benchmark run relies on, readable without a GPU (argparse exits before any device work)."""
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, "bench.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout
