"""An engine whose matrix is replaced: what the previous matrix left behind must not show.

Every upload replaces the whole of what the engine holds per matrix (plans, loss constants, stored-zero segments, per-row
scratch, row-sorted copy, captured graphs).  The tests run a live engine through one matrix, give it another, and ask
for the bits a fresh engine yields for the second matrix alone.  257 x 190 at K = 5: several blocks and LDS windows per
side, a second or so per case."""
from types import SimpleNamespace

import numpy as np
import pytest
from scipy.sparse import coo_matrix

from conftest import synthetic_counts

pytestmark = pytest.mark.gpu

N, G, K = 257, 190, 5
GAMMAS = ("xi", "theta", "eta", "beta")


@pytest.fixture(autouse=True, params=["tile", "gather"])
def plan_kind(request, monkeypatch):
    """The LDS-staged tile plan (what ships) and the L2-gather plan, as in tests/test_engine_gpu.py."""
    monkeypatch.setenv("SCHPF_PLAN", request.param)
    for v in ("SCHPF_HALF", "SCHPF_BALANCE", "SCHPF_WPB", "SCHPF_LOSS_SIDE", "SCHPF_DEVICE_PLAN", "SCHPF_TASKS",
              "SCHPF_GRAPH"):
        monkeypatch.delenv(v, raising=False)
    return request.param


def only_plans(*kinds):
    return pytest.mark.parametrize("plan_kind", list(kinds), indirect=True)


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def matrix_a():
    """About 10 % filled, five explicitly stored zeros, one non-integer value: unpacked entries, a zero list."""
    X = synthetic_counts(N, G, 0.1, seed=11)
    rng = np.random.RandomState(12)
    data = X.data.astype(np.float64)
    data[7] = 2.5
    row = np.concatenate([X.row, rng.randint(0, N, 5)]).astype(np.int32)
    col = np.concatenate([X.col, rng.randint(0, G, 5)]).astype(np.int32)
    return coo_matrix((np.concatenate([data, np.zeros(5)]), (row, col)), shape=(N, G))


def matrix_b():
    """About half of A's entries, integer counts, no stored zeros: packed entries."""
    return synthetic_counts(N, G, 0.05, seed=13)


@pytest.fixture(scope="module")
def mats():
    A, B = matrix_a(), matrix_b()
    assert (A.data == 0).sum() == 5 and (B.data > 0).all() and 1.8 * B.nnz < A.nnz < 2.2 * B.nnz
    return A, B


def fixed_state(n, dtype, seed=3):
    rng = np.random.RandomState(seed)
    g = lambda *d: (rng.uniform(0.2, 3.0, d).astype(dtype), rng.uniform(0.5, 2.0, d).astype(dtype))  # noqa: E731
    return {"xi": g(n), "theta": g(n, K), "eta": g(G), "beta": g(G, K)}


def set_state(eng, st):
    for name in GAMMAS:
        eng.set_gamma(name, *st[name])


def second_part(eng, B, st):
    """Upload B, a fixed state, two stretches of four iterations (from the second on a captured graph may replay)."""
    eng.upload(B, warn=False)
    set_state(eng, st)
    eng.steps(4)
    eng.steps(4)


def everything(eng):
    out = {name: eng.get_gamma(name) for name in GAMMAS}
    out["loss_terms"] = eng.loss_terms()
    out["loss_rows_cell"] = eng.loss_rows("cell")
    out["loss_rows_gene"] = eng.loss_rows("gene")
    out["elbo_terms"] = eng.elbo_terms(1.0, 1.0)
    out["marginals"] = eng.marginals()
    out["upload_info"], out["plan_info"], out["sweep_bytes"] = eng.upload_info(), eng.plan_info(), eng.sweep_bytes()
    return out


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def assert_identical(got, want):
    assert got.keys() == want.keys()
    for key, w in want.items():
        g = got[key]
        if isinstance(w, tuple) and isinstance(w[0], np.ndarray):
            assert len(g) == len(w) and all(same_bits(x, y) for x, y in zip(g, w)), key
        else:
            assert g == w, key


@pytest.fixture(scope="module")
def fresh(amd, mats):
    """What an engine that only ever saw B yields, once per (dtype, plan kind)."""
    cache = {}

    def get(dtype, kind):
        if (dtype, kind) not in cache:
            with amd.DeviceCAVI(N, G, K, dtype=dtype) as eng:
                second_part(eng, mats[1], fixed_state(N, dtype))
                cache[dtype, kind] = everything(eng)
        return cache[dtype, kind]
    return get


def live_engine_on_a(eng, A):
    """Everything that makes per-matrix scratch: iterations (graphs), the loss, per-row losses (zero segments), the ELBO."""
    eng.upload(A, warn=False)
    eng.init_phi_device(5)
    eng.steps(3)
    eng.loss_terms()
    eng.loss_rows("cell")
    eng.loss_rows("gene")
    eng.elbo_terms(1.0, 1.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reuploaded_engine_equals_a_fresh_one(amd, mats, fresh, plan_kind, dtype):
    A, B = mats
    with amd.DeviceCAVI(N, G, K, dtype=dtype) as eng:
        live_engine_on_a(eng, A)
        info_a = eng.upload_info()
        assert info_a["zeros"] == 5 and not info_a["packed"]
        second_part(eng, B, fixed_state(N, dtype))
        got = everything(eng)
    want = fresh(dtype, plan_kind)
    assert want["upload_info"]["zeros"] == 0 and want["upload_info"]["nnz"] == B.nnz
    assert want["upload_info"]["packed"] == (plan_kind == "tile")
    assert_identical(got, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_failed_upload_leaves_no_matrix_and_the_next_is_clean(amd, mats, fresh, plan_kind, dtype):
    from schpf_amd._lib import SchpfHipError
    A, B = mats
    bad_col = B.col.copy()
    bad_col[B.nnz // 2] = G
    bad = SimpleNamespace(row=B.row, col=bad_col, data=B.data, shape=(N, G))   # coo_matrix itself would refuse it
    with amd.DeviceCAVI(N, G, K, dtype=dtype) as eng:
        live_engine_on_a(eng, A)
        with pytest.raises(ValueError, match="out of range"):
            eng.upload(bad, warn=False)
        with pytest.raises(SchpfHipError, match="no count matrix"):
            eng.step()
        assert eng.upload_info()["nnz"] == 0    # deliberate difference: a failed upload reports an empty record, not the previous matrix's numbers
        second_part(eng, B, fixed_state(N, dtype))
        got = everything(eng)
    assert_identical(got, fresh(dtype, plan_kind))


@only_plans("tile")
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_batch_engine_gathered_twice(amd, mats, dtype):
    A, _ = mats
    n = 64
    rng = np.random.RandomState(21)
    rows1 = np.sort(rng.choice(N, n, replace=False)).astype(np.int32)
    rows2 = rng.permutation(N)[:n].astype(np.int32)
    assert (np.diff(rows2) < 0).any() and set(rows1) != set(rows2)
    st = fixed_state(n, dtype, seed=4)

    def one_step(batch, source):
        batch.upload_rows(source, rows2)
        set_state(batch, st)
        batch.step()
        return {name: batch.get_gamma(name) for name in GAMMAS}

    with amd.DeviceCAVI(N, G, K, dtype=dtype) as source:
        source.keep_rows()
        source.upload(A, warn=False)
        assert source.upload_info()["rows"]
        with amd.DeviceCAVI(n, G, K, dtype=dtype) as batch:
            batch.upload_rows(source, rows1)
            set_state(batch, fixed_state(n, dtype, seed=9))
            batch.step()
            got = one_step(batch, source)
        with amd.DeviceCAVI(n, G, K, dtype=dtype) as batch:
            want = one_step(batch, source)
    assert_identical(got, want)
