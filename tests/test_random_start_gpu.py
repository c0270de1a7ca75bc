"""The device-drawn first iteration (schpf_init_phi_device, MODE_RANDOM) against its own draws, element by element.

The draws are a pure function of (seed, cell, gene, k); tests/_random_start_reference.py restates them in NumPy, exact
up to the logarithm (float64 there, `__logf` on the device), and the oracle takes responsibilities from outside.  So a
case is: set a state, init_phi_device(seed), one step, read the four Gammas; the oracle's iteration from the same state
with xphi = x * phi of the restatement; compare all eight arrays.  A generator that ignores k or the seed, repeats a
gene's draw over the cells, swaps cell and gene in its key or decodes a wrong minor row passes every conservation
identity (test_device_random_phi_is_a_valid_start, check_random_start of the shapes module) and fails here.

  (a) every (plan, dtype, pair, layout) of tests/_sweep_shapes.py cases(): the 336 cases of the shapes module, on its
      matrices, each asserting the pair, workgroup and entry format it ran on (that module's assert_shape);
  (b) one matrix with stored zeros and repeated entries, K = 20 and 50, float64: tile, half-window, balanced and gather
      plans, host- and device-built plans, canonical and shuffled COO order and an upload from a device CSR agree with
      one another to rtol 1e-12 (they all call the same `__logf`: its error cancels); a seed repeats its bits and the
      next seed moves every row that has a nonzero;
  (c) frozen genes: beta and eta keep their bits, theta and xi match;
  (d) two row shards on one GPU: local cell numbers and rank seeds;
  (e) nonzeros placed where a draw has u = 1 (e = 0, phi_k = 0) and the smallest u (e = 17.33).

Tolerances.  Element-wise on the shapes, scaled error |got - want| / ((want - prior) + 2^-24 * rowsum): every summand
x * phi of shape - prior is positive, so a relative error of the draws carries through (first term); a draw next to
u = 1 is known to one step of u only (second term, rowsum = the row's sum of counts).  The same figure as a plain
relative error for the rates and the capacities' shapes.  Between the device and the reference the only inexact step in
float64 is `__logf`; nothing states its accuracy, so the bounds are 8 x the largest scaled error of the module's first
run on an MI355X, rounded up to one digit, under the caps 1e-5 (float64) and 1e-4 (float32) -- a single wrong draw of
one nonzero moves an element by about x * phi, at least 1e-3 of it on these matrices.

Largest scaled error over (a)-(e) on the first run (MI355X, 2026-10-20; test_zz_report_largest_scaled_errors) and the
bound taken from it:

    tile   float64  1.47e-7  (4x4, K = 29, balanced, 16-byte entries; beta shape)    -> 2e-6
    gather float64  1.47e-7  (10x8, K = 129; beta shape)                             -> 2e-6
    tile   float32  1.94e-6  (6x8, K = 161, 256 threads, 16-byte entries; beta shape) -> 2e-5
    gather float32  4.68e-7  (7x8, K = 193; theta shape)                             -> 4e-6

A float32 logarithm rounded to nearest in place of `__logf` gives 1.6e-7 on the float64 cases: the hardware logarithm is
as good as float32 allows on (0, 1], and no case failed when the module first ran.  The float32 tile kernel adds each
nonzero's x * phi in float32, the gather kernel accumulates in float64 and rounds once."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.sparse import coo_matrix

import _random_start_reference as rs
import _sweep_shapes as shapes
from conftest import synthetic_counts
from test_sweep_shapes_gpu import assert_shape, set_layout

pytestmark = pytest.mark.gpu

A, C, AP, CP = 0.3, 0.3, 1.0, 1.0
NAMES = ("xi", "theta", "eta", "beta")
SEED = 1234
CAP = {"float64": 1e-5, "float32": 1e-4}
# (plan, dtype) -> bound on the scaled error: 8 x the largest seen on the first run, one digit, rounded up
BOUND = {("tile", "float64"): 2e-6, ("tile", "float32"): 2e-5, ("gather", "float64"): 2e-6, ("gather", "float32"): 4e-6}
WORST = {}     # (plan, dtype) -> [largest scaled error, where]


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def test_bounds_are_under_the_caps():
    for (plan, dtype), b in BOUND.items():
        assert 0 < b <= CAP[dtype], (plan, dtype, b)


# ------------------------------------------------------------------------------------------------ reference
def start_state(oracle, X, K, dtype):
    """The state of the shapes module's cases: the reference's own setup, drawn from np.random.seed(K)."""
    np.random.seed(K)
    bp, dp, st = oracle.setup_state(X, K, np.dtype(dtype), A, AP, C, CP)
    st.xi_shape[:] = AP + K * A
    st.eta_shape[:] = CP + K * C
    for arr in st.arrays():
        arr.setflags(write=False)
    return bp, dp, st


def oracle_step(oracle, X, st, bp, dp, xphi, **flags):
    """One float64 oracle iteration from `st` with the given responsibilities; read-only."""
    st64 = st.cast(np.float64).copy()
    oracle.cavi_iteration(X.data, X.row, X.col, st64, A, C, bp, dp, xphi=xphi, **flags)
    for arr in st64.arrays():
        arr.setflags(write=False)
    return st64


@functools.lru_cache(maxsize=2)
def _case_phi(N, G, K):
    X = shapes.case_matrix(N, G, K, 1)           # the unpacked matrix has the same entries, one count differs
    p = rs.phi(SEED, X.row, X.col, K)
    p.setflags(write=False)
    return p


class Reference(object):
    def __init__(self, oracle, X, K, dtype, xphi, **flags):
        self.bp, self.dp, self.start = start_state(oracle, X, K, dtype)
        self.want = oracle_step(oracle, X, self.start, self.bp, self.dp, xphi, **flags)


@functools.lru_cache(maxsize=4)
def _case_reference(oracle, N, G, K, packed, dtype):
    X = shapes.case_matrix(N, G, K, packed)
    assert np.all(X.data > 0)
    return Reference(oracle, X, K, dtype, X.data[:, None].astype(np.float64) * _case_phi(N, G, K))


def load_engine(amd, X, K, dtype, ref, shape=None):
    N, G = shape or X.shape
    eng = amd.DeviceCAVI(N, G, K, dtype=np.dtype(dtype))
    eng.upload(X, warn=False)
    eng.set_hypers(A, C, ref.bp, ref.dp)
    for n in NAMES:
        eng.set_gamma(n, getattr(ref.start, n + "_shape"), getattr(ref.start, n + "_rate"))
    return eng


def drawn_step(eng, seed=SEED, **flags):
    eng.init_phi_device(seed)
    eng.step(**flags)
    return {n: eng.get_gamma(n) for n in NAMES}


def marginal_sums(X):
    x = np.where(X.data > 0, X.data, 0).astype(np.float64)
    return np.bincount(X.row, weights=x, minlength=X.shape[0]), np.bincount(X.col, weights=x, minlength=X.shape[1])


def check_against_reference(label, plan, dtype, got, want, X, names=NAMES):
    """All arrays of `names` at BOUND[(plan, dtype)]; records the largest scaled error."""
    dt = np.dtype(dtype)
    bound = BOUND[(plan, dt.name)]
    cell_sums, gene_sums = marginal_sums(X)
    worst = WORST.setdefault((plan, dt.name), [0.0, ""])
    bad = []
    for n in names:
        gs, gr = [np.asarray(v, dtype=np.float64) for v in got[n]]
        ws, wr = getattr(want, n + "_shape"), getattr(want, n + "_rate")
        assert got[n][0].dtype == dt and got[n][1].dtype == dt
        assert np.all(np.isfinite(gs)) and np.all(np.isfinite(gr)), "%s: %s is not finite" % (label, n)
        errs = {}
        if n in ("theta", "beta"):
            prior, sums = (A, cell_sums) if n == "theta" else (C, gene_sums)
            denom = (ws - prior) + 2.0 ** -24 * sums[:, None]
            empty = sums == 0
            # a row without a nonzero keeps the prior, in the engine's precision
            assert np.all(gs[empty] == np.float64(dt.type(prior))), "%s: %s shape of an empty row" % (label, n)
            assert np.all(denom[~empty] > 0)
            errs[n + " shape"] = np.abs(gs - ws)[~empty] / denom[~empty]
        else:
            errs[n + " shape"] = np.abs(gs - ws) / np.abs(ws)
        errs[n + " rate"] = np.abs(gr - wr) / np.abs(wr)
        for what, e in errs.items():
            top = float(e.max()) if e.size else 0.0
            if top >= worst[0]:
                worst[0], worst[1] = top, "%s, %s" % (label, what)
            if not top <= bound:
                bad.append("%s: %.3g" % (what, top))
    assert not bad, "%s: scaled errors beyond %.3g: %s" % (label, bound, ", ".join(bad))


# ------------------------------------------------------------------------------------------------ (a) every layout
def run_case(amd, oracle, monkeypatch, case):
    set_layout(monkeypatch, case)
    X = case.matrix()
    ref = _case_reference(oracle, case.N, case.G, case.K, case.layout.packed, case.dtype)
    with load_engine(amd, X, case.K, case.dtype, ref) as eng:
        assert_shape(eng, case)
        got = drawn_step(eng)
    check_against_reference(case.id, case.plan, case.dtype, got, ref.want, X)


TILE_CASES, GATHER_CASES = shapes.cases("tile"), shapes.cases("gather")
assert len(TILE_CASES) + len(GATHER_CASES) == 336


@pytest.mark.parametrize("case", TILE_CASES, ids=[c.id for c in TILE_CASES])
def test_tile_layout_draws_the_reference(amd, oracle, monkeypatch, case):
    run_case(amd, oracle, monkeypatch, case)


@pytest.mark.parametrize("case", GATHER_CASES, ids=[c.id for c in GATHER_CASES])
def test_gather_layout_draws_the_reference(amd, oracle, monkeypatch, case):
    run_case(amd, oracle, monkeypatch, case)


# ------------------------------------------------------------------------------------------------ (b) every route
ROUTES = {   # name -> (SCHPF_PLAN, further switches, how the matrix is handed over)
    "tile": ("tile", {}, "canonical"),
    "half": ("tile", {"SCHPF_HALF": "2"}, "canonical"),
    "balanced": ("tile", {"SCHPF_BALANCE": "1", "SCHPF_WPB": "16"}, "canonical"),
    "gather": ("gather", {}, "canonical"),
    "hostplan": ("tile", {"SCHPF_DEVICE_PLAN": "0"}, "canonical"),
    "deviceplan": ("tile", {"SCHPF_DEVICE_PLAN": "1"}, "canonical"),
    "shuffled": ("tile", {}, "shuffled"),
    "gather-shuffled": ("gather", {}, "shuffled"),
    "csr": ("tile", {}, "csr"),
}
ROUTE_KS = (20, 50)


def set_route(monkeypatch, route):
    plan, env, _ = ROUTES[route]
    monkeypatch.setenv("SCHPF_PLAN", plan)
    for v in shapes.CLEARED:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=1)
def route_matrix():
    """700 x 900, 5 % filled, plus repeated (cell, gene) entries and stored zeros, some of them in a cell and a gene
    that hold nothing else; sorted by (cell, gene), repeats next to each other."""
    X = synthetic_counts(700, 900, 0.05, seed=17)
    keep = (X.row != 77) & (X.col != 640)
    row, col, val = X.row[keep], X.col[keep], X.data[keep].astype(np.float64)
    rng = np.random.RandomState(5)
    n = row.shape[0] // 20
    pick = rng.randint(0, row.shape[0], n)
    zr, zc = rng.randint(0, 700, n), rng.randint(0, 900, n)
    zr[:2], zc[:2] = 77, [3, 5]
    row = np.concatenate([row, row[pick], zr]).astype(np.int32)
    col = np.concatenate([col, col[pick], zc]).astype(np.int32)
    val = np.concatenate([val, rng.randint(1, 5, n), np.zeros(n)])
    order = np.lexsort((col, row))
    X = coo_matrix((val[order], (row[order], col[order])), shape=(700, 900))
    for arr in (X.data, X.row, X.col):
        arr.setflags(write=False)
    return X


def handed_over(X, how):
    if how == "canonical":
        return X
    if how == "shuffled":
        perm = np.random.RandomState(11).permutation(X.nnz)
        return coo_matrix((X.data[perm], (X.row[perm], X.col[perm])), shape=X.shape)
    import warnings
    import torch
    indptr = np.concatenate([[0], np.cumsum(np.bincount(X.row, minlength=X.shape[0]))])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)      # torch: "Sparse CSR tensor support is in beta state"
        return torch.sparse_csr_tensor(torch.tensor(indptr).to(torch.int32).cuda(),
                                       torch.tensor(X.col).to(torch.int32).cuda(), torch.tensor(X.data).cuda(), size=X.shape)


@functools.lru_cache(maxsize=2)
def _route_reference(oracle, K):
    X = route_matrix()
    return Reference(oracle, X, K, "float64", rs.xphi(X, SEED, K))


_ROUTE_RESULTS = {}


def route_result(amd, oracle, monkeypatch, K, route, seed=SEED):
    """The eight arrays after init_phi_device(seed) and one step on a route; computed once per (K, route, seed)."""
    key = (K, route, seed)
    if key not in _ROUTE_RESULTS:
        X, ref = route_matrix(), _route_reference(oracle, K)
        with monkeypatch.context() as mp:
            set_route(mp, route)
            with load_engine(amd, handed_over(X, ROUTES[route][2]), K, "float64", ref, shape=X.shape) as eng:
                info, up = eng.plan_info(), eng.upload_info()
                assert (info["chunk_len"] > 0) == (ROUTES[route][0] == "gather"), (route, info)
                assert up["nnz"] == X.nnz and up["zeros"] == int((X.data == 0).sum()), (route, up)
                if route == "half":
                    assert (info["ring_cell"], info["ring_gene"]) == (2, 2), info
                if route == "balanced":
                    assert info["waves_per_block"] == 16, info
                got = drawn_step(eng, seed)
        for n in NAMES:
            for arr in got[n]:
                arr.setflags(write=False)
        _ROUTE_RESULTS[key] = got
    return _ROUTE_RESULTS[key]


def test_route_matrix_has_zeros_and_repeats():
    X = route_matrix()
    keys = X.row.astype(np.int64) * X.shape[1] + X.col
    assert (X.data == 0).sum() > 1000 and np.unique(keys).size < X.nnz - 1000
    assert np.any(X.row == 77) and np.all(X.data[X.row == 77] == 0) and np.all(X.data[X.col == 640] == 0)
    assert np.all(np.diff(keys) >= 0)


@pytest.mark.parametrize("K", ROUTE_KS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_draws_the_same_numbers(amd, oracle, monkeypatch, K, route):
    got = route_result(amd, oracle, monkeypatch, K, route)
    ref = _route_reference(oracle, K)
    check_against_reference("route %s K%d" % (route, K), ROUTES[route][0], "float64", got, ref.want, route_matrix())
    base = route_result(amd, oracle, monkeypatch, K, "tile")
    for n in NAMES:
        for part, g, b in zip(("shape", "rate"), got[n], base[n]):
            assert_allclose(g, b, rtol=1e-12, atol=0, err_msg="%s %s: route %s against the tile plan, K = %d"
                            % (n, part, route, K))


@pytest.mark.parametrize("K", ROUTE_KS)
@pytest.mark.parametrize("route", ["tile", "gather"])
def test_a_seed_repeats_its_bits_and_the_next_seed_moves_every_row(amd, oracle, monkeypatch, K, route):
    X, ref = route_matrix(), _route_reference(oracle, K)
    first = route_result(amd, oracle, monkeypatch, K, route)
    with monkeypatch.context() as mp:
        set_route(mp, route)
        with load_engine(amd, X, K, "float64", ref) as eng:
            again = drawn_step(eng, SEED)
            for n in NAMES:                                 # a second start on the same engine
                eng.set_gamma(n, getattr(ref.start, n + "_shape"), getattr(ref.start, n + "_rate"))
            twice = drawn_step(eng, SEED)
    for n in NAMES:
        for g, h, b in zip(again[n], twice[n], first[n]):
            assert_array_equal(g, b, err_msg=n)
            assert_array_equal(h, b, err_msg=n + ", second start of one engine")
    other = route_result(amd, oracle, monkeypatch, K, route, seed=SEED + 1)
    cell_sums, gene_sums = marginal_sums(X)
    for n, sums in (("theta", cell_sums), ("beta", gene_sums)):
        moved = np.any(other[n][0] != first[n][0], axis=1)
        assert_array_equal(moved, sums > 0, err_msg="%s rows that differ between seeds %d and %d" % (n, SEED, SEED + 1))
    want = oracle_step(oracle, X, ref.start, ref.bp, ref.dp, rs.xphi(X, SEED + 1, K))
    check_against_reference("route %s K%d seed %d" % (route, K, SEED + 1), ROUTES[route][0], "float64", other, want, X)


# ------------------------------------------------------------------------------------------------ (c) frozen genes
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("route", ["tile", "half", "balanced", "gather"])
def test_frozen_genes_keep_their_bits(amd, oracle, monkeypatch, route, dtype):
    X, K = route_matrix(), 20
    xphi = rs.xphi(X, SEED, K)
    ref = Reference(oracle, X, K, dtype, xphi, freeze_genes=True)
    set_route(monkeypatch, route)
    with load_engine(amd, X, K, dtype, ref) as eng:
        got = drawn_step(eng, freeze_genes=True)
    for n in ("eta", "beta"):
        for part, g in zip(("shape", "rate"), got[n]):
            assert_array_equal(g, getattr(ref.start, n + "_" + part), err_msg="%s %s changed under freeze_genes" % (n, part))
            assert_array_equal(getattr(ref.want, n + "_" + part), getattr(ref.start, n + "_" + part).astype(np.float64))
    check_against_reference("frozen %s %s" % (route, dtype), ROUTES[route][0], dtype, got, ref.want, X, names=("xi", "theta"))


# ------------------------------------------------------------------------------------------------ (d) shards
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("plan", ["tile", "gather"])
def test_two_shards_draw_with_local_cells_and_rank_seeds(amd, oracle, monkeypatch, plan, dtype):
    from schpf_amd.sharded import ThreadedShards
    X, K = route_matrix(), 20
    set_route(monkeypatch, plan)
    with ThreadedShards(X, K, np.dtype(dtype), devices=[0, 0], comm="emulated") as shards:
        bounds = [int(b) for b in shards.bounds]
        assert len(bounds) == 3 and 0 < bounds[1] < X.shape[0]
        xphi = rs.xphi_sharded(X, bounds, SEED, K, communicator=False)      # emulated: no communicator is attached
        ref = Reference(oracle, X, K, dtype, xphi)
        shards.set_hypers(A, C, ref.bp, ref.dp)
        for n in NAMES:
            shards.set_gamma(n, getattr(ref.start, n + "_shape"), getattr(ref.start, n + "_rate"))
        shards.init_phi_device(SEED)
        shards.steps(1)
        got = {n: shards.get_gamma(n) for n in NAMES}
        for e in shards.engines[1:]:
            for n in ("eta", "beta"):
                for g, h in zip(e.get_gamma(n), got[n]):
                    assert_array_equal(g, h, err_msg="replica of " + n)
    check_against_reference("shards %s %s" % (plan, dtype), plan, dtype, got, ref.want, X)
    # and the conventions matter: global cell numbers or one seed for all are another start
    theta = got["theta"][0].astype(np.float64)
    plain = oracle_step(oracle, X, ref.start, ref.bp, ref.dp, rs.xphi(X, SEED, K))
    assert np.abs(theta - plain.theta_shape).max() > 1e-2


# ------------------------------------------------------------------------------------------------ (e) the edge draws
def _case(cases, cid):
    return [c for c in cases if c.id == cid][0]


EDGE_CASES = [_case(TILE_CASES, "tile-f64-4x16-K113-t1024-packed"), _case(TILE_CASES, "tile-f64-4x16-K113-half-packed"),
              _case(GATHER_CASES, "gather-f64-8x16-K225-gather-packed")]


@pytest.mark.parametrize("bits, e_want", [(0xFFFFFF, 0.0), (0, 25 * np.log(2.0))], ids=["u_is_one", "smallest_u"])
@pytest.mark.parametrize("case", EDGE_CASES, ids=[c.id for c in EDGE_CASES])
def test_edge_draws(amd, oracle, monkeypatch, case, bits, e_want):
    """A nonzero (count 3) where draw k has the 24-bit value `bits` under SEED: u = 1, e = 0, phi_k = 0; or u = 2^-25,
    e = 17.33.  The state stays finite and matches the reference."""
    hit = rs.find_edge_draw(SEED, case.N, case.G, case.K, bits, limit=case.N * case.G // 40000 + 1)
    assert hit is not None, "no such draw in %d x %d x %d under seed %d" % (case.N, case.G, case.K, SEED)
    cell, gene, k = hit
    X0 = case.matrix()
    there = (X0.row == cell) & (X0.col == gene)
    X = coo_matrix((np.concatenate([X0.data[~there], [3]]), (np.concatenate([X0.row[~there], [cell]]),
                                                            np.concatenate([X0.col[~there], [gene]]))), shape=X0.shape)
    xphi = rs.xphi(X, SEED, case.K)
    assert rs.draws(SEED, np.array([cell]), np.array([gene]), case.K)[0, k] == e_want
    assert (xphi[-1, k] == 0.0) == (bits == 0xFFFFFF) and np.all(np.isfinite(xphi))
    ref = Reference(oracle, X, case.K, case.dtype, xphi)
    set_layout(monkeypatch, case)
    with load_engine(amd, X, case.K, case.dtype, ref) as eng:
        assert_shape(eng, case)
        got = drawn_step(eng)
    check_against_reference("%s %s" % (case.id, "u = 1" if bits else "smallest u"), case.plan, case.dtype, got, ref.want, X)


# ------------------------------------------------------------------------------------------------ report
def test_zz_report_largest_scaled_errors():
    """Not a check of its own: the largest scaled error the tests above saw per plan and dtype, and where."""
    print("largest scaled errors of the device-drawn start:")
    for (plan, dtype), (err, where) in sorted(WORST.items()):
        print("  START-WORST %-6s %s %.3g of bound %.3g  (%s)" % (plan, dtype, err, BOUND[(plan, dtype)], where))
    for key, (err, where) in WORST.items():
        assert err <= BOUND[key], (key, where)
