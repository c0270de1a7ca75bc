"""The sharded iteration on every instantiated sweep shape: two row shards on one GPU, one case per (plan, dtype,
(NV, LPC) pair, layout) of tests/_sweep_shapes.py, on the matrices of tests/_sharded_shapes.py (pinned on the host by
tests/test_sharded_shapes_host.py).

A rank of a sharded fit runs what no unsharded engine reaches, and it depends on K, KP and the plan: the packing of the
gene side's partial rows (combine_strided_kernel through pfirst / pcount / pstride at stride KP), the gene update from
the exchange buffer with the all-reduced sum of E[theta] read from its K-element tail in T, the mirror
colsum_reduce_kernel writes there, the plans of a hinted rank and the two-launch order.  The suite knew it at K = 5, 12
and 20.

  * test_tile_shards / test_gather_shards: ThreadedShards(devices=[0, 0], comm="emulated") and an unsharded engine
    under the case's layout switches, both from the oracle's start (seed K).  Every shard engine asserts the pair, KP,
    workgroup, ring and entry format it ran on, and more than one window per orientation where the case promises it.
    Two iterations; after each the whole state (theta / xi concatenated over the shards, beta / eta of shard 0) against
    the oracle at 1e-11 (float64) / 2e-5 * (it + 1) (float32) and against the unsharded engine at 1e-11 / 2e-5; beta
    and eta of shard 1 equal shard 0's bit for bit; the loss summed over the shards at 1e-11 / 1e-5.  The packed
    256-thread cases and the gather cases also start from init_phi_device with the rank seeds of sharded.py, against
    tests/_random_start_reference.py with local cell numbers at the bounds of tests/test_random_start_gpu.py.
  * test_library_driven_iteration_on_one_rank: every pair once per dtype (tile: packed, 1024 threads), a hinted engine
    joined to a one-rank communicator: steps(1), steps(4), steps(4) -- eager, captured, replayed -- against nine oracle
    iterations at 1e-10 / 2e-5 * 9; loss_terms_all against the oracle's loss of the state the device holds.
  * test_one_rank_sharded_iteration_equals_plain_steps: the same pairs on an UNHINTED engine against a twin running
    plain steps, both with SCHPF_FUSE_SUMS=0 and SCHPF_DUAL=0.  In float64 the two are the same operations: the plans
    are the twin's; the sweeps are the twin's two launches; combine_strided_kernel forms sum_strided of the row's
    partial rows exactly as the twin's SRC_STRIDED update does, and T = double stores it unrounded; the all-reduce over
    one rank adds nothing; the tail mirrors s_theta exactly.  So the bits must agree, and any slip of the packing or of
    the SRC_DENSE update shows.  float32 rounds the packed sums and the tail to float: 2e-5 after the first iteration,
    2e-5 * 9 after the ninth.
  * test_shard_edges: the edge matrix of _sharded_shapes (three shards, the middle one a single cell; genes one shard or
    every shard lacks, whose rows have pcount = 0 in that shard's packing; stored zeros and repeats) at K = 20 and 50,
    both dtypes, tile at 256 and 1024 threads and gather, through {}, {}, simultaneous, {}, freeze_genes, {} from an
    init_phi_host start, against the oracle; replicas bit for bit after every step.
  * test_plain_and_sharded_steps_mix: two shards of a matrix small enough for the fused column sums (700 x 450, K = 9),
    a plain step() per engine and a sharded iteration, in both orders, against the same sequence on oracle-backed
    engines.  On the code before this test existed the order plain, sharded FAILED: step_finish found sums_stale and
    reduced this rank's sum of E[theta] into the exchange buffer's tail behind the all-reduce, so beta's rate got a
    local sum and the replicas parted.  step_local now brings the sums up to date before the packing.

A case runs all of its checks, whatever an earlier one found.  The last test prints the largest error per plan, dtype
and quantity as a fraction of its bound (DESIGN.md "parity", which also holds the counts of failing tests on builds
with one change each to the packing, the gene update and the tail mirror).  492 tests, 109 s on an MI355X; a case is at
most 0.8 s, the first one-rank case (it loads RCCL) 4 s."""
import functools

import numpy as np
import pytest

import _random_start_reference as rs
import _sharded_shapes as sh
import _sweep_shapes as shapes
import test_random_start_gpu as start
from _oracle_engine import OracleShardEngine
from conftest import synthetic_counts
from test_sweep_shapes_gpu import assert_shape, set_layout

pytestmark = pytest.mark.gpu

A, C, NAMES = sh.A, sh.C, sh.NAMES
WORST = {}     # (plan, dtype, quantity) -> [largest error / bound, the case it came from]


def record(case, quantity, err, bound):
    w = WORST.setdefault((case.plan, case.dtype, quantity), [0.0, ""])
    if not err / bound < w[0]:
        w[0], w[1] = float(err / bound), case.id
    return err <= bound


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


@functools.lru_cache(maxsize=4)
def _reference(oracle, N, G, K, packed, dtype, steps):
    return sh.Reference(oracle, sh.case_matrix(N, G, K, packed), K, dtype, steps=steps)


def reference(oracle, case, steps=2):
    return _reference(oracle, case.N, case.G, case.K, case.layout.packed, case.dtype, steps)


def set_state(eng, ref, st=None):
    st = st or ref.states[0]
    eng.set_hypers(A, C, ref.bp, ref.dp)
    for n in NAMES:
        eng.set_gamma(n, getattr(st, n + "_shape"), getattr(st, n + "_rate"))
    return eng


def load_engine(amd, X, K, dtype, ref, hinted=False):
    eng = amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=np.dtype(dtype))
    if hinted:
        eng.hint_sharded()
    eng.upload(X, warn=False)
    return set_state(eng, ref)


def gammas(eng):
    return {n: eng.get_gamma(n) for n in NAMES}


def distances(got, want):
    """{'theta shape': largest |got - want| / |want|, ...} over every element of the eight arrays; `want` a state of
    the oracle or a dict of (shape, rate) pairs."""
    out = {}
    for n in NAMES:
        w2 = want[n] if isinstance(want, dict) else (getattr(want, n + "_shape"), getattr(want, n + "_rate"))
        for part, g, w in zip(("shape", "rate"), got[n], w2):
            assert g.shape == w.shape, (n, part, g.shape, w.shape)
            g, w = g.astype(np.float64), np.asarray(w, np.float64)
            d = np.abs(g - w) / np.abs(w)
            out["%s %s" % (n, part)] = float(d.max()) if np.all(np.isfinite(g)) else float("inf")
    return out


def check_state(bad, case, quantity, got, want, bound):
    for what, err in distances(got, want).items():
        if not record(case, quantity, err, bound):
            bad.append("%s, %s: %.3g beyond %.3g" % (quantity, what, err, bound))


def check_replicas(bad, shards, label):
    first = {n: shards.engines[0].get_gamma(n) for n in ("eta", "beta")}
    for r, e in enumerate(shards.engines[1:], 1):
        for n in ("eta", "beta"):
            for part, g, h in zip(("shape", "rate"), e.get_gamma(n), first[n]):
                if not np.array_equal(g, h):
                    bad.append("%s: %s %s of shard %d differs from shard 0's in %d elements"
                               % (label, n, part, r, int((g != h).sum())))


def check_shapes(bad, engines, case):
    for r, e in enumerate(engines):
        try:
            assert_shape(e, case)
        except AssertionError as exc:
            bad.append("shape of engine %d: %s" % (r, str(exc).splitlines()[0][:300]))


# ------------------------------------------------------------------------------------------ two shards, every case
def run_case(amd, oracle, monkeypatch, case):
    from schpf_amd.sharded import ThreadedShards
    set_layout(monkeypatch, case)
    X, ref = case.matrix(), reference(oracle, case)
    f32 = case.dtype == "float32"
    bad, plain = [], []
    with load_engine(amd, X, case.K, case.dtype, ref) as eng:
        check_shapes(bad, [eng], case)
        for it in range(2):
            eng.step()
            plain.append(gammas(eng))
    with ThreadedShards(X, case.K, np.dtype(case.dtype), devices=[0, 0], comm="emulated") as shards:
        assert [int(b) for b in shards.bounds] == case.bounds()
        check_shapes(bad, shards.engines, case)
        set_state(shards, ref)
        for it in range(2):
            shards.steps(1)
            got = gammas(shards)
            check_state(bad, case, "oracle, step %d" % (it + 1), got, ref.states[it + 1], sh.state_bound(case.dtype, it))
            check_state(bad, case, "unsharded, step %d" % (it + 1), got, plain[it], 2e-5 if f32 else 1e-11)
            check_replicas(bad, shards, "step %d" % (it + 1))
        loss = shards.mean_negative_pois_llh()
        if not record(case, "loss", abs(loss - ref.loss) / abs(ref.loss), 1e-5 if f32 else 1e-11):
            bad.append("loss: shards %.17g, oracle %.17g" % (loss, ref.loss))
    if case.layout.packed and case.layout.name in ("t256", "gather"):
        check_drawn_start(bad, monkeypatch, oracle, case, X, ref)
    assert not bad, "%s:\n  %s" % (case.id, "\n  ".join(bad))


def check_drawn_start(bad, monkeypatch, oracle, case, X, ref):
    """tests/test_random_start_gpu.py part (d) on this case: init_phi_device on the shards (rank seeds, local cell
    numbers) against the restated draws, that module's scaled error and bounds."""
    from schpf_amd.sharded import ThreadedShards
    want = start.oracle_step(oracle, X, ref.states[0], ref.bp, ref.dp,
                             rs.xphi_sharded(X, case.bounds(), start.SEED, case.K, communicator=False))
    with ThreadedShards(X, case.K, np.dtype(case.dtype), devices=[0, 0], comm="emulated") as shards:
        set_state(shards, ref)
        shards.init_phi_device(start.SEED)
        shards.steps(1)
        got = gammas(shards)
        check_replicas(bad, shards, "drawn start")
    seen = {}
    monkeypatch.setattr(start, "WORST", seen)
    try:
        start.check_against_reference(case.id, case.plan, case.dtype, got, want, X)
    except AssertionError as exc:
        bad.append("drawn start: %s" % str(exc).splitlines()[0][:300])
    for (plan, dtype), (err, _) in seen.items():
        record(case, "drawn start", err, start.BOUND[(plan, dtype)])


TILE_CASES, GATHER_CASES = sh.cases("tile"), sh.cases("gather")
assert len(TILE_CASES) + len(GATHER_CASES) == 336


@pytest.mark.parametrize("case", TILE_CASES, ids=[c.id for c in TILE_CASES])
def test_tile_shards(amd, oracle, monkeypatch, case):
    run_case(amd, oracle, monkeypatch, case)


@pytest.mark.parametrize("case", GATHER_CASES, ids=[c.id for c in GATHER_CASES])
def test_gather_shards(amd, oracle, monkeypatch, case):
    run_case(amd, oracle, monkeypatch, case)


# ------------------------------------------------------------------------------- the library-driven iteration, one rank
PAIR_CASES = sh.pair_cases("tile") + sh.pair_cases("gather")
assert len(PAIR_CASES) == 40 + 28      # 20 tile pairs and 16 (float64) + 12 (float32) reachable gather pairs
STRETCHES = (1, 4, 4)          # eager; captured (a one-rank communicator graphs its stretches); replayed


@pytest.mark.parametrize("case", PAIR_CASES, ids=[c.id for c in PAIR_CASES])
def test_library_driven_iteration_on_one_rank(amd, oracle, monkeypatch, case):
    from schpf_amd.engine import mean_negative
    from schpf_amd.sharded import NativeShard
    set_layout(monkeypatch, case)
    X, ref = case.matrix(), reference(oracle, case, steps=sum(STRETCHES))
    f32 = case.dtype == "float32"
    bad = []
    with load_engine(amd, X, case.K, case.dtype, ref, hinted=True) as eng:
        check_shapes(bad, [eng], case)
        shard = NativeShard(eng, amd.DeviceCAVI.comm_unique_id(), 0, 1)
        for n in STRETCHES:
            shard.steps(n)
        got = gammas(eng)
        n = sum(STRETCHES)
        check_state(bad, case, "one rank, %d steps" % n, got, ref.states[n], 2e-5 * n if f32 else 1e-10)
        llh, gl, nnz = eng.loss_terms_all()
        # the loss of the state the device holds, so that the bound is the loss pass's own
        want = float(oracle.mean_negative_pois_llh(X.data, X.row, X.col, got["theta"][0], got["theta"][1],
                                                   got["beta"][0], got["beta"][1]))
        if nnz != X.nnz or not record(case, "one rank, loss", abs(mean_negative(llh, gl, nnz) - want) / abs(want),
                                      1e-5 if f32 else 1e-11):
            bad.append("loss_terms_all: %r against the oracle's %.17g over %d entries" % ((llh, gl, nnz), want, X.nnz))
    assert not bad, "%s:\n  %s" % (case.id, "\n  ".join(bad))


@pytest.mark.parametrize("case", PAIR_CASES, ids=[c.id for c in PAIR_CASES])
def test_one_rank_sharded_iteration_equals_plain_steps(amd, oracle, monkeypatch, case):
    from schpf_amd.sharded import NativeShard
    set_layout(monkeypatch, case)
    monkeypatch.setenv("SCHPF_FUSE_SUMS", "0")
    monkeypatch.setenv("SCHPF_DUAL", "0")
    X, ref = case.matrix(), reference(oracle, case, steps=sum(STRETCHES))
    f32 = case.dtype == "float32"
    bad, twin = [], []
    with load_engine(amd, X, case.K, case.dtype, ref) as eng:
        for n in STRETCHES:
            eng.steps(n)
            twin.append(gammas(eng))
    with load_engine(amd, X, case.K, case.dtype, ref) as eng:
        check_shapes(bad, [eng], case)
        shard = NativeShard(eng, amd.DeviceCAVI.comm_unique_id(), 0, 1)
        done = 0
        for n, want in zip(STRETCHES, twin):
            shard.steps(n)
            done += n
            got = gammas(eng)
            if f32:
                check_state(bad, case, "plain steps, %d" % done, got, want, 2e-5 * done)
                continue
            for name in NAMES:
                for part, g, w in zip(("shape", "rate"), got[name], want[name]):
                    if not np.array_equal(g, w):
                        bad.append("after %d steps %s %s differs from the plain steps' in %d elements, by up to %.3g"
                                   % (done, name, part, int((g != w).sum()), float(np.max(np.abs(g - w) / np.abs(w)))))
    assert not bad, "%s:\n  %s" % (case.id, "\n  ".join(bad))


# --------------------------------------------------------------------------------------------------------- shard edges
EDGE_FLAGS = [{}, {}, {"simultaneous": True}, {}, {"freeze_genes": True}, {}]
EDGE_LAYOUTS = {"t256": {"SCHPF_PLAN": "tile", "SCHPF_WPB": "4"}, "t1024": {"SCHPF_PLAN": "tile", "SCHPF_WPB": "16"},
                "gather": {"SCHPF_PLAN": "gather"}}


class EdgeCase(object):
    def __init__(self, plan, dtype, K, layout):
        self.plan, self.dtype, self.K = plan, dtype, K
        self.id = "edge-%s-%s-K%d" % (layout, "f64" if dtype == "float64" else "f32", K)


@functools.lru_cache(maxsize=2)
def edge_reference(oracle, K, dtype):
    X = sh.edge_matrix()
    xphi = np.random.RandomState(K).dirichlet(np.ones(K), X.nnz) * X.data[:, None]
    xphi.setflags(write=False)
    return xphi, sh.Reference(oracle, X, K, dtype, steps=len(EDGE_FLAGS), flags=EDGE_FLAGS, xphi=xphi)


@pytest.mark.parametrize("layout", sorted(EDGE_LAYOUTS))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("K", sh.EDGE_KS)
def test_shard_edges(amd, oracle, monkeypatch, K, dtype, layout):
    from schpf_amd.sharded import ThreadedShards
    for v in ("SCHPF_PLAN",) + shapes.CLEARED:
        monkeypatch.delenv(v, raising=False)
    for k, v in EDGE_LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    case = EdgeCase("gather" if layout == "gather" else "tile", dtype, K, layout)
    X = sh.edge_matrix()
    xphi, ref = edge_reference(oracle, K, dtype)
    bad = []
    with ThreadedShards(X, K, np.dtype(dtype), devices=[0, 0, 0], comm="emulated") as shards:
        assert [int(b) for b in shards.bounds] == [0, 150, 151, 290]
        for r, e in enumerate(shards.engines):
            info, up = e.plan_info(), e.upload_info()
            assert (info["chunk_len"] < 0) == (case.plan == "tile"), (r, info)
            if case.plan == "tile":
                assert info["waves_per_block"] == (4 if layout == "t256" else 16) and up["packed"] == 1, (r, info, up)
            assert up["nnz"] == sh.EDGE_NNZ[r] and (up["zeros"] > 0) == (r != 1) and up["rounded"] == 0, (r, up)
        set_state(shards, ref)
        shards.init_phi_host(xphi)
        for it, flags in enumerate(EDGE_FLAGS):
            shards.steps(1, **flags)
            check_state(bad, case, "edges, step %d" % (it + 1), gammas(shards), ref.states[it + 1],
                        sh.state_bound(dtype, it))
            check_replicas(bad, shards, "step %d" % (it + 1))
        loss = shards.mean_negative_pois_llh()
        if not record(case, "edges, loss", abs(loss - ref.loss) / abs(ref.loss), 1e-5 if dtype == "float32" else 1e-11):
            bad.append("loss: shards %.17g, oracle %.17g" % (loss, ref.loss))
    assert not bad, "%s:\n  %s" % (case.id, "\n  ".join(bad))


# ------------------------------------------------------------------------------------- plain and sharded steps mixed
class MixCase(object):
    plan = "auto"

    def __init__(self, dtype, order):
        self.dtype, self.id = dtype, "mix-%s-%s" % ("f64" if dtype == "float64" else "f32", "-".join(order))


def plain_step(engine):
    if hasattr(engine, "step"):
        engine.step()
    else:                                  # the oracle-backed stand-in: both sweeps, then the updates from its own sums
        engine.step_local()
        engine.step_finish()


@pytest.mark.parametrize("order", [("plain", "sharded"), ("sharded", "plain"), ("plain", "sharded", "plain", "sharded")],
                         ids="-".join)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_plain_and_sharded_steps_mix(amd, oracle, monkeypatch, dtype, order):
    """A plain step() of a small engine leaves the column sums to the next reader (capi.hip sums_stale); a sharded
    iteration packs sum_i E[theta] for the all-reduce and must find it up to date.  Each shard's plain step runs on its
    own rows alone, so the replicas of beta and eta part there by design: every shard's state is compared with its
    stand-in's, not shard 1 with shard 0."""
    from schpf_amd.sharded import ThreadedShards
    for v in ("SCHPF_PLAN", "SCHPF_FUSE_SUMS") + shapes.CLEARED:
        monkeypatch.delenv(v, raising=False)
    X, K = synthetic_counts(700, 450, 0.07, seed=41), 9
    case = MixCase(dtype, order)
    bp, dp, st = sh.start_state(oracle, X, K, dtype)
    ref = type("Start", (), {"bp": bp, "dp": dp, "states": [st]})
    bad = []
    with ThreadedShards(X, K, np.dtype(dtype), devices=[0, 0], comm="emulated") as shards, \
            ThreadedShards(X, K, np.dtype(dtype), devices=[0, 1], comm="emulated", engine_factory=OracleShardEngine) as want:
        assert list(shards.bounds) == list(want.bounds)
        set_state(shards, ref)
        set_state(want, ref)
        for it, what in enumerate(order):
            for driver in (shards, want):
                if what == "plain":
                    for e in driver.engines:
                        plain_step(e)
                else:
                    driver.steps(1)
            for r in range(2):
                found = []
                check_state(found, case, "mixed steps", gammas(shards.engines[r]), gammas(want.engines[r]),
                            sh.state_bound(dtype, it))
                bad += ["shard %d after %s: %s" % (r, "-".join(order[:it + 1]), f) for f in found]
    assert not bad, "%s:\n  %s" % (case.id, "\n  ".join(bad))


def test_a_steady_sharded_stretch_launches_what_it_did(amd, oracle, monkeypatch):
    """Bringing the sums up to date in step_local costs a steady sharded stretch nothing: sums_stale is false there.
    profile_read() counts one cell sweep, one gene sweep and one update block per iteration, as before; after a plain
    fused step the same."""
    from schpf_amd.sharded import NativeShard
    for v in ("SCHPF_PLAN", "SCHPF_FUSE_SUMS") + shapes.CLEARED:
        monkeypatch.delenv(v, raising=False)
    X, K = synthetic_counts(700, 450, 0.07, seed=41), 9
    bp, dp, st = sh.start_state(oracle, X, K, "float64")
    ref = type("Start", (), {"bp": bp, "dp": dp, "states": [st]})
    with load_engine(amd, X, K, "float64", ref, hinted=True) as eng:
        shard = NativeShard(eng, amd.DeviceCAVI.comm_unique_id(), 0, 1)
        shard.steps(1)
        eng.profile(True)
        shard.steps(5)
        counts = {k: v["launches"] for k, v in eng.profile_read().items()}
        assert counts == {"cell_sweep": 5, "gene_sweep": 5, "loss_sweep": 0, "gamma_updates": 5}
        eng.step()
        eng.profile_read()
        shard.steps(3)
        counts = {k: v["launches"] for k, v in eng.profile_read().items()}
        assert counts == {"cell_sweep": 3, "gene_sweep": 3, "loss_sweep": 0, "gamma_updates": 3}


def test_zz_report_largest_scaled_errors():
    """Not a check of its own: the largest error the cases above saw per plan, dtype and quantity, as a fraction of its
    bound, and the case it came from."""
    print("largest errors of the sharded shapes, as a fraction of the bound:")
    for (plan, dtype, quantity), (frac, cid) in sorted(WORST.items()):
        print("  SHARD-WORST %-6s %s %-22s %.3g  (%s)" % (plan, dtype, quantity, frac, cid))
    for key, (frac, cid) in WORST.items():
        assert frac <= 1.0, (key, cid)
