"""The paired division of the float64 sweep (sweep_impl.h pair_own_sum / pair_quotients): in kernels
whose rows lie in two lanes, the even lane of a pair completes the normaliser of a step's first nonzero and divides for
it, the odd lane does the same for the second, and the two quotients are exchanged.  PAIRED below: the kernels that take
the path -- NV = 4 (K = 15, 16) on every layout and entry format, NV = 5 (K = 17...20) with 8-byte entries at 1024
threads; their neighbours with two lanes per row keep the general form and are run beside them.

Every case runs two engine iterations from identical state and compares every shape and rate with the CPU oracle at
the tolerance of the iteration tests (tests/test_engine_gpu.py, tests/test_sweep_shapes_gpu.py): rtol 1e-11.

  * every float64 tile pair with two lanes per row and two rows in registers -- (4,2) K = 15, (5,2) K = 17 and K = 20,
    (6,2) K = 21 on 1024-thread, balanced-window, half-window and 256-thread layouts, (7,2) K = 25 on the 256-thread
    layout -- with 8-byte entries and with 16-byte entries (one count beyond 16 bits), on the smallest matrices of
    tests/_sweep_shapes.py (more than one block, more than one window); on the plain packed layouts the dual launch
    must leave the bits of two single launches;
  * a matrix whose cells have an odd number of nonzeros in every window they touch, a tenth of them one nonzero in all:
    the second half of a row's last step slot is padding (count 0) and must add nothing;
  * extreme priors (test_underflow_fallback_matches_log_domain_oracle) on two matrices in which the nonzero whose
    normaliser underflows is (a) only ever the first of a step slot, (b) only ever the second, in both orientations:
    the quotient of either lane must poison both, or the group never reaches the log-domain path.  Which half a nonzero
    lies in is read back from the plan (schpf_debug_tile_halves: the library's host builder with SCHPF_BANK_ORDER=0,
    which the engine is made to use as well); with balanced windows the same matrices run without that claim;
  * real-valued data with stored zeros.
Never compares with a run of its own: the oracle and the other launch form are the only references."""
import ctypes
import functools

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.special import digamma

import _sweep_shapes as shapes

pytestmark = pytest.mark.gpu

A, C, AP, CP = 0.3, 0.3, 1.0, 1.0
NAMES = ("xi", "theta", "eta", "beta")
RTOL = 1e-11
DT = "float64"

LAYOUTS = {(lay.name, lay.packed): lay for lay in shapes.tile_layouts()}
PAIR_K = [((4, 2), 15), ((5, 2), 17), ((5, 2), 20), ((6, 2), 21)]
CASES = [shapes.Case("tile", DT, pair, K, LAYOUTS[key]) for pair, K in PAIR_K
         for key in (("t256", 1), ("t256", 0), ("t1024", 1), ("t1024", 0), ("balanced", 1), ("balanced", 0), ("half", 1))]
CASES += [shapes.Case("tile", DT, (7, 2), 25, LAYOUTS[("t256", p)]) for p in (1, 0)]   # 512-thread rule: paired there


@pytest.fixture(scope="module")
def amd():
    import schpf_amd
    from schpf_amd import _lib
    _lib.require_gpu()
    return schpf_amd


def start_state(oracle, X, K, extreme=None):
    """The iteration tests' start (random_state of tests/test_engine_gpu.py); extreme = (cell factor, gene factor):
    shape 5 at a row's own factor and 1e-4 elsewhere, the priors of the underflow test."""
    np.random.seed(K)
    bp, dp, st = oracle.setup_state(X, K, np.dtype(DT), A, AP, C, CP)
    st.xi_shape[:] = AP + K * A
    st.eta_shape[:] = CP + K * C
    if extreme is not None:
        pc, pg = extreme
        st.theta_shape[:] = 1e-4
        st.beta_shape[:] = 1e-4
        st.theta_shape[np.arange(X.shape[0]), pc] = 5.0
        st.beta_shape[np.arange(X.shape[1]), pg] = 5.0
    return bp, dp, st


class Reference(object):
    """The start and the oracle's state after one and two iterations; computed once per matrix, read-only."""

    def __init__(self, oracle, X, K, extreme=None):
        self.bp, self.dp, st = start_state(oracle, X, K, extreme)
        self.states = [st.copy()]
        for _ in range(2):
            oracle.cavi_iteration(X.data, X.row, X.col, st, A, C, self.bp, self.dp)
            self.states.append(st.copy())
        for s in self.states:
            for a in s.arrays():
                a.setflags(write=False)


@functools.lru_cache(maxsize=2)
def shape_reference(oracle, N, G, K, packed):
    return Reference(oracle, shapes.case_matrix(N, G, K, packed), K)


def set_layout(monkeypatch, layout, bank_order=None):
    monkeypatch.setenv("SCHPF_PLAN", "tile")
    for v in shapes.CLEARED + ("SCHPF_BANK_ORDER",):
        monkeypatch.delenv(v, raising=False)
    for k, v in layout.env.items():
        monkeypatch.setenv(k, v)
    if bank_order is not None:
        monkeypatch.setenv("SCHPF_BANK_ORDER", str(bank_order))


def load_engine(amd, X, K, ref):
    st = ref.states[0]
    eng = amd.DeviceCAVI(X.shape[0], X.shape[1], K, dtype=np.dtype(DT))
    eng.upload(X)
    eng.set_hypers(A, C, ref.bp, ref.dp)
    for n in NAMES:
        eng.set_gamma(n, getattr(st, n + "_shape"), getattr(st, n + "_rate"))
    return eng


def assert_kernels(eng, pair, layout, packed, label):
    """The engine runs the two-lane kernels of the layout the case names."""
    info, up = eng.plan_info(), eng.upload_info()
    nv, lpc = pair
    assert (info["LPC"], info["KL"], info["KP"]) == (lpc, nv * 2, nv * 2 * lpc), (label, info)
    assert info["waves_per_block"] == layout.wpb and info["chunk_len"] < 0, (label, info)
    assert (info["ring_cell"], info["ring_gene"]) == (layout.ring, layout.ring), (label, info)
    assert up["packed"] == packed, (label, up)
    return info


def two_steps(eng, ref, label):
    """Two iterations against the oracle; returns the bits they leave."""
    for it in range(2):
        eng.step()
        want, worst = ref.states[it + 1], []
        for n in NAMES:
            for part, got in zip(("shape", "rate"), eng.get_gamma(n)):
                w = getattr(want, n + "_" + part)
                worst.append((float(np.max(np.abs(got - w) / np.abs(w))) if np.all(np.isfinite(got)) else np.inf,
                              n + " " + part))
        print("PAIR-DIV %s step %d: largest relative error %.3g (%s)" % ((label, it + 1) + max(worst)))
        bad = ["%s: %.3g" % (what, err) for err, what in worst if not err <= RTOL]
        assert not bad, "%s step %d, relative errors beyond %.3g: %s" % (label, it + 1, RTOL, ", ".join(bad))
    return [eng.get_gamma(n) for n in NAMES]


def assert_same_bits_in_two_launches(amd, monkeypatch, X, K, ref, bits, label):
    monkeypatch.setenv("SCHPF_DUAL", "0")
    with load_engine(amd, X, K, ref) as eng:
        eng.step()
        eng.step()
        for n, (s0, r0) in zip(NAMES, bits):
            s1, r1 = eng.get_gamma(n)
            assert np.array_equal(s0, s1) and np.array_equal(r0, r1), "%s: %s differs between one launch and two" % (label, n)
    monkeypatch.delenv("SCHPF_DUAL")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_pair_shapes_match_oracle(amd, oracle, monkeypatch, case):
    set_layout(monkeypatch, case.layout)
    X, ref = case.matrix(), shape_reference(oracle, case.N, case.G, case.K, case.layout.packed)
    with load_engine(amd, X, case.K, ref) as eng:
        info = assert_kernels(eng, (case.NV, case.LPC), case.layout, case.layout.packed, case.id)
        assert info["windows_cell"] >= 2 and info["windows_gene"] >= 2, (case.id, info)
        bits = two_steps(eng, ref, case.id)
    if case.layout.packed and case.layout.name in ("t256", "t1024"):
        assert_same_bits_in_two_launches(amd, monkeypatch, X, case.K, ref, bits, case.id)


# ------------------------------------------------------------------------------------------- odd and single rows
def odd_rows_matrix(N, G, win_rows, seed):
    """Every cell has 1, 3 or 5 nonzeros in each window of genes (the last window may be narrow); every tenth cell
    has one nonzero in all."""
    rng = np.random.RandomState(seed)
    rows, cols = [], []
    bounds = list(range(0, G, win_rows)) + [G]
    for i in range(N):
        wins = [rng.randint(len(bounds) - 1)] if i % 10 == 3 else range(len(bounds) - 1)
        for w in wins:
            lo, hi = bounds[w], bounds[w + 1]
            n = 1 if i % 10 == 3 else min(int(rng.choice((1, 3, 5))), (hi - lo - 1) | 1)
            cols.extend(rng.choice(hi - lo, n, replace=False) + lo)
            rows.extend([i] * n)
    X = coo_matrix((rng.randint(1, 7, len(rows)), (np.array(rows, np.int32), np.array(cols, np.int32))), (N, G), dtype=np.int32)
    per = np.zeros((N, len(bounds) - 1), np.int64)
    np.add.at(per, (X.row, X.col // win_rows), 1)
    assert np.all((per % 2 == 1) | (per == 0)) and (per.sum(1) == 1).sum() >= N // 10
    return X


@pytest.mark.parametrize("pair,K", [((5, 2), 20), ((4, 2), 16)], ids=["5x2-K20", "4x2-K16"])
@pytest.mark.parametrize("name", ["t1024", "balanced", "t256"])
def test_odd_and_single_rows_pad_with_nothing(amd, oracle, monkeypatch, name, pair, K):
    layout = LAYOUTS[(name, 1)]
    N, G = shapes.matrix_shape("tile", pair, layout)
    win_rows = layout.lds_kib * 1024 // (pair[0] * 16 * pair[1])
    X = odd_rows_matrix(N, G, win_rows, seed=5)
    ref = Reference(oracle, X, K)
    set_layout(monkeypatch, layout)
    with load_engine(amd, X, K, ref) as eng:
        info = assert_kernels(eng, pair, layout, 1, name)
        assert -info["chunk_len"] == win_rows and info["windows_cell"] >= 2, info
        two_steps(eng, ref, "odd rows %dx%d K%d %s" % (pair + (K, name)))


# -------------------------------------------------------------------------------- underflow in one half of a slot
def plan_halves(major, minor, val, n_major, n_minor, lpc, wpb, win_rows):
    """Half (0 / 1) of its step slot in which the library's plan builder stores each nonzero (schpf_debug_tile_halves:
    the host builder, walked as the kernel walks it; reads SCHPF_BANK_ORDER), in the order of the arguments."""
    from schpf_amd import _lib
    lib = _lib.load()
    nnz = len(val)
    major, minor = np.ascontiguousarray(major, np.int32), np.ascontiguousarray(minor, np.int32)
    val = np.ascontiguousarray(val, np.float32)
    om, on, oh = np.empty(nnz, np.int32), np.empty(nnz, np.int32), np.empty(nnz, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _lib.check(lib.schpf_debug_tile_halves(nnz, p(major), p(minor), p(val), n_major, n_minor, lpc, wpb, win_rows, 1,
                                           p(om), p(on), p(oh)))
    key_in, key_out = major.astype(np.int64) * n_minor + minor, om.astype(np.int64) * n_minor + on
    oi, oo = np.argsort(key_in), np.argsort(key_out)
    assert np.array_equal(key_in[oi], key_out[oo])            # every nonzero once (the matrices have no duplicates)
    half = np.empty(nnz, np.int64)
    half[oi] = oh[oo]
    return half


def underflow_matrix(which, n, K, big):
    """n cells x 2 n genes; cell i prefers factor i % K.  An entry's normaliser underflows iff its cell and its gene
    prefer different factors.
      'first':  (i, i) underflows, (i, n + i) does not, (i - 1, n + i) underflows: rows and columns read
                [bad, good] [bad, padding];
      'second': (i, i) does not, (i, n + i) underflows, (i - 1, n + i) does not: [good, bad] [good, padding]."""
    i = np.arange(n)
    pc = i % K
    if which == "first":
        pg = np.r_[(i + 1) % K, i % K]
    else:
        pg = np.r_[i % K, (i - 1) % K]
    own = i if which == "first" else i[1:]          # 'second': no (0, n), which would underflow alone in its column
    row = np.r_[i, own, i[1:] - 1].astype(np.int32)
    col = np.r_[i, n + own, n + i[1:]].astype(np.int32)
    rng = np.random.RandomState(3)
    data = rng.randint(1, 6, len(row))
    bad = pc[row] != pg[col]
    if big:
        data[np.flatnonzero(~bad)[5]] = 70000       # one count beyond 16 bits: the 16-byte entry format
    return coo_matrix((data, (row, col)), (n, 2 * n), dtype=np.int32), pc, pg, bad


# the kernels on the path (PAIRED): the headline's, and NV = 4 with either entry format
@pytest.mark.parametrize("pair,K,packed", [((5, 2), 20, 1), ((4, 2), 16, 1), ((4, 2), 16, 0)],
                         ids=["5x2-K20-packed", "4x2-K16-packed", "4x2-K16-unpacked"])
@pytest.mark.parametrize("name", ["t1024", "balanced"])
@pytest.mark.parametrize("which", ["first", "second"])
def test_underflow_in_one_half_poisons_the_pair(amd, oracle, monkeypatch, which, name, pair, K, packed):
    layout, n = LAYOUTS[(name, packed)], 70
    X, pc, pg, bad = underflow_matrix(which, n, K, big=not packed)
    want_half = 0 if which == "first" else 1
    assert bad.sum() >= n - 1 and (~bad).sum() >= n
    ref = Reference(oracle, X, K, extreme=(pc, pg))
    # the normaliser of a `bad` entry is exactly zero in product form, the others are normal numbers
    st = ref.states[0]
    et = np.exp(digamma(st.theta_shape) - np.log(st.theta_rate))
    eb = np.exp(digamma(st.beta_shape) - np.log(st.beta_rate))
    s = np.einsum("ek,ek->e", et[X.row], eb[X.col])
    assert np.all(s[bad] == 0.0) and np.all(s[~bad] > 1e-100)
    set_layout(monkeypatch, layout, bank_order=0)
    if name == "t1024":
        monkeypatch.setenv("SCHPF_DEVICE_PLAN", "0")      # the engine's plan from the builder that plan_halves asks
    with load_engine(amd, X, K, ref) as eng:
        info = assert_kernels(eng, pair, layout, packed, which)
        assert info["windows_cell"] == 1 and info["windows_gene"] == 1, info
        win_rows = -info["chunk_len"]
        if name == "t1024":     # balanced windows renumber the minor rows block by block: no claim about the half there
            for major, minor, nM, nm in ((X.row, X.col, n, 2 * n), (X.col, X.row, 2 * n, n)):
                half = plan_halves(major, minor, X.data, nM, nm, pair[1], layout.wpb, win_rows)
                assert np.all(half[bad] == want_half) and np.any(half[~bad] == 1 - want_half)
        two_steps(eng, ref, "underflow in the %s half, %dx%d K%d %s %s"
                  % ((which,) + pair + (K, name, "packed" if packed else "unpacked")))


# ------------------------------------------------------------------------------------- real values, stored zeros
@pytest.mark.parametrize("pair,K", [((4, 2), 16), ((5, 2), 20)], ids=["4x2-K16", "5x2-K20"])   # (4,2): on the path
def test_real_values_and_stored_zeros(amd, oracle, monkeypatch, pair, K):
    layout = LAYOUTS[("t1024", 0)]
    N, G = shapes.matrix_shape("tile", pair, layout)
    base = shapes.case_matrix(N, G, K, 1)
    rng = np.random.RandomState(8)
    data = (base.data * rng.uniform(0.25, 1.75, base.nnz)).astype(np.float32).astype(np.float64)   # the device keeps float32
    nz = 40
    X = coo_matrix((np.r_[data, np.zeros(nz)], (np.r_[base.row, rng.randint(0, N, nz)].astype(np.int32),
                                                np.r_[base.col, rng.randint(0, G, nz)].astype(np.int32))), shape=(N, G))
    X.sum_duplicates()
    assert (X.data == 0).sum() >= nz // 2 and np.any(X.data != np.round(X.data))
    ref = Reference(oracle, X, K)
    set_layout(monkeypatch, layout)
    with load_engine(amd, X, K, ref) as eng:
        assert_kernels(eng, pair, layout, 0, "real values")
        assert eng.upload_info()["zeros"] == int((X.data == 0).sum())
        two_steps(eng, ref, "real values, stored zeros %dx%d K%d" % (pair + (K,)))
