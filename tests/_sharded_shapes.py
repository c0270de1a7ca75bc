"""The sharded iteration on every sweep shape: the cases of tests/_sweep_shapes.py as two row shards, and the matrix of
the shard edges (DESIGN.md "parity").

A rank of a sharded fit runs code no unsharded engine reaches (combine_strided_kernel, the gene update from the
exchange buffer and its tail, the plans of a hinted rank), and that code depends on K, KP and the plan.  This module
derives, for tests/test_sharded_shapes_host.py (which pins the arithmetic) and tests/test_sharded_shapes_gpu.py (which
runs it):

  * one sharded case per case of _sweep_shapes.cases(plan): the same (plan, dtype, pair, K, layout), on a matrix of
    N2 = 2 * (need + 96) cells and G = need + 65 genes, need = max(rows per block, rows per LDS window) under the cap of
    _sweep_shapes.matrix_shape, so that each of the two nnz-balanced row shards keeps more than one block of major
    rows and more than one window in both orientations (gather: 2 x 193 cells, 217 genes);
  * the unpacked cases with one count of 70 000 in EACH shard (in one shard alone, that shard would run 16-byte
    entries and the other 8-byte ones);
  * edge_matrix(): 290 cells in three shards, the middle one a single cell; genes that one shard or every shard lacks;
    stored zeros and repeated entries.

Never calls the device."""
import functools

import numpy as np
from scipy.sparse import coo_matrix

import _sweep_shapes as shapes
from conftest import synthetic_counts
from schpf_amd.sharded import row_partition

BIG_COUNT = 70000


class ShardedCase(object):
    def __init__(self, base):
        self.base = base
        self.plan, self.dtype, self.K, self.layout = base.plan, base.dtype, base.K, base.layout
        self.NV, self.LPC = base.NV, base.LPC
        if base.plan == "gather":
            self.need, self.N, self.G = 0, 2 * 193, 217
        else:
            self.need = shapes.matrix_shape(base.plan, (base.NV, base.LPC), base.layout)[0] - 41
            self.N, self.G = 2 * (self.need + 96), self.need + 65
        self.id = base.id

    win_rows = property(lambda self: self.base.win_rows)
    several_windows = property(lambda self: self.base.several_windows)

    @property
    def block_rows(self):
        return (64 // self.LPC) * self.layout.wpb

    def matrix(self):
        return case_matrix(self.N, self.G, self.K, self.layout.packed)

    def bounds(self):
        return [int(b) for b in row_partition(self.matrix(), 2)]


def big_count_positions(X):
    """Where the unpacked matrix of X's pattern holds its counts of 70 000: the middle stored entry of each shard."""
    bounds = row_partition(X, 2)
    keeps = [np.flatnonzero((X.row >= bounds[r]) & (X.row < bounds[r + 1])) for r in range(2)]
    return [int(k[k.size // 2]) for k in keeps]


@functools.lru_cache(maxsize=4)
def case_matrix(N, G, K, packed):
    X = synthetic_counts(N, G, min(0.12, 90000.0 / (N * G)), seed=K)
    if not packed:
        for at in big_count_positions(X):      # the partition reads the pattern alone: the counts do not move it
            X.data[at] = BIG_COUNT
    for a in (X.data, X.row, X.col):
        a.setflags(write=False)
    return X


def cases(plan):
    return [ShardedCase(c) for c in shapes.cases(plan)]


def pair_cases(plan):
    """One case per (dtype, pair) of a plan for the library-driven iteration on one rank: the packed 1024-thread layout
    of the tile pairs, the packed matrix of the gather pairs."""
    name = "t1024" if plan == "tile" else "gather"
    return [c for c in cases(plan) if c.layout.name == name and c.layout.packed]


# --------------------------------------------------------------------------------------------------------- shard edges
EDGE_CELLS = (150, 1, 139)            # cells per shard; the middle shard is one cell
EDGE_NNZ = (1200, 1290, 1110)         # stored entries per shard: cum = 1200 = T / 3 and 2490 >= 2 T / 3 = 2400
EDGE_GENES = 260
EDGE_KS = (20, 50)
# genes by where they have stored entries
EDGE_COMMON = (0, 200)                # every shard (the heavy cell draws from these alone)
EDGE_NOT_IN_1 = (200, 230)            # shards 0 and 2
EDGE_ONLY_0 = (230, 240)
EDGE_ONLY_2 = (240, 250)
EDGE_NOWHERE = (250, 260)


@functools.lru_cache(maxsize=1)
def edge_matrix():
    """290 x 260, 3 600 stored entries in the order drawn (not sorted, duplicates kept): cells 0..149 and 151..289 hold
    8 entries each (the last one 6), cell 150 holds 1 290 -- over 200 genes, so most of them repeat --, which is what
    the nnz-balanced partition needs to cut [0, 150, 151, 290].  Every tenth light cell repeats one of its genes; every
    17th stored entry of the light cells is a stored zero."""
    rng = np.random.RandomState(77)
    row, col = [], []
    cell = 0
    for shard, (ncells, nnz) in enumerate(zip(EDGE_CELLS, EDGE_NNZ)):
        if ncells == 1:
            row.append(np.full(nnz, cell))
            col.append(rng.randint(EDGE_COMMON[0], EDGE_COMMON[1], nnz))
            cell += 1
            continue
        own = EDGE_ONLY_0 if shard == 0 else EDGE_ONLY_2
        must = np.concatenate([np.arange(*EDGE_NOT_IN_1), np.arange(*own)])     # 40 genes, each taken in turn
        for i in range(ncells):
            n = 8 if i < ncells - 1 else nnz - 8 * (ncells - 1)
            genes = np.concatenate([[must[i % must.size]], rng.choice(EDGE_COMMON[1], n - 1, replace=False)])
            if i % 10 == 0:
                genes[2] = genes[1]
            row.append(np.full(n, cell))
            col.append(genes)
            cell += 1
    row, col = np.concatenate(row).astype(np.int32), np.concatenate(col).astype(np.int32)
    data = rng.negative_binomial(2, 0.5, row.size) + 1
    light = np.flatnonzero(row != EDGE_CELLS[0])
    data[light[::17]] = 0
    perm = rng.permutation(row.size)
    X = coo_matrix((data[perm].astype(np.int32), (row[perm], col[perm])), shape=(sum(EDGE_CELLS), EDGE_GENES))
    for a in (X.data, X.row, X.col):
        a.setflags(write=False)
    return X


# ----------------------------------------------------------------------------------------------------------- reference
A, C, AP, CP = 0.3, 0.3, 1.0, 1.0
NAMES = ("xi", "theta", "eta", "beta")


def start_state(oracle, X, K, dtype):
    """The start of tests/test_sweep_shapes_gpu.py Reference: the reference's own setup, drawn from np.random.seed(K)."""
    np.random.seed(K)
    bp, dp, st = oracle.setup_state(X, K, np.dtype(dtype), A, AP, C, CP)
    st.xi_shape[:] = AP + K * A
    st.eta_shape[:] = CP + K * C
    return bp, dp, st


def frozen(st):
    st = st.copy()
    for a in st.arrays():
        a.setflags(write=False)
    return st


class Reference(object):
    """The oracle on one (matrix, K, dtype): the start and the state after each of `steps` iterations (`flags` per
    iteration; `xphi`: the responsibilities of the first), the loss after the last.  Read-only."""

    def __init__(self, oracle, X, K, dtype, steps=2, flags=None, xphi=None):
        self.bp, self.dp, st = start_state(oracle, X, K, dtype)
        self.states = [frozen(st)]
        for it in range(steps):
            oracle.cavi_iteration(X.data, X.row, X.col, st, A, C, self.bp, self.dp, xphi=xphi if it == 0 else None,
                                  **(flags[it] if flags else {}))
            self.states.append(frozen(st))
        self.loss = float(oracle.mean_negative_pois_llh(X.data, X.row, X.col, st.theta_shape, st.theta_rate,
                                                        st.beta_shape, st.beta_rate))


def relative_distance(got, want):
    """Largest |got - want| / |want| over the eight arrays of two states, in float64."""
    worst = 0.0
    for g, w in zip(got.arrays(), want.arrays()):
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        worst = max(worst, float(np.max(np.abs(g - w) / np.abs(w))))
    return worst


def state_bound(dtype, it):
    """The shapes module's bound on the state after iteration `it` (0-based) against the oracle."""
    return 2e-5 * (it + 1) if np.dtype(dtype) == np.float32 else 1e-11
