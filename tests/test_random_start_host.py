"""What kind of start the device-drawn responsibilities are, on the NumPy restatement of the generator
(tests/_random_start_reference.py).  tests/test_random_start_gpu.py holds the device to that restatement element by
element, so what is pinned here holds for the device too: every factor's phi is Beta(1, K - 1) (a flat Dirichlet's
marginal), factors and seeds are uncorrelated, cell and gene are told apart, and the draws stay inside [0, 17.33].

Inputs of the statistical checks: 40 000 (cell, gene) pairs, RandomState(1), cells below 2600 and genes below 2700,
seed 1234, K = 2, 8, 50, 225.  The thresholds are conditions on the generator; the restatement met them at these inputs
with: worst mean 2.8 standard errors, smallest KS p 0.03, largest |correlation| of two factors 0.024 (K = 225), of two
seeds 0.002."""
import math

import numpy as np
import pytest
from scipy import stats

import _random_start_reference as rs

SEED, NPAIRS = 1234, 40000
KS = (2, 8, 50, 225)


def pairs():
    rng = np.random.RandomState(1)
    return rng.randint(0, 2600, NPAIRS), rng.randint(0, 2700, NPAIRS)


@pytest.fixture(scope="module", params=KS)
def drawn(request):
    K = request.param
    cell, gene = pairs()
    e = rs.draws(SEED, cell, gene, K)
    e.setflags(write=False)
    return K, cell, gene, e


# ------------------------------------------------------------------ the restatement itself
def scalar_draw_bits(seed, cell, gene, k):
    """The generator once more with Python's unbounded integers and explicit masks: what NumPy's wrapping arithmetic
    in the reference module has to give."""
    M64, M32 = 2 ** 64 - 1, 2 ** 32 - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    base = mix((seed & M64) ^ mix((cell * 0x100000001B3 + gene) & M64))
    z = (base & M32) ^ (((base >> 32) + k * 0x9E3779B9) & M32)
    z ^= z >> 16
    z = (z * 0x85EBCA6B) & M32
    z ^= z >> 13
    z = (z * 0xC2B2AE35) & M32
    z ^= z >> 16
    return z >> 8


def test_numpy_integer_steps_equal_python_integers():
    rng = np.random.RandomState(7)
    cell = np.concatenate([rng.randint(0, 2 ** 31 - 1, 60), [0, 2 ** 31 - 1, 2 ** 24, 2 ** 24 - 1]])
    gene = np.concatenate([rng.randint(0, 2 ** 31 - 1, 60), [0, 2 ** 31 - 1, 5, 2 ** 31 - 1]])
    for seed in (0, 1234, 2 ** 64 - 1, 1234 + 0x9E3779B97F4A7C15):
        got = rs.bits24(seed, cell, gene, 225)
        want = np.array([[scalar_draw_bits(seed, int(i), int(g), k) for k in range(225)] for i, g in zip(cell, gene)])
        assert np.array_equal(got, want)


def test_u_is_float32_arithmetic_as_written():
    """(float32(v) + 0.5f) * 2^-24 against the exact rational value rounded once to float32 (ties to even): the sum
    v + 0.5 needs 25 bits from v = 2^23 on, so it rounds; the product with 2^-24 is exact."""
    v = np.array([0, 1, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 23 + 2, 0xFFFFFE, 0xFFFFFF], dtype=np.uint32)
    u = (v.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    # below 2^23: exact; from 2^23 on a tie between v and v + 1: to the even one
    want = [0.5, 1.5, 2 ** 23 - 0.5, 2 ** 23, 2 ** 23 + 2, 2 ** 23 + 2, 0xFFFFFE, 2 ** 24]
    assert u.dtype == np.float32
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, np.array(want, dtype=np.float64))


def test_key_has_no_collisions_below_2_to_31():
    """cell * M + gene (mod 2^64), M = 0x100000001B3 = 2^40 + 435, tells every (cell, gene) with both below 2^31 apart.

    While cell * M stays below 2^64 (cell < 2^24) it is the plain argument gene < 2^31 < M: the key is a two-digit
    number in base M.  Beyond that the product wraps, so take two keys that agree: d * M = gene' - gene (mod 2^64) with
    d = cell - cell', 0 < |d| < 2^31, and |gene' - gene| < 2^31.  Write d = q * 2^24 + r, 0 <= r < 2^24.  Modulo 2^64,
    d * M = r * 2^40 + 435 d, and |435 d| < 435 * 2^31 < 2^40 - 2^37.
      r = 0: d * M = 435 d exactly, and |435 d| >= 435 * 2^24 > 2^31.
      r > 0: 2^37 < r * 2^40 + 435 d < 2^64 - 2^37, so the residue is further than 2^31 from 0 either way round.
    Neither can be a difference of two genes."""
    M, two31 = rs.KEY_MULTIPLIER, 2 ** 31
    assert M == 2 ** 40 + 435 and two31 < M
    assert 435 * two31 < 2 ** 40 - 2 ** 37 and 435 * 2 ** 24 > two31

    def distance_from_zero(d):          # of d * M modulo 2^64
        v = (d * M) % 2 ** 64
        return min(v, 2 ** 64 - v)
    rng = np.random.RandomState(3)
    ds = [1, 2, 435, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 127 * 2 ** 24, two31 - 1, two31 - 2 ** 24, two31 - 2 ** 24 + 1]
    ds += [int(q) * 2 ** 24 + int(r) for q in range(0, 128, 9) for r in (1, 2, 2 ** 24 - 1)]
    ds += [int(d) for d in rng.randint(1, two31, 2000)]
    assert min(distance_from_zero(d) for d in ds if 0 < d < two31) >= two31
    # and the restatement's own key on a grid that straddles the wrap: all distinct
    idx = np.unique(np.concatenate([np.arange(40), 2 ** 24 + np.arange(-20, 20), two31 - 1 - np.arange(40),
                                    rng.randint(0, two31, 100)]))
    cell, gene = [a.ravel() for a in np.meshgrid(idx, idx)]
    keys = rs.key(cell, gene)
    assert keys.dtype == np.uint64 and np.unique(keys).size == keys.size
    assert int(rs.key(np.array([two31 - 1]), np.array([7]))[0]) == ((two31 - 1) * M + 7) % 2 ** 64


# ------------------------------------------------------------------ the kind of start
def test_every_factor_has_mean_one_over_K(drawn):
    K, _, _, e = drawn
    p = e / e.sum(1, keepdims=True)
    se = math.sqrt((K - 1.0) / (K * K * (K + 1.0)) / NPAIRS)        # Beta(1, K - 1): variance (K - 1) / (K^2 (K + 1))
    worst = float(np.abs(p.mean(0) - 1.0 / K).max() / se)
    print("K = %d: worst mean of a factor, in standard errors: %.2f" % (K, worst))
    assert worst < 5.0
    assert np.allclose(p.sum(1), 1.0, rtol=1e-14, atol=0)


def test_phi_of_a_factor_is_beta_1_Kminus1(drawn):
    K, _, _, e = drawn
    p = e / e.sum(1, keepdims=True)
    pv = [stats.kstest(p[:, k], "beta", args=(1, K - 1)).pvalue for k in range(0, K, max(1, K // 8))]
    print("K = %d: smallest KS p over %d factors: %.3g" % (K, len(pv), min(pv)))
    assert min(pv) > 1e-4


def test_factors_are_uncorrelated(drawn):
    K, _, _, e = drawn
    c = np.corrcoef(e.T)
    np.fill_diagonal(c, 0.0)
    print("K = %d: largest |correlation| of two factors' draws: %.4f" % (K, np.abs(c).max()))
    assert np.abs(c).max() < 0.04


def test_next_seed_is_uncorrelated(drawn):
    K, cell, gene, e = drawn
    e2 = rs.draws(SEED + 1, cell, gene, K)
    r = float(np.corrcoef(e.ravel(), e2.ravel())[0, 1])
    print("K = %d: correlation of the draws under seeds %d and %d: %.4f" % (K, SEED, SEED + 1, r))
    assert abs(r) < 0.01
    assert np.all(np.any(e != e2, axis=1))              # and no nonzero keeps its draws


def test_swapping_cell_and_gene_changes_the_draws(drawn):
    K, cell, gene, e = drawn
    apart = cell != gene
    swapped = rs.draws(SEED, gene[apart], cell[apart], K)
    assert apart.sum() > NPAIRS * 0.99
    assert np.all(np.any(swapped != e[apart], axis=1))
    r = float(np.corrcoef(e[apart].ravel(), swapped.ravel())[0, 1])
    assert abs(r) < 0.01
    same = rs.draws(SEED, cell[~apart], gene[~apart], K)        # cell == gene: the same key, the same draws
    assert np.array_equal(same, e[~apart])


def test_k_is_part_of_the_key(drawn):
    """No two factors of a nonzero share a draw beyond chance: a generator that ignored k would give phi = 1 / K."""
    K, _, _, e = drawn
    assert np.all(e.max(1) > e.min(1))
    repeats = sum(int((e[:, k] == e[:, k + 1]).sum()) for k in range(K - 1))
    assert repeats <= 3 + 10 * NPAIRS * (K - 1) * 2.0 ** -24        # a 24-bit value repeats by chance at rate 2^-24


def test_draws_of_a_smaller_K_are_a_prefix(drawn):
    K, cell, gene, e = drawn
    assert np.array_equal(rs.draws(SEED, cell[:500], gene[:500], 2), e[:500, :2])


def test_range_of_the_draws(drawn):
    """u in (0, 1], so 0 <= e <= 25 ln 2; entries in [0, 1] and rows on the simplex."""
    K, cell, gene, e = drawn
    u = rs.uniforms(SEED, cell, gene, K)
    assert u.dtype == np.float32 and u.min() >= np.float32(2.0 ** -25) and u.max() <= np.float32(1.0)
    assert e.min() >= 0.0 and e.max() <= 25 * math.log(2.0)
    assert not np.any(np.signbit(e))


def test_u_equal_to_one_occurs_and_gives_phi_zero():
    """The all-ones 24-bit value is 16777215.5 before rounding and 2^24 after it: u = 1, e = 0 and phi_k = 0 exactly.
    At K = 225 a 2600 x 2624 matrix holds 1.5e9 draws per seed, so dozens of them; the search takes the first."""
    hit = rs.find_edge_draw(SEED, 2600, 2624, 225, 0xFFFFFF)
    assert hit is not None
    cell, gene, k = hit
    u = rs.uniforms(SEED, np.array([cell]), np.array([gene]), 225)
    assert u[0, k] == np.float32(1.0) and np.all(u[0] > 0)
    e = rs.draws(SEED, np.array([cell]), np.array([gene]), 225)
    p = rs.phi(SEED, np.array([cell]), np.array([gene]), 225)
    assert e[0, k] == 0.0 and not np.signbit(e[0, k]) and p[0, k] == 0.0
    assert np.isfinite(p).all() and abs(p.sum() - 1.0) < 1e-14


def test_smallest_u_gives_the_largest_draw():
    hit = rs.find_edge_draw(SEED, 2600, 2624, 225, 0)
    assert hit is not None
    cell, gene, k = hit
    u = rs.uniforms(SEED, np.array([cell]), np.array([gene]), 225)
    e = rs.draws(SEED, np.array([cell]), np.array([gene]), 225)
    assert u[0, k] == np.float32(2.0 ** -25)
    assert e[0, k] == 25 * math.log(2.0) and e[0, k] == e.max()


# ------------------------------------------------------------------ xphi and the shard conventions
def test_xphi_zeros_duplicates_and_stored_order():
    from scipy.sparse import coo_matrix
    row = np.array([3, 0, 3, 2, 3, 1], dtype=np.int32)
    col = np.array([1, 4, 1, 2, 1, 0], dtype=np.int32)
    val = np.array([2.0, 1.0, 5.0, 0.0, 2.0, 7.0])
    X = coo_matrix((val, (row, col)), shape=(4, 5))
    xp = rs.xphi(X, 99, 6)
    assert xp.shape == (6, 6) and np.all(xp[3] == 0.0)                      # a stored zero gets no draw
    assert np.allclose(xp.sum(1), val, rtol=1e-14, atol=0)
    assert np.array_equal(xp[0], xp[4])                                    # repeated (cell, gene): the same phi each
    assert np.allclose(xp[2] / 5.0, xp[0] / 2.0, rtol=1e-15, atol=0)
    perm = np.array([5, 2, 0, 3, 1, 4])
    Xp = coo_matrix((val[perm], (row[perm], col[perm])), shape=(4, 5))
    assert np.array_equal(rs.xphi(Xp, 99, 6), xp[perm])                    # a function of the entry, not of its position


def test_shard_conventions():
    from scipy.sparse import coo_matrix
    G64 = 0x9E3779B97F4A7C15
    assert rs.rank_seed(5, 0) == 5 + G64 and rs.rank_seed(5, 1) == (5 + 2 * G64) % 2 ** 64
    assert rs.rank_seed(5, 1, communicator=True) == (5 + 4 * G64) % 2 ** 64
    rng = np.random.RandomState(0)
    X = coo_matrix((rng.randint(1, 4, 50), (rng.randint(0, 10, 50), rng.randint(0, 8, 50))), shape=(10, 8))
    got = rs.xphi_sharded(X, [0, 4, 10], 5, 3)
    top, low = X.row < 4, X.row >= 4
    assert np.array_equal(got[top], X.data[top, None] * rs.phi(5 + G64, X.row[top], X.col[top], 3))
    assert np.array_equal(got[low], X.data[low, None] * rs.phi((5 + 2 * G64) % 2 ** 64, X.row[low] - 4, X.col[low], 3))
    assert not np.allclose(got, rs.xphi(X, 5, 3))
