"""Count thinning, the parts that need no GPU: the generator against its known answers, the library's
serial restatement (schpf_debug_thin_counts, the bit-identical reference of the kernels) against a NumPy restatement of
the definition, the invariants of a split, what is refused, and that nothing computes without a GPU."""
import ctypes
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse import coo_matrix

import _thin_reference as ref
from schpf_amd import _lib

from _thin_reference import debug_thin, matrix_with_heavy_tail, _p

FRACS = [2.0 ** -32, 0.1, 0.5, 1.0 - 2.0 ** -31]
SEEDS = [7, 0x9E3779B97F4A7C15]                                          # the second one has a high key word


@functools.lru_cache(maxsize=None)
def drawn(seed):
    """The NumPy restatement's words for the matrix above: once per seed, shared by the fractions."""
    row, col, val = matrix_with_heavy_tail()
    return ref.draw_words(row, col, val, seed)


def test_philox_known_answers():
    lib = _lib.load()
    for counter, key, want in ref.KNOWN_ANSWERS:
        c, k, out = np.array(counter, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
        assert lib.schpf_debug_philox(_p(c), _p(k), _p(out)) == 0
        assert [int(w) for w in out] == list(want)
        assert [int(w[0]) for w in ref.philox(*counter, *key)] == list(want)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("frac", FRACS)
def test_host_restatement_equals_numpy_bitwise(frac, seed):
    row, col, val = matrix_with_heavy_tail()
    assert 4800 < len(val) < 5100
    train, test, stats = debug_thin(row, col, val, frac, seed)
    want_train, want_test, want_stats = ref.thin(val, frac, drawn(seed))
    assert_array_equal(test, want_test)
    assert_array_equal(train, want_train)
    assert stats == want_stats
    # the invariants, on the library's own arrays
    assert_array_equal(train.astype(np.int64) + test, val)
    assert (train >= 0).all() and (test >= 0).all()
    assert stats == [int((train > 0).sum()), int((test > 0).sum()), int(train.sum(dtype=np.int64)),
                     int(test.sum(dtype=np.int64))]


def test_the_extreme_fractions_do_what_they_say():
    """T = 1 sends a trial to the test matrix with probability 2^-32, T = 2^32 - 2 keeps it with that probability:
    derived, not measured -- over the 2^24 + ~2e5 trials of the matrix the expected number of exceptions is 4e-3."""
    row, col, val = matrix_with_heavy_tail()
    _, test, _ = debug_thin(row, col, val, FRACS[0], 7)
    assert test.sum() <= 1
    train, _, _ = debug_thin(row, col, val, FRACS[-1], 7)
    assert train.sum() <= 1


def test_split_is_independent_of_storage():
    row, col, val = matrix_with_heavy_tail()
    train, test, stats = debug_thin(row, col, val, 0.3, 11)
    perm = np.random.RandomState(0).permutation(len(val))
    ptrain, ptest, pstats = debug_thin(row[perm], col[perm], val[perm], 0.3, 11)
    assert_array_equal(ptrain, train[perm])
    assert_array_equal(ptest, test[perm])
    assert pstats == stats
    for dtype in (np.int64, np.float32, np.float64):
        vtrain, vtest, vstats = debug_thin(row, col, val.astype(dtype), 0.3, 11)
        assert_array_equal(vtrain, train)
        assert_array_equal(vtest, test)
        assert vstats == stats
    # another seed, another fraction: another split
    assert not np.array_equal(debug_thin(row, col, val, 0.3, 12)[1], test)
    assert not np.array_equal(debug_thin(row, col, val, 0.31, 11)[1], test)


@pytest.mark.parametrize("bad", [2.5, -1.0, 2.0 ** 24 + 1, np.nan, np.inf])
def test_bad_values_are_refused_with_the_smallest_offender(bad):
    row, col = np.arange(10, dtype=np.int32), np.arange(10, dtype=np.int32)
    val = np.full(10, 3.0)
    val[4] = val[8] = bad
    with pytest.raises(ValueError, match=r"thinning needs integer counts in \[0, 2\^24\]; offending entry 4$"):
        debug_thin(row, col, val, 0.5, 0)
    if bad == -1.0:
        with pytest.raises(ValueError, match="offending entry 4$"):
            debug_thin(row, col, val.astype(np.int64), 0.5, 0)
    val[4] = val[8] = 2.0 ** 24            # the largest count there is
    train, test, _ = debug_thin(row, col, val, 0.5, 0)
    assert train[4] + test[4] == 2 ** 24


def test_bad_indices_are_refused_before_bad_values():
    row, col = np.arange(10, dtype=np.int32), np.arange(10, dtype=np.int32)
    val = np.full(10, 3, np.int32)
    val[2] = -1
    col[6] = -1
    row[9] = -1
    with pytest.raises(ValueError, match="COO index out of range at entry 6$"):
        debug_thin(row, col, val, 0.5, 0)


@pytest.mark.parametrize("frac", [0.0, 1.0, np.nan, -0.5, 1.5, 2.0 ** -33])
def test_bad_fractions_are_refused(frac):
    one = np.ones(1, np.int32)
    with pytest.raises(ValueError, match=r"frac must be in \(0, 1\)"):
        debug_thin(one, one, one, frac, 0)


def test_sizes_and_pointers():
    lib = _lib.load()
    stats = (ctypes.c_int64 * 4)(5, 5, 5, 5)
    assert lib.schpf_debug_thin_counts(0, None, None, None, 0, 0.5, 0, None, None, stats) == 0      # nnz = 0 succeeds
    assert list(stats) == [0, 0, 0, 0]
    assert lib.schpf_debug_thin_counts(3, None, None, None, 0, 0.5, 0, None, None, stats) != 0
    assert b"NULL" in lib.schpf_last_error()
    for fn, lead in ((lib.schpf_debug_thin_counts, ()), (lib.schpf_thin_counts, (0,))):
        assert fn(*lead, 2 ** 31, None, None, None, 0, 0.5, 0, None, None, stats) != 0
        assert b"2^31" in lib.schpf_last_error()
    assert lib.schpf_thin_counts_device(0, None, 2 ** 31, None, None, 0, None, 0, 0.5, 0, None, None, stats) != 0
    assert b"2^31" in lib.schpf_last_error()
    assert lib.schpf_thin_counts_device(0, None, 3, None, None, 0, None, 0, 0.5, 0, None, None, stats) != 0
    assert b"NULL" in lib.schpf_last_error()


def test_test_sum_is_binomial():
    """200 000 entries of x = 5 at frac = 0.1: the sum of the test counts is Binomial(10^6, 0.1) if the trials are
    independent and fair -- within 6 standard deviations of 10^5 (derived: 6 sqrt(10^6 * 0.1 * 0.9) = 1 800)."""
    n = 200000
    e = np.arange(n)
    train, test, stats = debug_thin(e // 1000, e % 1000, np.full(n, 5, np.int32), 0.1, 2024)
    assert stats[3] == int(test.sum())
    print("sum of test counts: %d" % stats[3])
    assert abs(stats[3] - 1e5) <= 6.0 * np.sqrt(1e6 * 0.1 * 0.9)
    # and the per-entry counts follow Binomial(5, 0.1): P(0) = 0.59049, 6 sigma of the count of zeros
    zeros = int((test == 0).sum())
    assert abs(zeros - n * 0.9 ** 5) <= 6.0 * np.sqrt(n * 0.9 ** 5 * (1 - 0.9 ** 5))


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_cpu_path():
    """Without a GPU the split raises; the host restatement is test infrastructure, not a fallback."""
    from schpf_amd import thin_counts
    X = coo_matrix((np.array([3, 1, 4]), (np.array([0, 1, 2]), np.array([2, 1, 0]))), shape=(3, 3))
    with pytest.raises(_lib.SchpfHipError):
        thin_counts(X, 0.2)
    one = np.ones(1, np.int32)
    stats = (ctypes.c_int64 * 4)()
    assert _lib.load().schpf_thin_counts(0, 1, _p(one), _p(one), _p(one), 0, 0.5, 0, _p(one.copy()), _p(one.copy()),
                                         stats) != 0


def test_python_surface():
    import schpf
    import schpf_amd
    from schpf_amd import loss, thinning
    assert schpf_amd.thin_counts is thinning.thin_counts and schpf.thin_counts is thinning.thin_counts
    assert "thinned_mean_negative_pois_llh" in loss.__all__ and hasattr(schpf.loss, "thinned_mean_negative_pois_llh")
    X = coo_matrix(np.ones((3, 3), int))
    for run in (schpf_amd.run_trials, schpf_amd.run_trials_pool):
        with pytest.raises(ValueError, match="thin cannot be combined"):
            run(X, 2, thin=0.2, vcells=X)
        with pytest.raises(ValueError, match="thin cannot be combined"):
            run(X, 2, thin=0.2, vX=X)
    from schpf_amd.cli import _parser
    for cmd in ("train", "train-pool"):
        args = _parser().parse_args([cmd, "-i", "x.mtx", "-k", "3", "--thin", "0.25", "--thin-seed", "9"])
        assert args.thin == 0.25 and args.thin_seed == 9
        args = _parser().parse_args([cmd, "-i", "x.mtx", "-k", "3"])
        assert args.thin is None and args.thin_seed == 0
