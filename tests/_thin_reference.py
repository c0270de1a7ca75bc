"""Count thinning restated in NumPy, from the definition alone: Philox4x32 with 10 rounds in uint64
arithmetic, vectorised over the draw blocks of all entries.  The host restatement of the library
(schpf_debug_thin_counts) and, through it, the kernels are held to this bit for bit.  Also what both thinning test files share: the matrix and the call of the host restatement."""
import ctypes

import numpy as np
from scipy.sparse import coo_matrix

from schpf_amd import _lib

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

# (counter, key, output) of Philox4x32-10
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox(c0, c1, c2, c3, k0, k1):
    """Arrays (or scalars) of 32-bit words -> the four output words, uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)).copy() for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2            # 32 x 32 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def threshold(frac):
    return int(np.floor(frac * 2.0 ** 32))


def draw_words(row, col, x, seed):
    """The words every trial of every entry reads: (entry, block number, the four words) per draw block.  Depends on the
    seed, not on the fraction: compute once, threshold many times (`thin`)."""
    row, col, x = (np.asarray(a).astype(np.int64) for a in (row, col, x))
    n_blocks = (x + 3) // 4
    entry = np.repeat(np.arange(x.shape[0]), n_blocks)                      # the entry of every draw block
    first = np.cumsum(n_blocks) - n_blocks
    j = np.arange(entry.shape[0], dtype=np.int64) - first[entry]            # its number within the entry
    return entry, j, philox(row[entry], col[entry], j, np.zeros_like(j), seed & 0xFFFFFFFF, seed >> 32)


def thin(x, frac, drawn):
    """(train, test) int32 arrays and the statistics [train nonzeros, test nonzeros, sum train, sum test] of the counts
    x under `frac`, from drawn = draw_words(row, col, x, seed)."""
    x = np.asarray(x).astype(np.int64)
    entry, j, words = drawn
    T = np.uint64(threshold(frac))
    hits = np.zeros(entry.shape[0], np.int64)
    for w, word in enumerate(words):
        hits += (4 * j + w < x[entry]) & (word < T)
    test = np.bincount(entry, weights=hits, minlength=x.shape[0]).astype(np.int64)
    train = x - test
    stats = [int((train > 0).sum()), int((test > 0).sum()), int(train.sum()), int(test.sum())]
    return train.astype(np.int32), test.astype(np.int32), stats


KINDS = {np.dtype(np.int32): _lib.VAL_I32, np.dtype(np.int64): _lib.VAL_I64,
         np.dtype(np.float32): _lib.VAL_F32, np.dtype(np.float64): _lib.VAL_F64}
HEAVY = [0, 1, 3, 4, 5, 255, 256, 257, 260, 1000, 65537, 2 ** 24]      # one entry each, behind the random matrix


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def debug_thin(row, col, val, frac, seed):
    row, col = np.ascontiguousarray(row, np.int32), np.ascontiguousarray(col, np.int32)
    val = np.ascontiguousarray(val)
    train, test = np.full(len(val), -7, np.int32), np.full(len(val), -7, np.int32)
    stats = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().schpf_debug_thin_counts(len(val), _p(row), _p(col), _p(val), KINDS[val.dtype], float(frac),
                                                   ctypes.c_uint64(seed), _p(train), _p(test), stats))
    return train, test, [int(s) for s in stats]


def matrix_with_heavy_tail():
    """257 x 1031, about 5 000 distinct entries with counts 0 .. 40, then one entry of each count of HEAVY."""
    rng = np.random.RandomState(3)
    X = coo_matrix((np.ones(5000, np.int32), (rng.randint(0, 257, 5000), rng.randint(0, 1031, 5000))), shape=(257, 1031))
    X.sum_duplicates()
    row, col = X.row.astype(np.int32), X.col.astype(np.int32)
    val = rng.randint(0, 41, row.shape[0]).astype(np.int32)
    hrow = np.arange(len(HEAVY), dtype=np.int32) * 20 + 1
    hcol = np.full(len(HEAVY), 1030, np.int32)
    free = ~((row[:, None] == hrow[None, :]) & (col[:, None] == hcol[None, :])).any(axis=1)     # distinct coordinates
    return (np.concatenate([row[free], hrow]), np.concatenate([col[free], hcol]),
            np.concatenate([val[free], np.array(HEAVY, np.int32)]))
