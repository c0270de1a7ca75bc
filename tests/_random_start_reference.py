"""NumPy restatement of the device-drawn first responsibilities (sweep_impl.h: mix64, draw_base, exp1_draw; MODE_RANDOM).

The generator is a pure function of (seed, cell, gene, k):

    base = mix64(seed ^ mix64(cell * 0x100000001B3 + gene))                  64-bit, wrapping (splitmix64's finaliser)
    z    = fmix32(lo32(base) ^ (hi32(base) + k * 0x9E3779B9))                murmur3's 32-bit finaliser, wrapping
    u    = (float32(z >> 8) + 0.5f) * 2^-24                                  float32, round to nearest even: in (0, 1]
    e_k  = -log(u),    phi_k = e_k / sum_k e_k,    xphi_k = x * phi_k

Every integer step is exact in NumPy's uint64 / uint32 and the float32 steps are restated as written, so `u` here is the
device's `u` bit for bit.  The one step that is not restated is the logarithm: the device takes `__logf(u)` (the hardware
base-2 logarithm times ln 2, float32), this module takes the float64 logarithm of that exact float32 `u`.  That makes it
the truth the device's logarithm is measured against (tests/test_random_start_gpu.py), not a copy of it.

u = 1 does occur: z >> 8 = 0xFFFFFF gives 16777215.5, which float32 rounds to 2^24.  Then e = 0 and phi_k = 0 exactly.
The smallest u is 2^-25 (z >> 8 = 0), e = 25 ln 2 = 17.33.

Entries with x <= 0 get no draw (xphi = 0); repeated (cell, gene) entries get the same phi each.

A rank of a sharded engine numbers its cells from 0 and is handed the seed `rank_seed(seed, rank)` by
schpf_amd/sharded.py; capi.hip init_phi_device adds the same offset once more where a communicator of more than one
rank is attached to the engine (`communicator=True`).

Never calls the device."""
import numpy as np

U64 = np.uint64
U32 = np.uint32
GOLDEN64 = 0x9E3779B97F4A7C15
KEY_MULTIPLIER = 0x100000001B3      # draw_base: cell * KEY_MULTIPLIER + gene
MASK64 = 2 ** 64 - 1


def mix64(z):
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = z + U64(GOLDEN64)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def key(cell, gene):
    """What draw_base hashes for a nonzero: cell * 0x100000001B3 + gene, modulo 2^64."""
    with np.errstate(over="ignore"):
        return np.asarray(cell).astype(U64) * U64(KEY_MULTIPLIER) + np.asarray(gene).astype(U64)


def draw_base(seed, cell, gene):
    return mix64(U64(int(seed) & MASK64) ^ mix64(key(cell, gene)))


def bits24(seed, cell, gene, K):
    """[n, K] uint32: the 24-bit value z >> 8 every draw is made of."""
    base = draw_base(seed, cell, gene)
    lo = (base & U64(0xFFFFFFFF)).astype(U32)[:, None]
    hi = (base >> U64(32)).astype(U32)[:, None]
    with np.errstate(over="ignore"):
        z = lo ^ (hi + np.arange(K, dtype=U32)[None, :] * U32(0x9E3779B9))
        z ^= z >> U32(16)
        z *= U32(0x85EBCA6B)
        z ^= z >> U32(13)
        z *= U32(0xC2B2AE35)
        z ^= z >> U32(16)
    return z >> U32(8)


def uniforms(seed, cell, gene, K):
    """[n, K] float32, the device's u bit for bit: (float32(z >> 8) + 0.5f) * 2^-24.  z >> 8 < 2^24 converts exactly;
    the sum rounds to nearest even in float32 (NumPy's float32 add does), the product with a power of two is exact."""
    v = bits24(seed, cell, gene, K).astype(np.float32)
    u = (v + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert u.dtype == np.float32
    return u


def draws(seed, cell, gene, K):
    """e[n, K] float64 = -log(u), the logarithm taken in float64 of the exact float32 u."""
    e = -np.log(uniforms(seed, cell, gene, K).astype(np.float64))
    return e + 0.0          # -log(1) = -0.0 -> +0.0


def phi(seed, cell, gene, K):
    e = draws(seed, cell, gene, K)
    return e / e.sum(1, keepdims=True)


def xphi(X, seed, K):
    """[nnz, K] float64: x * phi of every stored entry of the COO matrix X, in its stored order; 0 where x <= 0."""
    x = np.asarray(X.data, dtype=np.float64)
    out = np.zeros((x.shape[0], K))
    live = x > 0
    out[live] = x[live, None] * phi(seed, X.row[live], X.col[live], K)
    return out


def rank_seed(seed, rank, communicator=False):
    """The seed a rank's draws are keyed by: what sharded.py hands the rank's engine, plus what capi.hip adds itself
    when the engine belongs to a communicator of more than one rank."""
    times = 2 if communicator else 1
    return (int(seed) + times * GOLDEN64 * (rank + 1)) & MASK64


def xphi_sharded(X, bounds, seed, K, communicator=False):
    """xphi of the whole matrix as the row shards [bounds[r], bounds[r + 1]) draw it: local cell numbers, rank seeds."""
    x = np.asarray(X.data, dtype=np.float64)
    out = np.zeros((x.shape[0], K))
    for r in range(len(bounds) - 1):
        lo, hi = int(bounds[r]), int(bounds[r + 1])
        mine = (X.row >= lo) & (X.row < hi) & (x > 0)
        out[mine] = x[mine, None] * phi(rank_seed(seed, r, communicator), X.row[mine] - lo, X.col[mine], K)
    return out


def find_edge_draw(seed, N, G, K, want, chunk=40000, limit=400):
    """The first (cell, gene, k) of an N x G matrix, cells ascending, whose 24-bit value equals `want` under `seed`
    (0xFFFFFF: u rounds to 1; 0: the smallest u), or None after limit * chunk nonzeros."""
    start = 0
    for _ in range(limit):
        flat = np.arange(start, min(start + chunk, N * G), dtype=np.int64)
        if flat.size == 0:
            return None
        cell, gene = flat // G, flat % G
        hit = np.argwhere(bits24(seed, cell, gene, K) == U32(want))
        if hit.size:
            j, k = hit[0]
            return int(cell[j]), int(gene[j]), int(k)
        start += chunk
    return None
