"""NumPy / SciPy yardsticks and input makers of the neighbour-graph tests, and the ctypes calls of the three
entry points.  The yardsticks are written from the definition in include/schpf_hip.h, with np.exp in the place of the
library's exponential; the input makers build (idx, dist) directly -- no k-NN search is run."""
import ctypes

import numpy as np

UMAP, JACCARD = 0, 1       # SCHPF_GRAPH_*
METHODS = {"umap": UMAP, "jaccard": JACCARD}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------------- the yardstick
def _weight(e, s):
    """W(e, s) of the definition, elementwise: t = e / s; 0 beyond 708, else exp(-t)."""
    with np.errstate(over="ignore", divide="ignore"):
        t = e / s
    return np.where(t > 708.0, 0.0, np.exp(-np.clip(t, 0.0, 708.0)))


def numpy_calibration(dist):
    """(rho, sigma, w, stopped) of every row: the bisection of the definition run on all rows at once -- a row that has
    stopped is frozen -- with every sum serial in column order.  stopped: the loop ended by its tolerance and sigma is
    what it left."""
    dist = np.asarray(dist, np.float64)
    n, k = dist.shape
    target = np.log2(k + 1.0)
    positive = np.where(dist > 0, dist, np.inf)
    rho = positive.min(axis=1)
    rho[np.isinf(rho)] = 0.0
    total = np.zeros(n)
    for j in range(k):
        total = total + dist[:, j]
    e = dist - rho[:, None]
    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    live = np.ones(n, bool)
    for _ in range(64):
        psum = np.zeros(n)
        for j in range(k):
            psum = psum + np.where(e[:, j] > 0, _weight(e[:, j], mid), 1.0)
        live &= ~(np.abs(psum - target) < 1e-5)
        above = live & (psum > target)
        below = live & ~(psum > target)
        hi = np.where(above, mid, hi)
        lo = np.where(below, mid, lo)
        with np.errstate(invalid="ignore", over="ignore"):
            halfway = (lo + hi) / 2.0
        mid = np.where(above, halfway, np.where(below, np.where(np.isinf(hi), mid * 2.0, halfway), mid))
        if not live.any():
            break
    sigma = mid.copy()
    least = 1e-3 * (total / k)
    clamp = (rho > 0) & (sigma < least)
    sigma[clamp] = least[clamp]
    w = np.where(e <= 0, 1.0, _weight(e, sigma[:, None]))
    return rho, sigma, w, ~live & ~clamp


def numpy_graph(idx, dist, method):
    """The definition on dense n x n matrices -> (indptr, indices, data, rho, sigma, stopped); rho .. are None for jaccard."""
    idx = np.asarray(idx)
    n, k = idx.shape
    rows = np.repeat(np.arange(n), k)
    present = np.zeros((n, n), bool)
    present[rows, idx.ravel()] = True
    assert present.sum() == n * k and not present.diagonal().any()
    either = present | present.T
    rho = sigma = stopped = None
    if method == "umap":
        rho, sigma, w, stopped = numpy_calibration(dist)
        a = np.zeros((n, n))
        a[rows, idx.ravel()] = w.ravel()
        b = a.T
        c = (a + b) - a * b
    else:
        member = (present | np.eye(n, dtype=bool)).astype(np.int64)
        m = member @ member.T
        c = m / (2.0 * (k + 1) - m)
    indptr = np.concatenate([[0], np.cumsum(either.sum(axis=1))]).astype(np.int64)
    indices = np.nonzero(either)[1].astype(np.int32)
    return indptr, indices, c[either], rho, sigma, stopped


def scipy_graph(idx, dist, method, w=None):
    """The same graph by sparse matrices -- transpose, multiply and add -- as a user without the library would write it
    (what tools/graph_time.py times; w: the directed weights, where numpy_calibration has been run already).  CSR; explicit
    zeros are not kept apart from structural ones."""
    from scipy.sparse import csr_matrix, identity
    idx = np.asarray(idx)
    n, k = idx.shape
    indptr = np.arange(n + 1, dtype=np.int64) * k
    if method == "umap":
        w = numpy_calibration(dist)[2] if w is None else w
        a = csr_matrix((w.ravel(), idx.ravel(), indptr), shape=(n, n))
        t = a.T.tocsr()
        return (a + t - a.multiply(t)).tocsr()
    ones = csr_matrix((np.ones(n * k), idx.ravel(), indptr), shape=(n, n))
    member = (ones + identity(n, format="csr")).tocsr()
    shared = (member @ member.T).multiply(((ones + ones.T) > 0)).tocsr()
    shared.data = shared.data / (2.0 * (k + 1) - shared.data)
    return shared


# ------------------------------------------------------------------------------------------------------------ the inputs
def score_lists(n, k, seed=0, K=20):
    """The exact self graph of n Gamma-distributed score rows, ascending in distance (dense NumPy; small n)."""
    x = np.random.RandomState(seed).gamma(0.3, 2.0, (n, K))
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int32), np.sqrt(np.take_along_axis(d2, idx, axis=1))


def random_lists(n, k, seed=0):
    """Lists of any size without a search: half of a row's neighbours sit next to it on a ring (many mutual edges), the
    others anywhere; distances Gamma-distributed, ascending."""
    rng = np.random.RandomState(seed)
    i = np.arange(n, dtype=np.int64)[:, None]
    near = k // 2
    steps = np.array([(s // 2 + 1) * (1 if s % 2 == 0 else -1) for s in range(near)], np.int64)
    idx = np.empty((n, k), np.int64)
    idx[:, :near] = (i + steps[None, :]) % n
    idx[:, near:] = rng.randint(0, n, (n, k - near))
    while True:
        s = np.sort(idx, axis=1)
        again = (s[:, 1:] == s[:, :-1]).any(axis=1) | (idx == i).any(axis=1)
        if not again.any():
            break
        idx[again, near:] = rng.randint(0, n, (int(again.sum()), k - near))
    dist = np.sort(rng.gamma(2.0, 0.5, (n, k)), axis=1)
    return idx.astype(np.int32), dist


def ring_lists(n, k):
    """i +- 1 .. +- k/2 on a ring: every edge is mutual, nnz = n k."""
    assert k % 2 == 0 and k < n
    steps = np.concatenate([np.arange(1, k // 2 + 1), -np.arange(1, k // 2 + 1)])
    idx = (np.arange(n)[:, None] + steps[None, :]) % n
    return idx.astype(np.int32), np.abs(steps)[None, :] * np.linspace(0.5, 1.5, n)[:, None]


def chain_lists(n, k):
    """i -> i + 1 .. i + k (mod n), k < n / 2: no edge is mutual, nnz = 2 n k -- the capacity, exactly."""
    assert 2 * k < n
    steps = np.arange(1, k + 1)
    idx = (np.arange(n)[:, None] + steps[None, :]) % n
    return idx.astype(np.int32), steps[None, :] * np.linspace(1.0, 2.0, n)[:, None]


def hub_lists(n):
    """k = 2, every row lists {0, 1} except rows 0 and 1 themselves: in-degree n - 1."""
    idx = np.tile(np.array([0, 1], np.int32), (n, 1))
    idx[0] = [1, 2]
    idx[1] = [0, 2]
    dist = np.random.RandomState(n).gamma(2.0, 0.5, (n, 2))
    return idx, np.sort(dist, axis=1)


def duplicated_cells(idx, dist):
    """Rows 3 and 10: all distances 0 (rho = 0); row 5: zeros and positives mixed."""
    dist = dist.copy()
    dist[3] = 0.0
    dist[10] = 0.0
    dist[5, : dist.shape[1] // 2] = 0.0
    return idx, dist


def far_neighbour(idx, dist):
    """Rows 2 and 7: one neighbour at 1e6 times the rest -- t > 708, an explicit 0 weight."""
    dist = dist.copy()
    dist[2, -1] = 1e6 * dist[2, -2]
    dist[7, 0] = 1e6 * dist[7, 1:].max()
    return idx, dist


def unsorted(idx, dist):
    """The columns of every row in another order (the same for all rows): ascending distances are not assumed."""
    perm = np.random.RandomState(5).permutation(idx.shape[1])
    return np.ascontiguousarray(idx[:, perm]), np.ascontiguousarray(dist[:, perm])


# ------------------------------------------------------------------------------------------------------ the entry points
def _outputs(n, k, fill):
    return (np.full(n + 1, fill, np.int64), np.full(2 * n * k, fill, np.int32), np.full(2 * n * k, float(fill), np.float64),
            np.full(n, float(fill), np.float64), np.full(n, float(fill), np.float64))


def _cut(method, n, out):
    indptr, indices, data, rho, sigma = out
    nnz = int(indptr[n]) if n else 0
    return indptr, indices[:nnz], data[:nnz], (rho if method == UMAP else None), (sigma if method == UMAP else None)


def _prepare(idx, dist, method):
    idx = np.ascontiguousarray(idx, np.int32)
    dist = None if dist is None or method == JACCARD else np.ascontiguousarray(dist, np.float64)
    return idx, dist


def debug_graph(idx, dist, method):
    """schpf_debug_knn_graph: the library's serial restatement on the host -> (indptr, indices, data, rho, sigma)."""
    from schpf_amd import _lib
    idx, dist = _prepare(idx, dist, method)
    n, k = idx.shape
    out = _outputs(n, k, -7)
    _lib.check(_lib.load().schpf_debug_knn_graph(method, n, k, _p(idx), _p(dist), *[_p(a) for a in out]))
    return _cut(method, n, out)


def host_graph(idx, dist, method):
    """schpf_knn_graph: host pointers, staged through the device."""
    from schpf_amd import _lib
    idx, dist = _prepare(idx, dist, method)
    n, k = idx.shape
    out = _outputs(n, k, -7)
    _lib.check(_lib.load().schpf_knn_graph(0, method, n, k, _p(idx), _p(dist), *[_p(a) for a in out]))
    return _cut(method, n, out)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)
