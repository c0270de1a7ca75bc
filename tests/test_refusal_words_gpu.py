"""The refusal channel of the stateless operators with the offenders spread out.  The refusal tests of the
operators' own files use inputs of a few dozen items, so every offender sits in workgroup 0 and the minimum across
wavefronts and workgroups is never asked.  Here every check gets three offenders -- one in a late workgroup, one in a
middle workgroup at a lane of its second or third wavefront, one a few items above that one -- and the middle one must be
named, in the words of the library's serial restatement (schpf_debug_*), by the device entry and by its host-pointer twin,
with every output still holding the -7 it was filled with.  Each entry also runs once on the same shape with valid input
and must equal the restatement bit for bit.  The operators that read a count CSR (doublet_rows, axis_stats, submatrix,
group_stats, transpose) get the same treatment for the four refusals of the matrix they share: indptr, column range,
column order and, where the operator looks at values, a value that is no count.

The shape: 1 000 rows of 3 entries, so the kernels with a thread per entry span 12 workgroups of 256 and the ones with a
thread per row span 4; 640 root sets and 640 pairs (3 workgroups); a k-NN table of 128 padded rows x 16 factors (8
workgroups); neighbour lists of 300 rows (5 workgroups of 64 rows)."""
import ctypes

import numpy as np
import pytest

from _graph_reference import UMAP, random_lists
from _knn_reference import DTYPES, gamma_scores

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, PER_ROW, SETS = 1000, 3, 640
MIDDLE, ABOVE, LATE = 370, 374, 900          # rows; their first entries are 1110, 1122, 2700
S_MIDDLE, S_ABOVE, S_LATE = 326, 330, 600    # sets, roots and pairs
BAD_ROWS, BAD_SETS = [LATE, ABOVE, MIDDLE], [S_LATE, S_ABOVE, S_MIDDLE]


def test_the_offenders_are_where_the_reduction_is_asked():
    """In a middle workgroup of 256 threads, in its second or third wavefront; the late one in another workgroup."""
    for middle, above, late, items in ((MIDDLE, ABOVE, LATE, N), (PER_ROW * MIDDLE, PER_ROW * ABOVE, PER_ROW * LATE, PER_ROW * N),
                                       (S_MIDDLE, S_ABOVE, S_LATE, SETS)):
        last = (items - 1) // 256
        assert 0 < middle // 256 < last and (middle % 256) // 64 in (1, 2)
        assert middle < above < middle + 64 and above // 256 == middle // 256
        assert middle // 256 < late // 256 <= last


@pytest.fixture(scope="module")
def lib():
    from schpf_amd import _lib
    _lib.require_gpu()
    return _lib.load()


class In:
    """An input array (None: a NULL pointer): device memory for the device entry."""
    def __init__(self, array):
        self.array = None if array is None else np.ascontiguousarray(array)


class Out:
    """An output filled with -7: device memory for the device entry."""
    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, dtype


class HostOut(Out):
    """An output that is host memory for every entry (stats, wmax)."""


class Dev:
    """An argument that the device entry alone takes (the kinds of the index arrays of a count CSR)."""
    def __init__(self, value):
        self.value = value


def call(lib, name, how, spec):
    """schpf_debug_<name> / schpf_<name> / schpf_<name>_device on `spec` -> (status, message, the outputs as NumPy)."""
    fn = getattr(lib, {"debug": "schpf_debug_%s", "host": "schpf_%s", "device": "schpf_%s_device"}[how] % name)
    args = {"debug": [], "host": [0], "device": [0, None]}[how]
    spec = [item.value if isinstance(item, Dev) else item for item in spec if how == "device" or not isinstance(item, Dev)]
    kinds = fn.argtypes[len(args):]
    assert len(kinds) == len(spec)
    keep, outs = [], []
    for item, kind in zip(spec, kinds):
        if not isinstance(item, (In, Out)):
            args.append(item)
            continue
        a = item.array if isinstance(item, In) else np.full(item.shape, -7, item.dtype)
        on_device = how == "device" and not isinstance(item, HostOut) and a is not None
        t = torch.tensor(a, device="cuda:0") if on_device else a
        keep.append(t)
        if isinstance(item, Out):
            outs.append(t)
        if a is None or a.size == 0:
            args.append(None)
        elif on_device:
            args.append(ctypes.c_void_p(t.data_ptr()))
        else:
            args.append(a.ctypes.data_as(kind))
    if how == "device":
        torch.cuda.synchronize()
    status = fn(*args)
    message = lib.schpf_last_error().decode() if status else ""
    return status, message, [o.cpu().numpy() if how == "device" and not isinstance(o, np.ndarray) else o for o in outs]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def refused(lib, name, spec, words):
    status, want, _ = call(lib, name, "debug", spec)
    assert status != 0 and words in want
    for how in ("device", "host"):
        status, message, outs = call(lib, name, how, spec)
        assert status != 0 and message == want, (how, message, want)
        for o in outs:
            assert (o == -7).all(), how


def accepted(lib, name, spec, cut=lambda outs: outs):
    status, _, want = call(lib, name, "debug", spec)
    assert status == 0
    for how in ("device", "host"):
        status, message, outs = call(lib, name, how, spec)
        assert status == 0, (how, message)
        for k, (a, b) in enumerate(zip(cut(outs), cut(want))):
            assert same_bits(a, b), (how, k)


# -------------------------------------------------------------------------------------------------------------- the inputs
def ring_graph():
    """Row i holds the columns i - 1, i + 1 and i + 500 (mod 1000), ascending: symmetric, 3 entries in every row."""
    i = np.arange(N)
    cols = np.sort(np.stack([(i - 1) % N, (i + 1) % N, (i + N // 2) % N], axis=1), axis=1)
    rows = np.repeat(i, PER_ROW)
    data = 1.0 + ((rows + cols.ravel()) % 7) * 0.25
    return PER_ROW * np.arange(N + 1, dtype=np.int64), cols.ravel().astype(np.int32), data


def spoilt(array, where, value):
    out = array.copy()
    out[where] = value
    return out


def decreasing(ptr, at):
    """ptr[r + 1] < ptr[r] for r in `at`: the rows r offend, their neighbours do not."""
    out = ptr.copy()
    for r in at:
        out[r + 1] = out[r] - 1
    return out


INDPTR, INDICES, DATA = ring_graph()
FIRST = PER_ROW * np.array(BAD_ROWS)            # the first entry of every offending row
BAD_INDPTR = decreasing(INDPTR, BAD_ROWS)
BAD_COLUMNS = spoilt(INDICES, FIRST, N)
BAD_VALUES = spoilt(DATA, FIRST + 1, np.nan)
LABELS = (np.random.RandomState(1).randint(-1, 5, N)).astype(np.int32)
G = 5
SET_PTR = np.arange(SETS + 1, dtype=np.int64)   # one root per set: root e belongs to set e
ROOTS = ((np.arange(SETS) * 7) % N).astype(np.int32)
PAIRS = np.stack([np.arange(SETS) % G, (np.arange(SETS) % G + 1 + np.arange(SETS) % (G - 1)) % G], axis=1).astype(np.int32)


# --------------------------------------------------------------------------------------------------------------- the tests
def louvain(indptr=INDPTR, indices=INDICES, data=DATA):
    return [N, In(indptr), In(indices), In(data), 1.0, Out(N, np.int32), HostOut(4, np.int64)]


def test_louvain(lib):
    refused(lib, "louvain", louvain(indptr=BAD_INDPTR), "indptr must be 0 at row 0 and must be non-decreasing; offending row 370")
    refused(lib, "louvain", louvain(indices=BAD_COLUMNS), "strictly ascending within a row; offending row 370")
    refused(lib, "louvain", louvain(data=BAD_VALUES), "values must be finite and >= 0; offending row 370")
    accepted(lib, "louvain", louvain())


def components(indices=INDICES, within=None):
    return [N, In(INDPTR), In(indices), In(within), Out(N, np.int32), HostOut(6, np.int64)]


def test_components(lib):
    within = (np.arange(N) % 3 - 1).astype(np.int32)
    refused(lib, "components", components(indices=BAD_COLUMNS), "columns must be in [0, n); offending row 370")
    refused(lib, "components", components(within=spoilt(within, BAD_ROWS, -2)), "within must be >= -1; offending vertex 370")
    for w in (None, within):   # the rounds and passes of the device, stats[4..5], are outside the contract
        accepted(lib, "components", components(within=w), cut=lambda outs: [outs[0], outs[1][:4]])


def cluster_graph(data=DATA, labels=LABELS):
    return [N, In(INDPTR), In(INDICES), In(data), In(labels), G, Out(G, np.int64), Out((G, G), np.int64), Out((G, G), np.int64),
            HostOut(1, np.float64)]


def test_cluster_graph(lib):
    refused(lib, "cluster_graph", cluster_graph(data=BAD_VALUES), "values must be finite and >= 0; offending row 370")
    refused(lib, "cluster_graph", cluster_graph(labels=spoilt(LABELS, BAD_ROWS, G)), "labels must be in [-1, G); offending vertex 370")
    accepted(lib, "cluster_graph", cluster_graph())


def geodesic(set_ptr=SET_PTR, roots=ROOTS):
    return [N, In(INDPTR), In(INDICES), In(DATA), 0, SETS, In(set_ptr), In(roots), Out((SETS, N), np.float64), HostOut(3, np.int64)]


def test_geodesic(lib):
    refused(lib, "geodesic", geodesic(set_ptr=decreasing(SET_PTR, BAD_SETS)),
            "set_ptr must be 0 at set 0 and must be non-decreasing; offending set 326")
    refused(lib, "geodesic", geodesic(roots=spoilt(ROOTS, BAD_SETS, N)), "roots must be in [0, n); offending set 326")
    # the rounds and the lowering writes of the device, stats[1..2], are outside the contract
    accepted(lib, "geodesic", geodesic(), cut=lambda outs: [outs[0], outs[1][:1]])


def rank_sums(indptr=INDPTR, indices=INDICES, data=DATA, labels=LABELS):
    """The ring graph read gene-major: gene j is expressed by three cells."""
    return [N, N, In(indptr), In(indices), In(np.asarray(data, np.float32)), In(labels), G, Out(G, np.int64), Out(N, np.int64),
            Out(N, np.int64), Out((G, N), np.int64), Out((G, N), np.int64)]


def test_rank_sums(lib):
    refused(lib, "rank_sums", rank_sums(indptr=BAD_INDPTR), "indptr must be 0 at gene 0 and must be non-decreasing; offending gene 370")
    refused(lib, "rank_sums", rank_sums(indices=BAD_COLUMNS), "strictly ascending within a gene; offending gene 370")
    refused(lib, "rank_sums", rank_sums(data=BAD_VALUES), "values must be finite and >= 0; offending gene 370")
    refused(lib, "rank_sums", rank_sums(labels=spoilt(LABELS, BAD_ROWS, G)), "labels must be in [-1, ngroups); offending cell 370")
    accepted(lib, "rank_sums", rank_sums())


def pair_rank_sums(pairs=PAIRS):
    return [N, N, In(INDPTR), In(INDICES), In(DATA.astype(np.float32)), In(LABELS), G, In(pairs), SETS, Out(G, np.int64),
            Out((G, N), np.int64), Out((SETS, N), np.int64), Out((SETS, N), np.int64)]


def test_pair_rank_sums(lib):
    assert (PAIRS[:, 0] != PAIRS[:, 1]).all() and PAIRS.min() == 0 and PAIRS.max() == G - 1
    bad = PAIRS.copy()
    bad[BAD_SETS, 1] = bad[BAD_SETS, 0]
    refused(lib, "pair_rank_sums", pair_rank_sums(bad), "pairs must name two different groups in [0, ngroups); offending pair 326")
    accepted(lib, "pair_rank_sums", pair_rank_sums())


def knn(query, ref):
    n, K = query.shape
    return [DTYPES[query.dtype], n, len(ref), K, In(query), In(ref), 5, ctypes.c_int64(-1), Out((n, 5), np.int32), Out((n, 5), np.float64)]


def test_knn(lib):
    """Element (row, f) of the table is the thread of lane row % 64, wavefront f % 4, workgroup 4 * (row / 64) + f / 4: of
    8 workgroups, row 20 offends in the third wavefront of workgroup 1, row 23 in its second, row 70 in workgroup 6."""
    query, ref = gamma_scores(100, 16, seed=1), gamma_scores(100, 16, seed=2)
    bad = [(20, 6, np.nan), (23, 5, np.inf), (70, 9, -np.inf)]
    bad_query, bad_ref = query.copy(), ref.copy()
    for row, f, value in bad:
        bad_query[row, f] = bad_ref[row, f] = value
    refused(lib, "knn", knn(bad_query, bad_ref), "scores must be finite; offending row 20 of query")
    refused(lib, "knn", knn(query, bad_ref), "scores must be finite; offending row 20 of ref")
    accepted(lib, "knn", knn(query, ref))


def knn_graph(idx, dist):
    n, k = idx.shape
    return [UMAP, n, k, In(idx), In(dist), Out(n + 1, np.int64), Out(2 * n * k, np.int32), Out(2 * n * k, np.float64),
            Out(n, np.float64), Out(n, np.float64)]


def test_knn_graph(lib):
    """A wavefront of 64 rows is a workgroup: rows 70 and 75 offend in workgroup 1, row 200 in workgroup 3, of 5."""
    idx, dist = random_lists(300, 4, seed=3)
    rows = np.array([200, 75, 70])
    refused(lib, "knn_graph", knn_graph(spoilt(idx, (rows, 0), rows), dist), "other than the row itself; offending row 70")
    refused(lib, "knn_graph", knn_graph(idx, spoilt(dist, (rows, 1), -1.0)), "distances must be finite and >= 0; offending row 70")

    def stored(outs):   # the entries behind indptr[n] are not part of the result
        nnz = int(outs[0][-1])
        return [outs[0], outs[1][:nnz], outs[2][:nnz], outs[3], outs[4]]
    accepted(lib, "knn_graph", knn_graph(idx, dist), cut=stored)


# ------------------------------------------------------------------------------------------------------- the count CSR family
VAL_F32, IDX_I32, IDX_I64 = 2, 0, 1             # SCHPF_VAL_F32, SCHPF_IDX_*
NNZ = PER_ROW * N
COUNTS = (1 + (np.repeat(np.arange(N), PER_ROW) + INDICES) % 7).astype(np.float32)
BAD_ORDER = spoilt(INDICES, FIRST + 1, INDICES[FIRST])     # a column twice: in range, not above its left neighbour
BAD_COUNTS = spoilt(COUNTS, FIRST + 1, 2.5)
WORDS_INDPTR = ": indptr must be 0 at row 0, must be non-decreasing and must end at nnz; offending row 370"
WORDS_INDEX = ": column index out of range at entry 1110"
WORDS_ORDER = ": columns must be strictly ascending within a row; offending row 370"
WORDS_VALUE = ": values must be integer counts in [0, 2^24]; offending entry 1111"
PARENTS = np.stack([(np.arange(SETS) * 7) % N, (np.arange(SETS) * 11 + 3) % N], axis=1).astype(np.int32)


def counts_csr(indptr, indices, val):
    """The leading arguments of the family: the ring graph as a square count matrix, float32 values."""
    return [N, N, NNZ, In(indptr), Dev(IDX_I64), In(indices), Dev(IDX_I32), In(val), VAL_F32]


def refused_matrix(lib, name, tail, prefix, order=True, values=True):
    """The refusals of the matrix, each with three offenders; `tail`: the operator's arguments behind the matrix."""
    spoilt_by = [(BAD_INDPTR, INDICES, COUNTS, WORDS_INDPTR), (INDPTR, BAD_COLUMNS, COUNTS, WORDS_INDEX)]
    if order:
        spoilt_by.append((INDPTR, BAD_ORDER, COUNTS, WORDS_ORDER))
    if values:
        spoilt_by.append((INDPTR, INDICES, BAD_COUNTS, WORDS_VALUE))
    for indptr, indices, val, words in spoilt_by:
        refused(lib, name, counts_csr(indptr, indices, val) + tail, prefix + words)
    accepted(lib, name, counts_csr(INDPTR, INDICES, COUNTS) + tail)


def test_doublet_rows(lib):
    capacity = 2 * PER_ROW * SETS
    tail = [SETS, In(PARENTS), Out(SETS + 1, np.int64), Out(capacity, np.int32), Out(capacity, np.int32), capacity]
    refused_matrix(lib, "doublet_rows", tail, "doublets")


def test_axis_stats(lib):
    flags = (np.arange(N) % 4).astype(np.uint32)
    tail = [2, In(flags), Out(N, np.int64), Out(N, np.int64), Out((2, N), np.int64), Out(N, np.int64), Out(N, np.int64),
            Out(N, np.int64)]
    refused_matrix(lib, "axis_stats", tail, "qc")


def test_submatrix(lib):
    """The submatrix asks the column range alone: neither the order nor the values."""
    rows = ((np.arange(SETS) * 7) % N).astype(np.int32)
    keep = (np.arange(N) % 3 != 0).astype(np.uint8)
    tail = [SETS, In(rows), In(keep), HostOut(1, np.int64), Out(SETS + 1, np.int64), Out(NNZ, np.int32), Out(NNZ, np.float32), NNZ]
    refused_matrix(lib, "submatrix", tail, "qc", order=False, values=False)


def test_group_stats(lib):
    tail = [In(LABELS), G, Out(G, np.int64), Out((G, N), np.int64), Out((G, N), np.int64), Out((G, N), np.int64)]
    refused_matrix(lib, "group_stats", tail, "group_stats")


def test_transpose(lib):
    """The values of a transposed matrix mean nothing to the operator: they move as they are."""
    tail = [VAL_F32, Out(N + 1, np.int64), Out(NNZ, np.int32), Out(NNZ, np.float32), Out(NNZ, np.int64)]
    refused_matrix(lib, "transpose", tail, "transpose", values=False)
