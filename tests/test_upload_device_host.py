"""The upload of a count matrix from GPU memory, the parts that need no GPU: the C ABI's declarations and
their binding, and the classification of what DeviceCAVI.upload is given (schpf_amd/device_input.py) on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse import coo_matrix

from conftest import ROOT
from schpf_amd import _lib, device_input

torch = pytest.importorskip("torch")

NEW = {
    "schpf_upload_coo_device": [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                ctypes.c_void_p, ctypes.c_int],
    "schpf_upload_csr_device": [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                ctypes.c_int, ctypes.c_void_p, ctypes.c_int],
    "schpf_marginals": [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)],
    "schpf_set_state_device": [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p],
    "schpf_get_state_device": [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p],
}


def header():
    text = open(os.path.join(ROOT, "include", "schpf_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_new_calls_and_the_shim_binds_them():
    text = header()
    for name, argtypes in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in include/schpf_hip.h" % name
        assert len(m.group(1).split(",")) == len(argtypes), name
        assert _lib.SIGNATURES[name] == argtypes, name
    assert re.search(r"#define\s+SCHPF_IDX_I32\s+%d\b" % _lib.IDX_I32, text)
    assert re.search(r"#define\s+SCHPF_IDX_I64\s+%d\b" % _lib.IDX_I64, text)
    assert (_lib.IDX_I32, _lib.IDX_I64) == (0, 1)
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name).argtypes == NEW[name]


def small():
    """5 x 4 with a repeated entry, a stored zero and an unsorted order."""
    row = np.array([3, 0, 0, 4, 3, 1], np.int64)
    col = np.array([1, 2, 2, 0, 3, 1], np.int64)
    val = np.array([2, 1, 5, 0, 7, 3], np.float64)
    return row, col, val, (5, 4)


@pytest.mark.parametrize("vdtype, vkind", [(torch.int32, _lib.VAL_I32), (torch.int64, _lib.VAL_I64),
                                           (torch.float32, _lib.VAL_F32), (torch.float64, _lib.VAL_F64)])
def test_cpu_coo_tensor_is_routed_to_the_host_path(vdtype, vkind):
    row, col, val, shape = small()
    t = torch.sparse_coo_tensor(torch.tensor(np.stack([row, col])), torch.tensor(val).to(vdtype), shape)
    inp = device_input.classify(t, shape)
    assert inp.kind == "host" and inp.nnz == 6 and inp.shape == shape
    X = inp.matrix
    assert_array_equal(X.row, row)          # uncoalesced: the duplicates stay separate, the order stays
    assert_array_equal(X.col, col)
    assert_array_equal(X.data, val)
    assert X.shape == shape
    assert device_input._VALUE_KINDS[str(vdtype)] == vkind
    assert not device_input.on_gpu(t)


@pytest.mark.parametrize("idtype, ikind", [(torch.int32, _lib.IDX_I32), (torch.int64, _lib.IDX_I64)])
def test_cpu_csr_tensor_with_either_index_type(idtype, ikind):
    row, col, val, shape = small()
    S = coo_matrix((val, (row, col)), shape=shape).tocsr()       # sums the repeated entry
    t = torch.sparse_csr_tensor(torch.tensor(S.indptr).to(idtype), torch.tensor(S.indices).to(idtype),
                                torch.tensor(S.data), size=shape)
    assert device_input._kind(device_input._INDEX_KINDS, t.crow_indices(), "indices") == ikind
    inp = device_input.classify(t, shape)
    assert inp.kind == "host" and inp.nnz == S.nnz
    want = S.tocoo()
    assert_array_equal(inp.matrix.row, want.row)
    assert_array_equal(inp.matrix.col, want.col)
    assert_array_equal(inp.matrix.data, want.data)


def test_scipy_inputs_pass_through():
    row, col, val, shape = small()
    X = coo_matrix((val, (row, col)), shape=shape)
    assert device_input.classify(X, shape).matrix is X
    inp = device_input.classify(X.tocsr(), shape)
    assert inp.kind == "host" and inp.nnz == 5
    assert device_input.as_matrix(X) is X


def test_what_is_refused():
    row, col, val, shape = small()
    ind = torch.tensor(np.stack([row, col]))
    with pytest.raises(TypeError, match="float16"):
        device_input.classify(torch.sparse_coo_tensor(ind, torch.tensor(val).to(torch.float16), shape), shape)
    with pytest.raises(TypeError, match="sparse COO"):
        device_input.classify(torch.zeros(shape), shape)                         # dense
    with pytest.raises(ValueError, match="2-d"):
        device_input.classify(torch.sparse_coo_tensor(torch.zeros((3, 1), dtype=torch.int64), torch.ones(1), (2, 2, 2)))
    with pytest.raises(ValueError, match="engine was created for"):
        device_input.classify(torch.sparse_coo_tensor(ind, torch.tensor(val), shape), (5, 5))
    with pytest.raises(TypeError, match="SciPy"):
        device_input.classify(np.zeros(shape), shape)
    with pytest.raises(TypeError):
        device_input.classify(torch.sparse_coo_tensor(ind, torch.tensor(val), shape).to_sparse_csc(), shape)


def test_the_new_calls_fail_without_a_context():
    """No CPU fallback and no crash: without an engine the calls return a status and leave a message."""
    lib = _lib.load()
    assert lib.schpf_upload_coo_device(None, 0, None, None, 0, None, 0) != 0
    assert b"NULL" in lib.schpf_last_error()
    assert lib.schpf_upload_csr_device(None, 0, None, 0, None, 0, None, 0) != 0
    assert lib.schpf_marginals(None, None, None) != 0
    assert lib.schpf_set_state_device(None, 0, None, None) != 0
    assert lib.schpf_get_state_device(None, 0, None, None) != 0


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_gpu_no_upload():
    from schpf_amd import DeviceCAVI, loss, scHPF, HPF_Gamma
    row, col, val, shape = small()
    t = torch.sparse_coo_tensor(torch.tensor(np.stack([row, col])), torch.tensor(val), shape)
    with pytest.raises(_lib.SchpfHipError):
        DeviceCAVI(5, 4, 2).upload(t)
    g = lambda *d: HPF_Gamma(np.ones(d), np.ones(d))  # noqa: E731
    with pytest.raises(_lib.SchpfHipError):
        loss.genemean_negative_pois_llh(t, theta=g(5, 2), beta=g(4, 2))
    with pytest.raises(_lib.SchpfHipError):
        scHPF(2, verbose=False).fit(t)
