"""The mechanics of one call into the library, shared by the Python operators: the loaded library, pointers
of arrays and tensors, the device, the stream.  What an operator is handed -- matrices, graphs, labels -- is brought into
the library's forms in `device_input`; this module knows nothing of them.
"""
import ctypes
import os

from . import _lib


def library():
    """The loaded library, on a machine that has a GPU.  Both are asked of `_lib` at every call, so whatever stands there
    in their place (the host tests put the host restatements there) is what the operators get."""
    lib = _lib.load()
    _lib.require_gpu()
    return lib


def array_ptr(a):
    """A NumPy array's memory; NULL for None or an empty array, which is what the library takes for "not given"."""
    return None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)


def tensor_ptr(t):
    """A torch tensor's memory; NULL for None or an empty tensor."""
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def stats_ptr(a):
    """An int64 NumPy array as the `int64_t stats[]` of an entry point."""
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def device_of(device):
    """The HIP device ordinal: the one given, else $SCHPF_DEVICE, else 0."""
    return int(os.environ.get("SCHPF_DEVICE", "0")) if device is None else int(device)


def stream_of(dev):
    """torch's current stream on `dev` as the library takes it: a call there is ordered after whatever produced its inputs
    and before whatever reads its results.  STREAM_DEFAULT stands for the null stream, whose handle is 0."""
    import torch
    return ctypes.c_void_p(int(torch.cuda.current_stream(dev).cuda_stream) or _lib.STREAM_DEFAULT)


def same_device(index, device, noun, verb="is"):
    """Refuse a `device` argument that names another GPU than the one (`index`) the input lives on."""
    if device is not None and int(device) != index:
        raise ValueError("%s %s on GPU %d, device=%d was asked for" % (noun, verb, index, int(device)))
