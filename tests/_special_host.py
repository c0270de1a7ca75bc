"""The host build of schpf_amd/csrc/special.h that tests/test_special_host.py and tests/test_special_gpu.py share: the
header compiled with g++ into a small shared library (the device-specific pieces replaced as the header says), one
array-in / array-out wrapper per function."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

SRC = r"""
#include "special.h"
extern "C" {
void h_psi(long n, const double *x, double *o) { for (long i = 0; i < n; ++i) o[i] = schpf::digamma(x[i]); }
void h_psi_less_log(long n, const double *x, const double *rate, double *o)
{ for (long i = 0; i < n; ++i) o[i] = schpf::digamma_less_log(x[i], schpf::fast_rcp(rate[i])); }
void h_log(long n, const double *x, double *o) { for (long i = 0; i < n; ++i) o[i] = schpf::fast_log(x[i]); }
void h_exp(long n, const double *x, double *o) { for (long i = 0; i < n; ++i) o[i] = schpf::fast_exp(x[i]); }
void h_rcp(long n, const double *x, double *o) { for (long i = 0; i < n; ++i) o[i] = schpf::fast_rcp(x[i]); }
}
"""


def build_host(directory):
    """Compile SRC in `directory` (a pathlib.Path); returns call(name, *arrays) -> float64 array."""
    src = directory / "h.cpp"
    src.write_text(SRC)
    so = directory / "libspecial_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-fPIC", "-shared",
                           "-I", os.path.join(ROOT, "schpf_amd", "csrc"), str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))

    def call(name, *arrays):
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
        out = np.empty(arrays[0].shape[0])
        getattr(lib, name)(ctypes.c_long(out.shape[0]), *[a.ctypes.data_as(ctypes.c_void_p) for a in arrays],
                           out.ctypes.data_as(ctypes.c_void_p))
        return out
    return call
