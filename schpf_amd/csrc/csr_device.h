// What the translation units that read a caller's CSR in device memory share (doublets.hip, qc.hip): the loaders for the
// index and value kinds of include/schpf_hip.h, the matrix record, the wavefront minimum of the validation kernels, and
// the device / stream / grid choices of an entry point.
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>

#include "common.h"

namespace schpf {

__device__ __forceinline__ long long load_index(const void *p, int kind, int64_t j)
{
    return kind == SCHPF_IDX_I64 ? static_cast<const long long *>(p)[j] : (long long)static_cast<const int *>(p)[j];
}
// entry j of a value array of kind SCHPF_VAL_* (common.h read_count)
__device__ __forceinline__ double load_value(const void *p, int kind, int64_t j)
{
    switch (kind) {
    case SCHPF_VAL_I32: return (double)static_cast<const int *>(p)[j];
    case SCHPF_VAL_I64: return (double)static_cast<const long long *>(p)[j];
    case SCHPF_VAL_F32: return (double)static_cast<const float *>(p)[j];
    default: return static_cast<const double *>(p)[j];
    }
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

struct Matrix {   // a CSR in device memory whose indptr has been checked: every row lies in [0, nnz)
    int64_t ncells, ngenes;
    const void *indptr, *indices, *val;
    int indptr_kind, idx_kind, val_kind;
};

struct Row {
    int64_t from, len;
};
__device__ __forceinline__ Row row_of(const Matrix &m, int64_t r)
{
    const int64_t from = load_index(m.indptr, m.indptr_kind, r);
    return Row{from, load_index(m.indptr, m.indptr_kind, r + 1) - from};
}

inline unsigned grid_for(int64_t n, int per_block)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, 1 << 20));
}

inline void use_device(int device)
{
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) throw std::invalid_argument("no such HIP device");
    HIPCHK(hipSetDevice(device));
}

inline hipStream_t pick_stream(void *stream, std::unique_ptr<TempStream> &own)
{
    // NULL: a stream of the call's own; SCHPF_STREAM_DEFAULT: the device's null stream; else the given handle
    if (!stream) {
        own.reset(new TempStream);
        return own->st;
    }
    return stream == SCHPF_STREAM_DEFAULT ? nullptr : (hipStream_t)stream;
}

inline size_t value_size(int val_kind) { return val_kind == SCHPF_VAL_I32 || val_kind == SCHPF_VAL_F32 ? 4 : 8; }

}  // namespace schpf
