// What the translation units that read a caller's GRAPH in device memory share (louvain.hip, components.hip): an n x n CSR
// with int64 indptr, int32 indices and double values.  The validation of indptr with the words of its refusal, the row of
// every entry by bisection, Louvain's integer weights, the per-workgroup minimum of the validation kernels, rocPRIM's
// two-call protocol on one scratch buffer, and the grid and launch conventions of both files.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>
#include <string>

#include "csr_device.h"
#include "kernels.h"

namespace schpf {

typedef unsigned long long count_t;   // what rocPRIM writes a number of runs as

struct Larger {
    __host__ __device__ double operator()(const double &a, const double &b) const { return a > b ? a : b; }
};

// Louvain's integer weight of a stored value (include/schpf_hip.h): the one expression of louvain.hip, components.hip and
// host.cpp
__host__ __device__ __forceinline__ int64_t louvain_quantum(double value, double wmax) { return llrint(ldexp(value / wmax, 30)); }

__device__ __forceinline__ void block_min(int bad, int *__restrict__ part)
{
    __shared__ int red[256];
    red[threadIdx.x] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

#define GRID_STRIDE(v, n) for (int64_t v = blockIdx.x * (int64_t)256 + threadIdx.x; v < (n); v += (int64_t)gridDim.x * 256)

static __global__ __launch_bounds__(256) void louvain_indptr_kernel(const int64_t *__restrict__ indptr, int n, int *__restrict__ part)
{
    int bad = INT_MAX;
    GRID_STRIDE(i, n)
    {
        if ((i == 0 && indptr[0] != 0) || indptr[i + 1] < indptr[i]) bad = min(bad, (int)i);
    }
    block_min(bad, part);
}

// the largest row i < n with indptr[i] <= e: the row that holds entry e (indptr[0] = 0, indptr does not decrease)
static __global__ __launch_bounds__(256) void louvain_rows_kernel(const int64_t *__restrict__ indptr, int64_t n, int64_t nnz,
                                                                  int32_t *__restrict__ rowof)
{
    GRID_STRIDE(e, nnz)
    {
        int64_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (indptr[mid] <= e) lo = mid;
            else hi = mid;
        }
        rowof[e] = (int32_t)lo;
    }
}

// One thread per entry: column in range and, where `ascending`, above its left neighbour; value (data may be nullptr: not
// looked at) finite and >= 0
template <bool ascending>
__global__ __launch_bounds__(256) void louvain_check_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                            const double *__restrict__ data, const int32_t *__restrict__ rowof,
                                                            int n, int64_t nnz, int *__restrict__ part_col,
                                                            int *__restrict__ part_val)
{
    int bad_col = INT_MAX, bad_val = INT_MAX;
    GRID_STRIDE(e, nnz)
    {
        const int row = rowof[e], col = indices[e];
        if (col < 0 || col >= n || (ascending && e > indptr[row] && indices[e - 1] >= col)) bad_col = min(bad_col, row);
        if (data) {
            const double v = data[e];
            if (!(v >= 0.0 && v <= DBL_MAX)) bad_val = min(bad_val, row);
        }
    }
    block_min(bad_col, part_col);
    __syncthreads();   // the LDS of block_min is used again
    block_min(bad_val, part_val);
}

static __global__ __launch_bounds__(256) void louvain_quantise_kernel(const double *__restrict__ data, const double *__restrict__ wmax,
                                                                      int64_t nnz, int64_t *__restrict__ q)
{
    const double m = *wmax;
    GRID_STRIDE(e, nnz) q[e] = louvain_quantum(data[e], m);
}

inline unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1 << 20)); }

inline int bits_of(uint64_t largest)   // the bits a radix sort has to look at for keys up to `largest`
{
    int b = 1;
    while (b < 64 && (largest >> b)) ++b;
    return b;
}

#define LAUNCH(kernel, n, st, ...)                                                          \
    do {                                                                                    \
        hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(256), 0, st, __VA_ARGS__);      \
        HIPCHK(hipGetLastError());                                                          \
    } while (0)

// rocPRIM's two-call protocol on one scratch buffer that grows when a call asks for more
struct Scratch {
    DevBuf buf;
    template <typename F> void run(F &&f)
    {
        size_t bytes = 0;
        HIPCHK(f((void *)nullptr, bytes));
        if (bytes > buf.bytes || !buf.p) buf.alloc(bytes);   // hipFree waits for what still reads the old one
        HIPCHK(f(buf.p, bytes));
    }
};

// indptr[n + 1] in device memory: refused unless it starts at 0 and does not decrease.  Returns nnz = indptr[n]
inline int64_t louvain_indptr_on_device(hipStream_t st, int n, const int64_t *indptr)
{
    const int64_t blocks = grid_for(n);
    DevBuf part, bad;
    part.alloc((size_t)blocks * sizeof(int));
    bad.alloc(2 * sizeof(int));
    LAUNCH(louvain_indptr_kernel, n, st, indptr, n, part.as<int>());
    HIPCHK(launch_knn_bad(part.as<int>(), blocks, nullptr, 0, bad.as<int>(), st));
    int h_bad[2];
    int64_t nnz = 0;
    HIPCHK(hipMemcpyAsync(&nnz, indptr + n, sizeof nnz, hipMemcpyDeviceToHost, st));
    d2h(h_bad, bad, sizeof h_bad, st);
    if (h_bad[0] != INT_MAX) throw std::invalid_argument(louvain_bad_indptr(h_bad[0]));
    return nnz;
}

}  // namespace schpf
