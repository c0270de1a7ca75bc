// What the translation units that read a caller's CSR with int64 indptr and int32 indices in device memory share on top of
// device_call.h: the n x n graphs of louvain.hip, components.hip and geodesic.hip (double values), and the gene-major
// matrices of rank_sums.hip and pair_rank_sums.hip (through rank_sums_device.h).  The check of an indptr and the call that
// fetches its verdict and its last entry, the row of every entry by bisection, the check of a graph's entries, the check of
// labels in [-1, G), and Louvain's integer weights.  Every check ends in report_min (device_call.h).
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>
#include <string>

#include "device_call.h"

namespace schpf {

typedef unsigned long long count_t;   // what rocPRIM writes a number of runs as

struct Larger {
    __host__ __device__ double operator()(const double &a, const double &b) const { return a > b ? a : b; }
};

// Louvain's integer weight of a stored value (include/schpf_hip.h): the one expression of louvain.hip, components.hip and
// host.cpp
__host__ __device__ __forceinline__ int64_t louvain_quantum(double value, double wmax) { return llrint(ldexp(value / wmax, 30)); }

// indptr[n + 1] starts at 0 and does not decrease: the smallest offending row
static __global__ __launch_bounds__(256) void indptr_check_kernel(const int64_t *__restrict__ indptr, int n,
                                                                  unsigned long long *__restrict__ word)
{
    unsigned long long bad = NONE;
    GRID_STRIDE(i, n)
    {
        if ((i == 0 && indptr[0] != 0) || indptr[i + 1] < indptr[i]) offends(bad, i);
    }
    report_min(word, bad);
}

// the largest row i < n with indptr[i] <= e: the row that holds entry e (indptr[0] = 0, indptr does not decrease)
static __global__ __launch_bounds__(256) void entry_rows_kernel(const int64_t *__restrict__ indptr, int64_t n, int64_t nnz,
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

// One thread per entry of a graph: column in range and, where `ascending`, above its left neighbour; value (data may be
// nullptr: not looked at) finite and >= 0.  The smallest offending row of each
template <bool ascending>
__global__ __launch_bounds__(256) void graph_entries_check_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                  const double *__restrict__ data, const int32_t *__restrict__ rowof,
                                                                  int n, int64_t nnz, unsigned long long *__restrict__ bad_col_word,
                                                                  unsigned long long *__restrict__ bad_val_word)
{
    unsigned long long bad_col = NONE, bad_val = NONE;
    GRID_STRIDE(e, nnz)
    {
        const int row = rowof[e], col = indices[e];
        if (col < 0 || col >= n || (ascending && e > indptr[row] && indices[e - 1] >= col)) offends(bad_col, row);
        if (data) {
            const double v = data[e];
            if (!(v >= 0.0 && v <= DBL_MAX)) offends(bad_val, row);
        }
    }
    report_min(bad_col_word, bad_col);
    report_min(bad_val_word, bad_val);
}

// labels[i] in [-1, G): the smallest offending item
static __global__ __launch_bounds__(256) void labels_check_kernel(const int32_t *__restrict__ labels, int64_t n, int G,
                                                                  unsigned long long *__restrict__ word)
{
    unsigned long long bad = NONE;
    GRID_STRIDE(i, n)
    {
        if (labels[i] < -1 || labels[i] >= G) offends(bad, i);
    }
    report_min(word, bad);
}

static __global__ __launch_bounds__(256) void louvain_quantise_kernel(const double *__restrict__ data, const double *__restrict__ wmax,
                                                                      int64_t nnz, int64_t *__restrict__ q)
{
    const double m = *wmax;
    GRID_STRIDE(e, nnz) q[e] = louvain_quantum(data[e], m);
}

// indptr[n + 1] in device memory: refused, in the words of `refusal`, unless it starts at 0 and does not decrease.  Returns
// indptr[n], the number of entries, which the one synchronisation brings along
template <typename Words> int64_t indptr_on_device(hipStream_t st, int n, const int64_t *indptr, Words &&refusal)
{
    Offenders<1> w;
    w.reset(st);
    LAUNCH(indptr_check_kernel, n, st, indptr, n, w.dev());
    int64_t nnz = 0;
    HIPCHK(hipMemcpyAsync(&nnz, indptr + n, sizeof nnz, hipMemcpyDeviceToHost, st));
    w.fetch(st);
    w.refuse(0, refusal);
    return nnz;
}

}  // namespace schpf
