// What the translation units that read a caller's CSR in device memory share (doublets.hip, qc.hip, group_stats.hip,
// transpose.hip) on top of the scaffold of device_call.h: the loaders for the index and value kinds of include/schpf_hip.h,
// the matrix record, the bisection of a row, and -- in csr_checks -- the validation of a CSR to a level of csr_words.h: the
// two kernels, the words of their smallest offenders and the refusals in the words of csr_words.h.
#pragma once
#include <rocprim/device/device_scan.hpp>

#include "csr_words.h"
#include "device_call.h"
#include "philox.h"

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

// the first of the n ascending columns at p that is not below `key`
template <typename I> __device__ __forceinline__ int64_t lower_bound(const I *__restrict__ p, int64_t n, long long key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((long long)p[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

namespace csr_checks {

constexpr int CSR_THREADS = 256;
constexpr int CSR_CHECK_BLOCKS = 4096;   // workgroups of csr_entries_kernel at the most: 16 per CU
enum { W_BAD_INDPTR = 0, W_BAD_INDEX, W_BAD_ORDER, W_BAD_VALUE, W_BAD_ROW, W_BAD_LABEL, W_VMAX, W_COUNT };

// indptr starts at 0, does not decrease and ends at nnz: the smallest offending row.  Every lane of a wavefront leaves the
// loop before the reduction: no early return
static __global__ __launch_bounds__(CSR_THREADS) void csr_indptr_kernel(const void *__restrict__ indptr, int indptr_kind,
                                                                        int64_t ncells, int64_t nnz,
                                                                        unsigned long long *__restrict__ words)
{
    unsigned long long bad = NONE;
    for (int64_t r = blockIdx.x * (int64_t)CSR_THREADS + threadIdx.x; r <= ncells; r += (int64_t)gridDim.x * CSR_THREADS) {
        const long long here = load_index(indptr, indptr_kind, r);
        const bool wrong = (r == 0 && here != 0) || (r == ncells ? here != nnz : load_index(indptr, indptr_kind, r + 1) < here);
        if (wrong) offends(bad, r);
    }
    report_min(words + W_BAD_INDPTR, bad);
}

// A wavefront per row checks the entries to `level` (csr_words.h): every column in [0, ngenes); from CSR_ORDER on every
// column above its left neighbour; at CSR_COUNTS every value a count thinning accepts, and the largest value.  W_VMAX takes
// the largest value as the smallest complement: it starts at NONE like the offenders, and NONE is a largest value of 0
template <int level> __global__ __launch_bounds__(CSR_THREADS) void csr_entries_kernel(Matrix m, unsigned long long *__restrict__ words)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (CSR_THREADS / 64);
    unsigned long long bad_index = NONE, bad_order = NONE, bad_value = NONE, vmax = 0;
    for (int64_t r = blockIdx.x * (int64_t)(CSR_THREADS / 64) + (threadIdx.x >> 6); r < m.ncells; r += waves) {
        const int64_t from = load_index(m.indptr, m.indptr_kind, r), to = load_index(m.indptr, m.indptr_kind, r + 1);
        for (int64_t e = from + lane; e < to; e += 64) {
            const long long c = load_index(m.indices, m.idx_kind, e);
            if (c < 0 || c >= m.ngenes) offends(bad_index, e);
            if (level >= CSR_ORDER && e > from && load_index(m.indices, m.idx_kind, e - 1) >= c) offends(bad_order, r);
            if (level < CSR_COUNTS) continue;
            const double v = load_value(m.val, m.val_kind, e);
            if (thin_value_bad(v)) offends(bad_value, e);
            else if ((unsigned long long)v > vmax) vmax = (unsigned long long)v;
        }
    }
    report_min(words + W_BAD_INDEX, bad_index);
    if (level >= CSR_ORDER) report_min(words + W_BAD_ORDER, bad_order);
    if (level < CSR_COUNTS) return;
    report_min(words + W_BAD_VALUE, bad_value);
    const unsigned long long least = wave_min(~vmax);
    // a million wavefronts on one address is what this kernel would wait for: only a value above the one seen goes there
    if (lane == 0 && least < __atomic_load_n(words + W_VMAX, __ATOMIC_RELAXED)) atomicMin(words + W_VMAX, least);
}

#define CSR_LAUNCH(kernel, n, per_block, st, ...)                                                                          \
    do {                                                                                                                   \
        hipLaunchKernelGGL(kernel, dim3(grid_for(n, per_block)), dim3(schpf::csr_checks::CSR_THREADS), 0, st, __VA_ARGS__); \
        HIPCHK(hipGetLastError());                                                                                         \
    } while (0)

struct Words : Offenders<W_COUNT> {   // the smallest offenders and the largest value, and the refusals of operator `op`
    uint64_t vmax() const { return ~h[W_VMAX]; }
    void refuse_indptr(const char *op) const
    {
        refuse(W_BAD_INDPTR, [op](int64_t row) { return csr_bad_indptr(op, row); });
    }
    void refuse_entries(const char *op) const   // a word that the level of the check left alone refuses nothing
    {
        refuse(W_BAD_INDEX, [op](int64_t entry) { return csr_bad_index(op, entry); });
        refuse(W_BAD_ORDER, [op](int64_t row) { return csr_bad_order(op, row); });
        refuse(W_BAD_VALUE, [op](int64_t entry) { return csr_bad_value(op, entry); });
    }
};

// The two launches; the caller fetches the words and refuses.  The indptr comes first and is fetched before anything follows
// it into the entries.  A bounded grid for the entries: a wavefront walks many rows and reports once
inline void launch_indptr_check(hipStream_t st, const Matrix &m, int64_t nnz, Words &w)
{
    CSR_LAUNCH(csr_indptr_kernel, m.ncells + 1, CSR_THREADS, st, m.indptr, m.indptr_kind, m.ncells, nnz, w.dev());
}
template <int level> inline void launch_entries_check(hipStream_t st, const Matrix &m, Words &w)
{
    const int per_wave = CSR_THREADS / 64;
    CSR_LAUNCH(csr_entries_kernel<level>, std::min<int64_t>(m.ncells, CSR_CHECK_BLOCKS * per_wave), per_wave, st, m, w.dev());
}

// out[i] = in[0] + .. + in[i - 1] (rocPRIM)
inline void exclusive_scan(hipStream_t st, Scratch &temp, const int64_t *in, int64_t *out, size_t n)
{
    temp.run([&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, in, out, (int64_t)0, n, rocprim::plus<int64_t>(), st); });
}

}  // namespace csr_checks

}  // namespace schpf
