// Device passes of an upload from HBM (upload_device.h).  Plain HIP C++: streaming kernels whose lanes
// read consecutive elements, a fixed grid that walks the entries in tiles so that a wavefront adds its counts up in
// registers and touches the shared counters once, when it is done.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>

#include "common.h"
#include "upload_device.h"

namespace schpf {
namespace {

constexpr int CV_THREADS = 256, CV_UNROLL = 4, CV_TILE = CV_THREADS * CV_UNROLL;
constexpr unsigned long long NONE = ~0ull;
// slots of the statistics a convert pass leaves in device memory
enum { ST_ROUNDED = 0, ST_ZEROS, ST_BAD_INDEX, ST_BAD_VALUE, ST_FLAGS, ST_COUNT };
constexpr unsigned FLAG_WIDE = 1u, FLAG_NOT_ROW_COL = 2u, FLAG_NOT_COL_ROW = 4u;

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

struct ConvertArgs {
    int64_t nnz;
    const void *row, *col, *val;
    int row_kind, col_kind, val_kind, n_rows, n_cols;
    int32_t *out_row, *out_col;
    float *out_val;
};

// The host loop of schpf_upload_coo, one entry per lane: the same predicates on the same double / float values.
// Block b takes the tiles b, b + gridDim.x, ...; a tile is CV_UNROLL coalesced rows of CV_THREADS entries, loaded before
// any of them is looked at.  The order flags compare an entry with its predecessor: the lane below hands it over, lane
// 0 of a wavefront reads it from memory.
__global__ __launch_bounds__(CV_THREADS) void convert_kernel(ConvertArgs a, unsigned long long *__restrict__ stats)
{
    const int lane = threadIdx.x & 63;
    unsigned long long rounded = 0, zeros = 0;        // wavefront-uniform counts
    unsigned long long bad_index = NONE, bad_value = NONE;
    unsigned flags = 0;
    const int64_t n_tiles = (a.nnz + CV_TILE - 1) / CV_TILE;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t base = t * CV_TILE + threadIdx.x;
        long long r[CV_UNROLL], c[CV_UNROLL];
        double d[CV_UNROLL];
#pragma unroll
        for (int u = 0; u < CV_UNROLL; ++u) {
            int64_t j = base + (int64_t)u * CV_THREADS;
            if (j >= a.nnz) j = a.nnz - 1;   // lanes past the end re-read the last entry
            r[u] = load_index(a.row, a.row_kind, j);
            c[u] = load_index(a.col, a.col_kind, j);
            d[u] = load_value(a.val, a.val_kind, j);
        }
#pragma unroll
        for (int u = 0; u < CV_UNROLL; ++u) {
            const int64_t j = base + (int64_t)u * CV_THREADS;
            const bool live = j < a.nnz;
            const float f = (float)d[u];
            const bool index_bad = r[u] < 0 || r[u] >= a.n_rows || c[u] < 0 || c[u] >= a.n_cols;
            const bool value_bad = !(d[u] >= 0.0 && f <= 3.0e38f);
            const bool wide = !(f <= 65535.0f) || f != (float)(uint32_t)f;
            rounded += __popcll(__ballot(live && (double)f != d[u]));
            zeros += __popcll(__ballot(live && !index_bad && d[u] == 0.0));
            const int ri = (int)r[u], ci = (int)c[u];
            int pr = __shfl_up(ri, 1), pc = __shfl_up(ci, 1);
            if (live && j > 0) {
                if (lane == 0) {
                    pr = (int)load_index(a.row, a.row_kind, j - 1);
                    pc = (int)load_index(a.col, a.col_kind, j - 1);
                }
                if (ri < pr || (ri == pr && ci < pc)) flags |= FLAG_NOT_ROW_COL;
                if (ci < pc || (ci == pc && ri < pr)) flags |= FLAG_NOT_COL_ROW;
            }
            if (live) {
                if (index_bad && (unsigned long long)j < bad_index) bad_index = (unsigned long long)j;
                if (value_bad && (unsigned long long)j < bad_value) bad_value = (unsigned long long)j;
                if (wide) flags |= FLAG_WIDE;
                if (a.out_row) a.out_row[j] = ri;
                if (a.out_col) a.out_col[j] = ci;
                if (a.out_val) a.out_val[j] = f;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long oi = __shfl_down(bad_index, off), ov = __shfl_down(bad_value, off);
        bad_index = oi < bad_index ? oi : bad_index;
        bad_value = ov < bad_value ? ov : bad_value;
        flags |= __shfl_down(flags, off);
    }
    if (lane == 0) {
        if (rounded) atomicAdd(stats + ST_ROUNDED, rounded);
        if (zeros) atomicAdd(stats + ST_ZEROS, zeros);
        if (bad_index != NONE) atomicMin(stats + ST_BAD_INDEX, bad_index);
        if (bad_value != NONE) atomicMin(stats + ST_BAD_VALUE, bad_value);
        if (flags) atomicOr(stats + ST_FLAGS, (unsigned long long)flags);
    }
}

__global__ void csr_check_kernel(const void *__restrict__ indptr, int kind, int n_rows, int64_t nnz, int *__restrict__ bad)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= n_rows; i += (int64_t)gridDim.x * blockDim.x) {
        const long long p = load_index(indptr, kind, i);
        bool wrong = (i == 0 && p != 0) || (i == n_rows && p != nnz);
        if (i < n_rows) wrong = wrong || load_index(indptr, kind, i + 1) < p;
        if (wrong) atomicOr(bad, 1);
    }
}

// entry j lies in the last row r with indptr[r] <= j (rows without entries share their successor's pointer).  A search
// per entry, not a loop per row: a row may hold ten entries or a hundred thousand.  indptr has passed csr_check_kernel
__global__ void csr_expand_kernel(const void *__restrict__ indptr, int kind, int n_rows, int64_t nnz, int32_t *__restrict__ out_row)
{
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * blockDim.x) {
        int lo = 0, hi = n_rows - 1;
        while (lo < hi) {
            const int mid = (int)(((int64_t)lo + hi + 1) >> 1);
            if (load_index(indptr, kind, mid) <= j) lo = mid;
            else hi = mid - 1;
        }
        out_row[j] = lo;
    }
}

struct StoredZero {
    const void *val;
    int kind;
    __device__ bool operator()(int32_t j) const { return load_value(val, kind, j) == 0.0; }
};
__global__ void gather_pairs_kernel(int64_t n, const int32_t *__restrict__ pos, const int32_t *__restrict__ row,
                                    const int32_t *__restrict__ col, int32_t *__restrict__ out_row, int32_t *__restrict__ out_col)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        out_row[k] = row[pos[k]];
        out_col[k] = col[pos[k]];
    }
}

// the indices are in range (convert_kernel has passed); integer atomics: the counts do not depend on their order
__global__ void sample_histograms_kernel(int64_t n_samples, int64_t stride, const int32_t *__restrict__ row,
                                         const int32_t *__restrict__ col, int *__restrict__ hist_row, int *__restrict__ hist_col)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_samples; i += (int64_t)gridDim.x * blockDim.x) {
        atomicAdd(hist_row + row[i * stride], 1);
        atomicAdd(hist_col + col[i * stride], 1);
    }
}

unsigned grid_for(int64_t n, int per_block)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, 4096));
}

}  // namespace

bool csr_indptr_valid(void *stream, const void *d_indptr, int indptr_kind, int n_rows, int64_t nnz)
{
    hipStream_t st = (hipStream_t)stream;
    DevBuf bad;
    bad.alloc(sizeof(int), true, st);
    hipLaunchKernelGGL(csr_check_kernel, dim3(grid_for((int64_t)n_rows + 1, 256)), dim3(256), 0, st, d_indptr, indptr_kind,
                       n_rows, nnz, bad.as<int>());
    HIPCHK(hipGetLastError());
    int h = 0;
    d2h(&h, bad, sizeof h, st);
    return h == 0;
}

void csr_expand_rows(void *stream, const void *d_indptr, int indptr_kind, int n_rows, int64_t nnz, int32_t *d_out_row)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(csr_expand_kernel, dim3(grid_for(nnz, 256)), dim3(256), 0, (hipStream_t)stream, d_indptr, indptr_kind,
                       n_rows, nnz, d_out_row);
    HIPCHK(hipGetLastError());
}

ConvertStats convert_coo_device(void *stream, int64_t nnz, const void *d_row, int row_kind, const void *d_col, int col_kind,
                                const void *d_val, int val_kind, int n_rows, int n_cols, int32_t *d_out_row,
                                int32_t *d_out_col, float *d_out_val)
{
    ConvertStats out;
    if (nnz <= 0) return out;
    hipStream_t st = (hipStream_t)stream;
    DevBuf stats;
    stats.alloc(ST_COUNT * sizeof(unsigned long long), true, st);
    HIPCHK(hipMemsetAsync(stats.as<unsigned long long>() + ST_BAD_INDEX, 0xFF, 2 * sizeof(unsigned long long), st));   // NONE
    const ConvertArgs a{nnz, d_row, d_col, d_val, row_kind, col_kind, val_kind, n_rows, n_cols, d_out_row, d_out_col, d_out_val};
    hipLaunchKernelGGL(convert_kernel, dim3(grid_for(nnz, CV_TILE)), dim3(CV_THREADS), 0, st, a, stats.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    unsigned long long h[ST_COUNT];
    d2h(h, stats, sizeof h, st);
    out.rounded = (int64_t)h[ST_ROUNDED];
    out.zeros = (int64_t)h[ST_ZEROS];
    out.first_bad_index = h[ST_BAD_INDEX] == NONE ? -1 : (int64_t)h[ST_BAD_INDEX];
    out.first_bad_value = h[ST_BAD_VALUE] == NONE ? -1 : (int64_t)h[ST_BAD_VALUE];
    out.packed_ok = !(h[ST_FLAGS] & FLAG_WIDE);
    out.sorted[0] = !(h[ST_FLAGS] & FLAG_NOT_ROW_COL);
    out.sorted[1] = !(h[ST_FLAGS] & FLAG_NOT_COL_ROW);
    return out;
}

void compact_zeros_device(void *stream, int64_t nnz, const int32_t *d_row, const int32_t *d_col, const void *d_val,
                          int val_kind, int64_t n_zero, int32_t *d_zero_row, int32_t *d_zero_col)
{
    if (n_zero <= 0) return;
    hipStream_t st = (hipStream_t)stream;
    DevBuf pos, count, tmp;
    pos.alloc((size_t)n_zero * 4);
    count.alloc(sizeof(size_t));
    const StoredZero is_zero{d_val, val_kind};
    const rocprim::counting_iterator<int32_t> entries(0);
    size_t bytes = 0;
    HIPCHK(rocprim::select(nullptr, bytes, entries, pos.as<int32_t>(), count.as<size_t>(), (size_t)nnz, is_zero, st));
    tmp.alloc(bytes);
    HIPCHK(rocprim::select(tmp.p, bytes, entries, pos.as<int32_t>(), count.as<size_t>(), (size_t)nnz, is_zero, st));
    hipLaunchKernelGGL(gather_pairs_kernel, dim3(grid_for(n_zero, 256)), dim3(256), 0, st, n_zero, pos.as<int32_t>(), d_row,
                       d_col, d_zero_row, d_zero_col);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // the scratch dies with this scope
}

void sample_histograms_device(void *stream, int64_t nnz, const int32_t *d_row, const int32_t *d_col, int n_rows,
                              int n_cols, int64_t stride, int32_t *hist_row, int32_t *hist_col)
{
    hipStream_t st = (hipStream_t)stream;
    stride = std::max<int64_t>(1, stride);
    const int64_t n_samples = (nnz + stride - 1) / stride;
    DevBuf hist;
    hist.alloc(((size_t)n_rows + n_cols) * sizeof(int), true, st);
    int *hr = hist.as<int>(), *hc = hr + n_rows;
    if (n_samples > 0) {
        hipLaunchKernelGGL(sample_histograms_kernel, dim3(grid_for(n_samples, 256)), dim3(256), 0, st, n_samples, stride, d_row,
                           d_col, hr, hc);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(hist_row, hr, (size_t)n_rows * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hist_col, hc, (size_t)n_cols * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

}  // namespace schpf
