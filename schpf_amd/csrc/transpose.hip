// The gene-major form of a count matrix on the device (schpf_transpose[_device]): the CSC arrays of a CSR whose
// rows hold their columns in ascending order.  No comparison sort: the input's order is the output's order, so the work
// is "count, scan, place" in integers, and every entry is written once to a position that the input alone fixes: host.cpp's
// serial restatement gives the same bits, whatever the grid.
//
//   csr_indptr_kernel      indptr starts at 0, does not decrease and ends at nnz: the smallest offending row
//   csr_entries_kernel     at CSR_ORDER, a wavefront per row: every column in [0, ngenes) and above its left neighbour: the
//                          smallest offenders (both in csr_device.h).  The values are not looked at
//   transpose_count_kernel a workgroup per (window of TR_BINS columns, slab of TR_SLAB rows), as qc_gene_kernel cuts the
//                          matrix: TR_LANES lanes per row bisect the row for the window's first column and count its entries
//                          into the window's bins in LDS -- a row's columns ascend, so the lanes of a row never meet in a bin
//                          -- then one plain store per bin into table[slab][column]
//   transpose_scan_kernel  a thread per column walks the slabs: table[slab][c] becomes the entries of column c in the slabs
//                          before, count[c] their total
//   (rocPRIM exclusive scan of count: out_indptr)
//   transpose_place_kernel a workgroup per (window, slab) again; cursor[c] = out_indptr[c] + table[slab][c] in LDS.  It walks
//                          its slab in groups of TR_GROUP = 64 rows, TR_LANES lanes per row, in three steps with a barrier
//                          after each: every entry (row t of the group, column c) ORs bit t into mask[c] -- an OR commutes, so
//                          the mask is the same on every schedule; every entry goes to cursor[c] + the mask's bits below t,
//                          one plain store per output array; the entry of the lowest row in a bin (no bit below its own)
//                          moves cursor[c] on by the mask's bits and clears the mask.  Only touched bins are visited.  No
//                          floating-point operation and no atomic on global memory
#include <climits>
#include <cstdint>
#include <memory>
#include <string>

#include "common.h"
#include "csr_device.h"
#include "transpose.h"

namespace schpf {
namespace {

using namespace csr_checks;

#if defined(__HIP_DEVICE_COMPILE__)
// report_min and the checks reduce over 64 lanes.  The compiler names no wavefront size any more; the GFX9 / CDNA parts it
// builds for here run 64 lanes and nothing else
#if defined(__GFX9__)
constexpr int TR_WAVE = 64;
#else
constexpr int TR_WAVE = 32;
#endif
static_assert(TR_WAVE == 64, "the checks of csr_device.h that transpose.hip launches assume wavefronts of 64 lanes");
#endif

// the cut, open to an A/B of two builds (`make EXTRA=-DSCHPF_TR_SLAB=4096`); tests/_gene_major_reference.py names the same
#ifndef SCHPF_TR_BINS
#define SCHPF_TR_BINS 3072
#endif
#ifndef SCHPF_TR_SLAB
#define SCHPF_TR_SLAB 2048
#endif
constexpr int TR_THREADS = 1024;                  // 16 wavefronts share a window's bins
constexpr int TR_BINS = SCHPF_TR_BINS;            // W: columns per window; 8 + 4 bytes each in the placement, 36 KiB of LDS
constexpr int TR_SLAB = SCHPF_TR_SLAB;            // S: rows per slab; the table holds 4 bytes per slab and column
constexpr int TR_GROUP = 64;                      // 64 m rows per group, m = 1: one mask word per bin
constexpr int TR_LANES = TR_THREADS / TR_GROUP;   // lanes that share a row
constexpr unsigned TR_BLOCKS = 1u << 16;          // workgroups at the most; a workgroup takes every TR_BLOCKS-th task
enum { MOVE_4 = 0, MOVE_8, TO_F32 };              // what happens to a value on its way

struct Task {   // one (slab, window): rows [r0, r1), columns [w0, w1)
    int64_t slab, r0, r1;
    long long w0, w1;
};
__device__ __forceinline__ Task task_of(int64_t task, int64_t windows, int64_t ncells)
{
    const int64_t slab = task / windows, r0 = slab * TR_SLAB;
    const long long w0 = (long long)(task % windows) * TR_BINS;
    return Task{slab, r0, r0 + TR_SLAB < ncells ? r0 + TR_SLAB : ncells, w0, w0 + TR_BINS};
}

// [first, to): the entries of row r from the window's first column on
template <typename I> __device__ __forceinline__ void share_of(const Matrix &m, const I *__restrict__ indices, int64_t r, long long w0,
                                                               int64_t &first, int64_t &to)
{
    const Row row = row_of(m, r);
    to = row.from + row.len;
    first = row.from + (w0 > 0 ? lower_bound(indices + row.from, row.len, w0) : 0);
}

template <typename I>
__global__ __launch_bounds__(TR_THREADS) void transpose_count_kernel(Matrix m, int64_t windows, int64_t tasks, int32_t *__restrict__ table)
{
    __shared__ unsigned int bin[TR_BINS];
    const I *const indices = static_cast<const I *>(m.indices);
    for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {   // uniform in the workgroup
        const Task k = task_of(task, windows, m.ncells);
        for (int b = threadIdx.x; b < TR_BINS; b += TR_THREADS) bin[b] = 0;
        __syncthreads();
        for (int64_t r = k.r0 + (int)threadIdx.x / TR_LANES; r < k.r1; r += TR_GROUP) {
            int64_t first, to;
            share_of(m, indices, r, k.w0, first, to);
            for (int64_t e = first + (int)threadIdx.x % TR_LANES; e < to; e += TR_LANES) {
                const long long c = (long long)indices[e];
                if (c >= k.w1) break;   // columns ascend: the row's share of the window has ended
                atomicAdd(&bin[c - k.w0], 1u);
            }
        }
        __syncthreads();
        for (int b = threadIdx.x; b < TR_BINS && k.w0 + b < m.ngenes; b += TR_THREADS)
            table[k.slab * m.ngenes + k.w0 + b] = (int32_t)bin[b];
        __syncthreads();   // before the next task clears the bins
    }
}

// count[ngenes] = 0, the scan's last input.  A column holds fewer than 2^31 entries
__global__ __launch_bounds__(256) void transpose_scan_kernel(int32_t *__restrict__ table, int64_t slabs, int64_t ngenes,
                                                             int64_t *__restrict__ count)
{
    GRID_STRIDE(c, ngenes + 1) {
        int32_t run = 0;
        if (c < ngenes) {
#pragma unroll 8
            for (int64_t s = 0; s < slabs; ++s) {
                const int32_t here = table[s * ngenes + c];
                table[s * ngenes + c] = run;
                run += here;
            }
        }
        count[c] = run;
    }
}

template <typename I>
__global__ __launch_bounds__(TR_THREADS) void transpose_place_kernel(Matrix m, int mode, int64_t windows, int64_t tasks,
                                                                     const int32_t *__restrict__ table,
                                                                     const int64_t *__restrict__ out_indptr, int32_t *__restrict__ out_cells,
                                                                     void *__restrict__ out_values, int64_t *__restrict__ out_source)
{
    __shared__ unsigned long long mask[TR_BINS];
    __shared__ unsigned int cursor[TR_BINS];   // positions stay below nnz < 2^31
    const I *const indices = static_cast<const I *>(m.indices);
    const int t = (int)threadIdx.x / TR_LANES, lane = (int)threadIdx.x % TR_LANES;
    const unsigned long long bit = 1ull << t, below = bit - 1ull;   // t in [0, 63]: no shift by 64
    for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {   // uniform in the workgroup
        const Task k = task_of(task, windows, m.ncells);
        for (int b = threadIdx.x; b < TR_BINS; b += TR_THREADS) {
            mask[b] = 0;
            cursor[b] = k.w0 + b < m.ngenes ? (unsigned int)(out_indptr[k.w0 + b] + table[k.slab * m.ngenes + k.w0 + b]) : 0u;
        }
        __syncthreads();
        for (int64_t g = k.r0; g < k.r1; g += TR_GROUP) {   // uniform: every thread meets every barrier
            const int64_t r = g + t;
            int64_t first = 0, to = 0;
            if (r < k.r1) share_of(m, indices, r, k.w0, first, to);
            for (int64_t e = first + lane; e < to; e += TR_LANES) {
                const long long c = (long long)indices[e];
                if (c >= k.w1) break;
                atomicOr(&mask[c - k.w0], bit);
            }
            __syncthreads();
            for (int64_t e = first + lane; e < to; e += TR_LANES) {
                const long long c = (long long)indices[e];
                if (c >= k.w1) break;
                const int64_t o = (int64_t)cursor[c - k.w0] + __popcll(mask[c - k.w0] & below);   // < out_indptr[c + 1]: counted alike
                out_cells[o] = (int32_t)r;
                if (mode == MOVE_4) static_cast<uint32_t *>(out_values)[o] = static_cast<const uint32_t *>(m.val)[e];
                else if (mode == MOVE_8) static_cast<uint64_t *>(out_values)[o] = static_cast<const uint64_t *>(m.val)[e];
                else static_cast<float *>(out_values)[o] = transpose_value(load_value(m.val, m.val_kind, e));
                if (out_source) out_source[o] = e;
            }
            __syncthreads();
            for (int64_t e = first + lane; e < to; e += TR_LANES) {
                const long long c = (long long)indices[e];
                if (c >= k.w1) break;
                // the bin's lowest row alone sees a mask that is not empty and has no bit below its own; a row that reads
                // the cleared mask does nothing
                const unsigned long long seen = mask[c - k.w0];
                if (seen != 0 && (seen & below) == 0) {
                    cursor[c - k.w0] += (unsigned int)__popcll(seen);
                    mask[c - k.w0] = 0;
                }
            }
            __syncthreads();
        }
    }
}

// Everything on `st`, which is synchronised when this returns; all pointers are device memory and the matrix is not empty.
// The checks come first, indptr before anything that follows it into the entries: a refused call has written nothing
void transpose_on_device(hipStream_t st, const Matrix &m, int64_t nnz, int out_val_kind, int64_t *out_indptr, int32_t *out_cells,
                         void *out_values, int64_t *out_source)
{
    Words w;
    w.reset(st);
    launch_indptr_check(st, m, nnz, w);
    w.fetch(st);
    w.refuse_indptr("transpose");
    launch_entries_check<CSR_ORDER>(st, m, w);
    w.fetch(st);
    w.refuse_entries("transpose");

    const int64_t slabs = (m.ncells + TR_SLAB - 1) / TR_SLAB, windows = (m.ngenes + TR_BINS - 1) / TR_BINS, tasks = slabs * windows;
    DevBuf table, count;
    Scratch temp;
    table.alloc((size_t)slabs * (size_t)m.ngenes * sizeof(int32_t));
    count.alloc((size_t)(m.ngenes + 1) * sizeof(int64_t));
    const dim3 grid((unsigned)std::min<int64_t>(tasks, TR_BLOCKS));
    const bool wide = m.idx_kind == SCHPF_IDX_I64;
    hipLaunchKernelGGL(wide ? transpose_count_kernel<long long> : transpose_count_kernel<int>, grid, dim3(TR_THREADS), 0, st, m,
                       windows, tasks, table.as<int32_t>());
    HIPCHK(hipGetLastError());
    LAUNCH(transpose_scan_kernel, m.ngenes + 1, st, table.as<int32_t>(), slabs, m.ngenes, count.as<int64_t>());
    exclusive_scan(st, temp, count.as<int64_t>(), out_indptr, (size_t)(m.ngenes + 1));
    const int mode = out_val_kind != m.val_kind ? TO_F32 : value_size(m.val_kind) == 4 ? MOVE_4 : MOVE_8;
    hipLaunchKernelGGL(wide ? transpose_place_kernel<long long> : transpose_place_kernel<int>, grid, dim3(TR_THREADS), 0, st, m,
                       mode, windows, tasks, table.as<int32_t>(), out_indptr, out_cells, out_values, out_source);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_transpose_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr,
                           int indptr_kind, const void *indices, int idx_kind, const void *val, int val_kind, int out_val_kind,
                           int64_t *out_indptr, int32_t *out_cells, void *out_values, int64_t *out_source)
{
    if (const char *why = transpose_bad_args(ncells, ngenes, nnz, indptr, indptr_kind, indices, idx_kind, val, val_kind, out_val_kind,
                                             out_indptr, out_cells, out_values))
        return fail("%s", why);
    return guarded([&] {
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        if (transpose_empty(ncells, ngenes, nnz)) {   // the matrix is not read
            HIPCHK(hipMemsetAsync(out_indptr, 0, (size_t)(ngenes + 1) * sizeof(int64_t), st));
            HIPCHK(hipStreamSynchronize(st));
            return;
        }
        const Matrix m{ncells, ngenes, indptr, indices, val, indptr_kind, idx_kind, val_kind};
        transpose_on_device(st, m, nnz, out_val_kind, out_indptr, out_cells, out_values, out_source);
    });
}

int schpf_transpose(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                    const void *val, int val_kind, int out_val_kind, int64_t *out_indptr, int32_t *out_cells, void *out_values,
                    int64_t *out_source)
{
    if (const char *why = transpose_bad_args(ncells, ngenes, nnz, indptr, SCHPF_IDX_I64, indices, SCHPF_IDX_I32, val, val_kind,
                                             out_val_kind, out_indptr, out_cells, out_values))
        return fail("%s", why);
    return guarded([&] {
        use_device(device);
        const size_t J = (size_t)ngenes, n = (size_t)nnz, width = value_size(out_val_kind);
        if (transpose_empty(ncells, ngenes, nnz)) {
            std::fill(out_indptr, out_indptr + J + 1, (int64_t)0);
            return;
        }
        TempStream ts;
        DevBuf d_indptr, d_indices, d_val, d_out_indptr, d_cells, d_values, d_source;
        h2d<int64_t>(d_indptr, indptr, (size_t)ncells + 1, ts.st);
        h2d<int32_t>(d_indices, indices, n, ts.st);
        h2d<char>(d_val, val, n * value_size(val_kind), ts.st);
        d_out_indptr.alloc((J + 1) * sizeof(int64_t));
        d_cells.alloc(n * sizeof(int32_t));
        d_values.alloc(n * width);
        if (out_source) d_source.alloc(n * sizeof(int64_t));
        const Matrix m{ncells, ngenes, d_indptr.p, d_indices.p, d_val.p, SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind};
        transpose_on_device(ts.st, m, nnz, out_val_kind, d_out_indptr.as<int64_t>(), d_cells.as<int32_t>(), d_values.p,
                            out_source ? d_source.as<int64_t>() : nullptr);
        HIPCHK(hipMemcpyAsync(out_cells, d_cells.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ts.st));
        HIPCHK(hipMemcpyAsync(out_values, d_values.p, n * width, hipMemcpyDeviceToHost, ts.st));
        if (out_source) HIPCHK(hipMemcpyAsync(out_source, d_source.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        d2h(out_indptr, d_out_indptr, (J + 1) * sizeof(int64_t), ts.st);
    });
}

}  // extern "C"
