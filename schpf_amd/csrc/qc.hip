// Cell and gene filtering on the device (schpf_axis_stats[_device], schpf_submatrix[_device]): the sums a
// quality filter asks of a count matrix, per cell and per gene, and X[rows][:, kept genes] as a CSR.  Integer arithmetic
// only; the sums are integer adds, which commute, and every entry of a submatrix is written by exactly one lane: host.cpp's
// serial restatement gives the same bits, whatever the grid.
//
//   csr_indptr_kernel      indptr starts at 0, does not decrease and ends at nnz: the smallest offending row
//   csr_entries_kernel     a wavefront per row: every column in [0, ngenes); for the statistics also above its left
//                          neighbour, every value a count thinning accepts, and the largest value: the smallest offenders
//                          (both in csr_device.h, shared with group_stats.hip, as is the bisection of a row)
//   qc_cell_kernel         a wavefront per row: the entries > 0, their sum, and per gene set the sum of the entries whose
//                          gene carries the set's bit.  gene_flags is gathered through the cache.  A piece of 64 entries sums
//                          to at most 2^30, so a set's piece is reduced in 32 bits, and only where a lane carries the bit;
//                          lane s keeps the sum of set s.  One writer per output, no atomics
//   qc_gene_kernel         a workgroup per (window of QC_BINS columns, slab of rows): 64 or 16 lanes per row bisect the row
//                          for the window's first column and add its entries to the window's bins in LDS -- a row's columns
//                          ascend, so the lanes of a row never meet in a bin -- then one global integer atomic per
//                          statistic and bin that is not empty
//   qc_rows_kernel         one row number per thread: in [0, ncells)
//   qc_keep_kernel         gene_keep as 0 / 1 in int32, one more 0 behind it (rocPRIM exclusive scan: the new column numbers,
//                          and the kept genes in the last place)
//   qc_length_kernel       a wavefront per output row counts the kept entries of its input row: ballot and popcount.
//                          Without a mask qc_span_kernel, a thread per output row from indptr
//   (rocPRIM exclusive scan of the lengths: out_indptr)
//   qc_fill_kernel         a wavefront per output row walks the input row in pieces of 64 entries; a kept entry goes to the
//                          row's start + the kept entries of the earlier pieces + those below its lane in the ballot.  The
//                          compaction is stable.  Values move as 4 or 8 bytes, whatever they mean
#include <climits>
#include <cstdint>
#include <memory>
#include <string>

#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "csr_device.h"
#include "qc.h"

namespace schpf {
namespace {

using namespace csr_checks;

constexpr int QC_THREADS = CSR_THREADS;
constexpr int QC_GENE_THREADS = 1024;   // 16 wavefronts share a window's bins
constexpr int QC_BINS = 3072;           // columns per window: 4 + 8 + 8 bytes each, 60 KiB of LDS, two workgroups per CU
constexpr int QC_GENE_BLOCKS = 2048;    // workgroups of the gene side, where the matrix has the rows for them
constexpr int QC_NARROW_BELOW = 32;     // entries of a row per window below which 16 lanes share a row, not 64

__global__ __launch_bounds__(QC_THREADS) void qc_rows_kernel(const int32_t *__restrict__ rows, int64_t n_rows, int64_t ncells,
                                                             unsigned long long *__restrict__ words)
{
    unsigned long long bad = NONE;
    for (int64_t s = blockIdx.x * (int64_t)QC_THREADS + threadIdx.x; s < n_rows; s += (int64_t)gridDim.x * QC_THREADS) {
        const int64_t r = rows[s];
        if (r < 0 || r >= ncells) offends(bad, s);
    }
    report_min(words + W_BAD_ROW, bad);
}

__device__ __forceinline__ unsigned int wave_sum32(unsigned int v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The matrix has passed qc_entries_kernel<true>: columns in [0, ngenes), values integers in [0, 2^24]
__global__ __launch_bounds__(QC_THREADS) void qc_cell_kernel(Matrix m, int n_sets, const uint32_t *__restrict__ gene_flags,
                                                             int64_t *__restrict__ cell_n, int64_t *__restrict__ cell_total,
                                                             int64_t *__restrict__ cell_set_total)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (QC_THREADS / 64);
    for (int64_t r = blockIdx.x * (int64_t)(QC_THREADS / 64) + (threadIdx.x >> 6); r < m.ncells; r += waves) {
        const int64_t from = load_index(m.indptr, m.indptr_kind, r), to = load_index(m.indptr, m.indptr_kind, r + 1);
        unsigned long long n = 0, total = 0, mine = 0;   // mine: the sum of set `lane`
        for (int64_t base = from; base < to; base += 64) {   // wave-uniform
            const int64_t e = base + lane;
            unsigned int v = 0, flags = 0;
            if (e < to) {
                v = (unsigned int)load_value(m.val, m.val_kind, e);
                if (n_sets > 0 && v > 0) flags = gene_flags[load_index(m.indices, m.idx_kind, e)];
            }
            n += v > 0;
            total += v;
            for (int s = 0; s < n_sets; ++s) {
                const bool in = (flags >> s) & 1u;
                if (__ballot(in) == 0) continue;   // wave-uniform
                const unsigned int piece = wave_sum32(in ? v : 0u);
                if (lane == s) mine += piece;
            }
        }
        n = wave_sum64(n);
        total = wave_sum64(total);
        if (lane == 0) {
            cell_n[r] = (int64_t)n;
            cell_total[r] = (int64_t)total;
        }
        if (lane < n_sets) cell_set_total[(int64_t)lane * m.ncells + r] = (int64_t)mine;
    }
}

// blockIdx.x: the window of columns, blockIdx.y: the slab of rows_per_slab rows.  G lanes share a row -- 64 for long rows, 16
// where a row's share of a window is short, so that a wavefront keeps four rows' loads in flight -- and no lane waits for
// another: a lane stops at its first column past the window.  A bin is touched only by a column inside the window,
// whatever the order of the row
template <typename I, int G>
__global__ __launch_bounds__(QC_GENE_THREADS) void qc_gene_kernel(Matrix m, int64_t rows_per_slab, sum_t *__restrict__ gene_n,
                                                                  sum_t *__restrict__ gene_total, sum_t *__restrict__ gene_sumsq)
{
    __shared__ unsigned int bin_n[QC_BINS];
    __shared__ sum_t bin_total[QC_BINS], bin_sumsq[QC_BINS];
    for (int b = threadIdx.x; b < QC_BINS; b += QC_GENE_THREADS) {
        bin_n[b] = 0;
        bin_total[b] = 0;
        bin_sumsq[b] = 0;
    }
    __syncthreads();
    const I *const indices = static_cast<const I *>(m.indices);
    const long long w0 = (long long)blockIdx.x * QC_BINS, w1 = w0 + QC_BINS;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab, r1 = r0 + rows_per_slab < m.ncells ? r0 + rows_per_slab : m.ncells;
    for (int64_t r = r0 + (int)threadIdx.x / G; r < r1; r += QC_GENE_THREADS / G) {
        const Row row = row_of(m, r);
        const int64_t to = row.from + row.len;
        const int64_t first = row.from + (w0 > 0 ? lower_bound(indices + row.from, row.len, w0) : 0);
        for (int64_t e = first + (int)threadIdx.x % G; e < to; e += G) {
            const long long c = (long long)indices[e];
            if (c >= w1) break;   // columns ascend: the row's share of the window has ended
            if (c < w0) continue;
            const sum_t v = (sum_t)load_value(m.val, m.val_kind, e);
            if (v > 0) {
                atomicAdd(&bin_n[c - w0], 1u);
                atomicAdd(&bin_total[c - w0], v);
                atomicAdd(&bin_sumsq[c - w0], v * v);
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < QC_BINS && w0 + b < m.ngenes; b += QC_GENE_THREADS)
        if (bin_n[b]) {
            atomicAdd(&gene_n[w0 + b], (sum_t)bin_n[b]);
            atomicAdd(&gene_total[w0 + b], bin_total[b]);
            atomicAdd(&gene_sumsq[w0 + b], bin_sumsq[b]);
        }
}

__global__ __launch_bounds__(QC_THREADS) void qc_keep_kernel(const uint8_t *__restrict__ gene_keep, int64_t ngenes, int32_t *__restrict__ kept)
{
    for (int64_t j = blockIdx.x * (int64_t)QC_THREADS + threadIdx.x; j <= ngenes; j += (int64_t)gridDim.x * QC_THREADS)
        kept[j] = j < ngenes && gene_keep[j] != 0;
}

// Row s of the result is row rows[s] of the matrix, or row s where there is no list
__device__ __forceinline__ int64_t source_row(const int32_t *__restrict__ rows, int64_t s) { return rows ? (int64_t)rows[s] : s; }

// len[s] = the entries of row s of the result; len[n_rows] = 0, the scan's last input
__global__ __launch_bounds__(QC_THREADS) void qc_span_kernel(Matrix m, const int32_t *__restrict__ rows, int64_t n_rows,
                                                             int64_t *__restrict__ len)
{
    for (int64_t s = blockIdx.x * (int64_t)QC_THREADS + threadIdx.x; s <= n_rows; s += (int64_t)gridDim.x * QC_THREADS)
        len[s] = s < n_rows ? row_of(m, source_row(rows, s)).len : 0;
}

// colmap[j + 1] - colmap[j] is 1 where gene j is kept
__global__ __launch_bounds__(QC_THREADS) void qc_length_kernel(Matrix m, const int32_t *__restrict__ rows, int64_t n_rows,
                                                               const int32_t *__restrict__ colmap, int64_t *__restrict__ len)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (QC_THREADS / 64);
    for (int64_t s = blockIdx.x * (int64_t)(QC_THREADS / 64) + (threadIdx.x >> 6); s <= n_rows; s += waves) {
        int64_t kept = 0;   // wave-uniform
        if (s < n_rows) {
            const Row row = row_of(m, source_row(rows, s));
            for (int64_t base = 0; base < row.len; base += 64) {
                bool keep = false;
                if (base + lane < row.len) {
                    const long long c = load_index(m.indices, m.idx_kind, row.from + base + lane);
                    keep = colmap[c + 1] != colmap[c];
                }
                kept += __popcll(__ballot(keep));
            }
        }
        if (lane == 0) len[s] = kept;
    }
}

// V: an unsigned integer of the values' width.  colmap == nullptr: every gene is kept under its own number
template <typename V>
__global__ __launch_bounds__(QC_THREADS) void qc_fill_kernel(Matrix m, const int32_t *__restrict__ rows, int64_t n_rows,
                                                             const int32_t *__restrict__ colmap, const int64_t *__restrict__ out_indptr,
                                                             int32_t *__restrict__ out_indices, V *__restrict__ out_values)
{
    const V *const val = static_cast<const V *>(m.val);
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (QC_THREADS / 64);
    for (int64_t s = blockIdx.x * (int64_t)(QC_THREADS / 64) + (threadIdx.x >> 6); s < n_rows; s += waves) {
        const Row row = row_of(m, source_row(rows, s));
        int64_t out = out_indptr[s];   // the row's start + the kept entries of the earlier pieces: wave-uniform
        for (int64_t base = 0; base < row.len; base += 64) {
            const int64_t e = row.from + base + lane;
            bool keep = false;
            int32_t c = 0;
            V v = 0;
            if (base + lane < row.len) {
                const long long old = load_index(m.indices, m.idx_kind, e);
                v = val[e];
                c = colmap ? colmap[old] : (int32_t)old;
                keep = !colmap || colmap[old + 1] != c;
            }
            const unsigned long long mask = __ballot(keep);
            if (keep) {
                const int64_t o = out + __popcll(mask & ((1ull << lane) - 1ull));   // < out_indptr[s + 1]: the length pass counted the same
                out_indices[o] = c;
                out_values[o] = v;
            }
            out += __popcll(mask);
        }
    }
}

// Everything on `st`, which is synchronised when this returns; all pointers are device memory and nnz is at least 1.  The
// checks come first, indptr before anything that follows it into the entries: a refused call has written nothing
void stats_on_device(hipStream_t st, const Matrix &m, int64_t nnz, int n_sets, const uint32_t *gene_flags, int64_t *cell_n,
                     int64_t *cell_total, int64_t *cell_set_total, int64_t *gene_n, int64_t *gene_total, int64_t *gene_sumsq)
{
    const int per_wave = QC_THREADS / 64;
    Words w;
    w.reset(st);
    launch_indptr_check(st, m, nnz, w);
    w.fetch(st);
    w.refuse_indptr("qc");
    launch_entries_check<CSR_COUNTS>(st, m, w);
    w.fetch(st);
    w.refuse_entries("qc");
    if (qc_sumsq_overflows(w.vmax(), m.ncells)) throw std::invalid_argument(csr_bad_sumsq("qc", w.vmax(), m.ncells));

    CSR_LAUNCH(qc_cell_kernel, m.ncells, per_wave, st, m, n_sets, gene_flags, cell_n, cell_total, cell_set_total);
    for (int64_t *p : {gene_n, gene_total, gene_sumsq}) HIPCHK(hipMemsetAsync(p, 0, (size_t)m.ngenes * sizeof(int64_t), st));
    const int64_t windows = (m.ngenes + QC_BINS - 1) / QC_BINS;
    const bool narrow = nnz / m.ncells / windows < QC_NARROW_BELOW;   // the mean share of a window in a row
    const int64_t groups = QC_GENE_THREADS / (narrow ? 16 : 64);
    const int64_t slabs = std::max<int64_t>(1, std::min<int64_t>(QC_GENE_BLOCKS / windows, (m.ncells + groups - 1) / groups));
    const int64_t rows_per_slab = (m.ncells + slabs - 1) / slabs;
    const dim3 grid((unsigned)windows, (unsigned)((m.ncells + rows_per_slab - 1) / rows_per_slab));
    const bool wide = m.idx_kind == SCHPF_IDX_I64;
    const auto kernel = narrow ? (wide ? qc_gene_kernel<long long, 16> : qc_gene_kernel<int, 16>)
                               : (wide ? qc_gene_kernel<long long, 64> : qc_gene_kernel<int, 64>);
    hipLaunchKernelGGL(kernel, grid, dim3(QC_GENE_THREADS), 0, st, m, rows_per_slab, (sum_t *)gene_n, (sum_t *)gene_total,
                       (sum_t *)gene_sumsq);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
}

// As above; rows and gene_keep may be nullptr, out_ngenes is host memory.  With nnz = 0 or n_rows = 0 the matrix is not
// read.  Returns the entries of the result; out_indices == nullptr: out_ngenes and out_indptr alone are written
int64_t submatrix_on_device(hipStream_t st, const Matrix &m, int64_t nnz, int64_t n_rows, const int32_t *rows, const uint8_t *gene_keep,
                            int64_t *out_ngenes, int64_t *out_indptr, int32_t *out_indices, void *out_values, int64_t capacity)
{
    const int per_wave = QC_THREADS / 64;
    const bool empty = nnz == 0 || n_rows == 0;
    Words w;
    w.reset(st);
    if (!empty) {
        launch_indptr_check(st, m, nnz, w);
        w.fetch(st);
        w.refuse_indptr("qc");
        launch_entries_check<CSR_RANGE>(st, m, w);
    }
    if (rows && n_rows > 0) CSR_LAUNCH(qc_rows_kernel, n_rows, QC_THREADS, st, rows, n_rows, m.ncells, w.dev());
    w.fetch(st);
    w.refuse_entries("qc");
    w.refuse(W_BAD_ROW, qc_bad_rows);

    DevBuf kept, colmap, len, indptr;
    Scratch temp;
    int64_t ngenes_kept = m.ngenes, total = 0;
    if (gene_keep) {
        kept.alloc((size_t)(m.ngenes + 1) * sizeof(int32_t));
        colmap.alloc((size_t)(m.ngenes + 1) * sizeof(int32_t));
        CSR_LAUNCH(qc_keep_kernel, m.ngenes + 1, QC_THREADS, st, gene_keep, m.ngenes, kept.as<int32_t>());
        temp.run([&](void *t, size_t &b) {
            return rocprim::exclusive_scan(t, b, kept.as<int32_t>(), colmap.as<int32_t>(), (int32_t)0, (size_t)(m.ngenes + 1),
                                           rocprim::plus<int32_t>(), st);
        });
        int32_t last = 0;
        HIPCHK(hipMemcpyAsync(&last, colmap.as<int32_t>() + m.ngenes, sizeof last, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ngenes_kept = last;
    }
    const int32_t *const map = gene_keep ? colmap.as<int32_t>() : nullptr;
    if (!empty) {   // the lengths and their scan go to scratch: a capacity that is refused leaves out_indptr alone
        len.alloc((size_t)(n_rows + 1) * sizeof(int64_t));
        indptr.alloc((size_t)(n_rows + 1) * sizeof(int64_t));
        if (map) CSR_LAUNCH(qc_length_kernel, n_rows + 1, per_wave, st, m, rows, n_rows, map, len.as<int64_t>());
        else CSR_LAUNCH(qc_span_kernel, n_rows + 1, QC_THREADS, st, m, rows, n_rows, len.as<int64_t>());
        exclusive_scan(st, temp, len.as<int64_t>(), indptr.as<int64_t>(), (size_t)(n_rows + 1));
        HIPCHK(hipMemcpyAsync(&total, indptr.as<int64_t>() + n_rows, sizeof total, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (out_indices && capacity < total) throw std::invalid_argument(csr_bad_capacity(capacity, total));
    *out_ngenes = ngenes_kept;
    if (empty) HIPCHK(hipMemsetAsync(out_indptr, 0, (size_t)(n_rows + 1) * sizeof(int64_t), st));
    else HIPCHK(hipMemcpyAsync(out_indptr, indptr.p, (size_t)(n_rows + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    if (out_indices && total > 0) {
        if (value_size(m.val_kind) == 4)
            CSR_LAUNCH(qc_fill_kernel<uint32_t>, n_rows, per_wave, st, m, rows, n_rows, map, indptr.as<int64_t>(), out_indices,
                   static_cast<uint32_t *>(out_values));
        else
            CSR_LAUNCH(qc_fill_kernel<uint64_t>, n_rows, per_wave, st, m, rows, n_rows, map, indptr.as<int64_t>(), out_indices,
                   static_cast<uint64_t *>(out_values));
    }
    HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
    return total;
}

void zero_stats(hipStream_t st, int64_t ncells, int64_t ngenes, int n_sets, int64_t *cell_n, int64_t *cell_total,
                int64_t *cell_set_total, int64_t *gene_n, int64_t *gene_total, int64_t *gene_sumsq)
{
    for (int64_t *p : {cell_n, cell_total})
        if (ncells) HIPCHK(hipMemsetAsync(p, 0, (size_t)ncells * sizeof(int64_t), st));
    if (ncells && n_sets) HIPCHK(hipMemsetAsync(cell_set_total, 0, (size_t)ncells * n_sets * sizeof(int64_t), st));
    for (int64_t *p : {gene_n, gene_total, gene_sumsq})
        if (ngenes) HIPCHK(hipMemsetAsync(p, 0, (size_t)ngenes * sizeof(int64_t), st));
    HIPCHK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_axis_stats_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr,
                            int indptr_kind, const void *indices, int idx_kind, const void *val, int val_kind, int n_sets,
                            const uint32_t *gene_flags, int64_t *cell_n, int64_t *cell_total, int64_t *cell_set_total,
                            int64_t *gene_n, int64_t *gene_total, int64_t *gene_sumsq)
{
    if (const char *why = qc_stats_bad_args(ncells, ngenes, nnz, indptr, indices, val, n_sets, gene_flags, cell_n, cell_total,
                                            cell_set_total, gene_n, gene_total, gene_sumsq))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(indptr_kind, idx_kind, val_kind)) throw std::invalid_argument("unknown index or value kind");
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        if (nnz == 0) {   // every sum is empty: the matrix is not read
            zero_stats(st, ncells, ngenes, n_sets, cell_n, cell_total, cell_set_total, gene_n, gene_total, gene_sumsq);
            return;
        }
        const Matrix m{ncells, ngenes, indptr, indices, val, indptr_kind, idx_kind, val_kind};
        stats_on_device(st, m, nnz, n_sets, gene_flags, cell_n, cell_total, cell_set_total, gene_n, gene_total, gene_sumsq);
    });
}

int schpf_axis_stats(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                     const void *val, int val_kind, int n_sets, const uint32_t *gene_flags, int64_t *cell_n, int64_t *cell_total,
                     int64_t *cell_set_total, int64_t *gene_n, int64_t *gene_total, int64_t *gene_sumsq)
{
    if (const char *why = qc_stats_bad_args(ncells, ngenes, nnz, indptr, indices, val, n_sets, gene_flags, cell_n, cell_total,
                                            cell_set_total, gene_n, gene_total, gene_sumsq))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind)) throw std::invalid_argument("unknown index or value kind");
        use_device(device);
        const size_t N = (size_t)ncells, J = (size_t)ngenes, S = (size_t)n_sets;
        if (nnz == 0) {
            for (int64_t *p : {cell_n, cell_total}) std::fill(p, p + N, (int64_t)0);
            if (N && S) std::fill(cell_set_total, cell_set_total + N * S, (int64_t)0);
            for (int64_t *p : {gene_n, gene_total, gene_sumsq}) std::fill(p, p + J, (int64_t)0);
            return;
        }
        TempStream ts;
        DevBuf d_indptr, d_indices, d_val, d_flags, d_cell, d_gene;
        h2d<int64_t>(d_indptr, indptr, N + 1, ts.st);
        h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
        h2d<char>(d_val, val, (size_t)nnz * value_size(val_kind), ts.st);
        h2d<uint32_t>(d_flags, gene_flags, S ? J : 0, ts.st);
        d_cell.alloc((2 + S) * N * sizeof(int64_t));   // cell_n, cell_total, cell_set_total
        d_gene.alloc(3 * J * sizeof(int64_t));
        int64_t *const c = d_cell.as<int64_t>(), *const g = d_gene.as<int64_t>();
        const Matrix m{ncells, ngenes, d_indptr.p, d_indices.p, d_val.p, SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind};
        stats_on_device(ts.st, m, nnz, n_sets, d_flags.as<uint32_t>(), c, c + N, c + 2 * N, g, g + J, g + 2 * J);
        const auto back = [&](int64_t *dst, const int64_t *src, size_t n) {
            if (n) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        };
        back(cell_n, c, N);
        back(cell_total, c + N, N);
        back(cell_set_total, c + 2 * N, N * S);
        back(gene_n, g, J);
        back(gene_total, g + J, J);
        back(gene_sumsq, g + 2 * J, J);
        HIPCHK(hipStreamSynchronize(ts.st));
    });
}

int schpf_submatrix_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr,
                           int indptr_kind, const void *indices, int idx_kind, const void *val, int val_kind, int64_t n_rows,
                           const int32_t *rows, const uint8_t *gene_keep, int64_t *out_ngenes, int64_t *out_indptr,
                           int32_t *out_indices, void *out_values, int64_t capacity)
{
    if (const char *why = qc_submatrix_bad_args(ncells, ngenes, nnz, indptr, indices, val, n_rows, rows, out_ngenes, out_indptr,
                                                out_indices, out_values, capacity))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(indptr_kind, idx_kind, val_kind)) throw std::invalid_argument("unknown index or value kind");
        use_device(device);
        std::unique_ptr<TempStream> own;
        const Matrix m{ncells, ngenes, indptr, indices, val, indptr_kind, idx_kind, val_kind};
        submatrix_on_device(pick_stream(stream, own), m, nnz, n_rows, rows, gene_keep, out_ngenes, out_indptr, out_indices,
                            out_values, capacity);
    });
}

int schpf_submatrix(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                    const void *val, int val_kind, int64_t n_rows, const int32_t *rows, const uint8_t *gene_keep,
                    int64_t *out_ngenes, int64_t *out_indptr, int32_t *out_indices, void *out_values, int64_t capacity)
{
    if (const char *why = qc_submatrix_bad_args(ncells, ngenes, nnz, indptr, indices, val, n_rows, rows, out_ngenes, out_indptr,
                                                out_indices, out_values, capacity))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind)) throw std::invalid_argument("unknown index or value kind");
        use_device(device);
        const bool empty = nnz == 0 || n_rows == 0;
        const size_t width = value_size(val_kind);
        TempStream ts;
        DevBuf d_indptr, d_indices, d_val, d_rows, d_keep, d_out_indptr, d_out_indices, d_out_values;
        if (!empty) {
            h2d<int64_t>(d_indptr, indptr, (size_t)ncells + 1, ts.st);
            h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
            h2d<char>(d_val, val, (size_t)nnz * width, ts.st);
        }
        if (rows) h2d<int32_t>(d_rows, rows, (size_t)n_rows, ts.st);
        if (gene_keep) h2d<uint8_t>(d_keep, gene_keep, (size_t)ngenes, ts.st);
        d_out_indptr.alloc((size_t)(n_rows + 1) * sizeof(int64_t));
        if (out_indices) {
            d_out_indices.alloc((size_t)capacity * sizeof(int32_t));
            d_out_values.alloc((size_t)capacity * width);
        }
        const Matrix m{ncells, ngenes, d_indptr.p, d_indices.p, d_val.p, SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind};
        int64_t kept = 0;
        const int64_t total = submatrix_on_device(ts.st, m, nnz, n_rows, rows ? d_rows.as<int32_t>() : nullptr,
                                                  gene_keep ? d_keep.as<uint8_t>() : nullptr, &kept, d_out_indptr.as<int64_t>(),
                                                  out_indices ? d_out_indices.as<int32_t>() : nullptr,
                                                  out_indices ? d_out_values.p : nullptr, capacity);
        if (out_indices && total > 0) {
            HIPCHK(hipMemcpyAsync(out_indices, d_out_indices.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, ts.st));
            HIPCHK(hipMemcpyAsync(out_values, d_out_values.p, (size_t)total * width, hipMemcpyDeviceToHost, ts.st));
        }
        d2h(out_indptr, d_out_indptr, (size_t)(n_rows + 1) * sizeof(int64_t), ts.st);
        *out_ngenes = kept;
    });
}

}  // extern "C"
