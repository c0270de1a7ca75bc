// Pseudobulk on the device (schpf_group_stats[_device]): per group of cells and gene the cells with a count > 0,
// the sum of their counts and the sum of the squares, in exact int64.  qc_gene_kernel's sum with the cells ordered by group
// and the bins flushed per group.  Integer arithmetic only; the sums are integer adds, which commute and do not round: the
// result depends neither on the grid, nor on which workgroup's atomic lands first, nor on the order of the cells inside
// a group in `order` -- any permutation that lists the cells group after group gives the same bits, the stable one of the
// radix sort here as well as host.cpp's walk over the rows as they are stored.
//
//   csr_indptr_kernel, csr_entries_kernel   the refusals of the matrix and its largest value (csr_device.h, shared with qc.hip)
//   gs_keys_kernel         a thread per cell: the smallest label outside [-1, ngroups); the sort key of the cell -- its label,
//                          ngroups for a cell in no group, so that those end behind every group -- and the cell as the payload
//   (rocPRIM radix sort of (key, cell) over the bits ngroups occupies: `order`, the cells group after group)
//   gs_starts_kernel       a thread per group bisects the sorted keys for the group's first position and the next group's:
//                          starts[g], group_cells[g], and the slabs of GS_SLAB positions the group is cut into
//   (rocPRIM exclusive scan of the slabs per group: the first slab of every group, and their number in the last place)
//   gs_slabs_kernel        a thread per slab bisects that scan for its group: the slab table (group, first position, end).
//                          A slab lies inside one group; the last slab of a group may be short; an empty group has none
//   gs_sum_kernel          a workgroup per (window of GS_BINS columns, slab): 64 or 16 lanes per row -- the row is order[p], a
//                          gather through the cache -- bisect the row for the window's first column and add its entries to
//                          the window's bins in LDS, stop at the first column past the window; then one global integer atomic
//                          per statistic and bin that is not empty goes into row g of the outputs, and the bin is cleared for
//                          the workgroup's next slab.  No thread walks a whole group, and there is no float anywhere
//
// Scratch: 16 ncells (keys and cells, before and behind the sort) + 24 (ngroups + 1) (starts, slabs per group, their scan) +
// 12 bytes per slab (at most ncells / GS_SLAB + min(ngroups, ncells) slabs) + the sort's and the scan's own + a few words.
#include <climits>
#include <cstdint>
#include <memory>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"
#include "csr_device.h"
#include "group_stats.h"

namespace schpf {
namespace {

using namespace csr_checks;

constexpr int GS_THREADS = CSR_THREADS;
constexpr int GS_SUM_THREADS = 512;     // 8 wavefronts share a window's bins: 32 rows in flight at 16 lanes per row
constexpr int GS_BINS = 2048;           // columns per window: 4 + 8 + 8 bytes each, 40 KiB of LDS, four workgroups per CU
constexpr int GS_SLAB = 2048;           // positions of `order` per slab: a flush of <= GS_BINS bins per 2048 rows' entries
constexpr int GS_MAX_SLAB_BLOCKS = 65535;   // gridDim.y; a workgroup takes every gridDim.y-th slab
constexpr int GS_NARROW_BELOW = 32;     // entries of a row per window below which 16 lanes share a row, not 64

struct Slab {
    int32_t group, from, to;   // the positions [from, to) of `order`, all of group `group`
};

__global__ __launch_bounds__(GS_THREADS) void gs_keys_kernel(const int32_t *__restrict__ labels, int64_t ncells, int64_t ngroups,
                                                             int32_t *__restrict__ key, int32_t *__restrict__ cell,
                                                             unsigned long long *__restrict__ words)
{
    unsigned long long bad = NONE;
    for (int64_t i = blockIdx.x * (int64_t)GS_THREADS + threadIdx.x; i < ncells; i += (int64_t)gridDim.x * GS_THREADS) {
        const int64_t g = labels[i];
        if (g < -1 || g >= ngroups) offends(bad, i);
        key[i] = g >= 0 && g < ngroups ? (int32_t)g : (int32_t)ngroups;
        cell[i] = (int32_t)i;
    }
    report_min(words + W_BAD_LABEL, bad);
}

// key: the ncells sorted keys.  Thread g <= ngroups; group ngroups is the cells in no group and gets no slab
__global__ __launch_bounds__(GS_THREADS) void gs_starts_kernel(const int32_t *__restrict__ key, int64_t ncells, int64_t ngroups,
                                                               int64_t *__restrict__ starts, int64_t *__restrict__ slabs_of,
                                                               int64_t *__restrict__ group_cells)
{
    for (int64_t g = blockIdx.x * (int64_t)GS_THREADS + threadIdx.x; g <= ngroups; g += (int64_t)gridDim.x * GS_THREADS) {
        const int64_t from = lower_bound(key, ncells, g);
        starts[g] = from;
        if (g == ngroups) {
            slabs_of[g] = 0;
            continue;
        }
        const int64_t n = lower_bound(key + from, ncells - from, g + 1);
        slabs_of[g] = (n + GS_SLAB - 1) / GS_SLAB;
        group_cells[g] = n;
    }
}

// first_slab: the exclusive scan of slabs_of, ngroups + 1 long.  Slab s belongs to the last group whose first slab is <= s;
// the empty groups before it share its number and lie below it
__global__ __launch_bounds__(GS_THREADS) void gs_slabs_kernel(const int64_t *__restrict__ first_slab, const int64_t *__restrict__ starts,
                                                              int64_t ngroups, int64_t n_slabs, Slab *__restrict__ slabs)
{
    for (int64_t s = blockIdx.x * (int64_t)GS_THREADS + threadIdx.x; s < n_slabs; s += (int64_t)gridDim.x * GS_THREADS) {
        const int64_t g = lower_bound(first_slab, ngroups + 1, s + 1) - 1;   // in [0, ngroups): first_slab[0] = 0 <= s < first_slab[ngroups]
        const int64_t from = starts[g] + (s - first_slab[g]) * GS_SLAB, end = starts[g + 1];
        slabs[s] = Slab{(int32_t)g, (int32_t)from, (int32_t)(from + GS_SLAB < end ? from + GS_SLAB : end)};
    }
}

// blockIdx.x: the window of columns; blockIdx.y, and every gridDim.y-th after it: the slab.  G lanes share a row, as in
// qc_gene_kernel: a row's columns ascend, so the lanes of a row never meet in a bin, and a bin is touched only by a column
// inside the window.  The matrix has passed csr_entries_kernel<CSR_COUNTS>: columns in [0, ngenes), values integers in [0, 2^24];
// order[p] is a cell, in [0, ncells); g * ngenes + column stays below 2^31.  SQ: the sum of squares is asked for
template <typename I, int G, bool SQ>
__global__ __launch_bounds__(GS_SUM_THREADS) void gs_sum_kernel(Matrix m, const int32_t *__restrict__ order, const Slab *__restrict__ slabs,
                                                                int64_t n_slabs, sum_t *__restrict__ nexpr, sum_t *__restrict__ total,
                                                                sum_t *__restrict__ sumsq)
{
    __shared__ unsigned int bin_n[GS_BINS];
    __shared__ sum_t bin_total[GS_BINS], bin_sumsq[SQ ? GS_BINS : 1];
    for (int b = threadIdx.x; b < GS_BINS; b += GS_SUM_THREADS) {
        bin_n[b] = 0;
        bin_total[b] = 0;
        if (SQ) bin_sumsq[b] = 0;
    }
    __syncthreads();
    const I *const indices = static_cast<const I *>(m.indices);
    const long long w0 = (long long)blockIdx.x * GS_BINS, w1 = w0 + GS_BINS;
    for (int64_t s = blockIdx.y; s < n_slabs; s += gridDim.y) {   // uniform over the workgroup
        const Slab slab = slabs[s];
        for (int64_t p = slab.from + (int)threadIdx.x / G; p < slab.to; p += GS_SUM_THREADS / G) {
            const Row row = row_of(m, order[p]);
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
                    if (SQ) atomicAdd(&bin_sumsq[c - w0], v * v);
                }
            }
        }
        __syncthreads();
        const int64_t out = (int64_t)slab.group * m.ngenes + w0;
        for (int b = threadIdx.x; b < GS_BINS && w0 + b < m.ngenes; b += GS_SUM_THREADS)
            if (bin_n[b]) {   // the thread that flushes a bin clears it: the next slab finds zeros
                atomicAdd(&nexpr[out + b], (sum_t)bin_n[b]);
                atomicAdd(&total[out + b], bin_total[b]);
                bin_n[b] = 0;
                bin_total[b] = 0;
                if (SQ) {
                    atomicAdd(&sumsq[out + b], bin_sumsq[b]);
                    bin_sumsq[b] = 0;
                }
            }
        __syncthreads();
    }
}

template <typename I, int G> void launch_sum(hipStream_t st, dim3 grid, const Matrix &m, const int32_t *order, const Slab *slabs,
                                             int64_t n_slabs, int64_t *nexpr, int64_t *total, int64_t *sumsq)
{
    const auto kernel = sumsq ? gs_sum_kernel<I, G, true> : gs_sum_kernel<I, G, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(GS_SUM_THREADS), 0, st, m, order, slabs, n_slabs, (sum_t *)nexpr, (sum_t *)total, (sum_t *)sumsq);
    HIPCHK(hipGetLastError());
}

// Everything on `st`, which is synchronised when this returns; all pointers are device memory; sumsq may be nullptr.  The
// checks come first, indptr before anything that follows it into the entries: a refused call has written nothing.  With
// nnz = 0 the matrix is not read
void group_stats_on_device(hipStream_t st, const Matrix &m, int64_t nnz, const int32_t *labels, int64_t ngroups, int64_t *group_cells,
                           int64_t *nexpr, int64_t *total, int64_t *sumsq)
{
    const int64_t N = m.ncells;
    Words w;
    w.reset(st);
    DevBuf key_a, key_b, cell_a, cell_b, starts, slabs_of, first_slab, slabs;
    Scratch temp;
    for (DevBuf *b : {&key_a, &key_b, &cell_a, &cell_b}) b->alloc((size_t)N * sizeof(int32_t));
    if (nnz > 0) {
        launch_indptr_check(st, m, nnz, w);
        w.fetch(st);
        w.refuse_indptr("group_stats");
        launch_entries_check<CSR_COUNTS>(st, m, w);
    }
    if (N > 0) CSR_LAUNCH(gs_keys_kernel, N, GS_THREADS, st, labels, N, ngroups, key_a.as<int32_t>(), cell_a.as<int32_t>(), w.dev());
    w.fetch(st);
    w.refuse_entries("group_stats");
    w.refuse(W_BAD_LABEL, group_stats_bad_labels);
    if (sumsq && qc_sumsq_overflows(w.vmax(), N)) throw std::invalid_argument(csr_bad_sumsq("group_stats", w.vmax(), N));

    if (N > 0)
        temp.run([&](void *t, size_t &b) {
            return rocprim::radix_sort_pairs(t, b, key_a.as<uint32_t>(), key_b.as<uint32_t>(), cell_a.as<int32_t>(),
                                             cell_b.as<int32_t>(), (size_t)N, 0, bits_of((uint64_t)ngroups), st);
        });
    for (DevBuf *b : {&starts, &slabs_of, &first_slab}) b->alloc((size_t)(ngroups + 1) * sizeof(int64_t));
    CSR_LAUNCH(gs_starts_kernel, ngroups + 1, GS_THREADS, st, key_b.as<int32_t>(), N, ngroups, starts.as<int64_t>(), slabs_of.as<int64_t>(),
               group_cells);
    for (int64_t *p : {nexpr, total, sumsq})
        if (p && m.ngenes > 0) HIPCHK(hipMemsetAsync(p, 0, (size_t)(ngroups * m.ngenes) * sizeof(int64_t), st));
    if (nnz == 0 || m.ngenes == 0) {
        HIPCHK(hipStreamSynchronize(st));
        return;
    }
    exclusive_scan(st, temp, slabs_of.as<int64_t>(), first_slab.as<int64_t>(), (size_t)(ngroups + 1));
    int64_t n_slabs = 0;
    HIPCHK(hipMemcpyAsync(&n_slabs, first_slab.as<int64_t>() + ngroups, sizeof n_slabs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_slabs == 0) return;   // no cell is in a group
    slabs.alloc((size_t)n_slabs * sizeof(Slab));
    CSR_LAUNCH(gs_slabs_kernel, n_slabs, GS_THREADS, st, first_slab.as<int64_t>(), starts.as<int64_t>(), ngroups, n_slabs, slabs.as<Slab>());
    const int64_t windows = (m.ngenes + GS_BINS - 1) / GS_BINS;
    const bool narrow = nnz / N / windows < GS_NARROW_BELOW;   // the mean share of a window in a row
    const dim3 grid((unsigned)windows, (unsigned)std::min<int64_t>(n_slabs, GS_MAX_SLAB_BLOCKS));
    const bool wide = m.idx_kind == SCHPF_IDX_I64;
    const auto launch = narrow ? (wide ? launch_sum<long long, 16> : launch_sum<int, 16>) : (wide ? launch_sum<long long, 64> : launch_sum<int, 64>);
    launch(st, grid, m, cell_b.as<int32_t>(), slabs.as<Slab>(), n_slabs, nexpr, total, sumsq);
    HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_group_stats_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr, int indptr_kind,
                             const void *indices, int idx_kind, const void *val, int val_kind, const int32_t *labels, int64_t ngroups,
                             int64_t *group_cells, int64_t *nexpr, int64_t *total, int64_t *sumsq)
{
    if (const char *why = group_stats_bad_args(ncells, ngenes, nnz, indptr, indices, val, labels, ngroups, group_cells, nexpr, total))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(indptr_kind, idx_kind, val_kind)) throw std::invalid_argument("unknown index or value kind");
        use_device(device);
        std::unique_ptr<TempStream> own;
        const Matrix m{ncells, ngenes, indptr, indices, val, indptr_kind, idx_kind, val_kind};
        group_stats_on_device(pick_stream(stream, own), m, nnz, labels, ngroups, group_cells, nexpr, total, sumsq);
    });
}

int schpf_group_stats(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                      const void *val, int val_kind, const int32_t *labels, int64_t ngroups, int64_t *group_cells, int64_t *nexpr,
                      int64_t *total, int64_t *sumsq)
{
    if (const char *why = group_stats_bad_args(ncells, ngenes, nnz, indptr, indices, val, labels, ngroups, group_cells, nexpr, total))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind)) throw std::invalid_argument("unknown index or value kind");
        use_device(device);
        const size_t N = (size_t)ncells, G = (size_t)ngroups, GJ = G * (size_t)ngenes;
        TempStream ts;
        DevBuf d_indptr, d_indices, d_val, d_labels, d_cells, d_out;
        if (nnz > 0) {
            h2d<int64_t>(d_indptr, indptr, N + 1, ts.st);
            h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
            h2d<char>(d_val, val, (size_t)nnz * value_size(val_kind), ts.st);
        }
        h2d<int32_t>(d_labels, labels, N, ts.st);
        d_cells.alloc(G * sizeof(int64_t));
        d_out.alloc((sumsq ? 3 : 2) * GJ * sizeof(int64_t));
        int64_t *const o = d_out.as<int64_t>();
        const Matrix m{ncells, ngenes, d_indptr.p, d_indices.p, d_val.p, SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind};
        group_stats_on_device(ts.st, m, nnz, d_labels.as<int32_t>(), ngroups, d_cells.as<int64_t>(), o, o + GJ, sumsq ? o + 2 * GJ : nullptr);
        const auto back = [&](int64_t *dst, const int64_t *src, size_t n) {
            if (n) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        };
        back(group_cells, d_cells.as<int64_t>(), G);
        back(nexpr, o, GJ);
        back(total, o + GJ, GJ);
        if (sumsq) back(sumsq, o + 2 * GJ, GJ);
        HIPCHK(hipStreamSynchronize(ts.st));
    });
}

}  // extern "C"
