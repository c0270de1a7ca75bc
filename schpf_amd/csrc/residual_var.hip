// Pearson residual variance per gene under a negative-binomial null (schpf_residual_var / schpf_residual_var_device; DESIGN.md
// 26): S1_g and S2_g, the sums of the clipped residuals r_cg and of their squares over ALL cells of gene g, zeros included.
// The definition is in include/schpf_hip.h.  The residual of a zero entry, z(mu) = -min(clip, sqrt(mu / (1 + mu inv_theta))),
// depends on the cell only through its total n_c, so the sums split into a pass over genes x DISTINCT totals and a
// correction r - z, r^2 - z^2 over the stored entries with x > 0.
//
//   (graph_device.h: the check of indptr and the gene of every entry)
//   hvg_check_kernel         one thread per entry: cell id in range and above its left neighbour, value an integer count in
//                            [0, 2^24]; adds the count to its cell's total -- an integer atomic: exact, any order -- in a
//                            buffer of the call's own, which a refusal throws away
//   hvg_gene_totals_kernel   a workgroup per gene: s_g, and T += s_g (integer atomic)
//   (rocPRIM radix sort of the cell totals and a run-length encode: the distinct totals u_k ascending with their
//   multiplicities m_k, k < U)
//   hvg_runs_kernel          (double)u_k and (double)m_k
//   hvg_dense_kernel         a workgroup owns a strip of 16 genes, a wavefront 4 of them; lane l walks k = l, l + 64, ... with
//                            its 8 partial sums in registers: per (k, gene) mu = u_k q_g, z^2 = mu rcp(1 + mu inv_theta), one
//                            square root, the clip, two fmas weighted by m_k.  The 64 lanes of a gene are summed through the
//                            LDS in lane order by one thread, which writes sum[g], sumsq[g]: no atomics, no partial sums in
//                            HBM.  Only the multiset of the totals enters: renumbering the cells does not change a bit
//   hvg_sparse_kernel        a workgroup per gene: the gene's segment is cut into pieces of 4096 entries, a wavefront per
//                            piece, lane l takes the piece's entries l, l + 64, ... in order, then a fixed shuffle tree; the
//                            pieces' sums are added in piece order by one thread, which adds the result to sum[g], sumsq[g].
//                            A term's place is fixed by its position in the segment alone: the grid has no say in the bits.
//                            The cell order within a gene does have: this part is not invariant under renumbering
// No floating-point atomics anywhere.  fast_rcp (special.h) wants a normal argument with a normal reciprocal: 1 + mu
// inv_theta is in [1, inf) and mu <= 2^55, so up to inv_theta = 2^900 (residual_var.h) it is; above, the kernels divide.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

#include "graph_device.h"
#include "residual_var.h"
#include "special.h"

namespace schpf {
namespace {

constexpr int GENES_PER_THREAD = 4;                 // hvg_dense_kernel: genes a lane carries
constexpr int STRIP = 4 * GENES_PER_THREAD;         // genes of a workgroup: 4 wavefronts
constexpr int PIECE = 4096;                         // hvg_sparse_kernel: entries of a piece, 64 per lane

enum { H_BAD_CELLS = 0, H_BAD_VALUES, H_COUNT };
typedef Offenders<H_COUNT> HvgWords;

// |z(mu)|: the size of a zero entry's residual
template <bool FAST> __device__ __forceinline__ double zero_residual(double mu, double inv_theta, double clip)
{
    const double d = fma(mu, inv_theta, 1.0);
    const double z2 = FAST ? mu * fast_rcp(d) : mu / d;
    return fmin(sqrt(z2), clip);
}

__global__ __launch_bounds__(256) void hvg_check_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                        const float *__restrict__ data, const int32_t *__restrict__ geneof,
                                                        int64_t ncells, int64_t nnz, sum_t *__restrict__ cell_total,
                                                        unsigned long long *__restrict__ words)
{
    unsigned long long bad_cell = NONE, bad_val = NONE;
    GRID_STRIDE(e, nnz)
    {
        const int gene = geneof[e], cell = indices[e];
        const bool inside = cell >= 0 && cell < ncells;
        if (!inside || (e > indptr[gene] && indices[e - 1] >= cell)) offends(bad_cell, gene);
        int64_t x;
        const bool counted = hvg_count(data[e], x);
        if (!counted) offends(bad_val, gene);
        if (inside && counted && x > 0) atomicAdd(&cell_total[cell], (sum_t)x);
    }
    report_min(words + H_BAD_CELLS, bad_cell);
    report_min(words + H_BAD_VALUES, bad_val);
}

// the values have been checked; *total is 0 on entry
__global__ __launch_bounds__(256) void hvg_gene_totals_kernel(const int64_t *__restrict__ indptr, const float *__restrict__ data,
                                                              int64_t ngenes, int64_t *__restrict__ gene_total,
                                                              sum_t *__restrict__ total)
{
    __shared__ long long part[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t g = blockIdx.x; g < ngenes; g += gridDim.x) {
        const int64_t from = indptr[g], to = indptr[g + 1];
        long long s = 0;
        for (int64_t e = from + threadIdx.x; e < to; e += 256) {
            int64_t x;
            hvg_count(data[e], x);
            s += x;
        }
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
        if (lane == 0) part[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            s = part[0] + part[1] + part[2] + part[3];
            gene_total[g] = s;
            if (s) atomicAdd(total, (sum_t)s);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void hvg_runs_kernel(const uint64_t *__restrict__ value, const uint32_t *__restrict__ count,
                                                       const count_t *__restrict__ n_runs, int64_t bound, double *__restrict__ u,
                                                       double *__restrict__ m)
{
    const int64_t runs = (int64_t)*n_runs;
    GRID_STRIDE(k, bound)
    {
        if (k < runs) {
            u[k] = (double)(int64_t)value[k];
            m[k] = (double)count[k];
        }
    }
}

template <bool FAST>
__global__ __launch_bounds__(256) void hvg_dense_kernel(const double *__restrict__ u, const double *__restrict__ m,
                                                        const count_t *__restrict__ n_runs, const int64_t *__restrict__ gene_total,
                                                        const int64_t *__restrict__ total, int64_t ngenes, double inv_theta,
                                                        double clip, double *__restrict__ sum, double *__restrict__ sumsq)
{
    __shared__ double part1[STRIP][65], part2[STRIP][65];   // 65: the thread that sums a gene's row reads across the banks
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t U = (int64_t)*n_runs, T = *total;
    const int64_t strips = (ngenes + STRIP - 1) / STRIP;
    for (int64_t strip = blockIdx.x; strip < strips; strip += gridDim.x) {
        const int64_t g0 = strip * STRIP + wave * GENES_PER_THREAD;
        double q[GENES_PER_THREAD], s1[GENES_PER_THREAD], s2[GENES_PER_THREAD];
#pragma unroll
        for (int i = 0; i < GENES_PER_THREAD; ++i) {
            q[i] = g0 + i < ngenes ? hvg_share(gene_total[g0 + i], T) : 0.0;
            s1[i] = s2[i] = 0.0;
        }
        for (int64_t k = lane; k < U; k += 64) {
            const double uk = u[k], mk = m[k];
#pragma unroll
            for (int i = 0; i < GENES_PER_THREAD; ++i) {
                const double z = zero_residual<FAST>(uk * q[i], inv_theta, clip);
                s1[i] = fma(mk, z, s1[i]);
                s2[i] = fma(mk, z * z, s2[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < GENES_PER_THREAD; ++i) {
            part1[wave * GENES_PER_THREAD + i][lane] = s1[i];
            part2[wave * GENES_PER_THREAD + i][lane] = s2[i];
        }
        __syncthreads();
        const int64_t g = strip * STRIP + threadIdx.x;
        if (threadIdx.x < STRIP && g < ngenes) {
            double a = 0.0, b = 0.0;
            for (int l = 0; l < 64; ++l) {
                a += part1[threadIdx.x][l];
                b += part2[threadIdx.x][l];
            }
            sum[g] = 0.0 - a;   // z = -|z|
            sumsq[g] = b;
        }
        __syncthreads();   // before the next strip's partial sums
    }
}

// sum and sumsq hold the dense part; the cell ids and the values have been checked
template <bool FAST>
__global__ __launch_bounds__(256) void hvg_sparse_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                         const float *__restrict__ data, const int64_t *__restrict__ cell_total,
                                                         const int64_t *__restrict__ gene_total, const int64_t *__restrict__ total,
                                                         int64_t ngenes, double inv_theta, double clip, double *__restrict__ sum,
                                                         double *__restrict__ sumsq)
{
    __shared__ double piece1[4], piece2[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t T = *total;
    for (int64_t g = blockIdx.x; g < ngenes; g += gridDim.x) {
        const int64_t from = indptr[g], len = indptr[g + 1] - from;
        if (len == 0) continue;   // the whole workgroup
        const double q = hvg_share(gene_total[g], T);
        double t1 = 0.0, t2 = 0.0;   // thread 0: the pieces so far, in piece order
        for (int64_t base = 0; base < len; base += 4 * PIECE) {
            const int64_t first = base + (int64_t)wave * PIECE, last = first + PIECE < len ? first + PIECE : len;
            double a1 = 0.0, a2 = 0.0;
            for (int64_t p = first + lane; p < last; p += 64) {
                const double x = (double)data[from + p];
                if (x > 0.0) {
                    const double mu = (double)cell_total[indices[from + p]] * q;   // > 0: the cell and the gene hold x
                    const double z = zero_residual<FAST>(mu, inv_theta, clip);
                    double r = (x - mu) / sqrt(mu * fma(mu, inv_theta, 1.0));
                    r = fmin(fmax(r, -clip), clip);
                    a1 += r + z;
                    a2 += r * r - z * z;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                a1 += __shfl_down(a1, off);
                a2 += __shfl_down(a2, off);
            }
            if (lane == 0) {
                piece1[wave] = a1;
                piece2[wave] = a2;
            }
            __syncthreads();
            if (threadIdx.x == 0)
                for (int w = 0; w < 4 && base + (int64_t)w * PIECE < len; ++w) {
                    t1 += piece1[w];
                    t2 += piece2[w];
                }
            __syncthreads();   // before the next four pieces
        }
        if (threadIdx.x == 0) {
            sum[g] += t1;
            sumsq[g] += t2;
        }
    }
}

template <bool FAST>
void hvg_passes(hipStream_t st, int64_t J, const int64_t *indptr, const int32_t *indices, const float *data, const double *u,
                const double *m, const count_t *n_runs, const int64_t *cell_total, const int64_t *gene_total, const int64_t *total,
                double inv_theta, double clip, double *sum, double *sumsq)
{
    hipLaunchKernelGGL(hvg_dense_kernel<FAST>, dim3(grid_for(J, STRIP)), dim3(256), 0, st, u, m, n_runs, gene_total, total, J,
                       inv_theta, clip, sum, sumsq);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hvg_sparse_kernel<FAST>, dim3(grid_for(J, 1)), dim3(256), 0, st, indptr, indices, data, cell_total,
                       gene_total, total, J, inv_theta, clip, sum, sumsq);
    HIPCHK(hipGetLastError());
}

// indptr[J] == nnz and 0 at gene 0, non-decreasing -- or the refusal
void check_indptr(hipStream_t st, int64_t J, int64_t nnz, const int64_t *indptr)
{
    const int64_t last = indptr_on_device(st, (int)J, indptr, hvg_bad_indptr);
    if (last != nnz) throw std::invalid_argument(hvg_bad_indptr(J - 1));
}

// Everything on `st`, which is synchronised when this returns; all pointers are device memory, indptr has been checked, J
// is at least 1, and so is N unless there are entries, which are then refused.  The outputs are written after the last check: a refused call leaves them alone
void residual_var_on_device(hipStream_t st, int64_t N, int64_t J, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                            const float *data, double inv_theta, double clip, double *sum, double *sumsq, int64_t *cell_total,
                            int64_t *gene_total)
{
    HvgWords w;
    w.reset(st);
    DevBuf geneof, ctot, gtot, scalars;
    ctot.alloc((size_t)N * sizeof(int64_t), true, st);
    scalars.alloc(2 * sizeof(int64_t), true, st);
    int64_t *const total = scalars.as<int64_t>();
    count_t *const n_runs = scalars.as<count_t>() + 1;
    if (nnz > 0) {
        geneof.alloc((size_t)nnz * sizeof(int32_t));
        LAUNCH(entry_rows_kernel, nnz, st, indptr, J, nnz, geneof.as<int32_t>());
        LAUNCH(hvg_check_kernel, nnz, st, indptr, indices, data, geneof.as<int32_t>(), N, nnz, ctot.as<sum_t>(), w.dev());
    }
    w.fetch(st);
    w.refuse(H_BAD_CELLS, hvg_bad_cells);
    w.refuse(H_BAD_VALUES, hvg_bad_values);
    geneof.release();

    gtot.alloc((size_t)J * sizeof(int64_t));
    hipLaunchKernelGGL(hvg_gene_totals_kernel, dim3(grid_for(J, 1)), dim3(256), 0, st, indptr, data, J, gtot.as<int64_t>(),
                       (sum_t *)total);
    HIPCHK(hipGetLastError());

    // the distinct totals and how many cells have each
    Scratch temp;
    DevBuf sorted, value, count, u, m;
    sorted.alloc((size_t)N * sizeof(uint64_t));
    value.alloc((size_t)N * sizeof(uint64_t));
    count.alloc((size_t)N * sizeof(uint32_t));
    u.alloc((size_t)N * sizeof(double));
    m.alloc((size_t)N * sizeof(double));
    const int bits = std::min(64, bits_of((uint64_t)J << 24));   // a cell's total is at most J 2^24
    temp.run([&](void *t, size_t &b) {
        return rocprim::radix_sort_keys(t, b, ctot.as<uint64_t>(), sorted.as<uint64_t>(), (size_t)N, 0, bits, st);
    });
    temp.run([&](void *t, size_t &b) {
        return rocprim::run_length_encode(t, b, sorted.as<uint64_t>(), (size_t)N, value.as<uint64_t>(), count.as<uint32_t>(), n_runs,
                                          st);
    });
    LAUNCH(hvg_runs_kernel, N, st, value.as<uint64_t>(), count.as<uint32_t>(), n_runs, N, u.as<double>(), m.as<double>());

    if (inv_theta <= HVG_FAST_INV_THETA)
        hvg_passes<true>(st, J, indptr, indices, data, u.as<double>(), m.as<double>(), n_runs, ctot.as<int64_t>(), gtot.as<int64_t>(),
                         total, inv_theta, clip, sum, sumsq);
    else
        hvg_passes<false>(st, J, indptr, indices, data, u.as<double>(), m.as<double>(), n_runs, ctot.as<int64_t>(), gtot.as<int64_t>(),
                          total, inv_theta, clip, sum, sumsq);
    if (cell_total) HIPCHK(hipMemcpyAsync(cell_total, ctot.p, (size_t)N * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    if (gene_total) HIPCHK(hipMemcpyAsync(gene_total, gtot.p, (size_t)J * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_residual_var_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr,
                              const int32_t *indices, const float *data, double inv_theta, double clip, double *sum, double *sumsq,
                              int64_t *cell_total, int64_t *gene_total)
{
    if (const char *why = hvg_bad_args(ncells, ngenes, nnz, indptr, indices, data, inv_theta, clip, sum, sumsq)) return fail("%s", why);
    return guarded([&] {
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        const size_t N = (size_t)ncells, J = (size_t)ngenes;
        if (ngenes == 0 && nnz != 0) throw std::invalid_argument(hvg_bad_indptr(0));
        if (ngenes > 0) check_indptr(st, ngenes, nnz, indptr);
        if (ngenes == 0 || (ncells == 0 && nnz == 0)) {   // entries without cells: their refusal is the check's below
            if (J) HIPCHK(hipMemsetAsync(sum, 0, J * sizeof(double), st));
            if (J) HIPCHK(hipMemsetAsync(sumsq, 0, J * sizeof(double), st));
            if (cell_total && N) HIPCHK(hipMemsetAsync(cell_total, 0, N * sizeof(int64_t), st));
            if (gene_total && J) HIPCHK(hipMemsetAsync(gene_total, 0, J * sizeof(int64_t), st));
            HIPCHK(hipStreamSynchronize(st));
            return;
        }
        residual_var_on_device(st, ncells, ngenes, nnz, indptr, indices, data, inv_theta, clip, sum, sumsq, cell_total, gene_total);
    });
}

int schpf_residual_var(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                       const float *data, double inv_theta, double clip, double *sum, double *sumsq, int64_t *cell_total,
                       int64_t *gene_total)
{
    if (const char *why = hvg_bad_args(ncells, ngenes, nnz, indptr, indices, data, inv_theta, clip, sum, sumsq)) return fail("%s", why);
    return guarded([&] {
        use_device(device);
        TempStream ts;
        const size_t N = (size_t)ncells, J = (size_t)ngenes;
        DevBuf d_indptr, d_indices, d_data, d_sum, d_sumsq, d_ctot, d_gtot;
        if (ngenes == 0 && nnz != 0) throw std::invalid_argument(hvg_bad_indptr(0));
        if (ngenes > 0) {
            h2d<int64_t>(d_indptr, indptr, J + 1, ts.st);
            check_indptr(ts.st, ngenes, nnz, d_indptr.as<int64_t>());
        }
        if (ngenes == 0 || (ncells == 0 && nnz == 0)) {   // nothing more to stage
            std::fill(sum, sum + J, 0.0);
            std::fill(sumsq, sumsq + J, 0.0);
            if (cell_total) std::fill(cell_total, cell_total + N, (int64_t)0);
            if (gene_total) std::fill(gene_total, gene_total + J, (int64_t)0);
            return;
        }
        h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
        h2d<float>(d_data, data, (size_t)nnz, ts.st);
        d_sum.alloc(J * sizeof(double));
        d_sumsq.alloc(J * sizeof(double));
        d_ctot.alloc(N * sizeof(int64_t));
        d_gtot.alloc(J * sizeof(int64_t));
        residual_var_on_device(ts.st, ncells, ngenes, nnz, d_indptr.as<int64_t>(), d_indices.as<int32_t>(), d_data.as<float>(),
                               inv_theta, clip, d_sum.as<double>(), d_sumsq.as<double>(), d_ctot.as<int64_t>(), d_gtot.as<int64_t>());
        HIPCHK(hipMemcpyAsync(sum, d_sum.p, J * sizeof(double), hipMemcpyDeviceToHost, ts.st));
        HIPCHK(hipMemcpyAsync(sumsq, d_sumsq.p, J * sizeof(double), hipMemcpyDeviceToHost, ts.st));
        if (cell_total) HIPCHK(hipMemcpyAsync(cell_total, d_ctot.p, N * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        if (gene_total) HIPCHK(hipMemcpyAsync(gene_total, d_gtot.p, J * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        HIPCHK(hipStreamSynchronize(ts.st));
    });
}

}  // extern "C"
