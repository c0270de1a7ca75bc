// Wilcoxon rank sums of every gene for every group of cells (schpf_rank_sums / schpf_rank_sums_device).  With
// average ranks, twice a rank is an integer, so every output is an integer sum -- exact in any order.  The definition is in
// include/schpf_hip.h; host.cpp's serial restatement gives the same bits.
//
//   (graph_device.h, rank_sums_device.h: the checks of indptr, the cell ids, the values and the labels, each leaving its
//   smallest offender in a word of the call's record; the gene of every entry; n[g])
//   rank_sums_keys_kernel        per entry the key (gene << 32) | float bits -- non-negative floats order as their bits; a
//                                stored zero, -0.0 included, gets the bits 0 -- and the label of its cell as the payload
//   (rocPRIM radix sort over the occupied bits: a gene's entries stay in indptr[j] .. indptr[j + 1], ascending in value)
//   rank_sums_edges_kernel       per sorted entry p: p where a run of equal keys starts, else 0; p + 1 where one ends, else
//                                UINT32_MAX, stored back to front
//   (rocPRIM inclusive scans with max and with min: the start and the end of every entry's run.  The second one runs over
//   the reversed array, so it is a forward scan too)
//   rank_sums_zeros_kernel       per gene: z_j = N - entries + the stored zeros (the run of bits 0 at the gene's start),
//                                ties[j] = z_j^3 - z_j
//   rank_sums_base_kernel        per (g, j): rank2 = n_g (z_j + 1), nexpr = 0
//   rank_sums_accumulate_kernel  a workgroup per chunk of 2048 sorted entries: r2 - z_j - 1 and 1 into the LDS bin of
//                                (gene - the chunk's first gene, group), t^3 - t of a run's first entry into the LDS bin of
//                                the gene; then one global atomic add per bin that is not empty.  What falls outside the
//                                bins -- a chunk that spans many short genes -- goes to global memory directly: few entries
//                                share an address there
// The atomic adds are integer adds: the result does not depend on their order, nor on the grid.
#include <cmath>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "rank_sums_device.h"

namespace schpf {
namespace {

constexpr int CHUNK = 2048;       // sorted entries per pass of a workgroup: 8 per thread
constexpr int BINS = 2048;        // (gene, group) bins of a chunk in LDS: 24 KiB
constexpr int TIE_BINS = 256;     // gene bins of a chunk for the tie term

__global__ __launch_bounds__(256) void rank_sums_keys_kernel(const int32_t *__restrict__ geneof, const int32_t *__restrict__ indices,
                                                             const float *__restrict__ data, const int32_t *__restrict__ labels,
                                                             int64_t nnz, uint64_t *__restrict__ key, int32_t *__restrict__ lab)
{
    GRID_STRIDE(e, nnz)
    {
        const uint32_t bits = __float_as_uint(data[e]) & 0x7fffffffu;   // -0.0 is 0
        key[e] = ((uint64_t)(uint32_t)geneof[e] << 32) | (uint64_t)bits;
        lab[e] = labels[indices[e]];
    }
}

// head[p] and tail_rev[nnz - 1 - p] of the sorted keys, ready for the two scans
__global__ __launch_bounds__(256) void rank_sums_edges_kernel(const uint64_t *__restrict__ key, int64_t nnz,
                                                              uint32_t *__restrict__ head, uint32_t *__restrict__ tail_rev)
{
    GRID_STRIDE(p, nnz)
    {
        const uint64_t k = key[p];
        head[p] = (p == 0 || key[p - 1] != k) ? (uint32_t)p : 0u;
        tail_rev[nnz - 1 - p] = (p == nnz - 1 || key[p + 1] != k) ? (uint32_t)(p + 1) : UINT32_MAX;
    }
}

__global__ __launch_bounds__(256) void rank_sums_zeros_kernel(const int64_t *__restrict__ indptr, const uint64_t *__restrict__ key,
                                                              const uint32_t *__restrict__ end_rev, int64_t ncells, int64_t ngenes,
                                                              int64_t nnz, int64_t *__restrict__ zeros, int64_t *__restrict__ ties)
{
    GRID_STRIDE(j, ngenes)
    {
        const int64_t from = indptr[j], len = indptr[j + 1] - from;
        int64_t stored_zeros = 0;   // they sort to the gene's start, one run
        if (len > 0 && (uint32_t)key[from] == 0u) stored_zeros = (int64_t)end_rev[nnz - 1 - from] - from;
        const int64_t z = ncells - len + stored_zeros;
        zeros[j] = z;
        ties[j] = z * z * z - z;
    }
}

__global__ __launch_bounds__(256) void rank_sums_base_kernel(const int64_t *__restrict__ n, const int64_t *__restrict__ zeros,
                                                             int64_t ngroups, int64_t ngenes, int64_t *__restrict__ nexpr,
                                                             int64_t *__restrict__ rank2)
{
    GRID_STRIDE(x, ngroups * ngenes)
    {
        const int64_t g = x / ngenes, j = x - g * ngenes;
        nexpr[x] = 0;
        rank2[x] = n[g] * (zeros[j] + 1);
    }
}

__global__ __launch_bounds__(256) void rank_sums_accumulate_kernel(const uint64_t *__restrict__ key, const int32_t *__restrict__ lab,
                                                                   const uint32_t *__restrict__ start,
                                                                   const uint32_t *__restrict__ end_rev,
                                                                   const int64_t *__restrict__ indptr, const int64_t *__restrict__ zeros,
                                                                   int64_t ncells, int64_t ngenes, int64_t ngroups, int64_t nnz,
                                                                   sum_t *__restrict__ nexpr, sum_t *__restrict__ rank2,
                                                                   sum_t *__restrict__ ties)
{
    __shared__ sum_t bin_rank[BINS];
    __shared__ unsigned int bin_count[BINS];
    __shared__ sum_t bin_tie[TIE_BINS];
    const int64_t chunks = (nnz + CHUNK - 1) / CHUNK;
    for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        for (int b = threadIdx.x; b < BINS; b += 256) {
            bin_rank[b] = 0;
            bin_count[b] = 0;
        }
        for (int b = threadIdx.x; b < TIE_BINS; b += 256) bin_tie[b] = 0;
        __syncthreads();
        const int64_t first = chunk * CHUNK, last = first + CHUNK < nnz ? first + CHUNK : nnz;
        const int64_t j0 = (int64_t)(key[first] >> 32);   // the genes of the chunk ascend from here
        for (int64_t p = first + threadIdx.x; p < last; p += 256) {
            const uint64_t k = key[p];
            if ((uint32_t)k == 0u) continue;   // a stored zero: one of the z_j
            const int64_t j = (int64_t)(k >> 32), s = start[p], t = (int64_t)end_rev[nnz - 1 - p] - s;
            if (p == s && t > 1) {
                const sum_t cube = (sum_t)(t * t * t - t);
                if (j - j0 < TIE_BINS) atomicAdd(&bin_tie[j - j0], cube);
                else atomicAdd(&ties[j], cube);
            }
            const int64_t g = lab[p];
            if (g < 0) continue;
            const int64_t from = indptr[j], len = indptr[j + 1] - from;
            const int64_t lo = ncells - len + (s - from);   // z_j + the positive entries below: the stored zeros cancel
            const sum_t add = (sum_t)(2 * lo + t - zeros[j]);   // r2 - z_j - 1
            const int64_t slot = (j - j0) * ngroups + g;
            if (slot < BINS) {
                atomicAdd(&bin_rank[slot], add);
                atomicAdd(&bin_count[slot], 1u);
            } else {
                atomicAdd(&rank2[g * ngenes + j], add);
                atomicAdd(&nexpr[g * ngenes + j], (sum_t)1);
            }
        }
        __syncthreads();
        for (int b = threadIdx.x; b < BINS; b += 256)
            if (bin_count[b]) {   // a bin that was added to: its gene is below ngenes
                const int64_t j = j0 + b / ngroups, g = b % ngroups;
                atomicAdd(&rank2[g * ngenes + j], bin_rank[b]);
                atomicAdd(&nexpr[g * ngenes + j], (sum_t)bin_count[b]);
            }
        for (int b = threadIdx.x; b < TIE_BINS; b += 256)
            if (bin_tie[b]) atomicAdd(&ties[j0 + b], bin_tie[b]);
        __syncthreads();   // before the next chunk clears the bins
    }
}

// Everything on `st`, which is synchronised when this returns; all pointers are device memory, indptr has been checked,
// N and J are at least 1.  The outputs are written after the last check: a refused call leaves them alone
void rank_sums_on_device(hipStream_t st, int ncells, int ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                         const float *data, const int32_t *labels, int ngroups, int64_t *n, int64_t *zeros, int64_t *ties,
                         int64_t *nexpr, int64_t *rank2)
{
    const int64_t N = ncells, J = ngenes, G = ngroups;
    DevBuf geneof;
    RankWords w;
    entries_and_labels_on_device(st, ncells, ngenes, nnz, indptr, indices, data, labels, ngroups, geneof, w);

    HIPCHK(hipMemsetAsync(n, 0, (size_t)G * sizeof(int64_t), st));
    LAUNCH(rank_sums_count_kernel, N, st, labels, ncells, ngroups, (sum_t *)n);

    Scratch temp;
    DevBuf key_a, key_b, lab_a, lab_b, end_rev;
    uint32_t *const start = geneof.as<uint32_t>();   // the genes are in the keys from here on: their buffer takes the starts
    if (nnz > 0) {
        key_a.alloc((size_t)nnz * sizeof(uint64_t));
        key_b.alloc((size_t)nnz * sizeof(uint64_t));
        lab_a.alloc((size_t)nnz * sizeof(int32_t));
        lab_b.alloc((size_t)nnz * sizeof(int32_t));
        end_rev.alloc((size_t)nnz * sizeof(uint32_t));
        uint64_t *const ka = key_a.as<uint64_t>(), *const kb = key_b.as<uint64_t>();
        LAUNCH(rank_sums_keys_kernel, nnz, st, geneof.as<int32_t>(), indices, data, labels, nnz, ka, lab_a.as<int32_t>());
        const int bits = 32 + bits_of((uint64_t)(J - 1));
        temp.run([&](void *t, size_t &b) {
            return rocprim::radix_sort_pairs(t, b, ka, kb, lab_a.as<int32_t>(), lab_b.as<int32_t>(), (size_t)nnz, 0, bits, st);
        });
        // the unsorted keys are done with: their buffer holds the two flag arrays
        uint32_t *const head = key_a.as<uint32_t>(), *const tail_rev = key_a.as<uint32_t>() + nnz;
        LAUNCH(rank_sums_edges_kernel, nnz, st, kb, nnz, head, tail_rev);
        temp.run([&](void *t, size_t &b) {
            return rocprim::inclusive_scan(t, b, head, start, (size_t)nnz, rocprim::maximum<uint32_t>(), st);
        });
        temp.run([&](void *t, size_t &b) {
            return rocprim::inclusive_scan(t, b, tail_rev, end_rev.as<uint32_t>(), (size_t)nnz, rocprim::minimum<uint32_t>(), st);
        });
    }
    LAUNCH(rank_sums_zeros_kernel, J, st, indptr, key_b.as<uint64_t>(), end_rev.as<uint32_t>(), N, J, nnz, zeros, ties);
    LAUNCH(rank_sums_base_kernel, G * J, st, n, zeros, G, J, nexpr, rank2);
    if (nnz > 0) {
        const int64_t chunks = (nnz + CHUNK - 1) / CHUNK;
        hipLaunchKernelGGL(rank_sums_accumulate_kernel, dim3((unsigned)std::min<int64_t>(chunks, 1 << 20)), dim3(256), 0, st,
                           key_b.as<uint64_t>(), lab_b.as<int32_t>(), start, end_rev.as<uint32_t>(), indptr, zeros, N, J, G, nnz,
                           (sum_t *)nexpr, (sum_t *)rank2, (sum_t *)ties);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_rank_sums_device(int device, void *stream, int ncells, int ngenes, const int64_t *indptr, const int32_t *indices,
                           const float *data, const int32_t *labels, int ngroups, int64_t *n, int64_t *zeros, int64_t *ties,
                           int64_t *nexpr, int64_t *rank2)
{
    if (const char *why = rank_sums_bad_args(ncells, ngenes, ngroups, indptr, labels, n, zeros, ties, nexpr, rank2))
        return fail("%s", why);
    return guarded([&] {
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        if (ncells == 0 || ngenes == 0) {
            const size_t G = (size_t)ngroups, J = (size_t)ngenes;
            if (n) HIPCHK(hipMemsetAsync(n, 0, G * sizeof(int64_t), st));
            if (zeros && J) HIPCHK(hipMemsetAsync(zeros, 0, J * sizeof(int64_t), st));
            if (ties && J) HIPCHK(hipMemsetAsync(ties, 0, J * sizeof(int64_t), st));
            if (nexpr && J) HIPCHK(hipMemsetAsync(nexpr, 0, G * J * sizeof(int64_t), st));
            if (rank2 && J) HIPCHK(hipMemsetAsync(rank2, 0, G * J * sizeof(int64_t), st));
            HIPCHK(hipStreamSynchronize(st));
            return;
        }
        const int64_t nnz = indptr_on_device(st, ngenes, indptr, rank_sums_bad_indptr);
        if (const char *why = rank_sums_bad_nnz(nnz, indices, data)) throw std::invalid_argument(why);
        rank_sums_on_device(st, ncells, ngenes, nnz, indptr, indices, data, labels, ngroups, n, zeros, ties, nexpr, rank2);
    });
}

int schpf_rank_sums(int device, int ncells, int ngenes, const int64_t *indptr, const int32_t *indices, const float *data,
                    const int32_t *labels, int ngroups, int64_t *n, int64_t *zeros, int64_t *ties, int64_t *nexpr,
                    int64_t *rank2)
{
    if (const char *why = rank_sums_bad_args(ncells, ngenes, ngroups, indptr, labels, n, zeros, ties, nexpr, rank2))
        return fail("%s", why);
    const size_t G = (size_t)ngroups, J = (size_t)ngenes;
    if (ncells == 0 || ngenes == 0) {   // nothing to stage
        if (n) std::fill(n, n + G, (int64_t)0);
        if (zeros) std::fill(zeros, zeros + J, (int64_t)0);
        if (ties) std::fill(ties, ties + J, (int64_t)0);
        if (nexpr) std::fill(nexpr, nexpr + G * J, (int64_t)0);
        if (rank2) std::fill(rank2, rank2 + G * J, (int64_t)0);
        return 0;
    }
    return guarded([&] {
        use_device(device);
        TempStream ts;
        DevBuf d_indptr, d_indices, d_data, d_labels, d_n, d_zeros, d_ties, d_nexpr, d_rank2;
        h2d<int64_t>(d_indptr, indptr, J + 1, ts.st);
        const int64_t nnz = indptr_on_device(ts.st, ngenes, d_indptr.as<int64_t>(), rank_sums_bad_indptr);   // the host's indptr[J] if it passes
        if (const char *why = rank_sums_bad_nnz(nnz, indices, data)) throw std::invalid_argument(why);
        h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
        h2d<float>(d_data, data, (size_t)nnz, ts.st);
        h2d<int32_t>(d_labels, labels, (size_t)ncells, ts.st);
        d_n.alloc(G * sizeof(int64_t));
        d_zeros.alloc(J * sizeof(int64_t));
        d_ties.alloc(J * sizeof(int64_t));
        d_nexpr.alloc(G * J * sizeof(int64_t));
        d_rank2.alloc(G * J * sizeof(int64_t));
        rank_sums_on_device(ts.st, ncells, ngenes, nnz, d_indptr.as<int64_t>(), d_indices.as<int32_t>(), d_data.as<float>(),
                            d_labels.as<int32_t>(), ngroups, d_n.as<int64_t>(), d_zeros.as<int64_t>(), d_ties.as<int64_t>(),
                            d_nexpr.as<int64_t>(), d_rank2.as<int64_t>());
        HIPCHK(hipMemcpyAsync(n, d_n.p, G * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        HIPCHK(hipMemcpyAsync(zeros, d_zeros.p, J * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        HIPCHK(hipMemcpyAsync(ties, d_ties.p, J * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        HIPCHK(hipMemcpyAsync(nexpr, d_nexpr.p, G * J * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        d2h(rank2, d_rank2, G * J * sizeof(int64_t), ts.st);
    });
}

}  // extern "C"
