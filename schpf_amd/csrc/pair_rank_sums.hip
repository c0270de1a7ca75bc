// Rank sums between pairs of groups (schpf_pair_rank_sums / schpf_pair_rank_sums_device): twice the
// Mann-Whitney U of group a over group b and the tie term of a ∪ b, for every requested pair and every gene.  Every output is
// an integer sum -- exact in any order.  The definition is in include/schpf_hip.h; host.cpp's serial restatement gives the
// same bits.  One sort serves all pairs; no thread and no workgroup walks a gene.
//
//   (graph_device.h, rank_sums_device.h: the checks of indptr, the cell ids, the values and the labels, the gene of every
//   entry, n[g])
//   pair_check_kernel       one thread per pair: two different groups in [0, G); the smallest offending row into the last
//                           word of the call's record
//   pair_degree_kernel      deg[g] = the pair rows that name g; (rocPRIM exclusive scan: side_ptr[G + 1], T = 2 P sides)
//   pair_sides_kernel       the sides of group g at side_ptr[g] ..: the pair row and (other group) * 2 + (g is the row's first)
//   pair_keys_kernel        per entry the key ((gene * G + group) << 32) | float bits; an entry that is a stored zero or whose
//                           cell is in no group gets the key (G * J) << 32, which sorts behind all the others
//   (rocPRIM radix sort of the keys over the occupied bits, then run-length encode: the S sub-runs (gene, group, value) with
//   their counts, already in the order of the per-(gene, group) lists of distinct values; an exclusive scan of the counts
//   gives sub_start[S + 1] -- the entries of the list below a value are sub_start[i] - sub_start[the list's first])
//   pair_lists_kernel       list_ptr[s], s = gene * G + group in [0, G J]: the first sub-run of list s, by bisection
//   pair_nexpr_kernel       per (g, j): nexpr = the entries of the list
//   pair_base_kernel        per (p, j): u2 = z_a z_b, ties = t_0^3 - t_0
//   pair_accumulate_kernel  a workgroup per chunk of 512 sub-runs, a thread per sub-run (j, x, v), which steps through the
//                           sides of x: a bisection for v in the list (j, y) of the other group gives below_y(v) and c_y(v);
//                           c_x (2 below_y + c_y) goes to u2[p, j] where x is the row's first group, t^3 - t to ties[p, j] from
//                           the smaller group id where both hold v.  A wave whose lanes all add to one (p, j) -- a long list
//                           -- sums across its lanes first; the adds go to LDS bins of (gene, side) counted from the chunk's
//                           first list, then one global atomic add per bin that is not empty; what falls outside the bins --
//                           a chunk of many short lists, or thousands of pairs -- goes to global memory directly: few
//                           sub-runs share an address there
// The atomic adds are integer adds: the result does not depend on their order, nor on the grid.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include "rank_sums_device.h"

namespace schpf {
namespace {

constexpr int CHUNK = 512;    // sub-runs per pass of a workgroup: 2 per thread
constexpr int BINS = 2048;    // (gene, side) bins of a chunk in LDS, u2 and ties: 32 KiB

__global__ __launch_bounds__(256) void pair_check_kernel(const int32_t *__restrict__ pairs, int npairs, int ngroups,
                                                         unsigned long long *__restrict__ word)
{
    unsigned long long bad = NONE;
    GRID_STRIDE(p, npairs)
    {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || a >= ngroups || b < 0 || b >= ngroups || a == b) offends(bad, p);
    }
    report_min(word, bad);
}

// deg is 0 on entry
__global__ __launch_bounds__(256) void pair_degree_kernel(const int32_t *__restrict__ pairs, int npairs, uint32_t *__restrict__ deg)
{
    GRID_STRIDE(x, 2 * (int64_t)npairs) atomicAdd(&deg[pairs[x]], 1u);
}

// cursor is 0 on entry.  The order of a group's sides depends on the schedule; no output does
__global__ __launch_bounds__(256) void pair_sides_kernel(const int32_t *__restrict__ pairs, int npairs, const uint32_t *__restrict__ side_ptr,
                                                         uint32_t *__restrict__ cursor, int32_t *__restrict__ side_row,
                                                         uint32_t *__restrict__ side_other)
{
    GRID_STRIDE(x, 2 * (int64_t)npairs)
    {
        const int g = pairs[x], other = pairs[x ^ 1];
        const uint32_t at = side_ptr[g] + atomicAdd(&cursor[g], 1u);
        side_row[at] = (int32_t)(x >> 1);
        side_other[at] = (uint32_t)other * 2u + (uint32_t)(~x & 1);
    }
}

__global__ __launch_bounds__(256) void pair_keys_kernel(const int32_t *__restrict__ geneof, const int32_t *__restrict__ indices,
                                                        const float *__restrict__ data, const int32_t *__restrict__ labels,
                                                        int64_t nnz, int64_t ngroups, int64_t ngenes, uint64_t *__restrict__ key)
{
    GRID_STRIDE(e, nnz)
    {
        const uint32_t bits = __float_as_uint(data[e]) & 0x7fffffffu;   // -0.0 is 0
        const int64_t g = labels[indices[e]];
        const int64_t list = (bits == 0u || g < 0) ? ngroups * ngenes : (int64_t)geneof[e] * ngroups + g;
        key[e] = ((uint64_t)list << 32) | (uint64_t)(list == ngroups * ngenes ? 0u : bits);
    }
}

// the first sub-run whose list is at least s; nruns when there is none
__global__ __launch_bounds__(256) void pair_lists_kernel(const uint64_t *__restrict__ sub_key, int64_t nruns, int64_t nlists,
                                                         uint32_t *__restrict__ list_ptr)
{
    GRID_STRIDE(s, nlists + 1)
    {
        int64_t lo = 0, hi = nruns;   // the answer is in [lo, hi]
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)(sub_key[mid] >> 32) < s) lo = mid + 1;
            else hi = mid;
        }
        list_ptr[s] = (uint32_t)lo;
    }
}

__global__ __launch_bounds__(256) void pair_nexpr_kernel(const uint32_t *__restrict__ list_ptr, const uint32_t *__restrict__ sub_start,
                                                         int64_t ngroups, int64_t ngenes, int64_t *__restrict__ nexpr)
{
    GRID_STRIDE(x, ngroups * ngenes)
    {
        const int64_t g = x / ngenes, j = x - g * ngenes, s = j * ngroups + g;
        nexpr[x] = (int64_t)sub_start[list_ptr[s + 1]] - (int64_t)sub_start[list_ptr[s]];
    }
}

__global__ __launch_bounds__(256) void pair_base_kernel(const int32_t *__restrict__ pairs, const int64_t *__restrict__ n,
                                                        const int64_t *__restrict__ nexpr, int64_t npairs, int64_t ngenes,
                                                        int64_t *__restrict__ u2, int64_t *__restrict__ ties)
{
    GRID_STRIDE(x, npairs * ngenes)
    {
        const int64_t p = x / ngenes, j = x - p * ngenes, a = pairs[2 * p], b = pairs[2 * p + 1];
        const int64_t za = n[a] - nexpr[a * ngenes + j], zb = n[b] - nexpr[b * ngenes + j], t = za + zb;
        u2[x] = za * zb;
        ties[x] = t * t * t - t;
    }
}

__device__ __forceinline__ sum_t wave_sum(sum_t v)
{
    for (int w = 32; w > 0; w >>= 1) v += (sum_t)__shfl_xor((long long)v, w);
    return v;
}

__global__ __launch_bounds__(256) void pair_accumulate_kernel(const uint64_t *__restrict__ sub_key, const uint32_t *__restrict__ sub_start,
                                                              const uint32_t *__restrict__ list_ptr, const uint32_t *__restrict__ side_ptr,
                                                              const int32_t *__restrict__ side_row, const uint32_t *__restrict__ side_other,
                                                              const int64_t *__restrict__ n, int64_t ngroups, int64_t ngenes, int64_t nsides,
                                                              sum_t *__restrict__ u2, sum_t *__restrict__ ties)
{
    __shared__ sum_t bin_u2[BINS];
    __shared__ sum_t bin_tie[BINS];
    const int64_t nruns = list_ptr[ngroups * ngenes];   // the sub-runs of the lists; the dropped entries follow
    const int64_t chunks = (nruns + CHUNK - 1) / CHUNK;
    for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        for (int b = threadIdx.x; b < BINS; b += 256) {
            bin_u2[b] = 0;
            bin_tie[b] = 0;
        }
        __syncthreads();
        const int64_t first = chunk * CHUNK, last = first + CHUNK < nruns ? first + CHUNK : nruns;
        const int64_t list0 = (int64_t)(sub_key[first] >> 32), j0 = list0 / ngroups;   // the lists of the chunk ascend from here
        const int64_t slot0 = j0 * nsides + side_ptr[list0 - j0 * ngroups];
        for (int64_t round = first; round < last; round += 256) {   // the same trips for every lane: the waves vote below
            const int64_t i = round + threadIdx.x;
            int64_t j = 0, x = 0, cx = 0;
            uint32_t bits = 0, side = 0, deg = 0;
            if (i < last) {
                const uint64_t k = sub_key[i];
                const int64_t list = (int64_t)(k >> 32);
                bits = (uint32_t)k;
                j = list / ngroups;
                x = list - j * ngroups;
                cx = (int64_t)sub_start[i + 1] - (int64_t)sub_start[i];
                side = side_ptr[x];
                deg = side_ptr[x + 1] - side;
            }
            for (uint32_t q = 0; __any(q < deg); ++q) {
                const bool active = q < deg;
                int64_t slot = -1, out = 0;
                sum_t add_u = 0, add_t = 0;
                if (active) {
                    const uint32_t other = side_other[side + q];
                    const int64_t y = other >> 1, list_y = j * ngroups + y;
                    const int64_t from = list_ptr[list_y], to = list_ptr[list_y + 1];
                    const uint64_t want = ((uint64_t)list_y << 32) | bits;
                    int64_t lo = from, hi = to;   // the first sub-run of the list whose value is at least v
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (sub_key[mid] < want) lo = mid + 1;
                        else hi = mid;
                    }
                    const int64_t at = sub_start[lo], begin = sub_start[from], end = sub_start[to];
                    const int64_t cy = (lo < to && sub_key[lo] == want) ? (int64_t)sub_start[lo + 1] - at : 0;
                    const int64_t below = n[y] - (end - begin) + (at - begin);   // z_y and the positive entries below v
                    if (other & 1u) add_u = (sum_t)(cx * (2 * below + cy));
                    const int64_t t = cx + cy;
                    if (cy == 0 || x < y) add_t = (sum_t)(t * t * t - t);
                    slot = j * nsides + side + q - slot0;
                    out = (int64_t)side_row[side + q] * ngenes + j;
                }
                // a long list: every lane of the wave adds to the same (p, j)
                const unsigned long long voters = __ballot(active);
                const int64_t lead = __shfl((long long)slot, __ffsll((long long)voters) - 1);
                bool adds = active;
                if (__all(!active || slot == lead)) {   // the same answer in every lane: no lane leaves the vote
                    add_u = wave_sum(add_u);
                    add_t = wave_sum(add_t);
                    adds = (int)(threadIdx.x & 63) == __ffsll((long long)voters) - 1;
                }
                if (adds && slot < BINS) {
                    if (add_u) atomicAdd(&bin_u2[slot], add_u);
                    if (add_t) atomicAdd(&bin_tie[slot], add_t);
                } else if (adds) {
                    if (add_u) atomicAdd(&u2[out], add_u);
                    if (add_t) atomicAdd(&ties[out], add_t);
                }
            }
        }
        __syncthreads();
        for (int b = threadIdx.x; b < BINS; b += 256)
            if (bin_u2[b] | bin_tie[b]) {   // a bin that was added to: its gene and its side exist
                const int64_t slot = slot0 + b, j = slot / nsides, out = (int64_t)side_row[slot - j * nsides] * ngenes + j;
                if (bin_u2[b]) atomicAdd(&u2[out], bin_u2[b]);
                if (bin_tie[b]) atomicAdd(&ties[out], bin_tie[b]);
            }
        __syncthreads();   // before the next chunk clears the bins
    }
}

// Everything on `st`, which is synchronised when this returns; all pointers are device memory, indptr has been checked,
// N and J are at least 1.  The outputs are written after the last check: a refused call leaves them alone
void pair_rank_sums_on_device(hipStream_t st, int ncells, int ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                              const float *data, const int32_t *labels, int ngroups, const int32_t *pairs, int npairs, int64_t *n,
                              int64_t *nexpr, int64_t *u2, int64_t *ties)
{
    const int64_t N = ncells, J = ngenes, G = ngroups, P = npairs, T = 2 * P, lists = G * J;
    DevBuf geneof;
    RankWords w;
    entries_and_labels_on_device(st, ncells, ngenes, nnz, indptr, indices, data, labels, ngroups, geneof, w);
    if (P > 0) {   // after the labels, as the refusals are ordered: the word is still NONE
        LAUNCH(pair_check_kernel, P, st, pairs, npairs, ngroups, w.dev() + R_BAD_PAIRS);
        w.fetch(st);
        w.refuse(R_BAD_PAIRS, pair_rank_sums_bad_pairs);
    }

    HIPCHK(hipMemsetAsync(n, 0, (size_t)G * sizeof(int64_t), st));
    LAUNCH(rank_sums_count_kernel, N, st, labels, ncells, ngroups, (sum_t *)n);
    if (nnz == 0) {
        HIPCHK(hipMemsetAsync(nexpr, 0, (size_t)lists * sizeof(int64_t), st));
        if (P > 0) LAUNCH(pair_base_kernel, P * J, st, pairs, n, nexpr, P, J, u2, ties);
        HIPCHK(hipStreamSynchronize(st));
        return;
    }

    Scratch temp;
    DevBuf key_a, key_b, counts, sub_start, list_ptr, nruns_dev;
    key_a.alloc((size_t)nnz * sizeof(uint64_t));
    key_b.alloc((size_t)nnz * sizeof(uint64_t));
    counts.alloc((size_t)(nnz + 1) * sizeof(uint32_t), true, st);   // one past the runs stays 0: the scan runs over it
    sub_start.alloc((size_t)(nnz + 1) * sizeof(uint32_t));
    list_ptr.alloc((size_t)(lists + 1) * sizeof(uint32_t));
    nruns_dev.alloc(sizeof(uint32_t));
    uint64_t *const ka = key_a.as<uint64_t>(), *const kb = key_b.as<uint64_t>();
    LAUNCH(pair_keys_kernel, nnz, st, geneof.as<int32_t>(), indices, data, labels, nnz, G, J, ka);
    geneof.release();   // hipFree waits for the kernel
    const int bits = 32 + bits_of((uint64_t)lists);
    temp.run([&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, ka, kb, (size_t)nnz, 0, bits, st); });
    uint64_t *const sub_key = ka;   // the unsorted keys are done with
    temp.run([&](void *t, size_t &b) {
        return rocprim::run_length_encode(t, b, kb, (size_t)nnz, sub_key, counts.as<uint32_t>(), nruns_dev.as<uint32_t>(), st);
    });
    uint32_t h_runs = 0;
    d2h(&h_runs, nruns_dev, sizeof h_runs, st);
    const int64_t S = h_runs;   // the dropped entries are the last run, if there are any
    key_b.release();
    temp.run([&](void *t, size_t &b) {
        return rocprim::exclusive_scan(t, b, counts.as<uint32_t>(), sub_start.as<uint32_t>(), 0u, (size_t)(S + 1),
                                       rocprim::plus<uint32_t>(), st);
    });
    LAUNCH(pair_lists_kernel, lists + 1, st, sub_key, S, lists, list_ptr.as<uint32_t>());
    LAUNCH(pair_nexpr_kernel, lists, st, list_ptr.as<uint32_t>(), sub_start.as<uint32_t>(), G, J, nexpr);
    if (P > 0) {
        DevBuf deg, side_ptr, side_row, side_other;
        deg.alloc((size_t)(2 * (G + 1)) * sizeof(uint32_t), true, st);   // the degrees, then the cursors
        side_ptr.alloc((size_t)(G + 1) * sizeof(uint32_t));
        side_row.alloc((size_t)T * sizeof(int32_t));
        side_other.alloc((size_t)T * sizeof(uint32_t));
        uint32_t *const cursor = deg.as<uint32_t>() + (G + 1);
        LAUNCH(pair_degree_kernel, T, st, pairs, npairs, deg.as<uint32_t>());
        temp.run([&](void *t, size_t &b) {
            return rocprim::exclusive_scan(t, b, deg.as<uint32_t>(), side_ptr.as<uint32_t>(), 0u, (size_t)(G + 1),
                                           rocprim::plus<uint32_t>(), st);
        });
        LAUNCH(pair_sides_kernel, T, st, pairs, npairs, side_ptr.as<uint32_t>(), cursor, side_row.as<int32_t>(),
               side_other.as<uint32_t>());
        LAUNCH(pair_base_kernel, P * J, st, pairs, n, nexpr, P, J, u2, ties);
        const int64_t chunks = (S + CHUNK - 1) / CHUNK;
        hipLaunchKernelGGL(pair_accumulate_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks, 1 << 20))), dim3(256), 0,
                           st, sub_key, sub_start.as<uint32_t>(), list_ptr.as<uint32_t>(), side_ptr.as<uint32_t>(),
                           side_row.as<int32_t>(), side_other.as<uint32_t>(), n, G, J, T, (sum_t *)u2, (sum_t *)ties);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));   // before the sides are released
        return;
    }
    HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
}

void zero_outputs(hipStream_t st, int ngenes, int ngroups, int npairs, int64_t *n, int64_t *nexpr, int64_t *u2, int64_t *ties)
{
    const size_t G = (size_t)ngroups, J = (size_t)ngenes, P = (size_t)npairs;
    if (n) HIPCHK(hipMemsetAsync(n, 0, G * sizeof(int64_t), st));
    if (nexpr && G * J) HIPCHK(hipMemsetAsync(nexpr, 0, G * J * sizeof(int64_t), st));
    if (u2 && P * J) HIPCHK(hipMemsetAsync(u2, 0, P * J * sizeof(int64_t), st));
    if (ties && P * J) HIPCHK(hipMemsetAsync(ties, 0, P * J * sizeof(int64_t), st));
    HIPCHK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_pair_rank_sums_device(int device, void *stream, int ncells, int ngenes, const int64_t *indptr, const int32_t *indices,
                                const float *data, const int32_t *labels, int ngroups, const int32_t *pairs, int npairs, int64_t *n,
                                int64_t *nexpr, int64_t *u2, int64_t *ties)
{
    if (const char *why = pair_rank_sums_bad_args(ncells, ngenes, ngroups, indptr, labels, pairs, npairs, n, nexpr, u2, ties))
        return fail("%s", why);
    return guarded([&] {
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        if (ncells == 0 || ngenes == 0) {
            zero_outputs(st, ngenes, ngroups, npairs, n, nexpr, u2, ties);
            return;
        }
        const int64_t nnz = indptr_on_device(st, ngenes, indptr, rank_sums_bad_indptr);
        if (const char *why = rank_sums_bad_nnz(nnz, indices, data)) throw std::invalid_argument(why);
        pair_rank_sums_on_device(st, ncells, ngenes, nnz, indptr, indices, data, labels, ngroups, pairs, npairs, n, nexpr, u2, ties);
    });
}

int schpf_pair_rank_sums(int device, int ncells, int ngenes, const int64_t *indptr, const int32_t *indices, const float *data,
                         const int32_t *labels, int ngroups, const int32_t *pairs, int npairs, int64_t *n, int64_t *nexpr,
                         int64_t *u2, int64_t *ties)
{
    if (const char *why = pair_rank_sums_bad_args(ncells, ngenes, ngroups, indptr, labels, pairs, npairs, n, nexpr, u2, ties))
        return fail("%s", why);
    const size_t G = (size_t)ngroups, J = (size_t)ngenes, P = (size_t)npairs;
    if (ncells == 0 || ngenes == 0) {   // nothing to stage
        if (n) std::fill(n, n + G, (int64_t)0);
        if (nexpr) std::fill(nexpr, nexpr + G * J, (int64_t)0);
        if (u2) std::fill(u2, u2 + P * J, (int64_t)0);
        if (ties) std::fill(ties, ties + P * J, (int64_t)0);
        return 0;
    }
    return guarded([&] {
        use_device(device);
        TempStream ts;
        DevBuf d_indptr, d_indices, d_data, d_labels, d_pairs, d_n, d_nexpr, d_u2, d_ties;
        h2d<int64_t>(d_indptr, indptr, J + 1, ts.st);
        const int64_t nnz = indptr_on_device(ts.st, ngenes, d_indptr.as<int64_t>(), rank_sums_bad_indptr);   // the host's indptr[J] if it passes
        if (const char *why = rank_sums_bad_nnz(nnz, indices, data)) throw std::invalid_argument(why);
        h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
        h2d<float>(d_data, data, (size_t)nnz, ts.st);
        h2d<int32_t>(d_labels, labels, (size_t)ncells, ts.st);
        h2d<int32_t>(d_pairs, pairs, 2 * P, ts.st);
        d_n.alloc(G * sizeof(int64_t));
        d_nexpr.alloc(G * J * sizeof(int64_t));
        d_u2.alloc(P * J * sizeof(int64_t));
        d_ties.alloc(P * J * sizeof(int64_t));
        pair_rank_sums_on_device(ts.st, ncells, ngenes, nnz, d_indptr.as<int64_t>(), d_indices.as<int32_t>(), d_data.as<float>(),
                                 d_labels.as<int32_t>(), ngroups, d_pairs.as<int32_t>(), npairs, d_n.as<int64_t>(),
                                 d_nexpr.as<int64_t>(), d_u2.as<int64_t>(), d_ties.as<int64_t>());
        HIPCHK(hipMemcpyAsync(n, d_n.p, G * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        HIPCHK(hipMemcpyAsync(nexpr, d_nexpr.p, G * J * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        if (P) HIPCHK(hipMemcpyAsync(u2, d_u2.p, P * J * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        if (P) HIPCHK(hipMemcpyAsync(ties, d_ties.p, P * J * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        HIPCHK(hipStreamSynchronize(ts.st));
    });
}

}  // extern "C"
