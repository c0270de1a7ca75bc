// What rank_sums.hip and pair_rank_sums.hip share: the kernels that check a gene-major matrix and the
// labels of its cells, the count of the cells per group, and the small helpers of a stateless call on a stream.  Included by
// both translation units; everything is in an unnamed namespace, each has its own copy.
//
//   rank_sums_indptr_kernel      indptr starts at 0 and does not decrease: the smallest offending gene of each workgroup
//   rank_sums_genes_kernel       the gene of every entry, by bisection in indptr (a gene may be of any length, no kernel
//                                walks one)
//   rank_sums_check_kernel       one thread per entry: cell id in range and above its left neighbour, value finite and >= 0
//   rank_sums_labels_kernel      one thread per cell: label in [-1, G)
//   rank_sums_count_kernel       n[g]: a workgroup counts in LDS bins, then adds its bins that are not 0
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <memory>
#include <string>

#include "common.h"
#include "kernels.h"

namespace schpf {
namespace {

typedef unsigned long long sum_t;   // the int64 outputs as atomicAdd takes them; no sum here is negative

constexpr int COUNT_BINS = 2048;  // group bins of rank_sums_count_kernel

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

__global__ __launch_bounds__(256) void rank_sums_indptr_kernel(const int64_t *__restrict__ indptr, int ngenes, int *__restrict__ part)
{
    int bad = INT_MAX;
    GRID_STRIDE(j, ngenes)
    {
        if ((j == 0 && indptr[0] != 0) || indptr[j + 1] < indptr[j]) bad = min(bad, (int)j);
    }
    block_min(bad, part);
}

// the largest gene j < J with indptr[j] <= e: the gene that holds entry e (indptr[0] = 0, indptr does not decrease)
__global__ __launch_bounds__(256) void rank_sums_genes_kernel(const int64_t *__restrict__ indptr, int64_t ngenes, int64_t nnz,
                                                              int32_t *__restrict__ geneof)
{
    GRID_STRIDE(e, nnz)
    {
        int64_t lo = 0, hi = ngenes;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (indptr[mid] <= e) lo = mid;
            else hi = mid;
        }
        geneof[e] = (int32_t)lo;
    }
}

__global__ __launch_bounds__(256) void rank_sums_check_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                              const float *__restrict__ data, const int32_t *__restrict__ geneof,
                                                              int ncells, int64_t nnz, int *__restrict__ part_cell,
                                                              int *__restrict__ part_val)
{
    int bad_cell = INT_MAX, bad_val = INT_MAX;
    GRID_STRIDE(e, nnz)
    {
        const int gene = geneof[e], cell = indices[e];
        if (cell < 0 || cell >= ncells || (e > indptr[gene] && indices[e - 1] >= cell)) bad_cell = min(bad_cell, gene);
        const uint32_t bits = __float_as_uint(data[e]);   // by the bits: no denormal mode has a say
        if (!(bits < 0x7f800000u || bits == 0x80000000u)) bad_val = min(bad_val, gene);
    }
    block_min(bad_cell, part_cell);
    __syncthreads();   // the LDS of block_min is used again
    block_min(bad_val, part_val);
}

__global__ __launch_bounds__(256) void rank_sums_labels_kernel(const int32_t *__restrict__ labels, int ncells, int ngroups,
                                                               int *__restrict__ part)
{
    int bad = INT_MAX;
    GRID_STRIDE(i, ncells)
    {
        if (labels[i] < -1 || labels[i] >= ngroups) bad = min(bad, (int)i);
    }
    block_min(bad, part);
}

// n is 0 on entry
__global__ __launch_bounds__(256) void rank_sums_count_kernel(const int32_t *__restrict__ labels, int ncells, int ngroups,
                                                              sum_t *__restrict__ n)
{
    __shared__ unsigned int bin[COUNT_BINS];
    for (int b = threadIdx.x; b < COUNT_BINS; b += 256) bin[b] = 0;
    __syncthreads();
    GRID_STRIDE(i, ncells)
    {
        const int g = labels[i];
        if (g < 0) continue;
        if (g < COUNT_BINS) atomicAdd(&bin[g], 1u);
        else atomicAdd(&n[g], (sum_t)1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < COUNT_BINS && b < ngroups; b += 256)
        if (bin[b]) atomicAdd(&n[b], (sum_t)bin[b]);
}

unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1 << 20)); }

int bits_of(uint64_t largest)   // the bits a radix sort has to look at for keys up to `largest`
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

void use_device(int device)
{
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) throw std::invalid_argument("no such HIP device");
    HIPCHK(hipSetDevice(device));
}

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

hipStream_t pick_stream(void *stream, std::unique_ptr<TempStream> &own)
{
    // NULL: a stream of the call's own; SCHPF_STREAM_DEFAULT: the device's null stream; else the given handle
    if (!stream) {
        own.reset(new TempStream);
        return own->st;
    }
    return stream == SCHPF_STREAM_DEFAULT ? nullptr : (hipStream_t)stream;
}

// indptr[J + 1] in device memory: refused unless it starts at 0 and does not decrease.  Returns nnz = indptr[J]
int64_t indptr_on_device(hipStream_t st, int ngenes, const int64_t *indptr)
{
    const int64_t blocks = grid_for(ngenes);
    DevBuf part, bad;
    part.alloc((size_t)blocks * sizeof(int));
    bad.alloc(2 * sizeof(int));
    LAUNCH(rank_sums_indptr_kernel, ngenes, st, indptr, ngenes, part.as<int>());
    HIPCHK(launch_knn_bad(part.as<int>(), blocks, nullptr, 0, bad.as<int>(), st));
    int h_bad[2];
    int64_t nnz = 0;
    HIPCHK(hipMemcpyAsync(&nnz, indptr + ngenes, sizeof nnz, hipMemcpyDeviceToHost, st));
    d2h(h_bad, bad, sizeof h_bad, st);
    if (h_bad[0] != INT_MAX) throw std::invalid_argument(rank_sums_bad_indptr(h_bad[0]));
    return nnz;
}

// The checks after indptr, on `st`, all pointers device memory: the cell ids, the values, then the labels; throws the
// refusal of the smallest offending gene or cell.  geneof[nnz] is left holding the gene of every entry
void entries_and_labels_on_device(hipStream_t st, int ncells, int ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                                  const float *data, const int32_t *labels, int ngroups, DevBuf &geneof)
{
    DevBuf part_cell, part_val, part_lab, bad;
    const int64_t blocks = grid_for(nnz), lab_blocks = grid_for(ncells);
    geneof.alloc((size_t)nnz * sizeof(int32_t));
    part_cell.alloc((size_t)blocks * sizeof(int));
    part_val.alloc((size_t)blocks * sizeof(int));
    part_lab.alloc((size_t)lab_blocks * sizeof(int));
    bad.alloc(4 * sizeof(int));   // cells, values; labels, unused
    if (nnz > 0) {
        LAUNCH(rank_sums_genes_kernel, nnz, st, indptr, (int64_t)ngenes, nnz, geneof.as<int32_t>());
        LAUNCH(rank_sums_check_kernel, nnz, st, indptr, indices, data, geneof.as<int32_t>(), ncells, nnz, part_cell.as<int>(),
               part_val.as<int>());
    }
    LAUNCH(rank_sums_labels_kernel, ncells, st, labels, ncells, ngroups, part_lab.as<int>());
    HIPCHK(launch_knn_bad(part_cell.as<int>(), nnz > 0 ? blocks : 0, part_val.as<int>(), nnz > 0 ? blocks : 0, bad.as<int>(), st));
    HIPCHK(launch_knn_bad(part_lab.as<int>(), lab_blocks, nullptr, 0, bad.as<int>() + 2, st));
    int h_bad[4];
    d2h(h_bad, bad, sizeof h_bad, st);
    if (h_bad[0] != INT_MAX) throw std::invalid_argument(rank_sums_bad_cells(h_bad[0]));
    if (h_bad[1] != INT_MAX) throw std::invalid_argument(rank_sums_bad_values(h_bad[1]));
    if (h_bad[2] != INT_MAX) throw std::invalid_argument(rank_sums_bad_labels(h_bad[2]));
}

}  // namespace
}  // namespace schpf
