// What rank_sums.hip and pair_rank_sums.hip share on top of graph_device.h, whose indptr check, bisection
// for the gene of every entry and labels check they use: the check of a gene-major matrix's entries, the words of the
// call's refusals, and the count of the cells per group.  Included by both translation units; everything is in an unnamed
// namespace, each has its own copy.
//
//   rank_sums_check_kernel       one thread per entry: cell id in range and above its left neighbour, value finite and >= 0
//   rank_sums_count_kernel       n[g]: a workgroup counts in LDS bins, then adds its bins that are not 0
#pragma once
#include "graph_device.h"

namespace schpf {
namespace {

constexpr int COUNT_BINS = 2048;  // group bins of rank_sums_count_kernel

// the smallest offenders of a call, in the order they are asked; R_BAD_PAIRS is the pairwise call's
enum { R_BAD_CELLS = 0, R_BAD_VALUES, R_BAD_LABELS, R_BAD_PAIRS, R_COUNT };
typedef Offenders<R_COUNT> RankWords;

__global__ __launch_bounds__(256) void rank_sums_check_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                              const float *__restrict__ data, const int32_t *__restrict__ geneof,
                                                              int ncells, int64_t nnz, unsigned long long *__restrict__ words)
{
    unsigned long long bad_cell = NONE, bad_val = NONE;
    GRID_STRIDE(e, nnz)
    {
        const int gene = geneof[e], cell = indices[e];
        if (cell < 0 || cell >= ncells || (e > indptr[gene] && indices[e - 1] >= cell)) offends(bad_cell, gene);
        const uint32_t bits = __float_as_uint(data[e]);   // by the bits: no denormal mode has a say
        if (!(bits < 0x7f800000u || bits == 0x80000000u)) offends(bad_val, gene);
    }
    report_min(words + R_BAD_CELLS, bad_cell);
    report_min(words + R_BAD_VALUES, bad_val);
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

// The checks after indptr, on `st`, all pointers device memory: the cell ids, the values, then the labels; throws the
// refusal of the smallest offending gene or cell.  geneof[nnz] is left holding the gene of every entry, w reset and fetched
void entries_and_labels_on_device(hipStream_t st, int ncells, int ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                                  const float *data, const int32_t *labels, int ngroups, DevBuf &geneof, RankWords &w)
{
    w.reset(st);
    geneof.alloc((size_t)nnz * sizeof(int32_t));
    if (nnz > 0) {
        LAUNCH(entry_rows_kernel, nnz, st, indptr, (int64_t)ngenes, nnz, geneof.as<int32_t>());
        LAUNCH(rank_sums_check_kernel, nnz, st, indptr, indices, data, geneof.as<int32_t>(), ncells, nnz, w.dev());
    }
    LAUNCH(labels_check_kernel, ncells, st, labels, (int64_t)ncells, ngroups, w.dev() + R_BAD_LABELS);
    w.fetch(st);
    w.refuse(R_BAD_CELLS, rank_sums_bad_cells);
    w.refuse(R_BAD_VALUES, rank_sums_bad_values);
    w.refuse(R_BAD_LABELS, rank_sums_bad_labels);
}

}  // namespace
}  // namespace schpf
