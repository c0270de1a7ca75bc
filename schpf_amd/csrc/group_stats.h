// Pseudobulk: what the kernels of group_stats.hip and the serial restatement of host.cpp share -- the
// refusals of the entry points and their messages.  Like qc.h, plain C++ that compiles for the host and for the device.
#pragma once
#include <cstdint>
#include <string>

#include "qc.h"

namespace schpf {

// What schpf_group_stats, schpf_group_stats_device and schpf_debug_group_stats refuse alike, before anything is read;
// nnz = 0 is asked next by the caller.  sumsq may be NULL.  nullptr: the arguments are fine
inline const char *group_stats_bad_args(int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr, const void *indices,
                                        const void *val, const void *labels, int64_t ngroups, const void *group_cells,
                                        const void *nexpr, const void *total)
{
    if (const char *why = qc_bad_sizes(ncells, ngenes, nnz)) return why;
    if (ngroups < 1 || ngroups >= (int64_t)1 << 31) return "ngroups must be in [1, 2^31)";
    if (ngroups * ngenes >= (int64_t)1 << 31) return "ngroups * ngenes must be below 2^31";
    if (ncells > 0 && !labels) return "labels must not be NULL";
    if (!group_cells) return "group_cells must not be NULL";
    if (ngenes > 0 && (!nexpr || !total)) return "nexpr and total must not be NULL";
    if (nnz > 0 && (!indptr || !indices || !val)) return "indptr, indices and val must not be NULL";
    return nullptr;
}

// The refusals of the matrix and of the sum of squares are those of csr_words.h under the prefix "group_stats" (a group
// holds at most ncells cells: the rule of qc_sumsq_overflows); the labels come behind the matrix
inline std::string group_stats_bad_labels(int64_t cell)
{
    return "group_stats: labels must be in [-1, ngroups); offending cell " + std::to_string(cell);
}

}  // namespace schpf
