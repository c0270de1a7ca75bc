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

// The refusals of the matrix and the labels, in the order they are looked for; each names its smallest offender.  The
// wording is that of doublets.h and qc.h under the prefix of this section
inline std::string group_stats_from(const std::string &message, size_t old_prefix) { return "group_stats" + message.substr(old_prefix); }
inline std::string group_stats_bad_indptr(int64_t row) { return group_stats_from(doublet_bad_indptr(row), sizeof("doublets") - 1); }
inline std::string group_stats_bad_index(int64_t entry) { return group_stats_from(doublet_bad_index(entry), sizeof("doublets") - 1); }
inline std::string group_stats_bad_order(int64_t row) { return group_stats_from(doublet_bad_order(row), sizeof("doublets") - 1); }
inline std::string group_stats_bad_value(int64_t entry) { return group_stats_from(doublet_bad_value(entry), sizeof("doublets") - 1); }
inline std::string group_stats_bad_labels(int64_t cell)
{
    return "group_stats: labels must be in [-1, ngroups); offending cell " + std::to_string(cell);
}
// the rule of qc_sumsq_overflows: a group holds at most ncells cells
inline std::string group_stats_bad_sumsq(uint64_t vmax, int64_t ncells) { return group_stats_from(qc_bad_sumsq(vmax, ncells), sizeof("qc") - 1); }

}  // namespace schpf
