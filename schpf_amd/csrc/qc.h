// Cell and gene filtering: what the kernels of qc.hip and the serial restatement of host.cpp share -- the
// refusals of the entry points and their messages (those of the matrix itself: csr_words.h), and the overflow rule of the
// sum of squares.  Like doublets.h, plain C++ that compiles for the host and for the device.
#pragma once
#include <cstdint>
#include <string>

#include "csr_words.h"

namespace schpf {

constexpr int QC_MAX_SETS = 32;   // one bit of a gene's flag word per gene set

inline const char *qc_bad_sizes(int64_t ncells, int64_t ngenes, int64_t nnz)
{
    if (ncells < 0 || ncells >= (int64_t)1 << 31) return "ncells must be in [0, 2^31)";
    if (ngenes < 0 || ngenes >= (int64_t)1 << 31) return "ngenes must be in [0, 2^31)";
    if (nnz < 0 || nnz >= (int64_t)1 << 31) return "nnz must be in [0, 2^31)";
    return nullptr;
}

// What schpf_axis_stats, schpf_axis_stats_device and schpf_debug_axis_stats refuse alike, before anything is read; nnz = 0
// is asked next by the caller.  nullptr: the arguments are fine
inline const char *qc_stats_bad_args(int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr, const void *indices,
                                     const void *val, int n_sets, const void *gene_flags, const void *cell_n,
                                     const void *cell_total, const void *cell_set_total, const void *gene_n,
                                     const void *gene_total, const void *gene_sumsq)
{
    if (const char *why = qc_bad_sizes(ncells, ngenes, nnz)) return why;
    if (n_sets < 0 || n_sets > QC_MAX_SETS) return "n_sets must be in [0, 32]";
    if (ncells > 0 && (!cell_n || !cell_total)) return "cell_n and cell_total must not be NULL";
    if (ncells > 0 && n_sets > 0 && !cell_set_total) return "cell_set_total must not be NULL where n_sets > 0";
    if (ngenes > 0 && n_sets > 0 && !gene_flags) return "gene_flags must not be NULL where n_sets > 0";
    if (ngenes > 0 && (!gene_n || !gene_total || !gene_sumsq)) return "gene_n, gene_total and gene_sumsq must not be NULL";
    if (nnz > 0 && (!indptr || !indices || !val)) return "indptr, indices and val must not be NULL";
    return nullptr;
}

// What schpf_submatrix, schpf_submatrix_device and schpf_debug_submatrix refuse alike, before anything is read
inline const char *qc_submatrix_bad_args(int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr, const void *indices,
                                         const void *val, int64_t n_rows, const void *rows, const void *out_ngenes,
                                         const void *out_indptr, const void *out_indices, const void *out_values,
                                         int64_t capacity)
{
    if (const char *why = qc_bad_sizes(ncells, ngenes, nnz)) return why;
    if (n_rows < 0 || n_rows >= (int64_t)1 << 31) return "n_rows must be in [0, 2^31)";
    if (!rows && n_rows != ncells) return "n_rows must be ncells where rows is NULL";
    if ((out_indices == nullptr) != (out_values == nullptr)) return "out_indices and out_values must both be given or both be NULL";
    if (out_indices && capacity < 0) return "capacity must be >= 0";
    if (!out_ngenes || !out_indptr) return "out_ngenes and out_indptr must not be NULL";
    if (nnz > 0 && n_rows > 0 && (!indptr || !indices || !val)) return "indptr, indices and val must not be NULL";
    return nullptr;
}

// The refusals of the matrix are those of csr_words.h under the prefix "qc"; the row list comes behind them
inline std::string qc_bad_rows(int64_t position) { return "qc: rows must be in [0, ncells); offending position " + std::to_string(position); }

// gene_sumsq[j] <= vmax^2 * ncells must stay below 2^63, or the call is refused in the words of csr_bad_sumsq.  vmax <= 2^24
// and ncells < 2^31: the product is below 2^79
inline bool qc_sumsq_overflows(uint64_t vmax, int64_t ncells)
{
    return (unsigned __int128)(vmax * vmax) * (unsigned __int128)ncells >= (unsigned __int128)1 << 63;
}

}  // namespace schpf
