// The gene-major form of a count matrix: what the kernels of transpose.hip and the serial restatement of
// host.cpp share -- the refusals of the entry points and their messages (those of the matrix itself: csr_words.h), and the
// one expression of the value conversion.
// Like doublets.h, plain C++ that compiles for the host and for the device.
#pragma once
#include <cstdint>
#include <string>

#include "philox.h"
#include "qc.h"

namespace schpf {

// out_values[o] where out_val_kind is SCHPF_VAL_F32 and val_kind is not: v is what load_value / read_count read
SCHPF_PX float transpose_value(double v) { return (float)v; }

// nothing to transpose: out_indptr is zeros and nothing else is read
inline bool transpose_empty(int64_t ncells, int64_t ngenes, int64_t nnz) { return nnz == 0 || ncells == 0 || ngenes == 0; }

// What schpf_transpose, schpf_transpose_device and schpf_debug_transpose refuse alike, before anything is read.  nullptr: the
// arguments are fine
inline const char *transpose_bad_args(int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr, int indptr_kind,
                                      const void *indices, int idx_kind, const void *val, int val_kind, int out_val_kind,
                                      const void *out_indptr, const void *out_cells, const void *out_values)
{
    if (const char *why = qc_bad_sizes(ncells, ngenes, nnz)) return why;
    if (csr_kinds_bad(indptr_kind, idx_kind, val_kind)) return "unknown index or value kind";
    if (out_val_kind != val_kind && out_val_kind != SCHPF_VAL_F32) return "out_val_kind must be val_kind or SCHPF_VAL_F32";
    if (!out_indptr) return "out_indptr must not be NULL";
    if (transpose_empty(ncells, ngenes, nnz)) return nullptr;
    if (!indptr || !indices || !val) return "indptr, indices and val must not be NULL";
    if (!out_cells || !out_values) return "out_cells and out_values must not be NULL";
    return nullptr;
}

// The refusals of the matrix are those of csr_words.h under the prefix "transpose"

}  // namespace schpf
