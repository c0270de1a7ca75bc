// The contract of a caller's count CSR in the one form that the kernels of csr_device.h, the entry points of
// doublets.hip, qc.hip, group_stats.hip and transpose.hip and the serial restatements of host.cpp share: how much of the
// matrix an operator asks, the words of the refusals under the operator's prefix, and the bytes of a stored value.
// Plain C++ without HIP or rocPRIM: host.cpp and the .hip files include it alike.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/schpf_hip.h"

namespace schpf {

// What an operator asks of the entries, each level on top of the one before: every column in [0, ngenes) (the submatrix);
// every column above its left neighbour (the transpose, to which the values mean nothing); every value a count thinning
// accepts, and the largest value (the doublets and the statistics)
enum CsrLevel { CSR_RANGE = 0, CSR_ORDER, CSR_COUNTS };

// refused with "unknown index or value kind" by every entry point of the family
inline bool csr_kinds_bad(int indptr_kind, int idx_kind, int val_kind)
{
    return (indptr_kind != SCHPF_IDX_I32 && indptr_kind != SCHPF_IDX_I64) || (idx_kind != SCHPF_IDX_I32 && idx_kind != SCHPF_IDX_I64) ||
           val_kind < SCHPF_VAL_I32 || val_kind > SCHPF_VAL_F64;
}

// The refusals of the matrix, in the order they are looked for; each names its smallest offender.  op: "doublets", "qc",
// "group_stats" or "transpose"
inline std::string csr_bad_indptr(const char *op, int64_t row)
{
    return std::string(op) + ": indptr must be 0 at row 0, must be non-decreasing and must end at nnz; offending row " + std::to_string(row);
}
inline std::string csr_bad_index(const char *op, int64_t entry)
{
    return std::string(op) + ": column index out of range at entry " + std::to_string(entry);
}
inline std::string csr_bad_order(const char *op, int64_t row)
{
    return std::string(op) + ": columns must be strictly ascending within a row; offending row " + std::to_string(row);
}
inline std::string csr_bad_value(const char *op, int64_t entry)
{
    return std::string(op) + ": values must be integer counts in [0, 2^24]; offending entry " + std::to_string(entry);
}
// the rule of qc_sumsq_overflows (qc.h)
inline std::string csr_bad_sumsq(const char *op, uint64_t vmax, int64_t ncells)
{
    return std::string(op) + ": sum of squares may overflow: largest value " + std::to_string(vmax) + " over " + std::to_string(ncells) + " cells";
}

// a CSR that an operator writes (the doublets, the submatrix) into too little room; no prefix
inline std::string csr_bad_capacity(int64_t capacity, int64_t total)
{
    return "capacity must be at least the " + std::to_string(total) + " entries of the result, got " + std::to_string(capacity);
}

// the bytes of a stored value of kind SCHPF_VAL_*
inline size_t value_size(int val_kind) { return val_kind == SCHPF_VAL_I32 || val_kind == SCHPF_VAL_F32 ? 4 : 8; }

}  // namespace schpf
