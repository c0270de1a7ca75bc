// Device passes of an upload whose count matrix is already in HBM (schpf_upload_coo_device / _csr_device):
// what schpf_upload_coo does with host threads before the plan builders run -- validate and convert the triples, list
// the stored zeros, find the order of the COO, sample the major indices for the task-range model -- and the expansion
// of a CSR's row pointers.  hipStream_t is a pointer type; declared as void * so that host-only units need no HIP header.
#pragma once
#include <cstdint>

namespace schpf {

// What one validate + convert pass reports.  The counts are integer sums and the offenders integer minima: the same
// bits on every run.
struct ConvertStats {
    int64_t rounded = 0;          // values that float32 rounds
    int64_t zeros = 0;            // explicitly stored zeros (entries whose indices are in range)
    int64_t first_bad_index = -1; // smallest entry with an index < 0, >= its axis, or an int64 beyond int32; -1: none
    int64_t first_bad_value = -1; // smallest entry with a negative, NaN or beyond-float32 value; -1: none
    bool packed_ok = true;        // every value fits the packed 16-bit entry format
    bool sorted[2] = {true, true};   // the entries are in (row, col) / (col, row) order (plan.h coo_order_flags)
};

// CSR row pointers indptr[n_rows + 1] (SCHPF_IDX_I32 / _I64): true if indptr[0] == 0, non-decreasing, indptr[n_rows] ==
// nnz.  One flag comes back to the host.
bool csr_indptr_valid(void *stream, const void *d_indptr, int indptr_kind, int n_rows, int64_t nnz);
// ... and, for a valid one, out_row[j] = the row whose run holds entry j
void csr_expand_rows(void *stream, const void *d_indptr, int indptr_kind, int n_rows, int64_t nnz, int32_t *d_out_row);

// One pass over the entries.  row / col of idx kind row_kind / col_kind, val of SCHPF_VAL_* kind.  out_row / out_col /
// out_val: where the int32 / float32 copies go, or nullptr for an array that has that type already and is read in place.
ConvertStats convert_coo_device(void *stream, int64_t nnz, const void *d_row, int row_kind, const void *d_col, int col_kind,
                                const void *d_val, int val_kind, int n_rows, int n_cols, int32_t *d_out_row,
                                int32_t *d_out_col, float *d_out_val);

// The (row, col) of the n_zero stored zeros, in COO order (a stable selection on the caller's values: an entry is a
// stored zero when its value, as given, equals 0).  d_zero_row / d_zero_col: int32[n_zero], allocated by the caller.
void compact_zeros_device(void *stream, int64_t nnz, const int32_t *d_row, const int32_t *d_col, const void *d_val,
                          int val_kind, int64_t n_zero, int32_t *d_zero_row, int32_t *d_zero_col);

// Histograms of every stride-th row / col index (the sample positions i * stride of plan.cpp block_shares) into
// hist_row[n_rows] / hist_col[n_cols] on the HOST: n_rows + n_cols integers cross PCIe.
void sample_histograms_device(void *stream, int64_t nnz, const int32_t *d_row, const int32_t *d_col, int n_rows,
                              int n_cols, int64_t stride, int32_t *hist_row, int32_t *hist_col);

}  // namespace schpf
