// Simulated doublets: what the kernels of doublets.hip and the serial restatement of host.cpp share -- the
// draw of a simulated row's parents on the generator of philox.h, the refusals of the entry points and their messages
// (those of the matrix itself: csr_words.h).
// Like philox.h, plain C++ that compiles for the host and for the device.
#pragma once
#include <cstdint>
#include <string>

#include "csr_words.h"
#include "philox.h"

namespace schpf {

// Parents (a, b) of the simulated row s among N observed cells, 0 < N < 2^31: words 0 and 1 of the block with the counter
// (low word of s, high word of s, 0, 1) -- thinning's counters end in 0, so one seed gives unrelated streams -- each
// scaled to [0, N) by the high half of a 32 x 32 bit product.  a == b is allowed
SCHPF_PX void doublet_parents_of(uint64_t s, uint32_t N, uint32_t k0, uint32_t k1, int32_t *a, int32_t *b)
{
    const Philox4 w = philox4x32_10((uint32_t)s, (uint32_t)(s >> 32), 0u, 1u, k0, k1);
    *a = (int32_t)(((uint64_t)w.w[0] * N) >> 32);
    *b = (int32_t)(((uint64_t)w.w[1] * N) >> 32);
}

// What schpf_doublet_parents and schpf_doublet_parents_device refuse alike; n_sim = 0 is asked next by the caller
inline const char *doublet_parents_bad_args(int64_t first, int64_t n_sim, int64_t ncells, const void *parents)
{
    if (first < 0) return "first must be >= 0";
    if (n_sim < 0 || n_sim >= (int64_t)1 << 31) return "n_sim must be in [0, 2^31)";
    if (ncells < 1 || ncells >= (int64_t)1 << 31) return "ncells must be in (0, 2^31)";
    if (n_sim > 0 && !parents) return "parents must not be NULL";
    return nullptr;
}

// What schpf_doublet_rows, schpf_doublet_rows_device and schpf_debug_doublet_rows refuse alike, before anything is read;
// n_pairs = 0 or nnz = 0 is asked next by the caller.  nullptr: the arguments are fine
inline const char *doublet_rows_bad_args(int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr, const void *indices,
                                         const void *val, int64_t n_pairs, const void *parents, const void *out_indptr,
                                         const void *out_indices, const void *out_values, int64_t capacity)
{
    if (ncells < 0 || ncells >= (int64_t)1 << 31) return "ncells must be in [0, 2^31)";
    if (ngenes < 0 || ngenes >= (int64_t)1 << 31) return "ngenes must be in [0, 2^31)";
    if (nnz < 0 || nnz >= (int64_t)1 << 31) return "nnz must be in [0, 2^31)";
    if (n_pairs < 0 || n_pairs >= (int64_t)1 << 31) return "n_pairs must be in [0, 2^31)";
    if ((out_indices == nullptr) != (out_values == nullptr)) return "out_indices and out_values must both be given or both be NULL";
    if (out_indices && capacity < 0) return "capacity must be >= 0";
    if (n_pairs == 0 || nnz == 0) return nullptr;
    if (!indptr || !indices || !val || !parents || !out_indptr)
        return "indptr, indices, val, parents and out_indptr must not be NULL";
    return nullptr;
}
// The refusals of the matrix are those of csr_words.h under the prefix "doublets"; the pairs come behind them
inline std::string doublet_bad_parent(int64_t pair) { return "doublets: parents must be in [0, ncells); offending pair " + std::to_string(pair); }

}  // namespace schpf
