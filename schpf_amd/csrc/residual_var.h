// What residual_var.hip and host.cpp share: the refusals of schpf_residual_var, schpf_residual_var_device and
// schpf_debug_residual_var in their words and their order, the test of a stored value, and the two expressions of the
// definition every restatement evaluates alike -- a gene's share q_g and the bound on inv_theta below which the kernels
// may take the reciprocal of 1 + mu inv_theta with fast_rcp.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#if defined(__HIPCC__)
#define SCHPF_HVG_FN __host__ __device__ __forceinline__
#else
#define SCHPF_HVG_FN inline
#endif

namespace schpf {

// Refused before anything is read, in this order; N = 0 or J = 0 is asked next by the caller.  nullptr: the arguments are fine
inline const char *hvg_bad_args(int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr, const void *indices,
                                const void *data, double inv_theta, double clip, const void *sum, const void *sumsq)
{
    const int64_t limit = (int64_t)1 << 31;
    if (ncells < 0 || ncells >= limit || ngenes < 0 || ngenes >= limit || nnz < 0 || nnz >= limit)
        return "hvg: ncells, ngenes and nnz must be in [0, 2^31)";
    if (!(inv_theta >= 0.0 && inv_theta <= 1.7976931348623157e308)) return "hvg: inv_theta must be finite and >= 0";
    if (!(clip > 0.0)) return "hvg: clip must be > 0";
    if (ngenes > 0 && (!sum || !sumsq)) return "hvg: sum and sumsq must not be NULL";
    if (ngenes > 0 && !indptr) return "hvg: indptr must not be NULL";
    if (nnz > 0 && (!indices || !data)) return "hvg: indices and data must not be NULL";
    return nullptr;
}
inline std::string hvg_bad_indptr(int64_t gene)
{
    return "hvg: indptr must be 0 at gene 0, must be non-decreasing and must end at nnz; offending gene " + std::to_string(gene);
}
inline std::string hvg_bad_cells(int64_t gene)
{
    return "hvg: cell ids must be in [0, ncells) and strictly ascending within a gene; offending gene " + std::to_string(gene);
}
inline std::string hvg_bad_values(int64_t gene)
{
    return "hvg: values must be integer counts in [0, 2^24]; offending gene " + std::to_string(gene);
}

// A stored value as a count: true and the count if it is an integer in [0, 2^24] (-0.0 is 0).  By the bits, so that no
// denormal mode has a say: a denormal is refused on the host and on the device alike
SCHPF_HVG_FN bool hvg_count(float value, int64_t &count)
{
    uint32_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
    bits = __float_as_uint(value);
#else
    std::memcpy(&bits, &value, 4);
#endif
    count = 0;
    if (bits == 0u || bits == 0x80000000u) return true;
    if (bits < 0x3f800000u || bits > 0x4b800000u) return false;     // below 1, above 2^24, negative, inf or nan
    const int shift = 150 - (int)(bits >> 23);                      // the fraction bits of the mantissa: 23 at 1, 0 from 2^23 up
    const uint32_t mant = (bits & 0x7fffffu) | 0x800000u;
    if (shift > 0 && (mant & ((1u << shift) - 1u))) return false;
    count = shift >= 0 ? (int64_t)(mant >> shift) : (int64_t)mant << -shift;
    return true;
}

// q_g = s_g / T, 0 where nothing was counted
SCHPF_HVG_FN double hvg_share(int64_t gene_total, int64_t total) { return total > 0 ? (double)gene_total / (double)total : 0.0; }

// mu = n_c q_g is at most 2^55.  Up to this inv_theta, 1 + mu inv_theta and mu (1 + mu inv_theta) are normal numbers with
// normal reciprocals -- the domain of fast_rcp (special.h); above it the kernels divide
constexpr double HVG_FAST_INV_THETA = 0x1p900;

}  // namespace schpf
