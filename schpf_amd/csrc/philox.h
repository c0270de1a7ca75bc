// Count thinning: the counter-based generator and the draw of one entry, in integer arithmetic only, so
// that the kernels of thin.hip and the serial restatement of host.cpp (schpf_debug_thin_counts) give the same bits.
// Like special.h, plain C++ that compiles for the host and for the device.
//
// Generator: Philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
// SC'11).  Draw of the entry (row, col, x) under (seed, T): key = (low, high word of seed); block j =
// philox((row, col, j, 0), key); trial t < x reads word t % 4 of block t / 4 and goes to the test matrix iff that word
// < T, with T = floor(frac * 2^32) computed once on the host (thin_threshold).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SCHPF_PX __host__ __device__ __forceinline__
#else
#define SCHPF_PX inline
#endif

namespace schpf {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr double THIN_MAX_COUNT = 16777216.0;   // 2^24: float32 holds every count up to here, and a draw stays bounded
constexpr uint32_t THIN_LIGHT_MAX = 256;        // counts up to here (64 draw blocks) are drawn by one lane

struct Philox4 {
    uint32_t w[4];
};

SCHPF_PX Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// an index thinning accepts: in [0, 2^31) (an int64 beyond int32 is out of range, as in schpf_upload_coo_device)
SCHPF_PX bool thin_index_bad(long long i) { return i < 0 || i > 0x7fffffffLL; }
// a value thinning accepts: a non-negative integer <= 2^24 (NaN fails the first comparison)
SCHPF_PX bool thin_value_bad(double d) { return !(d >= 0.0 && d <= THIN_MAX_COUNT) || d != (double)(uint32_t)d; }

// how many of the trials 4j .. min(4j + 3, x - 1) of entry (row, col) go to the test matrix
SCHPF_PX uint32_t thin_block_hits(uint32_t row, uint32_t col, uint32_t j, uint32_t x, uint32_t k0, uint32_t k1, uint32_t T)
{
    const Philox4 b = philox4x32_10(row, col, j, 0u, k0, k1);
    const uint32_t left = x - 4u * j;   // trials from 4j on: >= 1 for every block of the entry
    uint32_t hits = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) hits += (w < left && b.w[w] < T) ? 1u : 0u;
    return hits;
}

// x_test of one VALIDATED entry, block after block: what a lane of the light pass and the host restatement run
SCHPF_PX uint32_t thin_draw(uint32_t row, uint32_t col, uint32_t x, uint32_t k0, uint32_t k1, uint32_t T)
{
    uint32_t hits = 0;
    const uint32_t n_blocks = (x + 3u) >> 2;
    for (uint32_t j = 0; j < n_blocks; ++j) hits += thin_block_hits(row, col, j, x, k0, k1, T);
    return hits;
}

// T = floor(frac * 2^32) for 0 < frac < 1 (the product is exact: a power of two); false if frac is outside (0, 1), NaN,
// or so small that T would be 0
inline bool thin_threshold(double frac, uint32_t *T)
{
    if (!(frac > 0.0 && frac < 1.0)) return false;
    const double scaled = frac * 4294967296.0;   // < 2^32: the largest double below 1 gives 2^32 - 2^-21
    if (scaled < 1.0) return false;
    *T = (uint32_t)scaled;
    return true;
}

}  // namespace schpf
