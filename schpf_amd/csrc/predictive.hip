// Posterior predictive row sums over ALL (cell, gene) pairs: with lambda_rm = sum_k E_major[r][k] *
// E_minor[m][k], per major row r the three sums over every minor row m
//     zeros[r] = sum_m exp(-lambda_rm),   rate[r] = sum_m lambda_rm,   rate2[r] = sum_m lambda_rm^2.
// The only pass of the library that is dense in both axes: no plan, no count matrix, nothing of the sweeps.
//
// Two steps, all arithmetic in double from the stored shape / rate in both model dtypes (as elbo_gamma_kernel):
//   predictive_e_kernel<T>   E = shape / rate of one side as doubles, in the layout the tiles are staged from
//   predictive_rows_kernel   a workgroup owns a strip of MAJ major rows and walks the minor rows in tiles of MIN;
//                            every thread owns 4 x 4 pairs; no atomics, no partial sums outside the workgroup
#include <cfloat>

#include "kernels.h"
#include "special.h"

namespace schpf {
namespace {

constexpr int KC = 32;   // factors staged per pass over a tile: (MAJ + MIN) * KC doubles of LDS

// The E table of a side: blocks of 64 rows, inside a block factor-major -- [row / 64][k][row % 64] -- so that the KC x 64
// slab a tile stages is one contiguous run, read coalesced and written to the LDS without a transpose.  Rows are padded
// to predictive_pad(n) with E = 0 (lambda = 0: nothing for rate and rate2; zeros masks them)
__device__ __forceinline__ size_t etab_index(int row, int k, int K)
{
    return ((size_t)(row >> 6) * (size_t)K + (size_t)k) * 64 + (size_t)(row & 63);
}

// One thread per element of the padded table.  An E that overflows is held at DBL_MAX: 0 * inf would be the only way
// to a NaN further down (every term is >= 0, so inf - inf cannot happen)
template <typename T>
__global__ __launch_bounds__(256) void predictive_e_kernel(const T *__restrict__ shape, const T *__restrict__ rate, int n,
                                                           int n_pad, int K, double *__restrict__ etab)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n_pad * (size_t)K) return;
    const size_t q = i >> 6;
    const int k = (int)(q % (size_t)K);
    const int row = (int)(q / (size_t)K) * 64 + (int)(i & 63);
    double e = 0.0;
    if (row < n) {
        e = (double)shape[(size_t)row * K + k] / (double)rate[(size_t)row * K + k];
        e = e < DBL_MAX ? e : DBL_MAX;
    }
    etab[i] = e;
}

// rows first_row .. first_row + WIDTH, factors k0 .. k0 + kc of a table -> dst[k][WIDTH]
template <int WIDTH>
__device__ __forceinline__ void stage(double *__restrict__ dst, const double *__restrict__ tab, int first_row, int k0, int kc,
                                      int K)
{
    for (int i = threadIdx.x; i < kc * WIDTH; i += 256) dst[i] = tab[etab_index(first_row + (i % WIDTH), k0 + i / WIDTH, K)];
}

// 256 threads; thread (ty, tx) = (t / TPR, t % TPR) owns the major rows {2 ty, 2 ty + 1} of both halves of the strip and
// the minor rows {2 tx, 2 tx + 1} of both halves of the tile: its four operand reads per factor are 16-byte reads, the
// 16 lanes of a read's lane group cover one 256-byte bank row (minor side) or share an address (major side).
// K > KC: the factors go through the LDS in passes of KC, the 16 accumulators stay in registers across the passes.
// out = [zeros | rate | rate2], n_major doubles each.
template <int MAJ>
__global__ __launch_bounds__(256) void predictive_rows_kernel(const double *__restrict__ e_major,
                                                              const double *__restrict__ e_minor, int n_major, int n_minor,
                                                              int K, double *__restrict__ out)
{
    constexpr int TPR = 256 / (MAJ / 4), MIN = 4 * TPR;
    static_assert(MAJ >= 32 && MAJ <= 64 && MIN <= 128, "tiles must stay inside the table's padding (predictive_pad)");
    static_assert(3 * MAJ * TPR <= (MAJ + MIN) * KC && 3 * MAJ <= 256, "the final reduction reuses the staging LDS");
    __shared__ __attribute__((aligned(16))) double lds[(MAJ + MIN) * KC];
    double *const sm = lds, *const sn = lds + MAJ * KC;
    const int t = threadIdx.x, tx = t % TPR, ty = t / TPR;
    const int row0 = blockIdx.x * MAJ;
    const int a_lo = 2 * ty, a_hi = MAJ / 2 + 2 * ty, b_lo = 2 * tx, b_hi = MIN / 2 + 2 * tx;
    const bool one_pass = K <= KC;   // the strip's own rows are then staged once
    double z[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (one_pass) stage<MAJ>(sm, e_major, row0, 0, K, K);
    for (int m0 = 0; m0 < n_minor; m0 += MIN) {
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        for (int k0 = 0; k0 < K; k0 += KC) {
            const int kc = K - k0 < KC ? K - k0 : KC;
            __syncthreads();   // the last pass has been read
            if (!one_pass) stage<MAJ>(sm, e_major, row0, k0, kc, K);
            stage<MIN>(sn, e_minor, m0, k0, kc, K);
            __syncthreads();
#pragma unroll 2
            for (int k = 0; k < kc; ++k) {
                const double2 a01 = *reinterpret_cast<const double2 *>(sm + k * MAJ + a_lo);
                const double2 a23 = *reinterpret_cast<const double2 *>(sm + k * MAJ + a_hi);
                const double2 b01 = *reinterpret_cast<const double2 *>(sn + k * MIN + b_lo);
                const double2 b23 = *reinterpret_cast<const double2 *>(sn + k * MIN + b_hi);
                const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
            }
        }
        // a tile that sticks out: its padding rows have lambda = 0, which only the zeros would see
        const bool in[4] = {m0 + b_lo < n_minor, m0 + b_lo + 1 < n_minor, m0 + b_hi < n_minor, m0 + b_hi + 1 < n_minor};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double l = acc[i][j];
                const double e = fast_exp(-l);   // special.h: 1 at 0, 0 from 746 on (and at inf), 2 ulp between
                z[i] += in[j] ? e : 0.0;
                s1[i] += l;
                s2[i] = fma(l, l, s2[i]);
            }
    }
    // the TPR threads that share a major row, summed in thread order by one thread per (sum, row)
    __syncthreads();
    double *const red = lds;   // [3][MAJ][TPR]
    const int mine[4] = {a_lo, a_lo + 1, a_hi, a_hi + 1};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        red[(0 * MAJ + mine[i]) * TPR + tx] = z[i];
        red[(1 * MAJ + mine[i]) * TPR + tx] = s1[i];
        red[(2 * MAJ + mine[i]) * TPR + tx] = s2[i];
    }
    __syncthreads();
    if (t < 3 * MAJ) {
        const int which = t / MAJ, r = t % MAJ;
        if (row0 + r < n_major) {
            const double *p = red + (which * MAJ + r) * TPR;
            double s = 0.0;
            for (int q = 0; q < TPR; ++q) s += p[q];
            out[(size_t)which * n_major + row0 + r] = s;
        }
    }
}

}  // namespace

template <typename T>
hipError_t launch_predictive_e(const T *shape, const T *rate, int n, int K, double *etab, hipStream_t st)
{
    const int n_pad = predictive_pad(n);
    const size_t total = (size_t)n_pad * (size_t)K;
    hipLaunchKernelGGL((predictive_e_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, shape, rate, n,
                       n_pad, K, etab);
    return hipGetLastError();
}

hipError_t launch_predictive_rows(const double *e_major, const double *e_minor, int n_major, int n_minor, int K, int strip,
                                  double *out, hipStream_t st)
{
    const dim3 grid((unsigned)((n_major + strip - 1) / strip)), block(256);
    if (strip == 64) hipLaunchKernelGGL((predictive_rows_kernel<64>), grid, block, 0, st, e_major, e_minor, n_major, n_minor, K, out);
    else if (strip == 32) hipLaunchKernelGGL((predictive_rows_kernel<32>), grid, block, 0, st, e_major, e_minor, n_major, n_minor, K, out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template hipError_t launch_predictive_e<float>(const float *, const float *, int, int, double *, hipStream_t);
template hipError_t launch_predictive_e<double>(const double *, const double *, int, int, double *, hipStream_t);

}  // namespace schpf
