// Exact k nearest neighbours between two sets of rows in factor space (schpf_knn / schpf_knn_device).  For
// every query row the k smallest keys (d2, r) over the reference rows r, d2 = sum_k (query[q][k] - ref[r][k])^2 in double
// with one subtraction and one fused multiply-add per factor, in factor order -- host.cpp's serial restatement gives the
// same bits.  The key is a total order, so the result does not depend on how the pairs were walked or merged.
//
//   knn_table_kernel<T>  one side as doubles in the layout the tiles are staged from; the smallest row that holds a
//                        non-finite value goes to the side's word of the call's record (device_call.h)
//   knn_select_kernel    a workgroup owns a strip of 64 query rows and walks (a segment of) the reference rows in tiles of
//                        64; every thread owns 4 x 4 pairs; the k best keys of every row of the strip stay in the LDS
//   knn_merge_kernel     reference axis cut into segments (kernels.h knn_segments): the segments' lists of a row -> one
// No atomics but the check's integer minimum: who writes what is fixed by the indices.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>

#include "device_call.h"
#include "kernels.h"

namespace schpf {
namespace {

constexpr int QS = 64, RT = 64;   // query rows of a strip, reference rows of a tile

// [row / 64][k][row % 64]: the kc x 64 slab a tile stages is one contiguous run (as predictive.hip's E tables)
__device__ __forceinline__ size_t tab_index(int row, int k, int K)
{
    return ((size_t)(row >> 6) * (size_t)K + (size_t)k) * 64 + (size_t)(row & 63);
}

// the order of section 16: the smaller d2 first, equal d2 by the smaller row
__device__ __forceinline__ bool key_less(double ad, int ai, double bd, int bi) { return ad < bd || (ad == bd && ai < bi); }

// One thread per element of the padded table; *bad_row takes the smallest row with a NaN or an infinity.  No early return:
// every lane reaches report_min
template <typename T>
__global__ __launch_bounds__(256) void knn_table_kernel(const T *__restrict__ x, int n, int n_pad, int K,
                                                        double *__restrict__ tab, unsigned long long *__restrict__ bad_row)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long bad = NONE;
    if (i < (size_t)n_pad * (size_t)K) {
        const size_t q = i >> 6;
        const int k = (int)(q % (size_t)K);
        const int row = (int)(q / (size_t)K) * 64 + (int)(i & 63);
        double v = 0.0;
        if (row < n) {
            v = (double)x[(size_t)row * K + k];
            if (!(fabs(v) <= DBL_MAX)) offends(bad, row);
        }
        tab[i] = v;
    }
    report_min(bad_row, bad);
}

// One wavefront merges up to 64 candidates (one per lane, `valid`) into a row's sorted list ld2 / lidx[0 .. cnt) of
// capacity k <= 128, lane l holding the list's elements l and l + 64.  All keys differ (a reference row is offered once),
// so every key's place in the merged order is the count of keys ahead of it: an element moves back by the candidates ahead
// of it, a candidate lands behind the elements and the other candidates ahead of it.  Whatever lands at k or beyond is
// dropped; who lands at k - 1 is the row's new threshold.  Correct for any number of candidates, the cost grows with it.
// Returns the new length.
__device__ __forceinline__ int merge_wave(double *ld2, int *lidx, int cnt, int k, bool valid, double cd, int ci,
                                          double *thr_d, int *thr_i)
{
    const int lane = threadIdx.x & 63;
    const bool have0 = lane < cnt, have1 = lane + 64 < cnt;
    const double e0d = have0 ? ld2[lane] : 0.0, e1d = have1 ? ld2[lane + 64] : 0.0;
    const int e0i = have0 ? lidx[lane] : 0, e1i = have1 ? lidx[lane + 64] : 0;
    int s0 = 0, s1 = 0, cr = 0;
    const unsigned long long offered = __ballot(valid);
    for (unsigned long long m = offered; m; m &= m - 1) {
        const int b = __ffsll((long long)m) - 1;   // the same in every lane
        const double bd = __shfl(cd, b);
        const int bi = __shfl(ci, b);
        const bool l0 = have0 && key_less(e0d, e0i, bd, bi), l1 = have1 && key_less(e1d, e1i, bd, bi);
        const int ahead = __popcll(__ballot(l0)) + __popcll(__ballot(l1));   // elements ahead of candidate b
        s0 += have0 && !l0;
        s1 += have1 && !l1;
        if (lane == b) cr += ahead;
        else if (valid && key_less(bd, bi, cd, ci)) ++cr;
    }
    const int p0 = lane + s0, p1 = lane + 64 + s1;
    if (have0 && p0 < k) { ld2[p0] = e0d; lidx[p0] = e0i; }
    if (have1 && p1 < k) { ld2[p1] = e1d; lidx[p1] = e1i; }
    if (valid && cr < k) { ld2[cr] = cd; lidx[cr] = ci; }
    if (have0 && p0 == k - 1) { *thr_d = e0d; *thr_i = e0i; }
    if (have1 && p1 == k - 1) { *thr_d = e1d; *thr_i = e1i; }
    if (valid && cr == k - 1) { *thr_d = cd; *thr_i = ci; }
    const int total = cnt + __popcll(offered);
    return total < k ? total : k;
}

struct KnnArgs {
    const double *qtab, *rtab;
    int n_query, n_ref, K, k, kc;   // kc: factors staged per pass
    int seg_tiles, n_seg;           // tiles per segment of the reference axis; segments (grid.y)
    long long self_first;
    int32_t *idx;                   // [(q * n_seg + s) * k + j]
    double *d2;
    int *cnt;                       // [q * n_seg + s]; nullptr: one segment, every list is full
};

// rows first_row .. first_row + 64, factors k0 .. k0 + kc of a table -> dst[k][64]
__device__ __forceinline__ void stage(double *__restrict__ dst, const double *__restrict__ tab, int first_row, int k0, int kc,
                                      int K)
{
    for (int i = threadIdx.x; i < kc * 64; i += 256) dst[i] = tab[tab_index(first_row + (i & 63), k0 + (i >> 6), K)];
}

// 256 threads; thread (ty, tx) = (t / 16, t % 16) owns the query rows {2 ty, 2 ty + 1, 32 + 2 ty, 33 + 2 ty} of the strip and
// the reference rows {2 tx, 2 tx + 1, 32 + 2 tx, 33 + 2 tx} of the tile (predictive.hip's 64 x 64 shape: 16-byte operand
// reads, a lane group's covers one bank row or shares an address).
// Selection: a thread compares its 16 keys with the thresholds of its four rows (the k-th key so far; +inf while the list
// is short) and writes the few that pass to pend[row][reference row of the tile], which holds NaN wherever nothing was
// offered -- d2 of finite inputs is never NaN -- and raises the row's flag.  Wave w then merges the flagged rows of
// 16 w .. 16 w + 15, one row at a time, and puts the NaN back.  A list and a pending row are read and written by the 64
// lanes of one wave at consecutive addresses: no bank is asked twice in a lane group.
__global__ __launch_bounds__(256) void knn_select_kernel(KnnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double knn_lds[];
    const int k = a.k, K = a.K;
    double *const sm = knn_lds, *const sn = sm + QS * a.kc, *const pend = sn + RT * a.kc, *const ld2 = pend + QS * RT;
    double *const thr_d = ld2 + QS * k;
    int *const lidx = reinterpret_cast<int *>(thr_d + QS), *const thr_i = lidx + QS * k, *const cnt = thr_i + QS,
               *const flag = cnt + QS;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63, wave = t >> 6;
    const int row0 = blockIdx.x * QS, seg = blockIdx.y;
    const int a_lo = 2 * ty, a_hi = QS / 2 + 2 * ty, b_lo = 2 * tx, b_hi = RT / 2 + 2 * tx;
    const int qrow[4] = {a_lo, a_lo + 1, a_hi, a_hi + 1}, brow[4] = {b_lo, b_lo + 1, b_hi, b_hi + 1};
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    for (int i = t; i < QS * RT; i += 256) pend[i] = nan;
    if (t < QS) {
        thr_d[t] = HUGE_VAL;
        thr_i[t] = INT_MAX;
        cnt[t] = 0;
        flag[t] = 0;
    }
    const int m_begin = seg * a.seg_tiles * RT;
    const long long seg_end = ((long long)seg + 1) * a.seg_tiles * RT;
    const int m_end = seg_end < a.n_ref ? (int)seg_end : a.n_ref;
    // the reference row a query row may not take: itself (self_first >= 0), by index
    long long self[4];
    bool qok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        self[i] = a.self_first >= 0 ? a.self_first + row0 + qrow[i] : -1;
        qok[i] = row0 + qrow[i] < a.n_query;
    }
    const bool one_pass = K <= a.kc;   // the strip's own rows are then staged once
    if (one_pass) stage(sm, a.qtab, row0, 0, K, K);
    for (int m0 = m_begin; m0 < m_end; m0 += RT) {
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        for (int k0 = 0; k0 < K; k0 += a.kc) {
            const int kc = K - k0 < a.kc ? K - k0 : a.kc;
            __syncthreads();   // the last pass has been read, the last tile's merges are done
            if (!one_pass) stage(sm, a.qtab, row0, k0, kc, K);
            stage(sn, a.rtab, m0, k0, kc, K);
            __syncthreads();
#pragma unroll 2
            for (int kk = 0; kk < kc; ++kk) {
                const double2 a01 = *reinterpret_cast<const double2 *>(sm + kk * QS + a_lo);
                const double2 a23 = *reinterpret_cast<const double2 *>(sm + kk * QS + a_hi);
                const double2 b01 = *reinterpret_cast<const double2 *>(sn + kk * RT + b_lo);
                const double2 b23 = *reinterpret_cast<const double2 *>(sn + kk * RT + b_hi);
                const double qa[4] = {a01.x, a01.y, a23.x, a23.y}, rb[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double d = qa[i] - rb[j];
                        acc[i][j] = fma(d, d, acc[i][j]);
                    }
            }
        }
        // padding rows, rows of the next segment and the self pair never become candidates
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double td = thr_d[qrow[i]];
            const int ti = thr_i[qrow[i]];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = m0 + brow[j];
                if (qok[i] && r < m_end && (long long)r != self[i] && key_less(acc[i][j], r, td, ti)) {
                    pend[qrow[i] * RT + brow[j]] = acc[i][j];
                    flag[qrow[i]] = 1;
                }
            }
        }
        __syncthreads();
        const int f = lane < 16 ? flag[wave * 16 + lane] : 0;
        for (unsigned long long rows = __ballot(f != 0); rows; rows &= rows - 1) {
            const int q = wave * 16 + __ffsll((long long)rows) - 1;
            const double v = pend[q * RT + lane];
            const bool valid = v == v;
            if (valid) pend[q * RT + lane] = nan;
            const int n = merge_wave(ld2 + q * k, lidx + q * k, cnt[q], k, valid, v, m0 + lane, thr_d + q, thr_i + q);
            if (lane == 0) cnt[q] = n;
        }
        if (lane < 16) flag[wave * 16 + lane] = 0;
    }
    __syncthreads();
    for (int i = t; i < QS * k; i += 256) {
        const int q = i / k, j = i - q * k;
        if (row0 + q < a.n_query && j < cnt[q]) {
            const size_t o = ((size_t)(row0 + q) * a.n_seg + seg) * k + j;
            a.idx[o] = lidx[i];
            a.d2[o] = ld2[i];
        }
    }
    if (a.cnt && t < QS && row0 + t < a.n_query) a.cnt[(size_t)(row0 + t) * a.n_seg + seg] = cnt[t];
}

// One wavefront per query row: the sorted lists its segments left, 64 keys at a time through the same merge
__global__ __launch_bounds__(64) void knn_merge_kernel(const int32_t *__restrict__ part_idx, const double *__restrict__ part_d2,
                                                       const int *__restrict__ part_cnt, int n_seg, int k,
                                                       int32_t *__restrict__ idx, double *__restrict__ d2)
{
    __shared__ double ld2[128], thr_d;
    __shared__ int lidx[128], thr_i;
    const int lane = threadIdx.x;
    const size_t q = blockIdx.x;
    if (lane == 0) {
        thr_d = HUGE_VAL;
        thr_i = INT_MAX;
    }
    __syncthreads();
    int cnt = 0;
    for (int s = 0; s < n_seg; ++s) {
        const int c = part_cnt[q * n_seg + s];
        const size_t base = (q * n_seg + s) * k;
        for (int off = 0; off < c; off += 64) {
            const int j = off + lane;
            const double cd = j < c ? part_d2[base + j] : 0.0;
            const int ci = j < c ? part_idx[base + j] : 0;
            const bool valid = j < c && key_less(cd, ci, thr_d, thr_i);
            if (__ballot(valid)) cnt = merge_wave(ld2, lidx, cnt, k, valid, cd, ci, &thr_d, &thr_i);
            __syncthreads();
        }
    }
    for (int j = lane; j < cnt; j += 64) {
        idx[q * k + j] = lidx[j];
        d2[q * k + j] = ld2[j];
    }
}

}  // namespace

template <typename T>
hipError_t launch_knn_table(const T *x, int n, int K, double *tab, unsigned long long *bad_row, hipStream_t st)
{
    hipLaunchKernelGGL((knn_table_kernel<T>), dim3((unsigned)knn_table_blocks(n, K)), dim3(256), 0, st, x, n, knn_pad(n), K,
                       tab, bad_row);
    return hipGetLastError();
}

hipError_t launch_knn_select(const double *qtab, const double *rtab, int n_query, int n_ref, int K, int k,
                             int64_t self_first, int seg_tiles, int n_seg, int32_t *idx, double *d2, int *cnt, hipStream_t st)
{
    if (k < 1 || k > 128 || n_seg < 1 || n_seg > 65535 || (n_seg > 1 && !cnt)) return hipErrorInvalidValue;
    if ((int64_t)seg_tiles * n_seg < ((int64_t)n_ref + RT - 1) / RT) return hipErrorInvalidValue;   // rows left over
    const int kc = knn_stage_factors(k);
    const size_t lds = knn_lds_bytes(k, kc);
    if (lds > 64 * 1024) {   // opt in to the 160 KiB of a compute unit
        const hipError_t e = hipFuncSetAttribute((const void *)knn_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 160 * 1024);
        if (e != hipSuccess) return e;
    }
    const KnnArgs a{qtab, rtab, n_query, n_ref, K, k, kc, seg_tiles, n_seg, (long long)self_first, idx, d2, cnt};
    hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)((n_query + QS - 1) / QS), (unsigned)n_seg), dim3(256), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_knn_merge(const int32_t *part_idx, const double *part_d2, const int *part_cnt, int n_query, int n_seg,
                            int k, int32_t *idx, double *d2, hipStream_t st)
{
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)n_query), dim3(64), 0, st, part_idx, part_d2, part_cnt, n_seg, k, idx,
                       d2);
    return hipGetLastError();
}

template hipError_t launch_knn_table<float>(const float *, int, int, double *, unsigned long long *, hipStream_t);
template hipError_t launch_knn_table<double>(const double *, int, int, double *, unsigned long long *, hipStream_t);

namespace {

// $SCHPF_KNN_SPLIT, read once per call: unset = the rule of knn_segments; 0 or 1 = one segment; n >= 2 = n segments
int segments_wanted(int n_query, int n_ref, int device)
{
    const char *e = getenv("SCHPF_KNN_SPLIT");
    if (e && *e) return std::max(1, std::min(atoi(e), 1024));
    int cu_count = 0;
    HIPCHK(hipDeviceGetAttribute(&cu_count, hipDeviceAttributeMultiprocessorCount, device));
    return knn_segments(n_query, n_ref, cu_count);
}

// query / ref: n x K values of `dtype` in device memory (query == ref: one table serves both).  Everything on `st`,
// which is synchronised when this returns; nothing is written to idx / d2 when an input is refused.
void knn_on_device(int device, hipStream_t st, int dtype, int n_query, int n_ref, int K, const void *query, const void *ref,
                   int k, int64_t self_first, int32_t *idx, double *d2)
{
    const bool shared = query == ref && n_query == n_ref;
    DevBuf qtab, rtab;
    enum { BAD_QUERY = 0, BAD_REF, BAD_COUNT };
    Offenders<BAD_COUNT> w;
    w.reset(st);
    auto table = [&](const void *x, int n, DevBuf &tab, int side) {
        tab.alloc((size_t)knn_pad(n) * K * sizeof(double));
        if (dtype == SCHPF_F32) HIPCHK(launch_knn_table<float>((const float *)x, n, K, tab.as<double>(), w.dev() + side, st));
        else HIPCHK(launch_knn_table<double>((const double *)x, n, K, tab.as<double>(), w.dev() + side, st));
    };
    table(query, n_query, qtab, BAD_QUERY);
    if (!shared) table(ref, n_ref, rtab, BAD_REF);
    w.fetch(st);
    w.refuse(BAD_QUERY, [](int64_t row) { return "scores must be finite; offending row " + std::to_string(row) + " of query"; });
    w.refuse(BAD_REF, [](int64_t row) { return "scores must be finite; offending row " + std::to_string(row) + " of ref"; });
    const double *rt = shared ? qtab.as<double>() : rtab.as<double>();
    const int n_tiles = (n_ref + RT - 1) / RT;
    const int wanted = std::min(segments_wanted(n_query, n_ref, device), n_tiles);
    const int seg_tiles = (n_tiles + wanted - 1) / wanted;
    const int n_seg = (n_tiles + seg_tiles - 1) / seg_tiles;   // no segment is empty
    if (n_seg == 1) {
        HIPCHK(launch_knn_select(qtab.as<double>(), rt, n_query, n_ref, K, k, self_first, seg_tiles, 1, idx, d2, nullptr, st));
        HIPCHK(hipStreamSynchronize(st));
    } else {
        DevBuf pidx, pd2, pcnt;
        const size_t lists = (size_t)n_query * n_seg;
        pidx.alloc(lists * k * sizeof(int32_t));
        pd2.alloc(lists * k * sizeof(double));
        pcnt.alloc(lists * sizeof(int));
        HIPCHK(launch_knn_select(qtab.as<double>(), rt, n_query, n_ref, K, k, self_first, seg_tiles, n_seg, pidx.as<int32_t>(),
                                 pd2.as<double>(), pcnt.as<int>(), st));
        HIPCHK(launch_knn_merge(pidx.as<int32_t>(), pd2.as<double>(), pcnt.as<int>(), n_query, n_seg, k, idx, d2, st));
        HIPCHK(hipStreamSynchronize(st));   // before the partial lists are released
    }
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_knn_device(int device, void *stream, int dtype, int n_query, int n_ref, int nfactors, const void *query,
                     const void *ref, int k, int64_t self_first, int32_t *idx, double *d2)
{
    if (const char *why = knn_bad_args(dtype, n_query, n_ref, nfactors, query, ref, k, self_first, idx, d2)) return fail("%s", why);
    if (n_query == 0) return 0;
    return guarded([&] {
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        knn_on_device(device, st, dtype, n_query, n_ref, nfactors, query, ref, k, self_first, idx, d2);
    });
}

int schpf_knn(int device, int dtype, int n_query, int n_ref, int nfactors, const void *query, const void *ref, int k,
              int64_t self_first, int32_t *idx, double *d2)
{
    if (const char *why = knn_bad_args(dtype, n_query, n_ref, nfactors, query, ref, k, self_first, idx, d2)) return fail("%s", why);
    if (n_query == 0) return 0;
    return guarded([&] {
        use_device(device);
        const size_t elem = dtype == SCHPF_F32 ? 4 : 8, out = (size_t)n_query * k;
        const bool shared = query == ref && n_query == n_ref;
        TempStream ts;
        DevBuf d_query, d_ref, d_idx, d_d2;
        h2d<char>(d_query, query, (size_t)n_query * nfactors * elem, ts.st);
        if (!shared) h2d<char>(d_ref, ref, (size_t)n_ref * nfactors * elem, ts.st);
        d_idx.alloc(out * sizeof(int32_t));
        d_d2.alloc(out * sizeof(double));
        knn_on_device(device, ts.st, dtype, n_query, n_ref, nfactors, d_query.p, shared ? d_query.p : d_ref.p, k, self_first,
                      d_idx.as<int32_t>(), d_d2.as<double>());
        HIPCHK(hipMemcpyAsync(idx, d_idx.p, out * sizeof(int32_t), hipMemcpyDeviceToHost, ts.st));
        d2h(d2, d_d2, out * sizeof(double), ts.st);
    });
}

}  // extern "C"
