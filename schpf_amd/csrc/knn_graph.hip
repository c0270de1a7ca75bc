// Weighted neighbour graphs from k-NN lists (schpf_knn_graph / schpf_knn_graph_device): UMAP's fuzzy
// simplicial set ("connectivities") and the shared-neighbour Jaccard graph, as one symmetric CSR matrix.  The definition is
// in include/schpf_hip.h; host.cpp's serial restatement gives the same bits.
//
//   graph_row_kernel    one thread per row, 64 rows per workgroup staged through the LDS ([column][row]: coalesced loads,
//                       no bank asked twice): the checks of the row, its indices sorted (adjacent equal = repeated), and
//                       for `umap` rho, sigma by bisection and the k directed weights, every sum serial in column order
//   graph_keys_kernel   every directed edge i -> j twice: as entry (i, j) of the matrix with direction bit 0 and as entry
//                       (j, i) with direction bit 1, key = ((row * n + col) << 1) | bit, value = its weight
//   (rocPRIM radix sort of the 2 n k keys: the transpose and the merge in one; the two directions of a pair end up adjacent,
//   bit 0 first, and a row's columns ascend.  A hub's in-degree is nothing special: no list is ever held by one workgroup)
//   graph_heads_kernel  1 where a key starts a new (row, col); rocPRIM's exclusive scan of that is the place in the CSR
//   graph_fill_kernel   one thread per sorted key: a head writes its column, its value -- the union of the one or two
//                       weights, or the Jaccard ratio from the two sorted lists -- and, where a row starts, indptr
// No atomics but the checks' integer minima (device_call.h): who writes what is fixed by the sorted order.
#include <cfloat>
#include <climits>
#include <cmath>
#include <memory>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "device_call.h"
#include "kernels.h"
#include "special.h"

namespace schpf {
namespace {

constexpr int ROWS = 64;   // rows of a workgroup of the row pass: one wavefront

struct GraphRowArgs {
    const int32_t *idx;   // [n][k]
    const double *dist;   // [n][k]; nullptr: jaccard
    int n, k;
    double target;        // log2(k + 1)
    double *w;            // [n][k] directed weights, in the caller's column order (umap)
    double *rho, *sigma;  // [n] (umap)
    int32_t *sorted;      // [n][k] the row's indices ascending (jaccard; nullptr: not kept)
    unsigned long long *bad_idx, *bad_dist;   // two words of the call's record: the smallest offending row of each check
};

// W(e, s) of the definition
__device__ __forceinline__ double graph_weight(double e, double s)
{
    const double t = e / s;
    return t > 708.0 ? 0.0 : fast_exp(-t);
}

// LDS: 64 k doubles, first used as 64 k ints.  Element (row r of the workgroup, column j) lives at [j * 64 + r]: lane r
// walks its row at stride 64 -- the 64 lanes of every access hit consecutive addresses
__global__ __launch_bounds__(ROWS) void graph_row_kernel(GraphRowArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double graph_lds[];
    int *const li = reinterpret_cast<int *>(graph_lds);
    double *const ld = graph_lds;
    const int lane = threadIdx.x, n = a.n, k = a.k;
    const int row0 = blockIdx.x * ROWS, row = row0 + lane;
    const int rows = n - row0 < ROWS ? n - row0 : ROWS;
    const int total = rows * k;
    const size_t base = (size_t)row0 * (size_t)k;

    for (int t = lane; t < total; t += ROWS) {
        const int r = t / k, j = t - r * k;
        li[j * ROWS + r] = a.idx[base + t];
    }
    __syncthreads();
    unsigned long long bad = NONE;
    if (lane < rows) {
        bool wrong = false;
        for (int j = 0; j < k; ++j) {
            const int v = li[j * ROWS + lane];
            wrong |= v < 0 || v >= n || v == row;
        }
        for (int j = 1; j < k; ++j) {   // insertion sort of the row's own column of the LDS
            const int v = li[j * ROWS + lane];
            int b = j - 1;
            while (b >= 0 && li[b * ROWS + lane] > v) {
                li[(b + 1) * ROWS + lane] = li[b * ROWS + lane];
                --b;
            }
            li[(b + 1) * ROWS + lane] = v;
        }
        for (int j = 1; j < k; ++j) wrong |= li[j * ROWS + lane] == li[(j - 1) * ROWS + lane];
        if (wrong) offends(bad, row);
    }
    __syncthreads();
    if (a.sorted)
        for (int t = lane; t < total; t += ROWS) {
            const int r = t / k, j = t - r * k;
            a.sorted[base + t] = li[j * ROWS + r];
        }
    report_min(a.bad_idx, bad);   // the one wavefront of the workgroup is here: nothing returns before it
    if (!a.dist) return;
    __syncthreads();   // the indices have been read
    for (int t = lane; t < total; t += ROWS) {
        const int r = t / k, j = t - r * k;
        ld[j * ROWS + r] = a.dist[base + t];
    }
    __syncthreads();
    bad = NONE;
    if (lane < rows) {
        double rho = HUGE_VAL, sum = 0.0;
        bool wrong = false;
        for (int j = 0; j < k; ++j) {
            const double d = ld[j * ROWS + lane];
            wrong |= !(d >= 0.0 && d <= DBL_MAX);
            rho = d > 0.0 && d < rho ? d : rho;
            sum += d;
        }
        if (wrong) offends(bad, row);
        rho = rho == HUGE_VAL ? 0.0 : rho;
        double lo = 0.0, hi = HUGE_VAL, mid = 1.0;
        for (int round = 0; round < 64; ++round) {
            double psum = 0.0;
            for (int j = 0; j < k; ++j) {
                const double e = ld[j * ROWS + lane] - rho;
                psum += e > 0.0 ? graph_weight(e, mid) : 1.0;
            }
            if (fabs(psum - a.target) < 1e-5) break;
            if (psum > a.target) {
                hi = mid;
                mid = (lo + hi) / 2.0;
            } else {
                lo = mid;
                mid = hi == HUGE_VAL ? mid * 2.0 : (lo + hi) / 2.0;
            }
        }
        double sigma = mid;
        if (rho > 0.0) {
            const double mean = sum / (double)k;
            const double floor_ = 1e-3 * mean;
            sigma = sigma < floor_ ? floor_ : sigma;
        }
        for (int j = 0; j < k; ++j) {
            const double e = ld[j * ROWS + lane] - rho;
            ld[j * ROWS + lane] = e <= 0.0 ? 1.0 : graph_weight(e, sigma);
        }
        a.rho[row] = rho;
        a.sigma[row] = sigma;
    }
    __syncthreads();
    for (int t = lane; t < total; t += ROWS) {
        const int r = t / k, j = t - r * k;
        a.w[base + t] = ld[j * ROWS + r];
    }
    report_min(a.bad_dist, bad);
}

// edge e = i * k + j' of the validated lists -> the records 2 e (entry (i, j), bit 0) and 2 e + 1 (entry (j, i), bit 1)
__global__ __launch_bounds__(256) void graph_keys_kernel(const int32_t *__restrict__ idx, const double *__restrict__ w, int n,
                                                         int k, int64_t n_edges, uint64_t *__restrict__ key,
                                                         double *__restrict__ val)
{
    for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < n_edges; e += (int64_t)gridDim.x * 256) {
        const uint64_t i = (uint64_t)(e / k), j = (uint64_t)idx[e];
        key[2 * e] = (i * (uint64_t)n + j) << 1;
        key[2 * e + 1] = ((j * (uint64_t)n + i) << 1) | 1;
        if (val) {
            const double v = w[e];
            val[2 * e] = v;
            val[2 * e + 1] = v;
        }
    }
}

__global__ __launch_bounds__(256) void graph_heads_kernel(const uint64_t *__restrict__ key, int64_t n_keys,
                                                          int64_t *__restrict__ head)
{
    for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < n_keys; p += (int64_t)gridDim.x * 256)
        head[p] = p == 0 || (key[p] >> 1) != (key[p - 1] >> 1);
}

// |a ∩ b| of two ascending lists of k
__device__ __forceinline__ int shared_members(const int32_t *__restrict__ a, const int32_t *__restrict__ b, int k)
{
    int x = 0, y = 0, m = 0;
    int va = a[0], vb = b[0];
    while (true) {
        if (va == vb) {
            ++m;
            if (++x == k || ++y == k) break;
            va = a[x];
            vb = b[y];
        } else if (va < vb) {
            if (++x == k) break;
            va = a[x];
        } else {
            if (++y == k) break;
            vb = b[y];
        }
    }
    return m;
}

// pos[p]: heads before p.  A head at p is entry pos[p] of the CSR; a second record of the same (row, col) can only be
// the other direction (bit 1 behind bit 0: the lists hold no index twice).  Every row has its k outgoing edges, so every
// row has a first entry, and that one writes indptr[row]; the last record writes indptr[n].
// val: the weights (umap); sorted: the ascending lists (jaccard)
__global__ __launch_bounds__(256) void graph_fill_kernel(const uint64_t *__restrict__ key, const double *__restrict__ val,
                                                         const int64_t *__restrict__ pos, const int32_t *__restrict__ sorted,
                                                         int64_t n_keys, int n, int k, int64_t *__restrict__ indptr,
                                                         int32_t *__restrict__ indices, double *__restrict__ data)
{
    for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < n_keys; p += (int64_t)gridDim.x * 256) {
        const uint64_t mine = key[p], cell = mine >> 1;
        const bool head = p == 0 || (key[p - 1] >> 1) != cell;
        const int64_t o = pos[p];
        if (p == n_keys - 1) indptr[n] = o + (head ? 1 : 0);
        if (!head) continue;
        const uint64_t row = cell / (uint64_t)n, col = cell - row * (uint64_t)n;
        if (p == 0 || (key[p - 1] >> 1) / (uint64_t)n != row) indptr[row] = o;
        const bool both = p + 1 < n_keys && (key[p + 1] >> 1) == cell;
        const bool out = !(mine & 1), in = (mine & 1) || both;   // col in row's list; row in col's list
        indices[o] = (int32_t)col;
        if (val) {
            const double a = out ? val[p] : 0.0;
            const double b = !out ? val[p] : both ? val[p + 1] : 0.0;
            data[o] = fma(-a, b, a + b);
        } else {
            const int m = shared_members(sorted + row * (uint64_t)k, sorted + col * (uint64_t)k, k) + (out ? 1 : 0) + (in ? 1 : 0);
            data[o] = (double)m / (double)(2 * (k + 1) - m);
        }
    }
}

}  // namespace

hipError_t launch_graph_rows(const int32_t *idx, const double *dist, int n, int k, double target, double *w, double *rho,
                             double *sigma, int32_t *sorted, unsigned long long *bad_idx, unsigned long long *bad_dist,
                             hipStream_t st)
{
    if (n < 1 || k < 1 || k > 128) return hipErrorInvalidValue;
    const GraphRowArgs a{idx, dist, n, k, target, w, rho, sigma, sorted, bad_idx, bad_dist};
    hipLaunchKernelGGL(graph_row_kernel, dim3((unsigned)graph_row_blocks(n)), dim3(ROWS), graph_row_lds_bytes(k), st, a);
    return hipGetLastError();
}

hipError_t launch_graph_keys(const int32_t *idx, const double *w, int n, int k, uint64_t *key, double *val, hipStream_t st)
{
    const int64_t n_edges = (int64_t)n * k;
    hipLaunchKernelGGL(graph_keys_kernel, dim3(grid_for(n_edges)), dim3(256), 0, st, idx, w, n, k, n_edges, key, val);
    return hipGetLastError();
}

hipError_t launch_graph_heads(const uint64_t *key, int64_t n_keys, int64_t *head, hipStream_t st)
{
    hipLaunchKernelGGL(graph_heads_kernel, dim3(grid_for(n_keys)), dim3(256), 0, st, key, n_keys, head);
    return hipGetLastError();
}

hipError_t launch_graph_fill(const uint64_t *key, const double *val, const int64_t *pos, const int32_t *sorted, int64_t n_keys,
                             int n, int k, int64_t *indptr, int32_t *indices, double *data, hipStream_t st)
{
    if (!val == !sorted) return hipErrorInvalidValue;   // the weights or the sorted lists, one of them
    hipLaunchKernelGGL(graph_fill_kernel, dim3(grid_for(n_keys)), dim3(256), 0, st, key, val, pos, sorted, n_keys, n, k, indptr,
                       indices, data);
    return hipGetLastError();
}

namespace {

// Everything on `st`, which is synchronised when this returns; all pointers are device memory.  Nothing is written to the
// outputs when the lists are refused: the row pass writes scratch only
void graph_on_device(hipStream_t st, int method, int n, int k, const int32_t *idx, const double *dist, int64_t *indptr,
                     int32_t *indices, double *data, double *rho, double *sigma)
{
    const bool umap = method == SCHPF_GRAPH_UMAP;
    const size_t n_edges = (size_t)n * (size_t)k, n_keys = 2 * n_edges;
    DevBuf w, d_rho, d_sigma, sorted;
    enum { BAD_LISTS = 0, BAD_DISTANCES, BAD_COUNT };
    Offenders<BAD_COUNT> bad;
    bad.reset(st);
    if (umap) {
        w.alloc(n_edges * sizeof(double));
        d_rho.alloc((size_t)n * sizeof(double));
        d_sigma.alloc((size_t)n * sizeof(double));
    } else {
        sorted.alloc(n_edges * sizeof(int32_t));
    }
    HIPCHK(launch_graph_rows(idx, umap ? dist : nullptr, n, k, std::log2((double)(k + 1)), w.as<double>(), d_rho.as<double>(),
                             d_sigma.as<double>(), umap ? nullptr : sorted.as<int32_t>(), bad.dev() + BAD_LISTS,
                             bad.dev() + BAD_DISTANCES, st));
    bad.fetch(st);
    bad.refuse(BAD_LISTS, graph_bad_lists);
    bad.refuse(BAD_DISTANCES, graph_bad_distances);

    // the alternate buffers of the sort are free once it is done: the head flags and their scan go there
    DevBuf k_in, k_out, v_in, v_out, temp;
    k_in.alloc(n_keys * sizeof(uint64_t));
    k_out.alloc(n_keys * sizeof(uint64_t));
    v_in.alloc(n_keys * sizeof(double));   // jaccard: no weights to carry, but the scan's output
    if (umap) v_out.alloc(n_keys * sizeof(double));
    HIPCHK(launch_graph_keys(idx, w.as<double>(), n, k, k_in.as<uint64_t>(), umap ? v_in.as<double>() : nullptr, st));
    int end_bit = 1;   // of the largest key, 2 n^2 - 1
    while (end_bit < 64 && (((uint64_t)n * (uint64_t)n * 2 - 1) >> end_bit)) ++end_bit;
    size_t sort_bytes = 0, scan_bytes = 0;
    if (umap)
        HIPCHK(rocprim::radix_sort_pairs(nullptr, sort_bytes, k_in.as<uint64_t>(), k_out.as<uint64_t>(), v_in.as<double>(),
                                         v_out.as<double>(), n_keys, 0, end_bit, st));
    else
        HIPCHK(rocprim::radix_sort_keys(nullptr, sort_bytes, k_in.as<uint64_t>(), k_out.as<uint64_t>(), n_keys, 0, end_bit, st));
    HIPCHK(rocprim::exclusive_scan(nullptr, scan_bytes, k_in.as<int64_t>(), v_in.as<int64_t>(), (int64_t)0, n_keys,
                                   rocprim::plus<int64_t>(), st));
    temp.alloc(std::max(sort_bytes, scan_bytes));
    if (umap)
        HIPCHK(rocprim::radix_sort_pairs(temp.p, sort_bytes, k_in.as<uint64_t>(), k_out.as<uint64_t>(), v_in.as<double>(),
                                         v_out.as<double>(), n_keys, 0, end_bit, st));
    else
        HIPCHK(rocprim::radix_sort_keys(temp.p, sort_bytes, k_in.as<uint64_t>(), k_out.as<uint64_t>(), n_keys, 0, end_bit, st));
    HIPCHK(launch_graph_heads(k_out.as<uint64_t>(), (int64_t)n_keys, k_in.as<int64_t>(), st));
    HIPCHK(rocprim::exclusive_scan(temp.p, scan_bytes, k_in.as<int64_t>(), v_in.as<int64_t>(), (int64_t)0, n_keys,
                                   rocprim::plus<int64_t>(), st));
    HIPCHK(launch_graph_fill(k_out.as<uint64_t>(), umap ? v_out.as<double>() : nullptr, v_in.as<int64_t>(),
                             umap ? nullptr : sorted.as<int32_t>(), (int64_t)n_keys, n, k, indptr, indices, data, st));
    if (umap && rho) HIPCHK(hipMemcpyAsync(rho, d_rho.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (umap && sigma) HIPCHK(hipMemcpyAsync(sigma, d_sigma.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_knn_graph_device(int device, void *stream, int method, int n, int k, const int32_t *idx, const double *dist,
                           int64_t *indptr, int32_t *indices, double *data, double *rho, double *sigma)
{
    if (const char *why = graph_bad_args(method, n, k, idx, dist, indptr, indices, data)) return fail("%s", why);
    if (n == 0) return 0;
    return guarded([&] {
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        graph_on_device(st, method, n, k, idx, dist, indptr, indices, data, rho, sigma);
    });
}

int schpf_knn_graph(int device, int method, int n, int k, const int32_t *idx, const double *dist, int64_t *indptr,
                    int32_t *indices, double *data, double *rho, double *sigma)
{
    if (const char *why = graph_bad_args(method, n, k, idx, dist, indptr, indices, data)) return fail("%s", why);
    if (n == 0) return 0;
    return guarded([&] {
        use_device(device);
        const bool umap = method == SCHPF_GRAPH_UMAP;
        const size_t n_edges = (size_t)n * (size_t)k;
        TempStream ts;
        DevBuf d_idx, d_dist, d_indptr, d_indices, d_data, d_rho, d_sigma;
        h2d<int32_t>(d_idx, idx, n_edges, ts.st);
        if (umap) h2d<double>(d_dist, dist, n_edges, ts.st);
        d_indptr.alloc(((size_t)n + 1) * sizeof(int64_t));
        d_indices.alloc(2 * n_edges * sizeof(int32_t));
        d_data.alloc(2 * n_edges * sizeof(double));
        if (umap && rho) d_rho.alloc((size_t)n * sizeof(double));
        if (umap && sigma) d_sigma.alloc((size_t)n * sizeof(double));
        graph_on_device(ts.st, method, n, k, d_idx.as<int32_t>(), umap ? d_dist.as<double>() : nullptr, d_indptr.as<int64_t>(),
                        d_indices.as<int32_t>(), d_data.as<double>(), umap && rho ? d_rho.as<double>() : nullptr,
                        umap && sigma ? d_sigma.as<double>() : nullptr);
        d2h(indptr, d_indptr, ((size_t)n + 1) * sizeof(int64_t), ts.st);
        const size_t nnz = (size_t)indptr[n];
        HIPCHK(hipMemcpyAsync(indices, d_indices.p, nnz * sizeof(int32_t), hipMemcpyDeviceToHost, ts.st));
        if (umap && rho) HIPCHK(hipMemcpyAsync(rho, d_rho.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ts.st));
        if (umap && sigma) HIPCHK(hipMemcpyAsync(sigma, d_sigma.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ts.st));
        d2h(data, d_data, nnz * sizeof(double), ts.st);
    });
}

}  // extern "C"
