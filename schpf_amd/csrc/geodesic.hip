// Exact shortest-path distances from sets of root vertices (schpf_geodesic*).  The distance is defined in
// include/schpf_hip.h as the greatest solution of d[root] = 0, d[v] = min over edges (u, v) of fl(d[u] + w_uv), one set of
// doubles, and restated in host.cpp as a serial Dijkstra; the bits are the same on every schedule.  The graph is read as
// components.hip reads it (graph_device.h): the row of every entry by bisection, one thread per entry.
//
// Root sets are processed in tiles of ROOT_TILE.  Inside a tile the working distances are vertex-major, work[v * TW + t], as
// the uint64 bit patterns of the doubles: doubles >= +0 order the way their bit patterns do and +inf is the largest.  TW is
// the tile's width, the smallest of 1, 2, 4, ROOT_TILE that holds the sets left; a column without a set stays at +inf.
//   (graph_device.h: the columns, the values and set_ptr; every check leaves its smallest offender in a word of the call's
//   one record, device_call.h: one fetch for the graph and set_ptr, one for the roots)
//   geodesic_roots_check_kernel  roots[e] in [0, n): the smallest offending set
//   geodesic_init_kernel         work = +inf, stamp = 0;  geodesic_roots_kernel: work[root * TW + t] = +0
//   geodesic_relax_kernel        round r, one thread per stored entry (i, j, w), j != i: both endpoints' lines are read past
//                                the L1; for each column t, cand = d[i] + w (one double add) goes to atomicMin(work[j]) only
//                                where it is below the value seen, and an undirected graph does the same from j to i.  A
//                                thread that sent a minimum raises flag[r]; a vertex that was lowered is stamped with r; a
//                                filtered round skips a direction whose source was not stamped in round r - 1 or r.  A round
//                                returns at once when the round before it in the batch raised nothing
//   The host launches ROUND_BATCH rounds and fetches their flags once.  After a filtered round that raised nothing it runs
//   an UNFILTERED round, and only such a round that raises nothing ends the loop: then d[j] <= fl(d[i] + w) holds on every
//   edge, whatever the filter skipped.  Every stored value is the fl-sum along a real path from a root, so it is never below
//   the fixed point; values only fall; the fixed point reached from +inf is the greatest one.
//   geodesic_transpose_kernel    the tile into the caller's root-major dist, and the finite entries (one integer add per
//                                wavefront of a bounded grid); the lowering writes are kept per wavefront without an atomic
#include <cfloat>
#include <climits>
#include <cmath>
#include <memory>
#include <string>

#include "common.h"
#include "graph_device.h"

namespace schpf {
namespace {

constexpr int ROOT_TILE = 8;         // root sets per tile: a vertex's 8 distances are one 64-byte line (schpf_amd.paths.ROOT_TILE)
constexpr int ROUND_BATCH = 16;      // rounds launched between two fetches of the flags
constexpr int RELAX_BLOCKS = 2048;   // workgroups of a round at the most: 8 wavefronts per SIMD of 256 CUs
constexpr int COUNT_BLOCKS = 1024;
constexpr unsigned long long INF_BITS = 0x7ff0000000000000ull;

// the smallest offenders of a call, in the order they are asked
enum { BAD_COLUMNS = 0, BAD_VALUES, BAD_SET_PTR, BAD_ROOTS, BAD_COUNT };

typedef unsigned long long bits_t;

__device__ __forceinline__ bits_t wave_sum(bits_t v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ bits_t load_past_l1(const bits_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(256) void geodesic_roots_check_kernel(const int32_t *__restrict__ roots, const int32_t *__restrict__ setof,
                                                                   int n, int64_t nroots, unsigned long long *__restrict__ word)
{
    unsigned long long bad = NONE;
    GRID_STRIDE(e, nroots)
    {
        if (roots[e] < 0 || roots[e] >= n) offends(bad, setof[e]);
    }
    report_min(word, bad);
}

__global__ __launch_bounds__(256) void geodesic_init_kernel(int64_t n, int64_t cells, bits_t *__restrict__ work, int *__restrict__ stamp)
{
    GRID_STRIDE(c, cells)
    {
        work[c] = INF_BITS;
        if (c < n) stamp[c] = 0;
    }
}

// the roots of the sets set0 .. set0 + tw - 1: the entries [from, to) of `roots`; setof[e] is the set of entry e
__global__ __launch_bounds__(256) void geodesic_roots_kernel(const int32_t *__restrict__ roots, const int32_t *__restrict__ setof,
                                                             int64_t from, int64_t to, int set0, int TW, bits_t *__restrict__ work)
{
    GRID_STRIDE(x, to - from)
    {
        const int64_t e = from + x;
        work[(int64_t)roots[e] * TW + (setof[e] - set0)] = 0;   // +0.0
    }
}

template <int TW, bool directed>
__global__ __launch_bounds__(256) void geodesic_relax_kernel(const int32_t *__restrict__ rowof, const int32_t *__restrict__ indices,
                                                             const double *__restrict__ data, int64_t nnz, bits_t *work, int *stamp,
                                                             int round, bool filtered, const int *before, int *flag,
                                                             bits_t *__restrict__ writes)
{
    if (before && *before == 0) return;   // the round before raised nothing: neither would this one
    bits_t mine = 0;
    bool sent = false;
    GRID_STRIDE(e, nnz)
    {
        const int i = rowof[e], j = indices[e];
        if (i == j) continue;
        bool fwd = true, bwd = !directed;
        if (filtered) {
            fwd = stamp[i] >= round - 1;
            bwd = !directed && stamp[j] >= round - 1;
            if (!fwd && !bwd) continue;
        }
        const double w = data ? data[e] : 1.0;
        bits_t *const wi = work + (int64_t)i * TW, *const wj = work + (int64_t)j * TW;
        bits_t di[TW], dj[TW];
#pragma unroll
        for (int t = 0; t < TW; ++t) di[t] = load_past_l1(wi + t);
#pragma unroll
        for (int t = 0; t < TW; ++t) dj[t] = load_past_l1(wj + t);
        bool low_i = false, low_j = false;
#pragma unroll
        for (int t = 0; t < TW; ++t) {
            // di + w < dj and dj + w < di cannot both hold: at most one direction sends for a column
            if (fwd && di[t] != INF_BITS) {
                const bits_t cand = (bits_t)__double_as_longlong(__longlong_as_double((long long)di[t]) + w);   // overflow: +inf, never lower
                if (cand < dj[t]) {
                    sent = true;
                    if (atomicMin(wj + t, cand) > cand) {
                        ++mine;
                        low_j = true;
                    }
                }
            }
            if (bwd && dj[t] != INF_BITS) {
                const bits_t cand = (bits_t)__double_as_longlong(__longlong_as_double((long long)dj[t]) + w);
                if (cand < di[t]) {
                    sent = true;
                    if (atomicMin(wi + t, cand) > cand) {
                        ++mine;
                        low_i = true;
                    }
                }
            }
        }
        // every writer of a round writes the same number; a reader that misses it this round sees it in the next
        if (low_j) stamp[j] = round;
        if (low_i) stamp[i] = round;
    }
    if (sent) *flag = 1;
    mine = wave_sum(mine);   // every lane is here: `continue` goes on to the next entry, nothing leaves the loop early
    if ((threadIdx.x & 63) == 0 && mine) writes[blockIdx.x * 4 + (threadIdx.x >> 6)] += mine;   // this wavefront's own word
}

// dist[(set0 + t) * n + v] = work[v * TW + t] for the tw sets of the tile; words[0] += the finite ones
__global__ __launch_bounds__(256) void geodesic_transpose_kernel(int64_t n, int TW, int tw, const bits_t *__restrict__ work,
                                                                 double *__restrict__ dist, bits_t *__restrict__ words)
{
    bits_t finite = 0;
    GRID_STRIDE(v, n)
    {
        for (int t = 0; t < tw; ++t) {
            const bits_t b = work[v * TW + t];
            dist[(int64_t)t * n + v] = __longlong_as_double((long long)b);
            finite += b != INF_BITS ? 1 : 0;
        }
    }
    finite = wave_sum(finite);
    if ((threadIdx.x & 63) == 0 && finite) atomicAdd(words, finite);
}

__global__ __launch_bounds__(256) void geodesic_writes_kernel(const bits_t *__restrict__ writes, bits_t *__restrict__ words)
{
    bits_t mine = 0;
    for (int x = threadIdx.x; x < RELAX_BLOCKS * 4; x += 256) mine += writes[x];
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(words + 1, mine);
}

template <int TW>
void launch_round(hipStream_t st, bool directed, const int32_t *rowof, const int32_t *indices, const double *data, int64_t nnz,
                  bits_t *work, int *stamp, int round, bool filtered, const int *before, int *flag, bits_t *writes)
{
    if (directed)
        LAUNCH_BOUNDED((geodesic_relax_kernel<TW, true>), nnz, RELAX_BLOCKS, st, rowof, indices, data, nnz, work, stamp, round,
                       filtered, before, flag, writes);
    else
        LAUNCH_BOUNDED((geodesic_relax_kernel<TW, false>), nnz, RELAX_BLOCKS, st, rowof, indices, data, nnz, work, stamp, round,
                       filtered, before, flag, writes);
}

int tile_width(int sets)   // the smallest of 1, 2, 4, ROOT_TILE that holds them
{
    int w = 1;
    while (w < sets && w < ROOT_TILE) w <<= 1;
    return w;
}

// Everything on `st`, which is synchronised when this returns; indptr has been checked, every pointer but stats is device
// memory.  dist is written after the last check: a refused call leaves it alone
void geodesic_on_device(hipStream_t st, int n, int64_t nnz, const int64_t *indptr, const int32_t *indices, const double *data,
                        bool directed, int nsets, const int64_t *set_ptr, const int32_t *roots, double *dist, int64_t *stats)
{
    DevBuf rowof;
    Offenders<BAD_COUNT> w;
    w.reset(st);
    if (nnz > 0) {
        rowof.alloc((size_t)nnz * sizeof(int32_t));
        LAUNCH(entry_rows_kernel, nnz, st, indptr, (int64_t)n, nnz, rowof.as<int32_t>());
        LAUNCH(graph_entries_check_kernel<false>, nnz, st, indptr, indices, data, rowof.as<int32_t>(), n, nnz, w.dev() + BAD_COLUMNS,
               w.dev() + BAD_VALUES);
    }
    // set_ptr is an indptr over the sets: the same kernel, other words.  Not through indptr_on_device: its verdict is asked
    // behind the graph's, and all of it comes to the host with the one fetch, not its last entry alone
    LAUNCH(indptr_check_kernel, nsets, st, set_ptr, nsets, w.dev() + BAD_SET_PTR);
    std::vector<int64_t> h_set_ptr((size_t)nsets + 1);
    HIPCHK(hipMemcpyAsync(h_set_ptr.data(), set_ptr, h_set_ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    w.fetch(st);
    w.refuse(BAD_COLUMNS, graph_bad_columns);
    w.refuse(BAD_VALUES, louvain_bad_values);
    w.refuse(BAD_SET_PTR, geodesic_bad_set_ptr);
    const int64_t nroots = h_set_ptr[(size_t)nsets];
    if (nroots > 0 && !roots) throw std::invalid_argument("roots must not be NULL");
    DevBuf setof;
    if (nroots > 0) {
        setof.alloc((size_t)nroots * sizeof(int32_t));
        LAUNCH(entry_rows_kernel, nroots, st, set_ptr, (int64_t)nsets, nroots, setof.as<int32_t>());
        LAUNCH(geodesic_roots_check_kernel, nroots, st, roots, setof.as<int32_t>(), n, nroots, w.dev() + BAD_ROOTS);
        w.fetch(st);
        w.refuse(BAD_ROOTS, geodesic_bad_roots);
    }

    const int widest = tile_width(nsets);
    DevBuf work, stamp, flags, writes, words;
    work.alloc((size_t)n * (size_t)widest * sizeof(bits_t));
    stamp.alloc((size_t)n * sizeof(int));
    flags.alloc(ROUND_BATCH * sizeof(int));
    writes.alloc((size_t)RELAX_BLOCKS * 4 * sizeof(bits_t), true, st);
    words.alloc(2 * sizeof(bits_t), true, st);
    int64_t rounds = 0;
    for (int set0 = 0; set0 < nsets; set0 += ROOT_TILE) {
        const int tw = std::min(ROOT_TILE, nsets - set0), TW = tile_width(tw);
        const int64_t cells = (int64_t)n * TW;
        LAUNCH(geodesic_init_kernel, cells, st, (int64_t)n, cells, work.as<bits_t>(), stamp.as<int>());
        const int64_t from = h_set_ptr[(size_t)set0], to = h_set_ptr[(size_t)(set0 + tw)];
        if (to > from) LAUNCH(geodesic_roots_kernel, to - from, st, roots, setof.as<int32_t>(), from, to, set0, TW, work.as<bits_t>());
        if (nnz > 0 && to > from) {
            int h_flags[ROUND_BATCH];
            int round = 1;
            // verify: the batch opens with an unfiltered round, and the loop ends when that round raises nothing
            for (bool verify = false, done = false; !done;) {
                HIPCHK(hipMemsetAsync(flags.p, 0, sizeof h_flags, st));
                for (int b = 0; b < ROUND_BATCH; ++b) {
                    const bool filtered = !(b == 0 && verify);
                    const int *before = b ? flags.as<int>() + b - 1 : nullptr;
                    int *flag = flags.as<int>() + b;
                    bits_t *const W = work.as<bits_t>();
                    int *const S = stamp.as<int>();
                    const int32_t *R = rowof.as<int32_t>();
                    switch (TW) {
                    case 1: launch_round<1>(st, directed, R, indices, data, nnz, W, S, round + b, filtered, before, flag, writes.as<bits_t>()); break;
                    case 2: launch_round<2>(st, directed, R, indices, data, nnz, W, S, round + b, filtered, before, flag, writes.as<bits_t>()); break;
                    case 4: launch_round<4>(st, directed, R, indices, data, nnz, W, S, round + b, filtered, before, flag, writes.as<bits_t>()); break;
                    default: launch_round<ROOT_TILE>(st, directed, R, indices, data, nnz, W, S, round + b, filtered, before, flag, writes.as<bits_t>()); break;
                    }
                }
                d2h(h_flags, flags, sizeof h_flags, st);   // the one fetch of the batch
                int quiet = 0;                             // the first round that raised nothing; the ones after it returned at once
                while (quiet < ROUND_BATCH && h_flags[quiet]) ++quiet;
                rounds += std::min(quiet + 1, ROUND_BATCH);
                done = verify && quiet == 0;
                verify = quiet < ROUND_BATCH;              // a round raised nothing under the filter: ask every entry next
                round += ROUND_BATCH;
                if (round > INT_MAX - 2 * ROUND_BATCH) throw std::runtime_error("geodesic: more than 2^31 rounds");
            }
        }
        LAUNCH_BOUNDED(geodesic_transpose_kernel, n, COUNT_BLOCKS, st, (int64_t)n, TW, tw, work.as<bits_t>(), dist + (int64_t)set0 * n,
                       words.as<bits_t>());
    }
    hipLaunchKernelGGL(geodesic_writes_kernel, dim3(1), dim3(256), 0, st, writes.as<bits_t>(), words.as<bits_t>());
    HIPCHK(hipGetLastError());
    bits_t h_words[2];
    d2h(h_words, words, sizeof h_words, st);
    stats[0] = (int64_t)h_words[0];
    stats[1] = rounds;
    stats[2] = (int64_t)h_words[1];
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_geodesic_device(int device, void *stream, int n, const int64_t *indptr, const int32_t *indices, const double *data,
                          int directed, int nsets, const int64_t *set_ptr, const int32_t *roots, double *dist, int64_t stats[3])
{
    if (const char *why = geodesic_bad_args(n, nsets, indptr, set_ptr, dist, stats)) return fail("%s", why);
    if (n == 0 || nsets == 0) {
        std::fill(stats, stats + 3, (int64_t)0);
        return 0;
    }
    return guarded([&] {
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        const int64_t nnz = indptr_on_device(st, n, indptr, louvain_bad_indptr);
        if (const char *why = components_bad_nnz(nnz, indices)) throw std::invalid_argument(why);
        int64_t result[3];
        geodesic_on_device(st, n, nnz, indptr, indices, data, directed != 0, nsets, set_ptr, roots, dist, result);
        std::copy(result, result + 3, stats);
    });
}

int schpf_geodesic(int device, int n, const int64_t *indptr, const int32_t *indices, const double *data, int directed, int nsets,
                   const int64_t *set_ptr, const int32_t *roots, double *dist, int64_t stats[3])
{
    if (const char *why = geodesic_bad_args(n, nsets, indptr, set_ptr, dist, stats)) return fail("%s", why);
    if (n == 0 || nsets == 0) {
        std::fill(stats, stats + 3, (int64_t)0);
        return 0;
    }
    return guarded([&] {
        use_device(device);
        TempStream ts;
        DevBuf d_indptr, d_indices, d_data, d_set_ptr, d_roots, d_dist;
        h2d<int64_t>(d_indptr, indptr, (size_t)n + 1, ts.st);
        const int64_t nnz = indptr_on_device(ts.st, n, d_indptr.as<int64_t>(), louvain_bad_indptr);   // the host's indptr[n] if it passes
        if (const char *why = components_bad_nnz(nnz, indices)) throw std::invalid_argument(why);
        h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
        if (data) h2d<double>(d_data, data, (size_t)nnz, ts.st);
        h2d<int64_t>(d_set_ptr, set_ptr, (size_t)nsets + 1, ts.st);
        // the roots go up only after set_ptr has passed on the device: until then its last entry is not a size.  The host's
        // copy is read here for the upload alone; a set_ptr that is refused below never has its roots looked at
        bool sets_fine = set_ptr[0] == 0;
        for (int r = 0; sets_fine && r < nsets; ++r) sets_fine = set_ptr[r + 1] >= set_ptr[r];
        const int64_t nroots = sets_fine ? set_ptr[nsets] : 0;
        if (nroots > 0 && !roots) throw std::invalid_argument("roots must not be NULL");
        h2d<int32_t>(d_roots, roots, (size_t)nroots, ts.st);
        const size_t cells = (size_t)nsets * (size_t)n;
        d_dist.alloc(cells * sizeof(double));
        int64_t result[3];
        geodesic_on_device(ts.st, n, nnz, d_indptr.as<int64_t>(), d_indices.as<int32_t>(), data ? d_data.as<double>() : nullptr,
                           directed != 0, nsets, d_set_ptr.as<int64_t>(), d_roots.as<int32_t>(), d_dist.as<double>(), result);
        d2h(dist, d_dist, cells * sizeof(double), ts.st);
        std::copy(result, result + 3, stats);
    });
}

}  // extern "C"
