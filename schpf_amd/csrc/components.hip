// Connected components of a graph and the graph of its clusters (schpf_components*, schpf_cluster_graph*).
// Both are defined in integers in include/schpf_hip.h and restated serially in host.cpp; the bits are the same on every
// schedule.  The graph is read as louvain.hip reads it (graph_device.h): the row of every entry by bisection, one thread per
// entry, so a row may be of any length and no thread walks one.
//
// components: min-label hooking with pointer doubling on p[n], p[i] = i at the start
//   (graph_device.h: the columns, and for the cluster graph the values and the labels; every check leaves its smallest
//   offender in a word of the call's one record, device_call.h, which is fetched once)
//   components_within_kernel    within[i] >= -1: the smallest offending vertex
//   components_edges_kernel     the number of entries that are edges (one integer add per wavefront)
//   per hook round:
//   components_hook_kernel      per edge (i, j) with p[i] != p[j]: atomicMin(p[max], min) and flags[0] = 1
//   components_shortcut_kernel  pass t: p[i] = p[p[i]]; flags[1 + t] = 1 where something changed.  A pass returns at once
//                               when the step before it (the hook round, or pass t - 1) changed nothing, so the host launches
//                               ceil(log2 n) + 1 of them -- doubling needs no more -- and fetches the flags once per round
//   p[i] <= i at all times (every write puts a smaller vertex of the same component there), so p has no cycles; the loop ends
//   when no edge joins two trees and every tree is a star, i.e. p[i] = the smallest vertex of i's component, whoever won a
//   race on the way.  The atomics are integer minima.
//   components_roots_kernel, (rocPRIM exclusive scan), components_label_kernel: the numbering by first member, comp, and the
//   sizes by integer atomicAdd (count_keys: runs in registers, LDS bins, and memory for the many small ones)
//   components_stats_kernel     C, the largest size, the components of size 1
// cluster graph: one aggregation step of louvain.hip with the caller's labels
//   labels_check_kernel         (graph_device.h) labels[i] in [-1, G): the smallest offending vertex
//   cluster_cells_kernel        group_cells
//   cluster_records_kernel      per entry the key a * G + b (G * G: does not count) and the value (1, q)
//   (rocPRIM radix sort over the occupied bits, reduce-by-key with the integer sum of both members)
//   cluster_scatter_kernel      the reduced records into the zeroed tables
#include <cfloat>
#include <climits>
#include <cmath>
#include <memory>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "graph_device.h"

namespace schpf {
namespace {

struct Tally {   // what an entry adds to its pair of groups
    int64_t cnt, w;
};
struct TallyPlus {
    __host__ __device__ Tally operator()(const Tally &a, const Tally &b) const { return Tally{a.cnt + b.cnt, a.w + b.w}; }
};

enum { W_EDGES = 0, W_LARGEST, W_SINGLE, W_COUNT_C, W_WORDS };
// the smallest offenders of a call, in the order they are asked; BAD_ITEMS: `within` (components), `labels` (cluster graph)
enum { BAD_COLUMNS = 0, BAD_VALUES, BAD_ITEMS, BAD_COUNT };

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// counters[key_of(i)] += 1 for every i < n with a key >= 0, in integers, by a grid of at most COUNT_BLOCKS workgroups.  Many
// adds on few addresses are what such a kernel waits for (a graph in one piece: every vertex names counter 0), so a
// wavefront whose lanes all name one counter keeps the run in a register until the counter changes, and the others add into
// LDS bins for the counters below COUNT_BINS -- numbered by first member, the large components have small numbers -- that
// the workgroup flushes once; only keys beyond the bins, which are many and so rarely the same, go to memory one by one
constexpr int COUNT_BINS = 4096, COUNT_BLOCKS = 1024;
template <typename T, typename KeyOf> __device__ __forceinline__ void count_keys(int64_t n, T *__restrict__ counters, KeyOf key_of)
{
    __shared__ int bins[COUNT_BINS];
    for (int b = threadIdx.x; b < COUNT_BINS; b += 256) bins[b] = 0;
    __syncthreads();
    const bool lane0 = (threadIdx.x & 63) == 0;   // has the smallest i of its wavefront: in the loop as long as any lane is
    auto add = [&](int key, unsigned amount) {
        if (key < COUNT_BINS) atomicAdd(bins + key, (int)amount);
        else atomicAdd(counters + key, (T)amount);
    };
    int run_key = -1;
    unsigned run = 0;
    GRID_STRIDE(i, n)
    {
        const int key = key_of(i);
        const unsigned long long active = __ballot(1);
        const int first = __builtin_amdgcn_readfirstlane(key);
        if (__all(key == first)) {
            if (first != run_key) {
                if (lane0 && run_key >= 0 && run) add(run_key, run);
                run_key = first;
                run = 0;
            }
            run += (unsigned)__popcll(active);
        } else if (key >= 0) {
            add(key, 1);
        }
    }
    if (lane0 && run_key >= 0 && run) add(run_key, run);
    __syncthreads();
    for (int b = threadIdx.x; b < COUNT_BINS; b += 256)
        if (bins[b]) atomicAdd(counters + b, (T)bins[b]);
}

__device__ __forceinline__ bool is_edge(int i, int j, const int32_t *__restrict__ within)
{
    if (j == i) return false;
    if (!within) return true;
    const int32_t wi = within[i];
    return wi >= 0 && wi == within[j];
}

__global__ __launch_bounds__(256) void components_within_kernel(const int32_t *__restrict__ within, int64_t n,
                                                                unsigned long long *__restrict__ word)
{
    unsigned long long bad = NONE;
    GRID_STRIDE(i, n)
    {
        if (within[i] < -1) offends(bad, i);
    }
    report_min(word, bad);
}

__global__ __launch_bounds__(256) void components_init_kernel(int64_t n, int32_t *__restrict__ p)
{
    GRID_STRIDE(i, n) p[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void components_edges_kernel(const int32_t *__restrict__ rowof, const int32_t *__restrict__ indices,
                                                               const int32_t *__restrict__ within, int64_t nnz,
                                                               unsigned long long *__restrict__ words)
{
    unsigned long long mine = 0;
    GRID_STRIDE(e, nnz) mine += is_edge(rowof[e], indices[e], within) ? 1 : 0;
    mine = wave_sum(mine);   // every lane is here: the loop has no early exit
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(words + W_EDGES, mine);
}

// p is read while other lanes lower it: whatever value a lane sees is a vertex of the same component that is not above the
// one it was read for, which is all the argument needs
__global__ __launch_bounds__(256) void components_hook_kernel(const int32_t *__restrict__ rowof, const int32_t *__restrict__ indices,
                                                              const int32_t *__restrict__ within, int64_t nnz, int32_t *p,
                                                              int *__restrict__ flags)
{
    bool hooked = false;
    GRID_STRIDE(e, nnz)
    {
        const int i = rowof[e], j = indices[e];
        if (!is_edge(i, j, within)) continue;
        const int32_t ri = p[i], rj = p[j];
        if (ri != rj) {
            // Late in a round most edges between two trees name a root that another lane has lowered already: a million
            // minima on one address is what the kernel would then wait for.  Only a value below the one seen goes there
            // (read past the L1, where the other lanes' minima are never seen); the flag does not depend on it
            const int32_t hi = max(ri, rj), lo = min(ri, rj);
            if (__hip_atomic_load(p + hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > lo) atomicMin(p + hi, lo);
            hooked = true;
        }
    }
    if (hooked) flags[0] = 1;
}

// pass t of the doubling.  flags[t] is what the step before it left: nothing changed -> p is where this pass would leave it
__global__ __launch_bounds__(256) void components_shortcut_kernel(int64_t n, int32_t *p, int *flags, int t, bool always)
{
    if (!always && flags[t] == 0) return;
    bool changed = false;
    GRID_STRIDE(i, n)
    {
        const int32_t a = p[i], b = p[a];
        if (b != a) {
            p[i] = b;
            changed = true;
        }
    }
    if (changed) flags[1 + t] = 1;
}

__global__ __launch_bounds__(256) void components_roots_kernel(int64_t n, const int32_t *__restrict__ p, int64_t *__restrict__ root)
{
    GRID_STRIDE(i, n) root[i] = p[i] == (int32_t)i ? 1 : 0;
}

__global__ __launch_bounds__(256) void components_label_kernel(int64_t n, const int32_t *__restrict__ p, const int64_t *__restrict__ renum,
                                                               int32_t *__restrict__ comp, int *__restrict__ size)
{
    count_keys(n, size, [&](int64_t i) {
        const int c = (int)renum[p[i]];
        comp[i] = c;
        return c;
    });
}

// size[c] = 0 for c >= C: neither the largest size nor the sizes of 1 see them
__global__ __launch_bounds__(256) void components_stats_kernel(int64_t n, const int *__restrict__ size, const int64_t *__restrict__ root,
                                                               const int64_t *__restrict__ renum, unsigned long long *__restrict__ words)
{
    unsigned long long largest = 0, single = 0;
    GRID_STRIDE(c, n)
    {
        const unsigned long long s = (unsigned long long)size[c];
        largest = s > largest ? s : largest;
        single += s == 1 ? 1 : 0;
    }
    largest = ~wave_min(~largest);
    single = wave_sum(single);
    if ((threadIdx.x & 63) == 0) {
        if (largest) atomicMax(words + W_LARGEST, largest);
        if (single) atomicAdd(words + W_SINGLE, single);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) words[W_COUNT_C] = (unsigned long long)(renum[n - 1] + root[n - 1]);
}

__global__ __launch_bounds__(256) void cluster_cells_kernel(const int32_t *__restrict__ labels, int64_t n, sum_t *__restrict__ cells)
{
    count_keys(n, cells, [&](int64_t i) { return (int)labels[i]; });
}

__global__ __launch_bounds__(256) void cluster_records_kernel(const int32_t *__restrict__ rowof, const int32_t *__restrict__ indices,
                                                              const double *__restrict__ data, const int32_t *__restrict__ labels,
                                                              double wmax, int64_t G, int64_t nnz, uint64_t *__restrict__ key,
                                                              Tally *__restrict__ val)
{
    GRID_STRIDE(e, nnz)
    {
        const int i = rowof[e], j = indices[e];
        const int64_t a = labels[i], b = labels[j];
        const bool take = j != i && a >= 0 && b >= 0;
        key[e] = take ? (uint64_t)(a * G + b) : (uint64_t)(G * G);
        const int64_t q = data && wmax > 0.0 ? louvain_quantum(data[e], wmax) : (int64_t)1 << 30;
        val[e] = take ? Tally{1, q} : Tally{0, 0};
    }
}

__global__ __launch_bounds__(256) void cluster_scatter_kernel(const uint64_t *__restrict__ key, const Tally *__restrict__ val,
                                                              const count_t *__restrict__ n_runs, int64_t bound, uint64_t limit,
                                                              int64_t *__restrict__ count, int64_t *__restrict__ weight)
{
    const int64_t runs = (int64_t)*n_runs;
    GRID_STRIDE(r, bound)
    {
        if (r >= runs) break;
        if (key[r] >= limit) continue;
        count[key[r]] = val[r].cnt;
        if (weight) weight[key[r]] = val[r].w;
    }
}

int doubling_passes(int n)   // ceil(log2 n) passes bring a tree of depth n - 1 to depth 1, and one more sees no change
{
    int l = 0;
    while (((int64_t)1 << l) < n) ++l;
    return l + 1;
}

// Everything on `st`, which is synchronised when this returns; indptr has been checked, every pointer but stats is device
// memory.  comp is written once, at the end: a refused call leaves it alone
void components_on_device(hipStream_t st, int n, int64_t nnz, const int64_t *indptr, const int32_t *indices, const int32_t *within,
                          int32_t *comp, int64_t *stats)
{
    const size_t N = (size_t)n;
    DevBuf rowof;
    Offenders<BAD_COUNT> w;   // no values here: BAD_VALUES stays NONE
    w.reset(st);
    if (nnz > 0) {
        rowof.alloc((size_t)nnz * sizeof(int32_t));
        LAUNCH(entry_rows_kernel, nnz, st, indptr, (int64_t)n, nnz, rowof.as<int32_t>());
        LAUNCH(graph_entries_check_kernel<false>, nnz, st, indptr, indices, (const double *)nullptr, rowof.as<int32_t>(), n, nnz,
               w.dev() + BAD_COLUMNS, w.dev() + BAD_VALUES);
    }
    if (within) LAUNCH(components_within_kernel, n, st, within, (int64_t)n, w.dev() + BAD_ITEMS);
    w.fetch(st);
    w.refuse(BAD_COLUMNS, graph_bad_columns);
    w.refuse(BAD_ITEMS, components_bad_within);

    DevBuf p, flags, words, root, renum, size;
    Scratch temp;
    const int L = doubling_passes(n);
    p.alloc(N * sizeof(int32_t));
    flags.alloc((size_t)(L + 1) * sizeof(int));
    words.alloc(W_WORDS * sizeof(unsigned long long), true, st);
    root.alloc(N * sizeof(int64_t));
    renum.alloc(N * sizeof(int64_t));
    size.alloc(N * sizeof(int), true, st);
    LAUNCH(components_init_kernel, n, st, (int64_t)n, p.as<int32_t>());

    int64_t rounds = 0, passes = 0;
    if (nnz > 0) {
        LAUNCH_BOUNDED(components_edges_kernel, nnz, COUNT_BLOCKS, st, rowof.as<int32_t>(), indices, within, nnz, words.as<unsigned long long>());
        std::vector<int> h_flags((size_t)L + 1);
        for (bool again = true, hook = true; again;) {
            HIPCHK(hipMemsetAsync(flags.p, 0, h_flags.size() * sizeof(int), st));
            if (hook) LAUNCH(components_hook_kernel, nnz, st, rowof.as<int32_t>(), indices, within, nnz, p.as<int32_t>(), flags.as<int>());
            for (int t = 0; t < L; ++t)
                LAUNCH(components_shortcut_kernel, n, st, (int64_t)n, p.as<int32_t>(), flags.as<int>(), t, !hook && t == 0);
            d2h(h_flags.data(), flags, h_flags.size() * sizeof(int), st);   // the one fetch of the round
            if (hook) ++rounds;
            for (int t = 0; t < L; ++t) passes += (t == 0 && !hook) || h_flags[(size_t)t] ? 1 : 0;
            // the last pass changed something: only a tree deeper than n could do that; finish the doubling all the same
            const bool unfinished = h_flags[(size_t)L] != 0;
            again = unfinished || (hook && h_flags[0] != 0);
            hook = !unfinished;
        }
    }

    LAUNCH(components_roots_kernel, n, st, (int64_t)n, p.as<int32_t>(), root.as<int64_t>());
    temp.run([&](void *t, size_t &b) {
        return rocprim::exclusive_scan(t, b, root.as<int64_t>(), renum.as<int64_t>(), (int64_t)0, N, rocprim::plus<int64_t>(), st);
    });
    LAUNCH_BOUNDED(components_label_kernel, n, COUNT_BLOCKS, st, (int64_t)n, p.as<int32_t>(), renum.as<int64_t>(), comp, size.as<int>());
    LAUNCH_BOUNDED(components_stats_kernel, n, COUNT_BLOCKS, st, (int64_t)n, size.as<int>(), root.as<int64_t>(), renum.as<int64_t>(),
           words.as<unsigned long long>());
    unsigned long long h_words[W_WORDS];
    d2h(h_words, words, sizeof h_words, st);
    stats[0] = (int64_t)h_words[W_COUNT_C];
    stats[1] = (int64_t)h_words[W_LARGEST];
    stats[2] = (int64_t)h_words[W_SINGLE];
    stats[3] = (int64_t)h_words[W_EDGES];
    stats[4] = rounds;
    stats[5] = passes;
}

// As above; group_cells, count and weight (may be nullptr) are device memory and written in full, *wmax is the host's
void cluster_graph_on_device(hipStream_t st, int n, int64_t nnz, const int64_t *indptr, const int32_t *indices, const double *data,
                             const int32_t *labels, int G, int64_t *group_cells, int64_t *count, int64_t *weight, double *wmax)
{
    const size_t GG = (size_t)G * (size_t)G;
    DevBuf rowof, d_wmax;
    Scratch temp;
    Offenders<BAD_COUNT> w;
    w.reset(st);
    d_wmax.alloc(sizeof(double), true, st);
    if (nnz > 0) {
        rowof.alloc((size_t)nnz * sizeof(int32_t));
        LAUNCH(entry_rows_kernel, nnz, st, indptr, (int64_t)n, nnz, rowof.as<int32_t>());
        LAUNCH(graph_entries_check_kernel<false>, nnz, st, indptr, indices, data, rowof.as<int32_t>(), n, nnz, w.dev() + BAD_COLUMNS,
               w.dev() + BAD_VALUES);
        if (data)
            temp.run([&](void *t, size_t &b) { return rocprim::reduce(t, b, data, d_wmax.as<double>(), 0.0, (size_t)nnz, Larger(), st); });
    }
    LAUNCH(labels_check_kernel, n, st, labels, (int64_t)n, G, w.dev() + BAD_ITEMS);
    double h_wmax = 0.0;
    HIPCHK(hipMemcpyAsync(&h_wmax, d_wmax.p, sizeof h_wmax, hipMemcpyDeviceToHost, st));
    w.fetch(st);
    w.refuse(BAD_COLUMNS, graph_bad_columns);
    w.refuse(BAD_VALUES, louvain_bad_values);
    w.refuse(BAD_ITEMS, cluster_graph_bad_labels);
    if (!data && nnz > 0) h_wmax = 1.0;   // all ones

    HIPCHK(hipMemsetAsync(group_cells, 0, (size_t)G * sizeof(int64_t), st));
    HIPCHK(hipMemsetAsync(count, 0, GG * sizeof(int64_t), st));
    if (weight) HIPCHK(hipMemsetAsync(weight, 0, GG * sizeof(int64_t), st));
    LAUNCH_BOUNDED(cluster_cells_kernel, n, COUNT_BLOCKS, st, labels, (int64_t)n, reinterpret_cast<sum_t *>(group_cells));
    if (nnz > 0) {
        DevBuf key_a, key_b, val_a, val_b, runs;
        key_a.alloc((size_t)nnz * sizeof(uint64_t));
        key_b.alloc((size_t)nnz * sizeof(uint64_t));
        val_a.alloc((size_t)nnz * sizeof(Tally));
        val_b.alloc((size_t)nnz * sizeof(Tally));
        runs.alloc(sizeof(count_t));
        uint64_t *const ka = key_a.as<uint64_t>(), *const kb = key_b.as<uint64_t>();
        Tally *const va = val_a.as<Tally>(), *const vb = val_b.as<Tally>();
        LAUNCH(cluster_records_kernel, nnz, st, rowof.as<int32_t>(), indices, data, labels, h_wmax, (int64_t)G, nnz, ka, va);
        temp.run([&](void *t, size_t &b) {
            return rocprim::radix_sort_pairs(t, b, ka, kb, va, vb, (size_t)nnz, 0, bits_of((uint64_t)GG), st);
        });
        temp.run([&](void *t, size_t &b) {
            return rocprim::reduce_by_key(t, b, kb, vb, (size_t)nnz, ka, va, runs.as<count_t>(), TallyPlus(),
                                          rocprim::equal_to<uint64_t>(), st);
        });
        // at most G * G + 1 runs, and no more than there are entries
        const int64_t bound = (int64_t)std::min<uint64_t>((uint64_t)nnz, (uint64_t)GG + 1);
        LAUNCH(cluster_scatter_kernel, bound, st, ka, va, runs.as<count_t>(), bound, (uint64_t)GG, count, weight);
        HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
    }
    HIPCHK(hipStreamSynchronize(st));
    *wmax = h_wmax;
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_components_device(int device, void *stream, int n, const int64_t *indptr, const int32_t *indices, const int32_t *within,
                            int32_t *comp, int64_t stats[6])
{
    if (const char *why = components_bad_args(n, indptr, comp, stats)) return fail("%s", why);
    if (n == 0) {
        std::fill(stats, stats + 6, (int64_t)0);
        return 0;
    }
    return guarded([&] {
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        const int64_t nnz = indptr_on_device(st, n, indptr, louvain_bad_indptr);
        if (const char *why = components_bad_nnz(nnz, indices)) throw std::invalid_argument(why);
        int64_t result[6];
        components_on_device(st, n, nnz, indptr, indices, within, comp, result);
        std::copy(result, result + 6, stats);
    });
}

int schpf_components(int device, int n, const int64_t *indptr, const int32_t *indices, const int32_t *within, int32_t *comp,
                     int64_t stats[6])
{
    if (const char *why = components_bad_args(n, indptr, comp, stats)) return fail("%s", why);
    if (n == 0) {
        std::fill(stats, stats + 6, (int64_t)0);
        return 0;
    }
    return guarded([&] {
        use_device(device);
        TempStream ts;
        DevBuf d_indptr, d_indices, d_within, d_comp;
        h2d<int64_t>(d_indptr, indptr, (size_t)n + 1, ts.st);
        const int64_t nnz = indptr_on_device(ts.st, n, d_indptr.as<int64_t>(), louvain_bad_indptr);   // the host's indptr[n] if it passes
        if (const char *why = components_bad_nnz(nnz, indices)) throw std::invalid_argument(why);
        h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
        if (within) h2d<int32_t>(d_within, within, (size_t)n, ts.st);
        d_comp.alloc((size_t)n * sizeof(int32_t));
        int64_t result[6];
        components_on_device(ts.st, n, nnz, d_indptr.as<int64_t>(), d_indices.as<int32_t>(),
                             within ? d_within.as<int32_t>() : nullptr, d_comp.as<int32_t>(), result);
        d2h(comp, d_comp, (size_t)n * sizeof(int32_t), ts.st);
        std::copy(result, result + 6, stats);
    });
}

int schpf_cluster_graph_device(int device, void *stream, int n, const int64_t *indptr, const int32_t *indices, const double *data,
                               const int32_t *labels, int ngroups, int64_t *group_cells, int64_t *count, int64_t *weight,
                               double *wmax)
{
    if (const char *why = cluster_graph_bad_args(n, indptr, labels, ngroups, group_cells, count, wmax)) return fail("%s", why);
    return guarded([&] {
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        const int64_t nnz = n ? indptr_on_device(st, n, indptr, louvain_bad_indptr) : 0;
        if (const char *why = components_bad_nnz(nnz, indices)) throw std::invalid_argument(why);
        double result = 0.0;
        cluster_graph_on_device(st, n, nnz, indptr, indices, data, labels, ngroups, group_cells, count, weight, &result);
        *wmax = result;
    });
}

int schpf_cluster_graph(int device, int n, const int64_t *indptr, const int32_t *indices, const double *data, const int32_t *labels,
                        int ngroups, int64_t *group_cells, int64_t *count, int64_t *weight, double *wmax)
{
    if (const char *why = cluster_graph_bad_args(n, indptr, labels, ngroups, group_cells, count, wmax)) return fail("%s", why);
    return guarded([&] {
        use_device(device);
        TempStream ts;
        const size_t G = (size_t)ngroups;
        DevBuf d_indptr, d_indices, d_data, d_labels, d_cells, d_count, d_weight;
        int64_t nnz = 0;
        if (n) {
            h2d<int64_t>(d_indptr, indptr, (size_t)n + 1, ts.st);
            nnz = indptr_on_device(ts.st, n, d_indptr.as<int64_t>(), louvain_bad_indptr);
        }
        if (const char *why = components_bad_nnz(nnz, indices)) throw std::invalid_argument(why);
        h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
        if (data) h2d<double>(d_data, data, (size_t)nnz, ts.st);
        h2d<int32_t>(d_labels, labels, (size_t)n, ts.st);
        d_cells.alloc(G * sizeof(int64_t));
        d_count.alloc(G * G * sizeof(int64_t));
        if (weight) d_weight.alloc(G * G * sizeof(int64_t));
        double result = 0.0;
        cluster_graph_on_device(ts.st, n, nnz, d_indptr.as<int64_t>(), d_indices.as<int32_t>(), data ? d_data.as<double>() : nullptr,
                                d_labels.as<int32_t>(), ngroups, d_cells.as<int64_t>(), d_count.as<int64_t>(),
                                weight ? d_weight.as<int64_t>() : nullptr, &result);
        HIPCHK(hipMemcpyAsync(group_cells, d_cells.p, G * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        if (weight) HIPCHK(hipMemcpyAsync(weight, d_weight.p, G * G * sizeof(int64_t), hipMemcpyDeviceToHost, ts.st));
        d2h(count, d_count, G * G * sizeof(int64_t), ts.st);
        *wmax = result;
    });
}

}  // extern "C"
