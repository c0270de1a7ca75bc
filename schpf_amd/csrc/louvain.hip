// Louvain clustering of a symmetric weighted graph (schpf_louvain / schpf_louvain_device).  The weights are
// quantised once to int64, so every sum of the algorithm is an integer sum -- exact in any order -- and the one score per
// candidate is a fixed expression of exact integers.  Moves are synchronous.  The definition is in include/schpf_hip.h;
// host.cpp's serial restatement gives the same bits.
//
// (the first four kernels are in graph_device.h, shared with components.hip, geodesic.hip and the rank sums)
//   indptr_check_kernel     indptr starts at 0 and does not decrease: the smallest offending row
//   entry_rows_kernel       the row of every entry, by bisection in indptr (once per level: a row may be of any length,
//                           no kernel walks one)
//   graph_entries_check_kernel  one thread per entry: column in range and above its left neighbour, value finite and >= 0;
//                           the smallest offending row of each into the call's record of two words (device_call.h)
//   (rocPRIM reduce: wmax)
//   louvain_quantise_kernel q = llrint(ldexp(data / wmax, 30))
//   per level: (rocPRIM reduce-by-key over the rows: k_i; reduce: W2)
//   per round:
//   louvain_records_kernel  per entry (i, j), j != i, of an eligible row: key i * n_l + c[j], value q; every other entry
//                           gets the key n_l^2, which sorts behind all of them
//   (rocPRIM radix sort over the occupied bits, reduce-by-key: K(i, d))
//   louvain_score_kernel    per reduced record: the record of the vertex's own community leaves K(a) in own[i] (its only
//                           writer), every other one becomes the candidate (score, d)
//   (rocPRIM reduce-by-key over the vertices with the operator "the better candidate": the key (score descending, d
//   ascending) is a total order, so the reduction's shape does not matter)
//   louvain_apply_kernel    per vertex that has a candidate: moves iff its score beats the own community's, strictly
//   (rocPRIM reduce: the moves of the round -- the one number that crosses to the host per round)
//   louvain_pairs_kernel, sort, reduce-by-key, louvain_scatter_kernel: tot[d] and the communities that have members
//   aggregation: (rocPRIM exclusive scan of the presence flags: the renumbering)
//   louvain_rekey_kernel    per entry the key c'(i) * n' + c'(j); sort and reduce-by-key give the next level's entries
//   louvain_fill_kernel     columns and, by bisection in the sorted keys, indptr (a row may be empty)
//   louvain_compose_kernel  labels through the renumbering
// No atomics in any kernel here: who writes what is fixed by the sorted order.  (The checks' one atomicMin per wavefront that
// found an offender is an integer minimum.)
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
#include "graph_device.h"   // what components.hip reads a graph with as well: the indptr, rows, check and quantise kernels
#include "kernels.h"

namespace schpf {
namespace {

struct Cand {
    double s;
    int64_t d;   // INT64_MAX: none
};
// the better of two candidates by the key (score descending, community ascending)
struct Better {
    __host__ __device__ Cand operator()(const Cand &a, const Cand &b) const
    {
        return (a.s > b.s || (a.s == b.s && a.d <= b.d)) ? a : b;
    }
};
__device__ __forceinline__ bool eligible(int64_t i, int round, int64_t k)
{
    return ((((uint64_t)i * 2654435761ull) >> 16) & 1) == (uint64_t)(round & 1) && k > 0;
}

// score(d) of the definition: one multiply, one division, one fma
__device__ __forceinline__ double score(int64_t k, int64_t base, int64_t w2, int64_t among, double gamma)
{
    const double p = (double)k * (double)base;
    const double t = p / (double)w2;
    return fma(-gamma, t, (double)among);
}

__global__ __launch_bounds__(256) void louvain_iota_kernel(int64_t n, int32_t *__restrict__ c)
{
    GRID_STRIDE(i, n) c[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void louvain_records_kernel(const int32_t *__restrict__ rowof, const int32_t *__restrict__ indices,
                                                              const int64_t *__restrict__ q, const int32_t *__restrict__ c,
                                                              const int64_t *__restrict__ k, int64_t nl, int64_t nnz, int round,
                                                              uint64_t *__restrict__ key, int64_t *__restrict__ val)
{
    GRID_STRIDE(e, nnz)
    {
        const int64_t i = rowof[e], j = indices[e];
        const bool take = j != i && eligible(i, round, k[i]);
        key[e] = take ? (uint64_t)i * (uint64_t)nl + (uint64_t)c[j] : (uint64_t)nl * (uint64_t)nl;
        val[e] = take ? q[e] : 0;
    }
}

// p < *n_runs: the reduced record (i, d, K).  Behind them, up to nnz: padding that belongs to the vertex n_l, which does
// not exist, so that the reduction over the vertices has a length the host knows
__global__ __launch_bounds__(256) void louvain_score_kernel(const uint64_t *__restrict__ key, const int64_t *__restrict__ among,
                                                            const count_t *__restrict__ n_runs, const int32_t *__restrict__ c,
                                                            const int64_t *__restrict__ k, const int64_t *__restrict__ tot,
                                                            const int64_t *__restrict__ w2, double gamma, int64_t nl, int64_t nnz,
                                                            int32_t *__restrict__ vertex, Cand *__restrict__ cand,
                                                            int64_t *__restrict__ own)
{
    const int64_t runs = (int64_t)*n_runs, total = *w2;
    GRID_STRIDE(p, nnz)
    {
        Cand mine{-HUGE_VAL, INT64_MAX};
        int64_t i = nl;
        if (p < runs && key[p] != (uint64_t)nl * (uint64_t)nl) {
            i = (int64_t)(key[p] / (uint64_t)nl);
            const int64_t d = (int64_t)(key[p] - (uint64_t)i * (uint64_t)nl);
            if (d == c[i]) own[i] = among[p];
            else mine = Cand{score(k[i], tot[d], total, among[p], gamma), d};
        }
        vertex[p] = (int32_t)i;
        cand[p] = mine;
    }
}

// u < *n_runs: vertex[u] and its best candidate.  moved[0 .. nl]: 1 where run u moved its vertex
__global__ __launch_bounds__(256) void louvain_apply_kernel(const int32_t *__restrict__ vertex, const Cand *__restrict__ best,
                                                            const count_t *__restrict__ n_runs, const int32_t *__restrict__ c,
                                                            const int64_t *__restrict__ k, const int64_t *__restrict__ tot,
                                                            const int64_t *__restrict__ own, const int64_t *__restrict__ w2,
                                                            double gamma, int64_t nl, int32_t *__restrict__ next,
                                                            int64_t *__restrict__ moved)
{
    const int64_t runs = (int64_t)*n_runs, total = *w2;
    GRID_STRIDE(u, nl + 1)
    {
        int64_t did = 0;
        if (u < runs && vertex[u] < nl && best[u].d != INT64_MAX) {
            const int64_t i = vertex[u];
            const int32_t a = c[i];
            if (best[u].s > score(k[i], tot[a] - k[i], total, own[i], gamma)) {
                next[i] = (int32_t)best[u].d;
                did = 1;
            }
        }
        moved[u] = did;
    }
}

__global__ __launch_bounds__(256) void louvain_pairs_kernel(const int32_t *__restrict__ c, const int64_t *__restrict__ k, int64_t nl,
                                                            uint64_t *__restrict__ key, int64_t *__restrict__ val)
{
    GRID_STRIDE(i, nl)
    {
        key[i] = (uint64_t)c[i];
        val[i] = k[i];
    }
}

// out[key[p]] = val[p] for the *n_runs reduced records (all keys differ); flag, where given, marks the keys that occur
__global__ __launch_bounds__(256) void louvain_scatter_kernel(const uint64_t *__restrict__ key, const int64_t *__restrict__ val,
                                                              const count_t *__restrict__ n_runs, int64_t bound,
                                                              int64_t *__restrict__ out, int64_t *__restrict__ flag)
{
    const int64_t runs = (int64_t)*n_runs;
    GRID_STRIDE(p, bound)
    {
        if (p >= runs) break;
        out[key[p]] = val[p];
        if (flag) flag[key[p]] = 1;
    }
}

__global__ __launch_bounds__(256) void louvain_rowkeys_kernel(const int32_t *__restrict__ rowof, int64_t nnz,
                                                              uint64_t *__restrict__ key)
{
    GRID_STRIDE(e, nnz) key[e] = (uint64_t)rowof[e];
}

__global__ __launch_bounds__(256) void louvain_rekey_kernel(const int32_t *__restrict__ rowof, const int32_t *__restrict__ indices,
                                                            const int32_t *__restrict__ c, const int64_t *__restrict__ renum,
                                                            int64_t n_next, int64_t nnz, uint64_t *__restrict__ key)
{
    GRID_STRIDE(e, nnz)
    key[e] = (uint64_t)renum[c[rowof[e]]] * (uint64_t)n_next + (uint64_t)renum[c[indices[e]]];
}

// The next level from its sorted, reduced keys: entry p's column, and indptr[r] = the first key that is not below r * n'
__global__ __launch_bounds__(256) void louvain_fill_kernel(const uint64_t *__restrict__ key, int64_t nnz_next, int64_t n_next,
                                                           int64_t *__restrict__ indptr, int32_t *__restrict__ indices)
{
    GRID_STRIDE(p, nnz_next) indices[p] = (int32_t)(key[p] % (uint64_t)n_next);
    GRID_STRIDE(r, n_next + 1)
    {
        const uint64_t first = (uint64_t)r * (uint64_t)n_next;
        int64_t lo = 0, hi = nnz_next;   // the answer is in [lo, hi]
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (key[mid] < first) lo = mid + 1;
            else hi = mid;
        }
        indptr[r] = lo;
    }
}

__global__ __launch_bounds__(256) void louvain_compose_kernel(const int32_t *__restrict__ c, const int64_t *__restrict__ renum,
                                                              int64_t n, int32_t *__restrict__ labels)
{
    GRID_STRIDE(v, n) labels[v] = (int32_t)renum[c[labels[v]]];
}

// Everything on `st`, which is synchronised when this returns; all pointers but stats are device memory, indptr has been
// checked.  labels is written once, at the end: a refused call leaves it alone
void louvain_on_device(hipStream_t st, int n, int64_t nnz, const int64_t *indptr, const int32_t *indices, const double *data,
                       double gamma, int32_t *labels, int64_t *stats)
{
    const size_t N = (size_t)n, cap = std::max<size_t>((size_t)nnz, N + 1);   // the longest list any pass makes
    DevBuf lab;
    lab.alloc(N * sizeof(int32_t));
    LAUNCH(louvain_iota_kernel, n, st, (int64_t)n, lab.as<int32_t>());
    auto finish = [&](int64_t n_comm, int64_t levels, int64_t rounds, int64_t w2) {
        HIPCHK(hipMemcpyAsync(labels, lab.p, N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
        stats[0] = n_comm;
        stats[1] = levels;
        stats[2] = rounds;
        stats[3] = w2;
    };
    if (nnz == 0) return finish(n, 0, 0, 0);

    Scratch temp;
    DevBuf rowof, scalars;
    enum { BAD_COLUMNS = 0, BAD_VALUES, BAD_COUNT };
    Offenders<BAD_COUNT> w;
    w.reset(st);
    rowof.alloc((size_t)nnz * sizeof(int32_t));
    // device scalars: [0] wmax (double), [1] W2, [2] the moves of a round, then the run counts of the reductions
    scalars.alloc(8 * sizeof(int64_t));
    double *const d_wmax = scalars.as<double>();
    int64_t *const d_w2 = scalars.as<int64_t>() + 1, *const d_moves = scalars.as<int64_t>() + 2;
    count_t *const d_runs = scalars.as<count_t>() + 3, *const d_vertices = scalars.as<count_t>() + 4,
                  *const d_comms = scalars.as<count_t>() + 5, *const d_next = scalars.as<count_t>() + 6;

    LAUNCH(entry_rows_kernel, nnz, st, indptr, (int64_t)n, nnz, rowof.as<int32_t>());
    LAUNCH(graph_entries_check_kernel<true>, nnz, st, indptr, indices, data, rowof.as<int32_t>(), n, nnz, w.dev() + BAD_COLUMNS,
           w.dev() + BAD_VALUES);
    temp.run([&](void *t, size_t &b) { return rocprim::reduce(t, b, data, d_wmax, 0.0, (size_t)nnz, Larger(), st); });
    double wmax = 0.0;
    HIPCHK(hipMemcpyAsync(&wmax, d_wmax, sizeof wmax, hipMemcpyDeviceToHost, st));
    w.fetch(st);
    w.refuse(BAD_COLUMNS, louvain_bad_columns);
    w.refuse(BAD_VALUES, louvain_bad_values);
    if (!(wmax > 0.0)) return finish(n, 0, 0, 0);

    // the level's graph: level 0 reads the caller's indptr and indices, the later ones two sets of buffers in turn
    DevBuf q0, next_ip[2], next_ix[2], next_q[2];
    q0.alloc((size_t)nnz * sizeof(int64_t));
    LAUNCH(louvain_quantise_kernel, nnz, st, data, d_wmax, nnz, q0.as<int64_t>());
    const int64_t *ip = indptr, *q = q0.as<int64_t>();
    const int32_t *ix = indices;
    int64_t nl = n, nnz_l = nnz;

    DevBuf key_a, key_b, val_a, val_b, cand, best, k, tot, own, present, renum, comm[2], moved;
    key_a.alloc(cap * sizeof(uint64_t));
    key_b.alloc(cap * sizeof(uint64_t));
    val_a.alloc(cap * sizeof(int64_t));
    val_b.alloc(cap * sizeof(int64_t));
    cand.alloc(cap * sizeof(Cand));
    best.alloc((N + 1) * sizeof(Cand));
    for (DevBuf *b : {&k, &tot, &own, &present, &renum}) b->alloc(N * sizeof(int64_t));
    moved.alloc((N + 1) * sizeof(int64_t));
    comm[0].alloc((N + 1) * sizeof(int32_t));
    comm[1].alloc((N + 1) * sizeof(int32_t));
    uint64_t *const ka = key_a.as<uint64_t>(), *const kb = key_b.as<uint64_t>();
    int64_t *const va = val_a.as<int64_t>(), *const vb = val_b.as<int64_t>();

    // sort (key_a, val_a)[0 .. count) by the low `bits` bits and add up the values of equal keys: the runs in (key_a, val_a)
    // again, their number in *n_runs
    auto sort_and_reduce = [&](int64_t count, int bits, count_t *n_runs) {
        temp.run([&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, ka, kb, va, vb, (size_t)count, 0, bits, st); });
        temp.run([&](void *t, size_t &b) {
            return rocprim::reduce_by_key(t, b, kb, vb, (size_t)count, ka, va, n_runs, rocprim::plus<int64_t>(),
                                          rocprim::equal_to<uint64_t>(), st);
        });
    };

    int64_t levels = 0, rounds = 0, w2_first = 0;
    for (int level = 0; level < LOUVAIN_LEVELS; ++level) {
        if (level > 0) LAUNCH(entry_rows_kernel, nnz_l, st, ip, nl, nnz_l, rowof.as<int32_t>());
        // k_i: the rows are runs of rowof already; rows without entries keep 0
        HIPCHK(hipMemsetAsync(k.p, 0, (size_t)nl * sizeof(int64_t), st));
        LAUNCH(louvain_rowkeys_kernel, nnz_l, st, rowof.as<int32_t>(), nnz_l, kb);
        temp.run([&](void *t, size_t &b) {
            return rocprim::reduce_by_key(t, b, kb, q, (size_t)nnz_l, ka, va, d_runs, rocprim::plus<int64_t>(),
                                          rocprim::equal_to<uint64_t>(), st);
        });
        LAUNCH(louvain_scatter_kernel, nl, st, ka, va, d_runs, nl, k.as<int64_t>(), (int64_t *)nullptr);
        temp.run([&](void *t, size_t &b) {
            return rocprim::reduce(t, b, q, d_w2, (int64_t)0, (size_t)nnz_l, rocprim::plus<int64_t>(), st);
        });
        if (level == 0) {
            HIPCHK(hipMemcpyAsync(&w2_first, d_w2, sizeof w2_first, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        int32_t *c = comm[0].as<int32_t>(), *next = comm[1].as<int32_t>();
        LAUNCH(louvain_iota_kernel, nl, st, nl, c);
        HIPCHK(hipMemcpyAsync(tot.p, k.p, (size_t)nl * sizeof(int64_t), hipMemcpyDeviceToDevice, st));

        bool level_moved = false;
        const int pair_bits = bits_of((uint64_t)nl * (uint64_t)nl);
        for (int r = 0; r < LOUVAIN_ROUNDS; ++r) {
            ++rounds;
            LAUNCH(louvain_records_kernel, nnz_l, st, rowof.as<int32_t>(), ix, q, c, k.as<int64_t>(), nl, nnz_l, r, ka, va);
            sort_and_reduce(nnz_l, pair_bits, d_runs);
            HIPCHK(hipMemsetAsync(own.p, 0, (size_t)nl * sizeof(int64_t), st));
            // the vertices of the reduced records go where the sorted keys were
            int32_t *const vertex = key_b.as<int32_t>(), *const run_vertex = val_b.as<int32_t>();
            LAUNCH(louvain_score_kernel, nnz_l, st, ka, va, d_runs, c, k.as<int64_t>(), tot.as<int64_t>(), d_w2, gamma, nl, nnz_l,
                   vertex, cand.as<Cand>(), own.as<int64_t>());
            temp.run([&](void *t, size_t &b) {
                return rocprim::reduce_by_key(t, b, vertex, cand.as<Cand>(), (size_t)nnz_l, run_vertex, best.as<Cand>(), d_vertices,
                                              Better(), rocprim::equal_to<int32_t>(), st);
            });
            HIPCHK(hipMemcpyAsync(next, c, (size_t)nl * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            LAUNCH(louvain_apply_kernel, nl + 1, st, run_vertex, best.as<Cand>(), d_vertices, c, k.as<int64_t>(), tot.as<int64_t>(),
                   own.as<int64_t>(), d_w2, gamma, nl, next, moved.as<int64_t>());
            temp.run([&](void *t, size_t &b) {
                return rocprim::reduce(t, b, moved.as<int64_t>(), d_moves, (int64_t)0, (size_t)nl + 1, rocprim::plus<int64_t>(), st);
            });
            int64_t moves = 0;
            HIPCHK(hipMemcpyAsync(&moves, d_moves, sizeof moves, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (moves == 0) break;
            level_moved = true;
            std::swap(c, next);
            HIPCHK(hipMemsetAsync(tot.p, 0, (size_t)nl * sizeof(int64_t), st));
            HIPCHK(hipMemsetAsync(present.p, 0, (size_t)nl * sizeof(int64_t), st));
            LAUNCH(louvain_pairs_kernel, nl, st, c, k.as<int64_t>(), nl, ka, va);
            sort_and_reduce(nl, bits_of((uint64_t)nl), d_comms);
            LAUNCH(louvain_scatter_kernel, nl, st, ka, va, d_comms, nl, tot.as<int64_t>(), present.as<int64_t>());
        }
        if (!level_moved) break;
        ++levels;

        // aggregation
        temp.run([&](void *t, size_t &b) {
            return rocprim::exclusive_scan(t, b, present.as<int64_t>(), renum.as<int64_t>(), (int64_t)0, (size_t)nl,
                                           rocprim::plus<int64_t>(), st);
        });
        count_t n_next = 0;
        HIPCHK(hipMemcpyAsync(&n_next, d_comms, sizeof n_next, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        LAUNCH(louvain_rekey_kernel, nnz_l, st, rowof.as<int32_t>(), ix, c, renum.as<int64_t>(), (int64_t)n_next, nnz_l, ka);
        HIPCHK(hipMemcpyAsync(va, q, (size_t)nnz_l * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        sort_and_reduce(nnz_l, bits_of((uint64_t)n_next * (uint64_t)n_next), d_next);
        count_t nnz_next = 0;
        HIPCHK(hipMemcpyAsync(&nnz_next, d_next, sizeof nnz_next, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const int into = level & 1;
        if (!next_ip[into].p) {   // sizes only shrink: the first allocation of each set holds every later level
            next_ip[into].alloc(((size_t)n_next + 1) * sizeof(int64_t));
            next_ix[into].alloc((size_t)nnz_next * sizeof(int32_t));
            next_q[into].alloc((size_t)nnz_next * sizeof(int64_t));
        }
        LAUNCH(louvain_fill_kernel, std::max<int64_t>((int64_t)nnz_next, (int64_t)n_next + 1), st, ka, (int64_t)nnz_next,
               (int64_t)n_next, next_ip[into].as<int64_t>(), next_ix[into].as<int32_t>());
        HIPCHK(hipMemcpyAsync(next_q[into].p, va, (size_t)nnz_next * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        LAUNCH(louvain_compose_kernel, n, st, c, renum.as<int64_t>(), (int64_t)n, lab.as<int32_t>());
        ip = next_ip[into].as<int64_t>();
        ix = next_ix[into].as<int32_t>();
        q = next_q[into].as<int64_t>();
        nl = (int64_t)n_next;
        nnz_l = (int64_t)nnz_next;
    }
    finish(nl, levels, rounds, w2_first);
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_louvain_device(int device, void *stream, int n, const int64_t *indptr, const int32_t *indices, const double *data,
                         double gamma, int32_t *labels, int64_t stats[4])
{
    if (const char *why = louvain_bad_args(n, indptr, gamma, labels, stats)) return fail("%s", why);
    if (n == 0) {
        std::fill(stats, stats + 4, (int64_t)0);
        return 0;
    }
    return guarded([&] {
        use_device(device);
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        const int64_t nnz = indptr_on_device(st, n, indptr, louvain_bad_indptr);
        if (const char *why = louvain_bad_nnz(nnz, indices, data)) throw std::invalid_argument(why);
        int64_t result[4];
        louvain_on_device(st, n, nnz, indptr, indices, data, gamma, labels, result);
        std::copy(result, result + 4, stats);
    });
}

int schpf_louvain(int device, int n, const int64_t *indptr, const int32_t *indices, const double *data, double gamma,
                  int32_t *labels, int64_t stats[4])
{
    if (const char *why = louvain_bad_args(n, indptr, gamma, labels, stats)) return fail("%s", why);
    if (n == 0) {
        std::fill(stats, stats + 4, (int64_t)0);
        return 0;
    }
    return guarded([&] {
        use_device(device);
        TempStream ts;
        DevBuf d_indptr, d_indices, d_data, d_labels;
        h2d<int64_t>(d_indptr, indptr, (size_t)n + 1, ts.st);
        const int64_t nnz = indptr_on_device(ts.st, n, d_indptr.as<int64_t>(), louvain_bad_indptr);   // the host's indptr[n] if it passes
        if (const char *why = louvain_bad_nnz(nnz, indices, data)) throw std::invalid_argument(why);
        h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
        h2d<double>(d_data, data, (size_t)nnz, ts.st);
        d_labels.alloc((size_t)n * sizeof(int32_t));
        int64_t result[4];
        louvain_on_device(ts.st, n, nnz, d_indptr.as<int64_t>(), d_indices.as<int32_t>(), d_data.as<double>(), gamma,
                          d_labels.as<int32_t>(), result);
        d2h(labels, d_labels, (size_t)n * sizeof(int32_t), ts.st);
        std::copy(result, result + 4, stats);
    });
}

}  // extern "C"
