// Simulated doublets on the device (schpf_doublet_parents_device, schpf_doublet_rows[_device]): row s of the
// result is the sum of the two rows of a canonical CSR count matrix that `parents` names.  Integer arithmetic only and
// every output entry written by exactly one lane: host.cpp's serial restatement gives the same bits, whatever the grid.
//
//   doublet_parents_kernel   one simulated row per thread: the draw of doublets.h
//   csr_indptr_kernel        indptr starts at 0, does not decrease and ends at nnz: the smallest offending row
//   csr_entries_kernel       a wavefront per row of the matrix: every column in [0, ngenes) and above its left neighbour,
//                            every value a count thinning accepts: the smallest offending entry / row
//                            (both in csr_device.h, shared with qc.hip, group_stats.hip and transpose.hip, as is the
//                            bisection of a row)
//   doublet_pairs_kernel     one pair per thread: both parents in [0, ncells); reports into the spare word W_BAD_ROW
//   doublet_length_kernel    a wavefront per pair: |A| + |B| - the columns they share, which the lanes find by bisection
//   (rocPRIM exclusive scan of the lengths: out_indptr)
//   doublet_fill_kernel      a wavefront per pair walks A, then B, in pieces of DOUBLET_PIECE = 64 entries.  A lane bisects
//                            the other parent for its column: the rank there, plus its rank at home, minus the shared
//                            columns before it -- a ballot, a popcount below the lane, and the count carried over from the
//                            earlier pieces -- is its place in the output.  A writes every entry (with B's value added
//                            where the column is shared), B the entries A does not hold.  No sort, no atomics; a row of
//                            any length is a longer loop.
// The other parent is read where it lies: a piece's window in it has no bound, and its few KiB stay in the vector cache
// over the ten or so steps of a bisection.
#include <climits>
#include <cstdint>
#include <memory>
#include <string>

#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "csr_device.h"
#include "doublets.h"

namespace schpf {
namespace {

using namespace csr_checks;

constexpr int DB_THREADS = CSR_THREADS;
constexpr int DOUBLET_PIECE = 64;   // entries of a parent per pass of a wavefront: one per lane

__global__ __launch_bounds__(DB_THREADS) void doublet_parents_kernel(uint64_t first, int64_t n_sim, uint32_t N, uint32_t k0,
                                                                     uint32_t k1, int32_t *__restrict__ parents)
{
    for (int64_t t = blockIdx.x * (int64_t)DB_THREADS + threadIdx.x; t < n_sim; t += (int64_t)gridDim.x * DB_THREADS) {
        int32_t a, b;
        doublet_parents_of(first + (uint64_t)t, N, k0, k1, &a, &b);
        parents[2 * t] = a;
        parents[2 * t + 1] = b;
    }
}

// Every lane of a wavefront leaves the loop before the reduction: no early return
__global__ __launch_bounds__(DB_THREADS) void doublet_pairs_kernel(const int32_t *__restrict__ parents, int64_t n_pairs, int64_t ncells,
                                                                   unsigned long long *__restrict__ words)
{
    unsigned long long bad = NONE;
    for (int64_t s = blockIdx.x * (int64_t)DB_THREADS + threadIdx.x; s < n_pairs; s += (int64_t)gridDim.x * DB_THREADS) {
        const int64_t a = parents[2 * s], b = parents[2 * s + 1];
        if (a < 0 || a >= ncells || b < 0 || b >= ncells) offends(bad, s);
    }
    report_min(words + W_BAD_ROW, bad);
}

// len[s] = the stored columns of parent a or parent b; len[n_pairs] = 0, the scan's last input.  The shorter parent is
// walked, the longer one bisected
template <typename I>
__global__ __launch_bounds__(DB_THREADS) void doublet_length_kernel(Matrix m, const int32_t *__restrict__ parents, int64_t n_pairs,
                                                                    int64_t *__restrict__ len)
{
    const I *const indices = static_cast<const I *>(m.indices);
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (DB_THREADS / 64);
    for (int64_t s = blockIdx.x * (int64_t)(DB_THREADS / 64) + (threadIdx.x >> 6); s <= n_pairs; s += waves) {
        if (s == n_pairs) {   // wave-uniform
            if (lane == 0) len[s] = 0;
            continue;
        }
        Row A = row_of(m, parents[2 * s]), B = row_of(m, parents[2 * s + 1]);
        if (A.len > B.len) { const Row t = A; A = B; B = t; }
        int64_t shared = 0;   // wave-uniform
        for (int64_t base = 0; base < A.len; base += DOUBLET_PIECE) {
            const int64_t i = base + lane;
            bool match = false;
            if (i < A.len) {
                const long long c = (long long)indices[A.from + i];
                const int64_t pos = lower_bound(indices + B.from, B.len, c);
                match = pos < B.len && (long long)indices[B.from + pos] == c;
            }
            shared += __popcll(__ballot(match));
        }
        if (lane == 0) len[s] = A.len + B.len - shared;
    }
}

// One parent's share of output row s.  `home` is walked; a lane's entry goes to out + its rank at home + its rank in
// `other` - the shared columns before it.  first: write every entry, a shared one with the other parent's value added;
// else: only the entries the other parent does not hold
template <typename I, bool first>
__device__ __forceinline__ void doublet_place(const Matrix &m, const I *__restrict__ indices, const Row home, const Row other, int lane,
                                              int64_t out, int32_t *__restrict__ out_indices, int32_t *__restrict__ out_values)
{
    int64_t carry = 0;   // the shared columns of the earlier pieces: wave-uniform
    for (int64_t base = 0; base < home.len; base += DOUBLET_PIECE) {
        const int64_t i = base + lane;
        const bool active = i < home.len;
        long long c = 0;
        int64_t pos = 0;
        bool match = false;
        int32_t v = 0;
        if (active) {
            c = (long long)indices[home.from + i];
            v = (int32_t)load_value(m.val, m.val_kind, home.from + i);   // asked for before the search, not behind it
            pos = lower_bound(indices + other.from, other.len, c);
            match = pos < other.len && (long long)indices[other.from + pos] == c;
        }
        const unsigned long long mask = __ballot(match);
        if (active && (first || !match)) {
            const int64_t before = carry + __popcll(mask & ((1ull << lane) - 1ull));
            const int64_t o = out + i + pos - before;   // < out + the row's length: the entries below this one, counted once
            if (first && match) v += (int32_t)load_value(m.val, m.val_kind, other.from + pos);
            out_indices[o] = (int32_t)c;
            out_values[o] = v;
        }
        carry += __popcll(mask);
    }
}

template <typename I>
__global__ __launch_bounds__(DB_THREADS) void doublet_fill_kernel(Matrix m, const int32_t *__restrict__ parents, int64_t n_pairs,
                                                                  const int64_t *__restrict__ out_indptr,
                                                                  int32_t *__restrict__ out_indices, int32_t *__restrict__ out_values)
{
    const I *const indices = static_cast<const I *>(m.indices);
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (DB_THREADS / 64);
    for (int64_t s = blockIdx.x * (int64_t)(DB_THREADS / 64) + (threadIdx.x >> 6); s < n_pairs; s += waves) {
        const Row A = row_of(m, parents[2 * s]), B = row_of(m, parents[2 * s + 1]);
        const int64_t out = out_indptr[s];
        doublet_place<I, true>(m, indices, A, B, lane, out, out_indices, out_values);
        doublet_place<I, false>(m, indices, B, A, lane, out, out_indices, out_values);
    }
}

void parents_on_device(hipStream_t st, int64_t first, int64_t n_sim, int64_t ncells, uint64_t seed, int32_t *parents)
{
    CSR_LAUNCH(doublet_parents_kernel, n_sim, DB_THREADS, st, (uint64_t)first, n_sim, (uint32_t)ncells, (uint32_t)seed,
           (uint32_t)(seed >> 32), parents);
    HIPCHK(hipStreamSynchronize(st));
}

// Everything on `st`, which is synchronised when this returns; all pointers are device memory, nnz and n_pairs are at least 1.
// The checks come first, indptr before anything that follows it into the entries: a refused call has written nothing.
// Returns the entries of the result; out_indices == nullptr: out_indptr alone is written
int64_t rows_on_device(hipStream_t st, const Matrix &m, int64_t nnz, int64_t n_pairs, const int32_t *parents, int64_t *out_indptr,
                       int32_t *out_indices, int32_t *out_values, int64_t capacity)
{
    const int per_wave = DB_THREADS / 64;
    DevBuf len;
    Scratch temp;
    Words w;
    w.reset(st);
    launch_indptr_check(st, m, nnz, w);
    w.fetch(st);
    w.refuse_indptr("doublets");
    launch_entries_check<CSR_COUNTS>(st, m, w);
    CSR_LAUNCH(doublet_pairs_kernel, n_pairs, DB_THREADS, st, parents, n_pairs, m.ncells, w.dev());
    w.fetch(st);
    w.refuse_entries("doublets");
    w.refuse(W_BAD_ROW, doublet_bad_parent);

    const bool wide = m.idx_kind == SCHPF_IDX_I64;
    len.alloc((size_t)(n_pairs + 1) * sizeof(int64_t));
    if (wide) CSR_LAUNCH(doublet_length_kernel<long long>, n_pairs + 1, per_wave, st, m, parents, n_pairs, len.as<int64_t>());
    else CSR_LAUNCH(doublet_length_kernel<int>, n_pairs + 1, per_wave, st, m, parents, n_pairs, len.as<int64_t>());
    exclusive_scan(st, temp, len.as<int64_t>(), out_indptr, (size_t)(n_pairs + 1));
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, out_indptr + n_pairs, sizeof total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!out_indices) return total;
    if (capacity < total) throw std::invalid_argument(csr_bad_capacity(capacity, total));
    if (total > 0) {
        if (wide) CSR_LAUNCH(doublet_fill_kernel<long long>, n_pairs, per_wave, st, m, parents, n_pairs, out_indptr, out_indices, out_values);
        else CSR_LAUNCH(doublet_fill_kernel<int>, n_pairs, per_wave, st, m, parents, n_pairs, out_indptr, out_indices, out_values);
    }
    HIPCHK(hipStreamSynchronize(st));   // before the scratch is released
    return total;
}

}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_doublet_parents_device(int device, void *stream, int64_t first, int64_t n_sim, int64_t ncells, uint64_t seed,
                                 int32_t *parents)
{
    if (const char *why = doublet_parents_bad_args(first, n_sim, ncells, parents)) return fail("%s", why);
    return guarded([&] {
        use_device(device);
        if (n_sim == 0) return;
        std::unique_ptr<TempStream> own;
        parents_on_device(pick_stream(stream, own), first, n_sim, ncells, seed, parents);
    });
}

int schpf_doublet_rows_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr,
                              int indptr_kind, const void *indices, int idx_kind, const void *val, int val_kind, int64_t n_pairs,
                              const int32_t *parents, int64_t *out_indptr, int32_t *out_indices, int32_t *out_values,
                              int64_t capacity)
{
    if (const char *why = doublet_rows_bad_args(ncells, ngenes, nnz, indptr, indices, val, n_pairs, parents, out_indptr, out_indices,
                                                out_values, capacity))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(indptr_kind, idx_kind, val_kind)) throw std::invalid_argument("unknown index or value kind");
        use_device(device);
        std::unique_ptr<TempStream> own;
        if (n_pairs == 0 || nnz == 0) {   // every row of the result is empty: no input is read
            if (!out_indptr) return;
            hipStream_t st = pick_stream(stream, own);
            HIPCHK(hipMemsetAsync(out_indptr, 0, (size_t)(n_pairs + 1) * sizeof(int64_t), st));
            HIPCHK(hipStreamSynchronize(st));
            return;
        }
        const Matrix m{ncells, ngenes, indptr, indices, val, indptr_kind, idx_kind, val_kind};
        rows_on_device(pick_stream(stream, own), m, nnz, n_pairs, parents, out_indptr, out_indices, out_values, capacity);
    });
}

int schpf_doublet_rows(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                       const void *val, int val_kind, int64_t n_pairs, const int32_t *parents, int64_t *out_indptr,
                       int32_t *out_indices, int32_t *out_values, int64_t capacity)
{
    if (const char *why = doublet_rows_bad_args(ncells, ngenes, nnz, indptr, indices, val, n_pairs, parents, out_indptr, out_indices,
                                                out_values, capacity))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind)) throw std::invalid_argument("unknown index or value kind");
        use_device(device);
        if (n_pairs == 0 || nnz == 0) {
            if (out_indptr) std::fill(out_indptr, out_indptr + n_pairs + 1, (int64_t)0);
            return;
        }
        TempStream ts;
        DevBuf d_indptr, d_indices, d_val, d_parents, d_out_indptr, d_out_indices, d_out_values;
        h2d<int64_t>(d_indptr, indptr, (size_t)ncells + 1, ts.st);
        h2d<int32_t>(d_indices, indices, (size_t)nnz, ts.st);
        h2d<char>(d_val, val, (size_t)nnz * value_size(val_kind), ts.st);
        h2d<int32_t>(d_parents, parents, (size_t)n_pairs * 2, ts.st);
        d_out_indptr.alloc((size_t)(n_pairs + 1) * sizeof(int64_t));
        if (out_indices) {
            d_out_indices.alloc((size_t)capacity * sizeof(int32_t));
            d_out_values.alloc((size_t)capacity * sizeof(int32_t));
        }
        const Matrix m{ncells, ngenes, d_indptr.p, d_indices.p, d_val.p, SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind};
        const int64_t total = rows_on_device(ts.st, m, nnz, n_pairs, d_parents.as<int32_t>(), d_out_indptr.as<int64_t>(),
                                             out_indices ? d_out_indices.as<int32_t>() : nullptr,
                                             out_indices ? d_out_values.as<int32_t>() : nullptr, capacity);
        if (out_indices && total > 0) {
            HIPCHK(hipMemcpyAsync(out_indices, d_out_indices.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, ts.st));
            HIPCHK(hipMemcpyAsync(out_values, d_out_values.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, ts.st));
        }
        d2h(out_indptr, d_out_indptr, (size_t)(n_pairs + 1) * sizeof(int64_t), ts.st);
    });
}

}  // extern "C"
