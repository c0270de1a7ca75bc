// Count thinning on the device (schpf_thin_counts / schpf_thin_counts_device): every stored count x is
// split into x_test ~ Binomial(x, frac) and x_train = x - x_test with the counter-based draw of philox.h.  Two passes on
// the caller's stream: the light pass validates every entry and draws the small counts, one entry per lane; the heavy
// pass gives each count above THIN_LIGHT_MAX a wavefront.  Integer arithmetic only: host.cpp's serial restatement gives
// the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <memory>

#include "csr_words.h"
#include "device_call.h"
#include "philox.h"

namespace schpf {
namespace {

constexpr int TH_THREADS = 256;
constexpr unsigned TH_BLOCKS = 4096;   // workgroups of a pass at the most: every wavefront ends in atomics
// the words both passes share in device memory: the four statistics of the C ABI, the length of the heavy list, and
// the smallest offending entries
enum { W_TRAIN_NNZ = 0, W_TEST_NNZ, W_TRAIN_SUM, W_TEST_SUM, W_HEAVY, W_BAD_INDEX, W_BAD_VALUE, W_COUNT };

__device__ __forceinline__ long long load_index(const void *p, int kind, int64_t j)
{
    return kind == SCHPF_IDX_I64 ? static_cast<const long long *>(p)[j] : (long long)static_cast<const int *>(p)[j];
}
// entry j of a value array of kind SCHPF_VAL_* (common.h read_count)
__device__ __forceinline__ double load_value(const void *p, int kind, int64_t j)
{
    switch (kind) {
    case SCHPF_VAL_I32: return (double)static_cast<const int *>(p)[j];
    case SCHPF_VAL_I64: return (double)static_cast<const long long *>(p)[j];
    case SCHPF_VAL_F32: return (double)static_cast<const float *>(p)[j];
    default: return static_cast<const double *>(p)[j];
    }
}

struct ThinArgs {
    int64_t nnz;
    const void *row, *col, *val;
    int idx_kind, val_kind;
    uint32_t k0, k1, T;
    int32_t *train, *test;
    int32_t *heavy;   // [nnz]: the entries the heavy pass draws
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the pair of one entry and its share of the statistics
struct Tally {
    unsigned long long train_nnz = 0, test_nnz = 0, train_sum = 0, test_sum = 0;
    __device__ __forceinline__ void add(uint32_t x, uint32_t hits)
    {
        train_nnz += x > hits;
        test_nnz += hits > 0;
        train_sum += x - hits;
        test_sum += hits;
    }
};

// One entry per lane, grid-stride.  An invalid entry is recorded (atomicMin at the end of the wavefront's walk) and
// never drawn; a count above THIN_LIGHT_MAX is appended to the heavy list.  Every lane of a wavefront leaves the loop
// before the reductions: no early return.
__global__ __launch_bounds__(TH_THREADS) void thin_light_kernel(ThinArgs a, unsigned long long *__restrict__ words)
{
    Tally tally;
    unsigned long long bad_index = NONE, bad_value = NONE;
    for (int64_t e = blockIdx.x * (int64_t)TH_THREADS + threadIdx.x; e < a.nnz; e += (int64_t)gridDim.x * TH_THREADS) {
        const long long r = load_index(a.row, a.idx_kind, e), c = load_index(a.col, a.idx_kind, e);
        const double d = load_value(a.val, a.val_kind, e);
        if (thin_index_bad(r) || thin_index_bad(c)) {
            offends(bad_index, e);
            continue;
        }
        if (thin_value_bad(d)) {
            offends(bad_value, e);
            continue;
        }
        const uint32_t x = (uint32_t)d;
        if (x > THIN_LIGHT_MAX) {
            const unsigned long long slot = atomicAdd(words + W_HEAVY, 1ull);   // < nnz: one append per entry at most
            a.heavy[slot] = (int32_t)e;
            continue;
        }
        const uint32_t hits = thin_draw((uint32_t)r, (uint32_t)c, x, a.k0, a.k1, a.T);
        a.train[e] = (int32_t)(x - hits);
        a.test[e] = (int32_t)hits;
        tally.add(x, hits);
    }
    tally.train_nnz = wave_sum(tally.train_nnz);
    tally.test_nnz = wave_sum(tally.test_nnz);
    tally.train_sum = wave_sum(tally.train_sum);
    tally.test_sum = wave_sum(tally.test_sum);
    report_min(words + W_BAD_INDEX, bad_index);
    report_min(words + W_BAD_VALUE, bad_value);
    if ((threadIdx.x & 63) == 0) {
        if (tally.train_nnz) atomicAdd(words + W_TRAIN_NNZ, tally.train_nnz);
        if (tally.test_nnz) atomicAdd(words + W_TEST_NNZ, tally.test_nnz);
        if (tally.train_sum) atomicAdd(words + W_TRAIN_SUM, tally.train_sum);
        if (tally.test_sum) atomicAdd(words + W_TEST_SUM, tally.test_sum);
    }
}

// One wavefront per listed entry (the list holds validated entries only): lane l draws the blocks l, l + 64, ...; the
// integer counts are summed across the wavefront, lane 0 writes the pair and keeps the wavefront's tally.
__global__ __launch_bounds__(TH_THREADS) void thin_heavy_kernel(ThinArgs a, int64_t n_heavy, unsigned long long *__restrict__ words)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (TH_THREADS / 64);
    Tally tally;   // lane 0's
    for (int64_t i = blockIdx.x * (int64_t)(TH_THREADS / 64) + (threadIdx.x >> 6); i < n_heavy; i += waves) {
        const int64_t e = a.heavy[i];
        const uint32_t r = (uint32_t)load_index(a.row, a.idx_kind, e), c = (uint32_t)load_index(a.col, a.idx_kind, e);
        const uint32_t x = (uint32_t)load_value(a.val, a.val_kind, e);   // <= 2^24: the light pass has checked it
        const uint32_t n_blocks = (x + 3u) >> 2;
        uint32_t hits = 0;
        for (uint32_t j = (uint32_t)lane; j < n_blocks; j += 64u) hits += thin_block_hits(r, c, j, x, a.k0, a.k1, a.T);
        for (int off = 32; off > 0; off >>= 1) hits += __shfl_xor(hits, off);
        if (lane == 0) {
            a.train[e] = (int32_t)(x - hits);
            a.test[e] = (int32_t)hits;
            tally.add(x, hits);
        }
    }
    if (lane == 0) {
        if (tally.train_nnz) atomicAdd(words + W_TRAIN_NNZ, tally.train_nnz);
        if (tally.test_nnz) atomicAdd(words + W_TEST_NNZ, tally.test_nnz);
        if (tally.train_sum) atomicAdd(words + W_TRAIN_SUM, tally.train_sum);
        if (tally.test_sum) atomicAdd(words + W_TEST_SUM, tally.test_sum);
    }
}

struct ThinOutcome {
    int64_t stats[4] = {0, 0, 0, 0};
    int64_t first_bad_index = -1, first_bad_value = -1;   // smallest offending entry of this call's range; -1: none
};

// the scratch of a call: the shared words and the heavy list (capacity entries)
struct ThinScratch {
    DevBuf words, heavy;
    void alloc(int64_t capacity)
    {
        words.alloc(W_COUNT * sizeof(unsigned long long));
        heavy.alloc((size_t)capacity * sizeof(int32_t));
    }
};

// Both passes over nnz > 0 entries in device memory, on `st`; synchronises it.  The outputs of a call that reports an
// offender are incomplete.
ThinOutcome thin_on_device(hipStream_t st, ThinScratch &scratch, int64_t nnz, const void *row, const void *col, int idx_kind,
                           const void *val, int val_kind, uint32_t T, uint64_t seed, int32_t *train, int32_t *test)
{
    unsigned long long *words = scratch.words.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(words, 0, W_BAD_INDEX * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(words + W_BAD_INDEX, 0xFF, 2 * sizeof(unsigned long long), st));   // NONE
    const ThinArgs a{nnz, row, col, val, idx_kind, val_kind, (uint32_t)seed, (uint32_t)(seed >> 32), T, train, test,
                     scratch.heavy.as<int32_t>()};
    hipLaunchKernelGGL(thin_light_kernel, dim3(std::min(grid_for(nnz, TH_THREADS), TH_BLOCKS)), dim3(TH_THREADS), 0, st, a, words);
    HIPCHK(hipGetLastError());
    unsigned long long h[W_COUNT];
    d2h(h, scratch.words, sizeof h, st);   // the one small copy between the passes
    ThinOutcome out;
    out.first_bad_index = h[W_BAD_INDEX] == NONE ? -1 : (int64_t)h[W_BAD_INDEX];
    out.first_bad_value = h[W_BAD_VALUE] == NONE ? -1 : (int64_t)h[W_BAD_VALUE];
    const int64_t n_heavy = (int64_t)h[W_HEAVY];
    if (n_heavy > nnz) throw std::logic_error("thinning: the heavy list is longer than the matrix");
    if (n_heavy > 0 && out.first_bad_index < 0 && out.first_bad_value < 0) {
        hipLaunchKernelGGL(thin_heavy_kernel, dim3(std::min(grid_for(n_heavy, TH_THREADS / 64), TH_BLOCKS)), dim3(TH_THREADS), 0, st, a, n_heavy,
                           words);
        HIPCHK(hipGetLastError());
        d2h(h, scratch.words, W_BAD_INDEX * sizeof(unsigned long long), st);
    }
    for (int k = 0; k < 4; ++k) out.stats[k] = (int64_t)h[k];
    return out;
}

void check_kinds(int idx_kind, int val_kind)
{
    if (idx_kind != SCHPF_IDX_I32 && idx_kind != SCHPF_IDX_I64) throw std::invalid_argument("unknown index kind");
    if (val_kind < SCHPF_VAL_I32 || val_kind > SCHPF_VAL_F64) throw std::invalid_argument("unknown value kind");
}

uint32_t threshold_or_throw(double frac)
{
    uint32_t T = 0;
    if (!thin_threshold(frac, &T)) throw std::invalid_argument("frac must be in (0, 1) and at least 2^-32");
    return T;
}

// an index error before a value error, the rule of schpf_upload_coo_device
void throw_offender(int64_t first_bad_index, int64_t first_bad_value)
{
    if (first_bad_index >= 0)
        throw std::invalid_argument("COO index out of range at entry " + std::to_string(first_bad_index));
    if (first_bad_value >= 0)
        throw std::invalid_argument("thinning needs integer counts in [0, 2^24]; offending entry " +
                                    std::to_string(first_bad_value));
}


}  // namespace
}  // namespace schpf

using namespace schpf;

extern "C" {

int schpf_thin_counts_device(int device, void *stream, int64_t nnz, const void *row, const void *col, int idx_kind,
                             const void *val, int val_kind, double frac, uint64_t seed, int32_t *train, int32_t *test,
                             int64_t stats[4])
{
    if (!stats) return fail("stats is NULL");
    if (nnz < 0 || nnz >= (1ll << 31)) return fail("nnz must be in [0, 2^31)");
    if (nnz > 0 && (!row || !col || !val || !train || !test))
        return fail("row, col, val, train and test must be device pointers, not NULL");
    return guarded([&] {
        check_kinds(idx_kind, val_kind);
        const uint32_t T = threshold_or_throw(frac);
        use_device(device);
        for (int k = 0; k < 4; ++k) stats[k] = 0;
        if (nnz == 0) return;
        std::unique_ptr<TempStream> own;
        hipStream_t st = pick_stream(stream, own);
        ThinScratch scratch;
        scratch.alloc(nnz);
        const ThinOutcome out = thin_on_device(st, scratch, nnz, row, col, idx_kind, val, val_kind, T, seed, train, test);
        throw_offender(out.first_bad_index, out.first_bad_value);
        for (int k = 0; k < 4; ++k) stats[k] = out.stats[k];
    });
}

int schpf_thin_counts(int device, int64_t nnz, const int32_t *row, const int32_t *col, const void *val, int val_kind,
                      double frac, uint64_t seed, int32_t *train, int32_t *test, int64_t stats[4])
{
    if (!stats) return fail("stats is NULL");
    if (nnz < 0 || nnz >= (1ll << 31)) return fail("nnz must be in [0, 2^31)");
    if (nnz > 0 && (!row || !col || !val || !train || !test)) return fail("row, col, val, train and test must not be NULL");
    return guarded([&] {
        check_kinds(SCHPF_IDX_I32, val_kind);
        const uint32_t T = threshold_or_throw(frac);
        use_device(device);
        for (int k = 0; k < 4; ++k) stats[k] = 0;
        if (nnz == 0) return;
        // slabs of the entries go through the device one after the other; $SCHPF_THIN_SLAB (entries) is for tests
        int64_t slab = 1 << 22;
        if (const char *e = getenv("SCHPF_THIN_SLAB")) slab = std::max<int64_t>(1, atoll(e));
        slab = std::min(slab, nnz);
        const size_t vs = value_size(val_kind);
        TempStream ts;
        ThinScratch scratch;
        scratch.alloc(slab);
        DevBuf d_row, d_col, d_val, d_train, d_test;
        d_row.alloc((size_t)slab * 4); d_col.alloc((size_t)slab * 4); d_val.alloc((size_t)slab * vs);
        d_train.alloc((size_t)slab * 4); d_test.alloc((size_t)slab * 4);
        // every slab is looked at, also after an offender: the smallest index offender of the WHOLE matrix goes first
        int64_t first_bad_index = -1, first_bad_value = -1, total[4] = {0, 0, 0, 0};
        for (int64_t b = 0; b < nnz; b += slab) {
            const int64_t n = std::min(slab, nnz - b);
            HIPCHK(hipMemcpyAsync(d_row.p, row + b, (size_t)n * 4, hipMemcpyHostToDevice, ts.st));
            HIPCHK(hipMemcpyAsync(d_col.p, col + b, (size_t)n * 4, hipMemcpyHostToDevice, ts.st));
            HIPCHK(hipMemcpyAsync(d_val.p, (const char *)val + (size_t)b * vs, (size_t)n * vs, hipMemcpyHostToDevice, ts.st));
            const ThinOutcome out = thin_on_device(ts.st, scratch, n, d_row.p, d_col.p, SCHPF_IDX_I32, d_val.p, val_kind, T, seed,
                                                   d_train.as<int32_t>(), d_test.as<int32_t>());
            if (out.first_bad_index >= 0 && first_bad_index < 0) first_bad_index = b + out.first_bad_index;
            if (out.first_bad_value >= 0 && first_bad_value < 0) first_bad_value = b + out.first_bad_value;
            if (first_bad_index >= 0 || first_bad_value >= 0) continue;
            HIPCHK(hipMemcpyAsync(train + b, d_train.p, (size_t)n * 4, hipMemcpyDeviceToHost, ts.st));
            HIPCHK(hipMemcpyAsync(test + b, d_test.p, (size_t)n * 4, hipMemcpyDeviceToHost, ts.st));
            HIPCHK(hipStreamSynchronize(ts.st));
            for (int k = 0; k < 4; ++k) total[k] += out.stats[k];
        }
        throw_offender(first_bad_index, first_bad_value);
        for (int k = 0; k < 4; ++k) stats[k] = total[k];
    });
}

}  // extern "C"
