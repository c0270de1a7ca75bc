// What every translation unit behind the C ABI shares: the per-thread error string of schpf_last_error, the exception ->
// status mapping of an entry point (guarded), and the RAII device buffer with its small copy helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/schpf_hip.h"
#include "plan.h"

namespace schpf {

extern thread_local std::string g_err;   // one per thread for ALL entry points; defined in capi.hip (schpf_last_error)

inline int fail(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

struct HipError : std::runtime_error {
    hipError_t code;
    HipError(const std::string &what, hipError_t code_ = hipErrorUnknown) : std::runtime_error(what), code(code_) {}
};

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            char b_[512];                                                                    \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                     __FILE__, __LINE__);                                                    \
            throw schpf::HipError(b_, e_);                                                   \
        }                                                                                    \
    } while (0)

template <typename F> int guarded(F &&f)
{
    // status SCHPF_ERR_NO_MEMORY: the device (hipErrorOutOfMemory) or the host (std::bad_alloc while building plans) ran
    // out of memory -- the one failure a caller may answer with a smaller layout; everything else is 1
    try {
        f();
        return 0;
    } catch (const HipError &e) {
        g_err = e.what();
        if (e.code == hipErrorOutOfMemory) (void)hipGetLastError();
        return e.code == hipErrorOutOfMemory ? SCHPF_ERR_NO_MEMORY : 1;
    } catch (const DeviceNoMemory &e) {
        g_err = e.what();
        return SCHPF_ERR_NO_MEMORY;
    } catch (const std::bad_alloc &) {
        g_err = "out of host memory (std::bad_alloc)";
        return SCHPF_ERR_NO_MEMORY;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    } catch (...) {
        g_err = "unknown error";
        return 1;
    }
}

inline bool bad_dtype(int dtype) { return dtype != SCHPF_F32 && dtype != SCHPF_F64; }

// entry i of a caller's value array of kind SCHPF_VAL_*
inline double read_count(const void *val, int kind, int64_t i)
{
    switch (kind) {
    case SCHPF_VAL_I32: return (double)((const int32_t *)val)[i];
    case SCHPF_VAL_I64: return (double)((const int64_t *)val)[i];
    case SCHPF_VAL_F32: return (double)((const float *)val)[i];
    default: return ((const double *)val)[i];
    }
}

// What schpf_knn, schpf_knn_device and schpf_debug_knn refuse alike (include/schpf_hip.h); n_query = 0 is asked first by
// the caller.  nullptr: the arguments are fine
inline const char *knn_bad_args(int dtype, int n_query, int n_ref, int nfactors, const void *query, const void *ref, int k,
                                int64_t self_first, const void *idx, const void *d2)
{
    if (bad_dtype(dtype)) return "dtype must be SCHPF_F32 or SCHPF_F64";
    if (nfactors < 1 || nfactors > 256) return "nfactors must be in [1, 256]";
    if (k < 1 || k > 128) return "k must be in [1, 128]";
    if (self_first < -1) return "self_first must be -1 or the reference row of query row 0";
    if (n_query < 0 || n_query > INT32_MAX - 128 || n_ref > INT32_MAX - 128) return "n_query and n_ref must be in [0, 2^31 - 128)";
    if (n_query == 0) return nullptr;
    if (n_ref < 1) return "n_ref must be at least 1";
    if (!query || !ref || !idx || !d2) return "query, ref, idx and d2 must not be NULL";
    // query row 0 loses a reference row iff self_first names one, and no row loses more than one
    const int admissible = n_ref - (self_first >= 0 && self_first < n_ref ? 1 : 0);
    if (k > admissible) return "k must be at most the admissible reference rows of every query row";
    return nullptr;
}

// What schpf_knn_graph, schpf_knn_graph_device and schpf_debug_knn_graph refuse alike (include/schpf_hip.h); n = 0 is asked
// next by the caller.  nullptr: the arguments are fine
inline const char *graph_bad_args(int method, int n, int k, const void *idx, const void *dist, const void *indptr,
                                  const void *indices, const void *data)
{
    if (method != SCHPF_GRAPH_UMAP && method != SCHPF_GRAPH_JACCARD) return "method must be SCHPF_GRAPH_UMAP or SCHPF_GRAPH_JACCARD";
    if (k < 1 || k > 128) return "k must be in [1, 128]";
    if (n < 0 || n > INT32_MAX - 128) return "n must be in [0, 2^31 - 128)";
    if (n == 0) return nullptr;
    if (k > n - 1) return "k must be at most n - 1: the rows other than the row itself";
    if (!idx || !indptr || !indices || !data) return "idx, indptr, indices and data must not be NULL";
    if (method == SCHPF_GRAPH_UMAP && !dist) return "dist must not be NULL for SCHPF_GRAPH_UMAP";
    return nullptr;
}
inline std::string graph_bad_lists(int64_t row)
{
    return "neighbour lists must hold k distinct rows other than the row itself; offending row " + std::to_string(row);
}
inline std::string graph_bad_distances(int64_t row) { return "distances must be finite and >= 0; offending row " + std::to_string(row); }

// What schpf_louvain, schpf_louvain_device and schpf_debug_louvain refuse alike (include/schpf_hip.h); n = 0 is asked next
// by the caller.  nullptr: the arguments are fine
inline const char *louvain_bad_args(int n, const void *indptr, double gamma, const void *labels, const void *stats)
{
    if (n < 0 || n > INT32_MAX - 128) return "n must be in [0, 2^31 - 128)";
    if (!(gamma > 0.0 && gamma <= 1.7976931348623157e308)) return "gamma must be finite and > 0";
    if (!stats) return "stats must not be NULL";
    if (n == 0) return nullptr;
    if (!indptr || !labels) return "indptr and labels must not be NULL";
    return nullptr;
}
inline const char *louvain_bad_nnz(int64_t nnz, const void *indices, const void *data)
{
    if (nnz >= (int64_t)1 << 32) return "nnz must be below 2^32";
    if (nnz > 0 && (!indices || !data)) return "indices and data must not be NULL";
    return nullptr;
}
inline std::string louvain_bad_indptr(int64_t row)
{
    return "indptr must be 0 at row 0 and must be non-decreasing; offending row " + std::to_string(row);
}
inline std::string louvain_bad_columns(int64_t row)
{
    return "columns must be in [0, n) and strictly ascending within a row; offending row " + std::to_string(row);
}
inline std::string louvain_bad_values(int64_t row) { return "values must be finite and >= 0; offending row " + std::to_string(row); }
constexpr int LOUVAIN_ROUNDS = 32, LOUVAIN_LEVELS = 32;   // the caps of the definition

// What schpf_components, schpf_components_device and schpf_debug_components refuse alike before anything is read
// (include/schpf_hip.h); n = 0 is asked next by the caller.  nullptr: the arguments are fine
inline const char *components_bad_args(int n, const void *indptr, const void *comp, const void *stats)
{
    if (n < 0) return "n must be in [0, 2^31)";
    if (!stats) return "stats must not be NULL";
    if (n == 0) return nullptr;
    if (!indptr || !comp) return "indptr and comp must not be NULL";
    return nullptr;
}
inline const char *components_bad_nnz(int64_t nnz, const void *indices)
{
    if (nnz >= (int64_t)1 << 32) return "nnz must be below 2^32";
    if (nnz > 0 && !indices) return "indices must not be NULL";
    return nullptr;
}
inline std::string graph_bad_columns(int64_t row) { return "columns must be in [0, n); offending row " + std::to_string(row); }
inline std::string components_bad_within(int64_t vertex)
{
    return "components: within must be >= -1; offending vertex " + std::to_string(vertex);
}

// What schpf_cluster_graph, schpf_cluster_graph_device and schpf_debug_cluster_graph refuse alike before anything is read
inline const char *cluster_graph_bad_args(int n, const void *indptr, const void *labels, int ngroups, const void *group_cells,
                                          const void *count, const void *wmax)
{
    if (n < 0) return "n must be in [0, 2^31)";
    if (ngroups < 1) return "ngroups must be at least 1";
    if ((int64_t)ngroups * (int64_t)ngroups >= (int64_t)1 << 31) return "ngroups * ngroups must be below 2^31";
    if (!group_cells || !count || !wmax) return "group_cells, count and wmax must not be NULL";
    if (n == 0) return nullptr;
    if (!indptr || !labels) return "indptr and labels must not be NULL";
    return nullptr;
}
inline std::string cluster_graph_bad_labels(int64_t vertex)
{
    return "cluster_graph: labels must be in [-1, G); offending vertex " + std::to_string(vertex);
}

// What schpf_geodesic, schpf_geodesic_device and schpf_debug_geodesic refuse alike before anything is read
// (include/schpf_hip.h); n = 0 or nsets = 0 is asked next by the caller.  nullptr: the arguments are fine.  The graph's own
// refusals are those of the components and of the cluster graph (components_bad_nnz, louvain_bad_indptr, graph_bad_columns,
// louvain_bad_values)
inline const char *geodesic_bad_args(int n, int nsets, const void *indptr, const void *set_ptr, const void *dist, const void *stats)
{
    if (n < 0) return "n must be in [0, 2^31)";
    if (nsets < 0) return "nsets must be in [0, 2^31)";
    if (!stats) return "stats must not be NULL";
    if (n == 0 || nsets == 0) return nullptr;
    if ((int64_t)nsets * (int64_t)n > INT64_MAX / 8) return "the bytes of dist, 8 * nsets * n, must be below 2^63";
    if (!indptr || !set_ptr || !dist) return "indptr, set_ptr and dist must not be NULL";
    return nullptr;
}
inline std::string geodesic_bad_set_ptr(int64_t set)
{
    return "geodesic: set_ptr must be 0 at set 0 and must be non-decreasing; offending set " + std::to_string(set);
}
inline std::string geodesic_bad_roots(int64_t set) { return "geodesic: roots must be in [0, n); offending set " + std::to_string(set); }

// What schpf_rank_sums, schpf_rank_sums_device and schpf_debug_rank_sums refuse alike (include/schpf_hip.h), before anything
// is read; ncells = 0 or ngenes = 0 is asked next by the caller.  nullptr: the arguments are fine
constexpr int RANK_SUMS_MAX_CELLS = 1 << 21;   // the tie term, a sum of cubes, stays under 2^63
inline const char *rank_sums_bad_args(int ncells, int ngenes, int ngroups, const void *indptr, const void *labels, const void *n,
                                      const void *zeros, const void *ties, const void *nexpr, const void *rank2)
{
    if (ncells < 0 || ncells >= RANK_SUMS_MAX_CELLS) return "ncells must be in [0, 2^21)";
    if (ngenes < 0) return "ngenes must be >= 0";
    if (ngroups < 1) return "ngroups must be at least 1";
    if ((int64_t)ngroups * (int64_t)ngenes >= (int64_t)1 << 31) return "ngroups * ngenes must be below 2^31";
    if (ncells == 0 || ngenes == 0) return nullptr;
    if (!indptr || !labels) return "indptr and labels must not be NULL";
    if (!n || !zeros || !ties || !nexpr || !rank2) return "n, zeros, ties, nexpr and rank2 must not be NULL";
    return nullptr;
}
inline const char *rank_sums_bad_nnz(int64_t nnz, const void *indices, const void *data)
{
    if (nnz >= (int64_t)1 << 32) return "nnz must be below 2^32";
    if (nnz > 0 && (!indices || !data)) return "indices and data must not be NULL";
    return nullptr;
}
inline std::string rank_sums_bad_indptr(int64_t gene)
{
    return "indptr must be 0 at gene 0 and must be non-decreasing; offending gene " + std::to_string(gene);
}
inline std::string rank_sums_bad_cells(int64_t gene)
{
    return "cell ids must be in [0, ncells) and strictly ascending within a gene; offending gene " + std::to_string(gene);
}
inline std::string rank_sums_bad_values(int64_t gene) { return "values must be finite and >= 0; offending gene " + std::to_string(gene); }
inline std::string rank_sums_bad_labels(int64_t cell) { return "labels must be in [-1, ngroups); offending cell " + std::to_string(cell); }

// What schpf_pair_rank_sums, schpf_pair_rank_sums_device and schpf_debug_pair_rank_sums refuse alike before anything is
// read: the refusals of the rank sums in their order, with those of the pairs where the sizes and the pointers are asked
inline const char *pair_rank_sums_bad_args(int ncells, int ngenes, int ngroups, const void *indptr, const void *labels,
                                           const void *pairs, int npairs, const void *n, const void *nexpr, const void *u2,
                                           const void *ties)
{
    if (ncells < 0 || ncells >= RANK_SUMS_MAX_CELLS) return "ncells must be in [0, 2^21)";
    if (ngenes < 0) return "ngenes must be >= 0";
    if (ngroups < 1) return "ngroups must be at least 1";
    if ((int64_t)ngroups * (int64_t)ngenes >= (int64_t)1 << 31) return "ngroups * ngenes must be below 2^31";
    if (npairs < 0) return "npairs must be >= 0";
    if ((int64_t)npairs * (int64_t)ngenes >= (int64_t)1 << 31) return "npairs * ngenes must be below 2^31";
    if (ncells == 0 || ngenes == 0) return nullptr;
    if (!indptr || !labels) return "indptr and labels must not be NULL";
    if (npairs > 0 && !pairs) return "pairs must not be NULL";
    if (!n || !nexpr || (npairs > 0 && (!u2 || !ties))) return "n, nexpr, u2 and ties must not be NULL";
    return nullptr;
}
inline std::string pair_rank_sums_bad_pairs(int64_t pair)
{
    return "pairs must name two different groups in [0, ngroups); offending pair " + std::to_string(pair);
}

// RAII device buffer
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { adopt(o.p, o.bytes); o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // takes ownership of a hipMalloc'ed pointer (plan_device.hip hands its results over as void *)
    void adopt(void *p_, size_t bytes_)
    {
        release();
        p = p_;
        bytes = bytes_;
    }
    void alloc(size_t n, bool zero = false, hipStream_t st = nullptr)
    {
        release();
        bytes = n ? n : 16;
        HIPCHK(hipMalloc(&p, bytes));
        if (zero) HIPCHK(hipMemsetAsync(p, 0, bytes, st));
    }
    template <typename U> U *as() const { return reinterpret_cast<U *>(p); }
};

template <typename U, typename A> void upload(DevBuf &b, const std::vector<U, A> &v, hipStream_t st)
{
    b.alloc(v.size() * sizeof(U));
    if (!v.empty()) HIPCHK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice, st));
}

template <typename U> void h2d(DevBuf &b, const void *src, size_t count, hipStream_t st)
{
    b.alloc(count * sizeof(U));
    if (count) HIPCHK(hipMemcpyAsync(b.p, src, count * sizeof(U), hipMemcpyHostToDevice, st));
}
inline void d2h(void *dst, const DevBuf &b, size_t bytes, hipStream_t st)
{
    if (bytes) HIPCHK(hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

struct TempStream {
    hipStream_t st = nullptr;
    TempStream() { HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); }
    ~TempStream() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } }
};

// f(1, st) on a helper thread -- bound to `device`; st is a stream of its own, drained before the thread ends, where
// the caller asks for one, else nullptr -- while f(0, mine) runs here.  Joins; the caller's own exception goes first,
// else the helper's is rethrown
template <typename F> void on_both_sides(int device, hipStream_t mine, bool own_stream, F &&f)
{
    std::exception_ptr err;
    std::thread helper([&] {
        try {
            HIPCHK(hipSetDevice(device));
            if (!own_stream) { f(1, (hipStream_t) nullptr); return; }
            TempStream ts;
            f(1, ts.st);
            HIPCHK(hipStreamSynchronize(ts.st));
        } catch (...) { err = std::current_exception(); }
    });
    try { f(0, mine); } catch (...) { helper.join(); throw; }
    helper.join();
    if (err) std::rethrow_exception(err);
}

}  // namespace schpf
