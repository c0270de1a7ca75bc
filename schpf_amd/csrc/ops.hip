// The stateless operator mirrors of the C ABI (include/schpf_hip.h): each uploads its arguments, runs the kernels of
// one reference operator on a stream of its own and copies the result back.  No engine, no plan.
#include <algorithm>

#include "common.h"
#include "kernels.h"

using namespace schpf;

namespace {

void check_indices(int64_t nnz, const int32_t *ix, int n, const char *what)
{
    for (int64_t i = 0; i < nnz; ++i)
        if (ix[i] < 0 || ix[i] >= n) throw std::invalid_argument(std::string(what) + " index out of range");
}

template <typename T>
void xphi_or_llh(bool want_llh, int64_t nnz, int N, int G, int K, const void *x, const int32_t *row,
                 const int32_t *col, const void *ths, const void *thr, const void *bes, const void *ber, void *out)
{
    check_indices(nnz, row, N, "row");
    check_indices(nnz, col, G, "col");
    TempStream ts;
    DevBuf dx, dr, dc, a, b, c, d, tt, tb, o;
    h2d<T>(dx, x, (size_t)nnz, ts.st);
    h2d<int32_t>(dr, row, (size_t)nnz, ts.st);
    h2d<int32_t>(dc, col, (size_t)nnz, ts.st);
    h2d<T>(a, ths, (size_t)N * K, ts.st); h2d<T>(b, thr, (size_t)N * K, ts.st);
    h2d<T>(c, bes, (size_t)G * K, ts.st); h2d<T>(d, ber, (size_t)G * K, ts.st);
    tt.alloc((size_t)N * K * sizeof(T)); tb.alloc((size_t)G * K * sizeof(T));
    if (want_llh) {
        HIPCHK(schpf::launch_ratio<T>(a.as<T>(), b.as<T>(), (int64_t)N * K, tt.as<T>(), ts.st));
        HIPCHK(schpf::launch_ratio<T>(c.as<T>(), d.as<T>(), (int64_t)G * K, tb.as<T>(), ts.st));
        o.alloc((size_t)nnz * sizeof(T));
        HIPCHK(schpf::launch_llh_coo<T>(dx.as<T>(), dr.as<int>(), dc.as<int>(), tt.as<T>(), tb.as<T>(), nnz, K,
                                        o.as<T>(), ts.st));
        d2h(out, o, (size_t)nnz * sizeof(T), ts.st);
    } else {
        HIPCHK(schpf::launch_elog<T>(a.as<T>(), b.as<T>(), (int64_t)N * K, tt.as<T>(), ts.st));
        HIPCHK(schpf::launch_elog<T>(c.as<T>(), d.as<T>(), (int64_t)G * K, tb.as<T>(), ts.st));
        o.alloc((size_t)nnz * K * sizeof(T));
        HIPCHK(schpf::launch_xphi_coo<T>(dx.as<T>(), dr.as<int>(), dc.as<int>(), tt.as<T>(), tb.as<T>(), nnz, K,
                                         o.as<T>(), ts.st));
        d2h(out, o, (size_t)nnz * K * sizeof(T), ts.st);
    }
}

template <typename T>
void shape_update(int64_t nnz, int K, const void *xphi, const int32_t *keep, int nkeep, double prior, void *out)
{
    check_indices(nnz, keep, nkeep, "keep");
    schpf::BigVec<int32_t> order;
    std::vector<int64_t> ptr;
    schpf::counting_sort_positions(nnz, keep, nkeep, order, ptr);
    TempStream ts;
    DevBuf dx, dord, dptr, o;
    h2d<T>(dx, xphi, (size_t)nnz * K, ts.st);
    upload(dord, order, ts.st);
    upload(dptr, ptr, ts.st);
    o.alloc((size_t)nkeep * K * sizeof(T));
    HIPCHK(schpf::launch_shape_update<T>(dx.as<T>(), dord.as<int>(), dptr.as<int64_t>(), nkeep, K, prior,
                                         o.as<T>(), ts.st));
    d2h(out, o, (size_t)nkeep * K * sizeof(T), ts.st);
}

template <typename T>
void rate_update(int n, int m, int K, const void *ps, const void *pr, const void *os, const void *orr, void *out)
{
    TempStream ts;
    DevBuf a, b, c, d, part, S, o;
    h2d<T>(a, ps, (size_t)n, ts.st); h2d<T>(b, pr, (size_t)n, ts.st);
    h2d<T>(c, os, (size_t)m * K, ts.st); h2d<T>(d, orr, (size_t)m * K, ts.st);
    const int rb = 256 / K;
    const int nb = std::max(1, std::min((m + rb - 1) / rb, 512));
    part.alloc((size_t)nb * K * sizeof(double));
    S.alloc((size_t)K * sizeof(double));
    HIPCHK(schpf::launch_ratio_colsum<T>(c.as<T>(), d.as<T>(), m, K, part.as<double>(), nb, ts.st));
    HIPCHK(schpf::launch_colsum_reduce(part.as<double>(), nb, K, S.as<double>(), nullptr, 0, ts.st));
    o.alloc((size_t)n * K * sizeof(T));
    HIPCHK(schpf::launch_rate_update<T>(a.as<T>(), b.as<T>(), S.as<double>(), n, K, o.as<T>(), ts.st));
    d2h(out, o, (size_t)n * K * sizeof(T), ts.st);
}

template <typename T> void capacity_rate(int n, int K, const void *shape, const void *rate, double prior, void *out)
{
    TempStream ts;
    DevBuf a, b, o;
    h2d<T>(a, shape, (size_t)n * K, ts.st); h2d<T>(b, rate, (size_t)n * K, ts.st);
    o.alloc((size_t)n * sizeof(T));
    HIPCHK(schpf::launch_capacity_rate<T>(a.as<T>(), b.as<T>(), n, K, prior, o.as<T>(), ts.st));
    d2h(out, o, (size_t)n * sizeof(T), ts.st);
}

void special_array(bool gammaln, int64_t n, const double *x, double *out)
{
    TempStream ts;
    DevBuf a, o;
    h2d<double>(a, x, (size_t)n, ts.st);
    o.alloc((size_t)n * sizeof(double));
    if (gammaln) HIPCHK(schpf::launch_gammaln_array(a.as<double>(), n, o.as<double>(), ts.st));
    else HIPCHK(schpf::launch_digamma_array(a.as<double>(), n, o.as<double>(), ts.st));
    d2h(out, o, (size_t)n * sizeof(double), ts.st);
}

// f(T()) for the dtype's T, as an entry point: bad dtypes and exceptions become a status.  The one check of nfactors
// for all five operators, on the host and ahead of every allocation, upload and launch: at least 1 everywhere (the
// kernels read factor 0 of a row unasked), at most max_k where an operator has a limit -- ratio_colsum_kernel deals
// its 256 threads out as 256 / K rows of K factors, so the rate update stops at 256; the other four loop over K
template <typename F> int by_dtype(int dtype, int K, int max_k, F &&f)
{
    if (bad_dtype(dtype)) return fail("dtype must be SCHPF_F32 or SCHPF_F64");
    if (max_k > 0 && (K < 1 || K > max_k)) return fail("nfactors must be in [1, %d]", max_k);
    if (K < 1) return fail("nfactors must be at least 1");
    return guarded([&] {
        if (dtype == SCHPF_F64) f(double());
        else f(float());
    });
}

}  // namespace

extern "C" {

int schpf_digamma(int64_t n, const double *x, double *out) { return guarded([&] { special_array(false, n, x, out); }); }
int schpf_gammaln(int64_t n, const double *x, double *out) { return guarded([&] { special_array(true, n, x, out); }); }

int schpf_xphi(int dtype, int64_t nnz, int N, int G, int K, const void *x, const int32_t *row, const int32_t *col,
               const void *ths, const void *thr, const void *bes, const void *ber, void *out)
{
    return by_dtype(dtype, K, 0, [&](auto t) { xphi_or_llh<decltype(t)>(false, nnz, N, G, K, x, row, col, ths, thr, bes, ber, out); });
}
int schpf_pois_llh_pointwise(int dtype, int64_t nnz, int N, int G, int K, const void *x, const int32_t *row,
                             const int32_t *col, const void *ths, const void *thr, const void *bes,
                             const void *ber, void *out)
{
    return by_dtype(dtype, K, 0, [&](auto t) { xphi_or_llh<decltype(t)>(true, nnz, N, G, K, x, row, col, ths, thr, bes, ber, out); });
}
int schpf_shape_update(int dtype, int64_t nnz, int K, const void *xphi, const int32_t *keep, int nkeep,
                       double prior, void *out)
{
    return by_dtype(dtype, K, 0, [&](auto t) { shape_update<decltype(t)>(nnz, K, xphi, keep, nkeep, prior, out); });
}
int schpf_rate_update(int dtype, int n, int m, int K, const void *ps, const void *pr, const void *os,
                      const void *orr, void *out)
{
    return by_dtype(dtype, K, 256, [&](auto t) { rate_update<decltype(t)>(n, m, K, ps, pr, os, orr, out); });
}
int schpf_capacity_rate_update(int dtype, int n, int K, const void *shape, const void *rate, double prior,
                               void *out)
{
    return by_dtype(dtype, K, 0, [&](auto t) { capacity_rate<decltype(t)>(n, K, shape, rate, prior, out); });
}

}  // extern "C"
