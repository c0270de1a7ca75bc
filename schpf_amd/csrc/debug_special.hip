// Test hook schpf_debug_special (include/schpf_hip.h): the functions of special.h evaluated on the DEVICE, one thread per
// element, through the same inline bodies the update kernel (kernels.hip gamma_update_kernel) calls -- the hardware
// reciprocal seed, the frexp builtins and fma_c's scalar-operand v_fma_f64, which the host build of
// tests/test_special_host.py replaces.  A translation unit of its own: the code objects of the hot path do not change
// when a hook is added here.
#include "common.h"
#include "special.h"

using namespace schpf;

namespace {

__global__ __launch_bounds__(256) void special_kernel(int which, int64_t n, const double *__restrict__ x,
                                                      const double *__restrict__ y, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double r;
    switch (which) {   // uniform over the launch
    case SCHPF_SPECIAL_RCP: r = fast_rcp(v); break;
    case SCHPF_SPECIAL_LOG: r = fast_log(v); break;
    case SCHPF_SPECIAL_EXP: r = fast_exp(v); break;
    case SCHPF_SPECIAL_PSI: r = digamma(v); break;
    default: r = digamma_less_log(v, fast_rcp(y[i])); break;   // SCHPF_SPECIAL_PSI_LESS_LOG, as the kernel pairs them
    }
    out[i] = r;
}

}  // namespace

extern "C" int schpf_debug_special(int which, int64_t n, const double *x, const double *y, double *out)
{
    if (which < SCHPF_SPECIAL_RCP || which > SCHPF_SPECIAL_PSI_LESS_LOG)
        return fail("which must be one of SCHPF_SPECIAL_RCP .. SCHPF_SPECIAL_PSI_LESS_LOG, got %d", which);
    if (n < 0 || n >= (int64_t)1 << 31) return fail("n must be in [0, 2^31)");
    if (n == 0) return 0;
    if (!x || !out) return fail("x and out must not be NULL");
    if (which == SCHPF_SPECIAL_PSI_LESS_LOG && !y) return fail("y (the rates) must not be NULL for SCHPF_SPECIAL_PSI_LESS_LOG");
    return guarded([&] {
        TempStream ts;
        DevBuf a, b, o;
        h2d<double>(a, x, (size_t)n, ts.st);
        if (which == SCHPF_SPECIAL_PSI_LESS_LOG) h2d<double>(b, y, (size_t)n, ts.st);
        o.alloc((size_t)n * sizeof(double));
        hipLaunchKernelGGL(special_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ts.st, which, n,
                           a.as<double>(), b.as<double>(), o.as<double>());
        HIPCHK(hipGetLastError());
        d2h(out, o, (size_t)n * sizeof(double), ts.st);
    });
}
