// The scaffold of a stateless call: what every operator that reads a caller's arrays in device memory, checks
// them, and refuses or computes shares, each defined here and nowhere else.  A header of its own and not a part of
// csr_device.h: knn.hip, knn_graph.hip and thin.hip read no CSR, and csr_device.h brings rocPRIM and the matrix record.
//
//   use_device, pick_stream             the device and the stream of an entry point
//   grid_for, GRID_STRIDE, LAUNCH,      one thread per item in workgroups of 256, the grid capped at 2^20 workgroups (or at
//   LAUNCH_BOUNDED                      `blocks` for a kernel that ends in an atomic per wavefront) and walked by stride
//   bits_of, Scratch                    rocPRIM: the bits a radix sort looks at, and the two-call protocol on one buffer
//   sum_t, wave_min                     the integer outputs as atomicAdd takes them; the minimum of a wavefront
//   NONE, report_min, Offenders<N>      the refusal channel: N words in device memory that start at NONE and take the
//                                       smallest offender of each check.  A kernel keeps its smallest offender per thread and
//                                       ends in report_min, which every lane of a wavefront must reach: no early return
//                                       before it.  One atomicMin per wavefront that found something, none on a valid input;
//                                       a minimum does not depend on the order it was taken in, so the word, and with it the
//                                       refusal, is the same on every schedule.  The host fetches the record once per
//                                       synchronisation point and words its refusals in the order it asks the words
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>

#include "common.h"

namespace schpf {

inline void use_device(int device)
{
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) throw std::invalid_argument("no such HIP device");
    HIPCHK(hipSetDevice(device));
}

inline hipStream_t pick_stream(void *stream, std::unique_ptr<TempStream> &own)
{
    // NULL: a stream of the call's own; SCHPF_STREAM_DEFAULT: the device's null stream; else the given handle
    if (!stream) {
        own.reset(new TempStream);
        return own->st;
    }
    return stream == SCHPF_STREAM_DEFAULT ? nullptr : (hipStream_t)stream;
}

inline unsigned grid_for(int64_t n, int per_block)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, 1 << 20));
}
inline unsigned grid_for(int64_t n) { return grid_for(n, 256); }

#define GRID_STRIDE(v, n) for (int64_t v = blockIdx.x * (int64_t)256 + threadIdx.x; v < (n); v += (int64_t)gridDim.x * 256)

// a grid of at most `blocks` workgroups
#define LAUNCH_BOUNDED(kernel, n, blocks, st, ...)                                                                           \
    do {                                                                                                                     \
        hipLaunchKernelGGL(kernel, dim3(std::min<unsigned>(schpf::grid_for(n), blocks)), dim3(256), 0, st, __VA_ARGS__);    \
        HIPCHK(hipGetLastError());                                                                                           \
    } while (0)
#define LAUNCH(kernel, n, st, ...) LAUNCH_BOUNDED(kernel, n, 1u << 20, st, __VA_ARGS__)

inline int bits_of(uint64_t largest)   // the bits a radix sort has to look at for keys up to `largest`
{
    int b = 1;
    while (b < 64 && (largest >> b)) ++b;
    return b;
}

// rocPRIM's two-call protocol on one scratch buffer that grows when a call asks for more
struct Scratch {
    DevBuf buf;
    template <typename F> void run(F &&f)
    {
        size_t bytes = 0;
        HIPCHK(f((void *)nullptr, bytes));
        if (bytes > buf.bytes || !buf.p) buf.alloc(bytes);   // hipFree waits for what still reads the old one
        HIPCHK(f(buf.p, bytes));
    }
};

typedef unsigned long long sum_t;   // the int64 outputs as atomicAdd takes them; no sum here is negative

__device__ __forceinline__ int wave_min(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

constexpr unsigned long long NONE = ~0ull;   // a word no check has written to: nothing offends

// a thread's smallest offender so far, and item i as a candidate for it
__device__ __forceinline__ void offends(unsigned long long &bad, int64_t i)
{
    if ((unsigned long long)i < bad) bad = (unsigned long long)i;
}

// The end of a validation kernel in workgroups of whole wavefronts: `bad` is the thread's smallest offender or NONE
__device__ __forceinline__ void report_min(unsigned long long *word, unsigned long long bad)
{
    bad = wave_min(bad);
    if ((threadIdx.x & 63) == 0 && bad != NONE) atomicMin(word, bad);
}

template <int N> struct Offenders {   // the words in device memory, and their copy on the host
    DevBuf d;
    unsigned long long h[N];
    unsigned long long *dev() const { return d.as<unsigned long long>(); }
    void reset(hipStream_t st)
    {
        d.alloc(N * sizeof(unsigned long long));
        HIPCHK(hipMemsetAsync(d.p, 0xFF, N * sizeof(unsigned long long), st));   // NONE
    }
    void fetch(hipStream_t st) { d2h(h, d, sizeof h, st); }   // synchronises st
    // the refusal of word k, if a check wrote to it
    template <typename Words> void refuse(int k, Words &&words) const
    {
        if (h[k] != NONE) throw std::invalid_argument(words((int64_t)h[k]));
    }
};

}  // namespace schpf
