// RCCL, bound at run time.  The library has no DT_NEEDED on RCCL for the reason it has none on
// the HIP runtime (Makefile): a process must use ONE copy, and PyTorch bundles its own.  The copy
// already in the process is taken when there is one (RTLD_NOLOAD), else $SCHPF_RCCL_PATH, else
// the system's.  Only the handful of entry points the sharded iteration needs; the types are the
// C ABI of rccl.h (ncclUniqueId = 128 opaque bytes, ncclFloat32 = 7, ncclFloat64 = 8, ncclSum = 0).
#pragma once
#include <dlfcn.h>

#include <cstdlib>
#include <stdexcept>
#include <string>

namespace schpf {

struct RcclUniqueId { char internal[128]; };
struct Rccl {
    void *handle = nullptr;
    int (*GetUniqueId)(RcclUniqueId *) = nullptr;
    int (*CommInitRank)(void **, int, RcclUniqueId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, void *stream) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
inline Rccl load_rccl()
{
    Rccl r;
    const char *env = getenv("SCHPF_RCCL_PATH");
    const char *names[] = {"librccl.so", "librccl.so.1", env && *env ? env : nullptr, "librccl.so", "librccl.so.1",
                           "/opt/rocm/lib/librccl.so"};
    for (int i = 0; i < 6 && !r.handle; ++i) {
        if (!names[i]) continue;
        r.handle = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL | (i < 2 ? RTLD_NOLOAD : 0));
    }
    if (!r.handle) throw std::runtime_error("cannot load RCCL (librccl.so): set SCHPF_RCCL_PATH");
    auto sym = [&](const char *n) {
        void *p = dlsym(r.handle, n);
        if (!p) throw std::runtime_error(std::string("RCCL lacks ") + n);
        return p;
    };
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
    r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
    return r;
}
inline Rccl &rccl()
{
    static Rccl r = load_rccl();   // thread-safe; a failed load throws and is tried again by the next caller
    return r;
}
#define RCCLCHK(expr)                                                                                            \
    do {                                                                                                         \
        const int r_ = (expr);                                                                                   \
        if (r_ != 0) throw std::runtime_error(std::string(#expr " failed: ") + schpf::rccl().GetErrorString(r_)); \
    } while (0)

}  // namespace schpf
