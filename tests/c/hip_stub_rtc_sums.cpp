// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The HIP module calls of rocoder_amd/csrc/rc_rtc.cpp for engine_dk_sums_asan, in place of tests/c/hip_stub_rtc.cpp: a
// module knows two functions, rc_user_dk and rc_user_dk_sums_pass, every lookup and every launch is logged with the
// argument block it carried, and the pass writes the RC_SUMS floats of every row of its grid, so that a scratch that is
// too small, or rows outside it, are a finding of the sanitizer.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../rocoder_amd/csrc/rc_rtc.h"
#include "hip_stub_rtc_sums.h"

// AddressSanitizer's allocator interface (sanitizer/allocator_interface.h; this stub is built with ASan only)
extern "C" int __sanitizer_get_ownership(const volatile void *p);
extern "C" size_t __sanitizer_get_allocated_size(const volatile void *p);

namespace {
struct Fn {
    int pass;  // 0: rc_user_dk, 1: rc_user_dk_sums_pass
};
struct Mod {
    Fn fn[2];
};
std::mutex g_mu;
std::vector<RtcSumsLaunch> g_launches;
std::vector<std::string> g_lookups;
}  // namespace

std::vector<RtcSumsLaunch> rtc_sums_stub_take_launches() {
    std::lock_guard<std::mutex> lk(g_mu);
    std::vector<RtcSumsLaunch> v;
    v.swap(g_launches);
    return v;
}
std::vector<std::string> rtc_sums_stub_take_lookups() {
    std::lock_guard<std::mutex> lk(g_mu);
    std::vector<std::string> v;
    v.swap(g_lookups);
    return v;
}

extern "C" {
hipError_t hipModuleLoadData(hipModule_t *m, const void *) {
    Mod *mod = (Mod *)malloc(sizeof(Mod));
    if (!mod) return hipErrorOutOfMemory;
    mod->fn[0].pass = 0;
    mod->fn[1].pass = 1;
    *m = (hipModule_t)mod;
    return hipSuccess;
}
hipError_t hipModuleUnload(hipModule_t m) {
    free((void *)m);
    return hipSuccess;
}
hipError_t hipModuleGetFunction(hipFunction_t *f, hipModule_t m, const char *name) {
    const int pass = strcmp(name, "rc_user_dk_sums_pass") == 0;
    if (!pass && strcmp(name, "rc_user_dk") != 0) return hipErrorNotFound;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_lookups.push_back(name);
    }
    *f = (hipFunction_t)&((Mod *)m)->fn[pass];
    return hipSuccess;
}
hipError_t hipModuleLaunchKernel(hipFunction_t f, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned, unsigned,
                                 unsigned, hipStream_t s, void **args, void **) {
    RtcSumsLaunch l;
    l.pass = ((const Fn *)f)->pass;
    l.gx = gx;
    l.gy = gy;
    l.gz = gz;
    l.bx = bx;
    l.stream = (const void *)s;
    memcpy(&l.a, args[0], sizeof l.a);
    l.scratch_bytes = 0;
    if (l.pass) {
        // what rc_user_dk_sums_pass stores: n_sums floats for every row of this launch, rows counted from the first halo row
        float *base = const_cast<float *>(l.a.sums) - (size_t)l.a.halo * l.a.n_sums;
        if (__sanitizer_get_ownership(base)) l.scratch_bytes = __sanitizer_get_allocated_size(base);
        for (uint64_t r = l.a.row_first; r < l.a.row_first + gy; ++r)
            for (uint32_t i = 0; i < l.a.n_sums; ++i) base[r * l.a.n_sums + i] = (float)r;
        // and what it reads: the first and the last bin of every row
        const float2 *in = l.a.in - (size_t)l.a.halo * l.a.n;
        volatile float sink = 0;
        for (uint64_t r = l.a.row_first; r < l.a.row_first + gy; ++r) sink = sink + in[r * l.a.n].x + in[r * l.a.n + l.a.n - 1].y;
        (void)sink;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    g_launches.push_back(l);
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
}
