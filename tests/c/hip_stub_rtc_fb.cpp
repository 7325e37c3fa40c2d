// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The HIP module calls of rocoder_amd/csrc/rc_rtc.cpp for engine_dk_fb_asan, in place of tests/c/hip_stub_rtc.cpp: every
// lookup and every launch is logged with the argument block it carried. A launch of rc_user_dk that carries a feedback
// state walks its hops as the kernel does: for every channel of its grid and every hop of its sub-range it checks the ring
// row index against the block (channel below rc_config::channels, slot below feedback + 1), writes the hop number over the
// row's first and last bin, reads the first and last bin of the hop's input row and writes those of its output row - so a
// state that is too small, a row outside it, or a hop outside the chunk is a finding of the sanitizer or an abort here.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../rocoder_amd/csrc/rc_rtc.h"
#include "hip_stub_rtc_fb.h"

// AddressSanitizer's allocator interface (sanitizer/allocator_interface.h; this stub is built with ASan only)
extern "C" int __sanitizer_get_ownership(const volatile void *p);
extern "C" size_t __sanitizer_get_allocated_size(const volatile void *p);

namespace {
struct Fn {
    int pass;
};
struct Mod {
    Fn fn[2];
};
std::mutex g_mu;
std::vector<RtcFbLaunch> g_launches;
std::vector<std::string> g_lookups;

void require(bool ok, const char *what) {
    if (ok) return;
    fprintf(stderr, "hip_stub_rtc_fb: %s\n", what);
    abort();
}
}  // namespace

std::vector<RtcFbLaunch> rtc_fb_stub_take_launches() {
    std::lock_guard<std::mutex> lk(g_mu);
    std::vector<RtcFbLaunch> v;
    v.swap(g_launches);
    return v;
}
std::vector<std::string> rtc_fb_stub_take_lookups() {
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
    RtcFbLaunch l;
    l.pass = ((const Fn *)f)->pass;
    l.gx = gx;
    l.gy = gy;
    l.gz = gz;
    l.bx = bx;
    l.stream = (const void *)s;
    memcpy(&l.a, args[0], sizeof l.a);
    l.state_bytes = 0;
    const rc::UserDkArgs &a = l.a;
    if (!l.pass && a.state) {
        if (__sanitizer_get_ownership(a.state)) l.state_bytes = __sanitizer_get_allocated_size(a.state);
        require(a.feedback >= 1 && a.feedback <= rc::DK_MAX_FEEDBACK, "feedback outside 1 ... 4");
        require(a.fb_hop_count >= 1 && (uint64_t)a.fb_hop_first + a.fb_hop_count <= a.hop_count, "hops outside the chunk");
        require(gx == 1 || a.fb_hop_count == 1, "more than one hop in a launch of several workgroups per channel");
        const uint64_t rows = a.feedback + 1;
        volatile float sink = 0;
        for (uint64_t ci = a.row_first; ci < a.row_first + gy; ++ci) {
            const uint64_t channel = a.ch_first + ci;
            require(channel < a.channels, "a channel outside the job");
            const uint64_t ch = channel - a.in_ch_first;
            require(ch < a.in_ch_count, "a channel outside the input block");
            for (uint64_t hl = a.fb_hop_first; hl < (uint64_t)a.fb_hop_first + a.fb_hop_count; ++hl) {
                const uint64_t k = (uint64_t)a.hop_first + hl, slot = k % rows;
                require((channel * rows + slot + 1) * a.n * sizeof(float2) <= l.state_bytes, "a ring row outside the state");
                float2 *row = a.state + (channel * rows + slot) * a.n;
                row[0].x = row[a.n - 1].y = (float)k;
                const float2 *in = a.in + (ch * a.in_rows + hl) * a.n;
                sink = sink + in[0].x + in[a.n - 1].y;
                float2 *out = a.out + (ci * a.hop_count + hl) * a.n;
                out[0].x = out[a.n - 1].y = (float)k;
            }
        }
        (void)sink;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    g_launches.push_back(l);
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
}
