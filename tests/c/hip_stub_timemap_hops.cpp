// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// What the engine hands the hop launchers, seen without touching tests/c/hip_stub.cpp: the program of
// tests/c/engine_host_driver_timemap.cpp is linked with --wrap for rc::launch_hop, rc::launch_prep and hipMemcpyAsync
// (rocoder_amd/csrc/host/sanitize.mk), so the engine's calls of those three arrive here. Each is logged and handed on to
// the stub's own function, which does what it did. The other drivers are linked without --wrap and never see this file.
//   rc_stub_hop_log   every rc::launch_hop: the mode and the HopParams fields that say where a hop reads its input
//   rc_stub_prep_log  every rc::launch_prep: whether a padded tail copy was asked for, and of how many samples
//   rc_stub_h2d_log   every host-to-device hipMemcpyAsync: target and bytes (the copy workers call it from their
//                     threads: the log is written under a mutex)
#include <hip/hip_runtime_api.h>

#include <mutex>

#include "../../rocoder_amd/csrc/rc_kernels.h"

struct RcStubHopLaunch {
    int mode;
    int64_t in_origin, in_len, hop_first, hop_count, tail_hop_first;
    uint64_t in_stride;
    uint32_t step, pitch, ch_first, n_channels;
    uintptr_t x;
};
struct RcStubPrepLaunch {
    uint64_t tail_len, real;
    int has_tail;
};
struct RcStubH2D {
    uintptr_t dst;
    uint64_t bytes;
};
RcStubHopLaunch rc_stub_hop_log[256];
uint32_t rc_stub_hop_launches = 0;
RcStubPrepLaunch rc_stub_prep_log[256];
uint32_t rc_stub_prep_launches = 0;
RcStubH2D rc_stub_h2d_log[1024];
uint32_t rc_stub_h2d_copies = 0;
static std::mutex h2d_mutex;

// the stub's own functions, under the names --wrap gives them
hipError_t real_launch_hop(int, rc::HopMode, const rc::HopParams &, hipStream_t) __asm__("__real__ZN2rc10launch_hopEiNS_7HopModeERKNS_9HopParamsEP12ihipStream_t");
hipError_t real_launch_prep(const rc::PrepParams &, hipStream_t) __asm__("__real__ZN2rc11launch_prepERKNS_10PrepParamsEP12ihipStream_t");
extern "C" hipError_t __real_hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t);
// ... and what the engine's calls resolve to
hipError_t wrap_launch_hop(int, rc::HopMode, const rc::HopParams &, hipStream_t) __asm__("__wrap__ZN2rc10launch_hopEiNS_7HopModeERKNS_9HopParamsEP12ihipStream_t");
hipError_t wrap_launch_prep(const rc::PrepParams &, hipStream_t) __asm__("__wrap__ZN2rc11launch_prepERKNS_10PrepParamsEP12ihipStream_t");

hipError_t wrap_launch_hop(int log2n, rc::HopMode mode, const rc::HopParams &p, hipStream_t s) {
    if (rc_stub_hop_launches < 256)
        rc_stub_hop_log[rc_stub_hop_launches] = RcStubHopLaunch{(int)mode, p.in_origin, p.in_len, p.hop_first, p.hop_count, p.tail_hop_first,
                                                               (uint64_t)p.in_stride, p.step, p.pitch, p.ch_first, p.n_channels, (uintptr_t)p.x};
    ++rc_stub_hop_launches;
    return real_launch_hop(log2n, mode, p, s);
}

hipError_t wrap_launch_prep(const rc::PrepParams &p, hipStream_t s) {
    if (rc_stub_prep_launches < 256)
        rc_stub_prep_log[rc_stub_prep_launches] = RcStubPrepLaunch{(uint64_t)p.tail_len, (uint64_t)p.real, p.xtail != nullptr};
    ++rc_stub_prep_launches;
    return real_launch_prep(p, s);
}

extern "C" hipError_t __wrap_hipMemcpyAsync(void *d, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s) {
    if (kind == hipMemcpyHostToDevice) {
        std::lock_guard<std::mutex> lk(h2d_mutex);
        if (rc_stub_h2d_copies < 1024) rc_stub_h2d_log[rc_stub_h2d_copies] = RcStubH2D{(uintptr_t)d, (uint64_t)n};
        ++rc_stub_h2d_copies;
    }
    return __real_hipMemcpyAsync(d, src, n, kind, s);
}
