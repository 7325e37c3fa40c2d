// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launcher of rocoder_amd/csrc/rc_frames_limit.hip for the host-only engine builds (tests/c/hip_stub.cpp and the
// other hip_stub_frames*.cpp have the rest). The stub's device memory is host memory, so a pointer, a stride or a range
// that the engine's lag bookkeeping gets wrong is an AddressSanitizer finding.
//   - It refuses what the real launcher refuses: a range that needs a frame inside [0, n) but outside
//     [src0, src0 + src_len); the frames needed are [t0 - 2 L, t1 + 2 L).
//   - It reads every frame of that halo that lies inside [0, n), every channel, writes rc_stub_limit_mark over the frames
//     [t0, t1) of every channel of dst, and adds t1 - t0 to the stats words' count.
//   - It logs every launch (rc_stub_limit_log, rc_stub_limit_launches; the driver zeroes the count): [t0, t1), src0,
//     src_len, n, the settings, the strides, the rows that the launch's pointers imply and the first and the last float of
//     the input range [t0, t1) of channel 0 as it was when the launch ran (a fade launch that ran in front left its mark).
#include <hip/hip_runtime_api.h>

#include "../../rocoder_amd/csrc/rc_frames.h"

struct RcStubLimitLaunch {
    uint64_t t0, t1, src0, src_len, n, stride, dst_stride;
    uint32_t L, channels;
    float drive, ceiling;
    uintptr_t src_row0, dst_row0;  // where frame 0 of the first channel lies, by this launch's pointers
    float in_first, in_last;       // src's frames need_lo and need_hi - 1 of channel 0, as read
};
RcStubLimitLaunch rc_stub_limit_log[256];
uint32_t rc_stub_limit_launches = 0;
uint32_t rc_stub_limit_refused = 0;
float rc_stub_limit_mark = 0.125f;
float rc_stub_limit_sum = 0.0f;  // (what the launcher read: keeps the reads alive)

namespace rc {
hipError_t launch_frames_limit(const FramesLimitParams &p, hipStream_t) {
    if (p.t1 <= p.t0) return hipSuccess;
    if (!p.src || !p.dst || !p.stats || p.channels == 0 || p.channels > 65535u || p.L > kLimitMaxLookahead || p.t1 > p.n ||
        !(p.drive > 0.0f) || !(p.ceiling > 0.0f))
        return hipErrorInvalidValue;
    const uint64_t halo = 2 * (uint64_t)p.L;
    const uint64_t need_lo = p.t0 > halo ? p.t0 - halo : 0, need_hi = p.t1 + halo < p.n ? p.t1 + halo : p.n;
    if (need_lo < need_hi && (need_lo < p.src0 || need_hi > p.src0 + p.src_len)) {
        ++rc_stub_limit_refused;
        return hipErrorInvalidValue;
    }
    if (rc_stub_limit_launches < 256)
        rc_stub_limit_log[rc_stub_limit_launches] = RcStubLimitLaunch{
            p.t0, p.t1, p.src0, p.src_len, p.n, p.stride, p.dst_stride, p.L, p.channels, p.drive, p.ceiling,
            (uintptr_t)p.src - (uintptr_t)(p.src0 * sizeof(float)), (uintptr_t)p.dst - (uintptr_t)(p.t0 * sizeof(float)),
            p.src[need_lo - p.src0], p.src[need_hi - 1 - p.src0]};
    ++rc_stub_limit_launches;
    for (uint32_t c = 0; c < p.channels; ++c) {
        for (uint64_t k = need_lo; k < need_hi; ++k) rc_stub_limit_sum += p.src[(uint64_t)c * p.stride + (k - p.src0)];
        for (uint64_t i = 0; i < p.t1 - p.t0; ++i) p.dst[(uint64_t)c * p.dst_stride + i] = rc_stub_limit_mark;
    }
    p.stats->limited += p.t1 - p.t0;
    return hipSuccess;
}
}  // namespace rc
