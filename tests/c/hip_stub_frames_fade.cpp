// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launcher of rocoder_amd/csrc/rc_frames.hip's fade kernel for the host-only engine builds (tests/c/hip_stub.cpp and
// the other hip_stub_frames*.cpp have the rest). The stub's device memory is host memory, so a pointer, a stride or a
// frame range that the engine's intersection of a chunk with the fade ranges gets wrong is an AddressSanitizer finding.
//   - It reads every sample of the frames [t0, t1) of every channel and writes rc_stub_fade_mark over it. The stubbed
//     hop kernels compute nothing, so the rows hold zeros, or the marks of earlier calls: a driver that gives every call
//     a mark of its own finds in the output exactly the samples that went through this launcher in front of the pack
//     launch or the download that read them. The default mark is beyond full scale, so the PCM pack launcher counts
//     those samples as clipped.
//   - It logs every launch (rc_stub_fade_log, rc_stub_fade_launches; the driver zeroes the count): the frame range, the
//     channels, the row of frame 0 that the launch's pointer implies, and how many samples the peak launcher
//     (hip_stub_frames_norm.cpp) had covered when it ran - a fade launch must come in front of the peak launch that reads
//     its frames.
#include <hip/hip_runtime_api.h>

#include "../../rocoder_amd/csrc/rc_frames.h"

extern uint64_t rc_stub_peak_samples;  // tests/c/hip_stub_frames_norm.cpp

struct RcStubFadeLaunch {
    uint64_t t0, t1, in_len, out_start, out_len, stride, peak_samples_before;
    uint32_t channels;
    uintptr_t row0;  // where frame 0 of the first channel lies, by this launch's pointer
};
RcStubFadeLaunch rc_stub_fade_log[256];
uint32_t rc_stub_fade_launches = 0;
float rc_stub_fade_mark = 2.0f;
float rc_stub_fade_sum = 0.0f;  // (what the launcher read: keeps the reads alive)

namespace rc {
hipError_t launch_frames_fade(const FramesFadeParams &p, hipStream_t) {
    if (p.t1 <= p.t0) return hipSuccess;
    if (!p.planar || p.channels == 0 || p.channels > 65535u) return hipErrorInvalidValue;
    if (rc_stub_fade_launches < 256)
        rc_stub_fade_log[rc_stub_fade_launches] = RcStubFadeLaunch{p.t0, p.t1, p.in_len, p.out_start, p.out_len, p.stride,
                                                                   rc_stub_peak_samples, p.channels,
                                                                   (uintptr_t)p.planar - (uintptr_t)(p.t0 * sizeof(float))};
    ++rc_stub_fade_launches;
    for (uint32_t c = 0; c < p.channels; ++c)
        for (uint64_t i = 0; i < p.t1 - p.t0; ++i) {
            float &x = p.planar[(uint64_t)c * p.stride + i];
            rc_stub_fade_sum += x;
            x = rc_stub_fade_mark;
        }
    return hipSuccess;
}
}  // namespace rc
