// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The two launchers of rocoder_amd/csrc/rc_frames_loud.hip for the host-only engine builds (tests/c/hip_stub.cpp and the
// other hip_stub_frames*.cpp have the rest). The stub's device memory is host memory, so a pointer, a stride or a count that
// the middle of rc_engine_stretch_frames_loud gets wrong is an AddressSanitizer finding.
//   energy     refuses what the real launcher refuses; reads every frame [0, nb * sub) of every channel and every word of
//              coef and step; writes rc_stub_loud_level * sub to every energy word, so that the gate on the host gives
//              -0.691 + 10 log10(channels * level) for nb >= 4; logs the launch.
//   true peak  reads every frame [0, n) of every channel and the 256 floats of the table, and joins rc_stub_loud_peak to
//              the peak word as the kernel's atomicMax would.
// Both log the first float of channel 0 they read: a limiter or a resampler that ran in front left its mark there.
#include <hip/hip_runtime_api.h>

#include <cstring>

#include "../../rocoder_amd/csrc/rc_frames.h"

struct RcStubLoudLaunch {
    uint64_t n, nb, stride, e_stride;
    uint32_t sub, channels;
    float first;
    double coef0, step_last;
};
RcStubLoudLaunch rc_stub_loud_energy_log[16], rc_stub_loud_peak_log[16];
uint32_t rc_stub_loud_energy_launches = 0, rc_stub_loud_peak_launches = 0;
uint64_t rc_stub_loud_energy_frames = 0, rc_stub_loud_peak_frames = 0;
float rc_stub_loud_level = 0.01f, rc_stub_loud_peak = 0.5f;
double rc_stub_loud_sum = 0.0;  // (what the launchers read: keeps the reads alive)

namespace rc {
hipError_t launch_frames_loud_energy(const FramesLoudEnergyParams &p, hipStream_t) {
    if (p.nb == 0) return hipSuccess;
    if (!p.planar || !p.energy || p.channels == 0 || p.channels > 65535u || p.sub < kLoudMinSub || p.nb > p.n / p.sub || p.e_stride < p.nb ||
        p.stride < p.n)
        return hipErrorInvalidValue;
    for (int i = 0; i < 10; ++i) rc_stub_loud_sum += p.coef[i];
    for (int k = 0; k < 8; ++k)
        for (int i = 0; i < 16; ++i) rc_stub_loud_sum += p.step[k][i];
    if (rc_stub_loud_energy_launches < 16)
        rc_stub_loud_energy_log[rc_stub_loud_energy_launches] =
            RcStubLoudLaunch{p.n, p.nb, p.stride, p.e_stride, p.sub, p.channels, p.planar[0], p.coef[0], p.step[7][15]};
    ++rc_stub_loud_energy_launches;
    for (uint32_t c = 0; c < p.channels; ++c) {
        for (uint64_t t = 0; t < p.nb * p.sub; ++t) rc_stub_loud_sum += p.planar[(uint64_t)c * p.stride + t];
        for (uint64_t j = 0; j < p.nb; ++j) p.energy[(uint64_t)c * p.e_stride + j] = rc_stub_loud_level * (float)p.sub;
    }
    rc_stub_loud_energy_frames += p.nb * p.sub * p.channels;
    return hipSuccess;
}

hipError_t launch_frames_true_peak(const FramesTruePeakParams &p, hipStream_t) {
    if (p.n == 0) return hipSuccess;
    if (!p.planar || !p.table || !p.norm || p.channels == 0 || p.channels > 65535u || p.stride < p.n) return hipErrorInvalidValue;
    for (int i = 0; i < 256; ++i) rc_stub_loud_sum += p.table[i];
    if (rc_stub_loud_peak_launches < 16)
        rc_stub_loud_peak_log[rc_stub_loud_peak_launches] = RcStubLoudLaunch{p.n, 0, p.stride, 0, 0, p.channels, p.planar[0], 0.0, 0.0};
    ++rc_stub_loud_peak_launches;
    for (uint32_t c = 0; c < p.channels; ++c)
        for (uint64_t t = 0; t < p.n; ++t) rc_stub_loud_sum += p.planar[(uint64_t)c * p.stride + t];
    rc_stub_loud_peak_frames += p.n * p.channels;
    uint32_t b;
    memcpy(&b, &rc_stub_loud_peak, 4);
    if (b > p.norm->peak_bits) p.norm->peak_bits = b;
    return hipSuccess;
}
}  // namespace rc
