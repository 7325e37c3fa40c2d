// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launcher of rocoder_amd/csrc/rc_frames_mix.hip for the host-only engine builds (tests/c/hip_stub.cpp and the other
// hip_stub_frames*.cpp have the rest). The stub's device memory is host memory, so a pointer, a stride or a range that the
// engine gets wrong is an AddressSanitizer finding.
//   - It refuses what the real launcher refuses: t1 < t0, more than kMixMaxKeys keys, and with a non-empty range a null
//     pointer, a null send with CL != CB, a bus that is not aligned as rc_frames.h states.
//   - It reads every row sample of the range, every key and every send word, and adds 1.0f to every bus word the range lands
//     on - so a bus word counts the launches that covered it.
//   - It logs every launch (rc_stub_mix_log, rc_stub_mix_launches; the driver zeroes the count).
#include <hip/hip_runtime_api.h>

#include "../../rocoder_amd/csrc/rc_frames.h"

struct RcStubMixLaunch {
    uint64_t t0, t1, stride, bus_stride, bus_frames;
    int64_t offset;
    uint32_t channels, bus_channels, n_keys, has_send;
    uintptr_t row0, bus0;  // where layer frame 0 of the first channel lies, by this launch's pointers; the bus base
};
RcStubMixLaunch rc_stub_mix_log[256];
uint32_t rc_stub_mix_launches = 0;
double rc_stub_mix_sum = 0.0;  // (what the launcher read: keeps the reads alive)

namespace rc {
hipError_t launch_frames_mix(const FramesMixParams &p, hipStream_t) {
    if (p.t1 < p.t0 || p.n_keys > kMixMaxKeys) return hipErrorInvalidValue;
    if (p.t1 == p.t0) return hipSuccess;
    if (!p.rows || !p.bus || (p.n_keys && (!p.key_frame || !p.key_amp)) || p.channels == 0 || p.bus_channels == 0 ||
        (!p.send && p.channels != p.bus_channels) || (p.bus_stride & 3u) || ((uintptr_t)p.bus & 15u) || p.bus_stride < p.bus_frames)
        return hipErrorInvalidValue;
    if (rc_stub_mix_launches < 256)
        rc_stub_mix_log[rc_stub_mix_launches] = RcStubMixLaunch{p.t0, p.t1, p.stride, p.bus_stride, p.bus_frames, p.offset, p.channels, p.bus_channels,
                                                                 p.n_keys, p.send ? 1u : 0u, (uintptr_t)p.rows - (uintptr_t)(p.t0 * sizeof(float)),
                                                                 (uintptr_t)p.bus};
    ++rc_stub_mix_launches;
    for (uint32_t k = 0; k < p.n_keys; ++k) rc_stub_mix_sum += (double)p.key_frame[k] + (double)p.key_amp[k];
    if (p.send)
        for (uint32_t i = 0; i < p.channels * p.bus_channels; ++i) rc_stub_mix_sum += (double)p.send[i];
    for (uint32_t c = 0; c < p.channels; ++c)
        for (uint64_t t = p.t0; t < p.t1; ++t) rc_stub_mix_sum += (double)p.rows[(uint64_t)c * p.stride + (t - p.t0)];
    for (uint64_t t = p.t0; t < p.t1; ++t) {
        const int64_t u = p.offset + (int64_t)t;
        if (u < 0 || u >= (int64_t)p.bus_frames) continue;
        for (uint32_t cb = 0; cb < p.bus_channels; ++cb) p.bus[(uint64_t)cb * p.bus_stride + (uint64_t)u] += 1.0f;
    }
    return hipSuccess;
}
}  // namespace rc
