// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launchers of rocoder_amd/csrc/rc_frames.hip's peak kernel and of its PCM pack kernels with a gain, for the
// host-only engine builds (tests/c/hip_stub.cpp, hip_stub_frames.cpp and hip_stub_frames_pcm.cpp have the rest). The
// stub's device memory is host memory, so a range, a phase or a pointer that the two-phase bookkeeping of
// rc_engine_stretch_frames_norm gets wrong is an AddressSanitizer finding.
//   peak  reads every sample of the range it is handed and folds it into the peak word. The stubbed hop kernels
//         compute nothing, so the rows hold zeros; to give the driver something to hold the engine to, the launcher
//         also folds in (float)(1 + the samples all peak launches have covered since the driver last zeroed
//         rc_stub_peak_samples): the peak word then ends at (float)(1 + channels * frames) exactly when every output
//         sample was covered once.
//   pack  forms the gain as the kernels do, stores it where store_gain says so (counted in rc_stub_gain_stores), and
//         writes the marks of hip_stub_frames_pcm.cpp's launcher. The gain the driver reads back is target / that
//         final peak only if every peak launch came in front of the first pack launch.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>

#include "../../rocoder_amd/csrc/rc_frames.h"

uint64_t rc_stub_peak_samples = 0;
uint64_t rc_stub_gain_stores = 0;

namespace rc {
static uint32_t bits_of(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}

hipError_t launch_frames_peak(const FramesPeakParams &p, hipStream_t) {
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || !p.norm) return hipErrorInvalidValue;
    uint32_t m = p.norm->peak_bits;
    for (uint32_t c = 0; c < p.channels; ++c)
        for (uint64_t f = 0; f < p.n_frames; ++f) {
            const uint32_t b = bits_of(p.planar[(uint64_t)c * p.stride + f]) & 0x7fffffffu;
            if (b < 0x7f800000u && b > m) m = b;
        }
    rc_stub_peak_samples += p.n_frames * p.channels;
    const uint32_t mark = bits_of((float)(1 + rc_stub_peak_samples));
    p.norm->peak_bits = mark > m ? mark : m;
    return hipSuccess;
}

hipError_t launch_frames_pack_pcm_gain(uint32_t format, const FramesPackPcmGainParams &pp, hipStream_t s) {
    if (!pcm_bytes(format)) return hipErrorInvalidValue;
    if (pp.pack.n_frames == 0) return hipSuccess;
    if (!pp.norm || !(pp.target_peak > 0.0f) || !std::isfinite(pp.target_peak)) return hipErrorInvalidValue;
    float peak;
    memcpy(&peak, &pp.norm->peak_bits, 4);
    const float q = pp.target_peak / peak, g = (peak > 0.0f && std::isfinite(q)) ? q : 1.0f;
    if (pp.store_gain) {
        pp.norm->gain = g;
        ++rc_stub_gain_stores;
    }
    // (the rows hold zeros and zero times the gain is zero: the plain launcher's marks and its count are the gain's)
    return launch_frames_pack_pcm(format, pp.pack, s);
}
}  // namespace rc
