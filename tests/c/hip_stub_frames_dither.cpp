// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launchers of rocoder_amd/csrc/rc_frames.hip's dithered PCM pack kernels for the host-only engine builds
// (tests/c/hip_stub.cpp and the other hip_stub_frames*.cpp have the rest). They refuse what the real launchers refuse,
// read every planar sample of the range they are handed and the launch's entries of the key table, and write exactly the
// bytes the real launchers may write: n_frames * channels * bytes from target + phase on, and the counter. The stub's
// device memory is host memory, so a byte offset, a phase, a count or a key table that the engine gets wrong is an
// AddressSanitizer finding. Each byte written carries the low three bits of its sample's absolute frame t0 + f, the low
// two of its job channel channel0 + c, the mode and the byte number (rc_stub_dither_mark), and every launch is logged with
// its exact t0, frame count, channel0, channel count and mode (rc_stub_dither_log; the driver zeroes the count): a chunk
// that was handed a wrong t0 or a wrong channel0 is visible in the log whatever it is, and in the output wherever it is
// wrong in its low bits. The gain variant forms and stores the gain as hip_stub_frames_norm.cpp's does.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>

#include "../../rocoder_amd/csrc/rc_frames.h"

extern uint64_t rc_stub_gain_stores;  // tests/c/hip_stub_frames_norm.cpp

struct RcStubDitherLaunch {
    uint64_t t0, n_frames;
    uint32_t channel0, channels, mode;
};
RcStubDitherLaunch rc_stub_dither_log[256];
uint64_t rc_stub_dither_launches = 0;
uint64_t rc_stub_dither_key_sum = 0;  // (what the launchers read of the table: keeps the reads alive, and says which keys)

unsigned char rc_stub_dither_mark(uint64_t t, uint32_t channel, uint32_t mode, uint32_t byte) {
    return (unsigned char)(((uint32_t)(t & 7u) << 5) | ((channel & 3u) << 3) | ((mode == 2u ? 1u : 0u) << 2) | (byte & 3u));
}

namespace rc {
static hipError_t pack_dithered(uint32_t format, const FramesPackPcmParams &p, const FramesDitherParams &d) {
    const uint32_t B = pcm_bytes(format);
    if (!B) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.phase > 3 || ((uintptr_t)p.target & 3) || !p.clipped) return hipErrorInvalidValue;
    if ((d.mode != 1u && d.mode != 2u) || !d.keys || (format != PCM_U8 && format != PCM_I16 && format != PCM_I24)) return hipErrorInvalidValue;
    if (rc_stub_dither_launches < 256) rc_stub_dither_log[rc_stub_dither_launches] = RcStubDitherLaunch{d.t0, p.n_frames, d.channel0, p.channels, d.mode};
    ++rc_stub_dither_launches;
    unsigned char *dst = p.target + p.phase;
    uint64_t beyond = 0;
    for (uint32_t c = 0; c < p.channels; ++c) rc_stub_dither_key_sum += d.keys[d.channel0 + c];
    for (uint64_t f = 0; f < p.n_frames; ++f)
        for (uint32_t c = 0; c < p.channels; ++c) {
            const float x = p.planar[(uint64_t)c * p.stride + f];
            beyond += !(x >= -1.0f && x <= 1.0f);
            for (uint32_t b = 0; b < B; ++b) dst[(f * p.channels + c) * B + b] = rc_stub_dither_mark(d.t0 + f, d.channel0 + c, d.mode, b);
        }
    *p.clipped += beyond;
    return hipSuccess;
}

hipError_t launch_frames_pack_pcm_dither(uint32_t format, const FramesPackPcmDitherParams &pp, hipStream_t) {
    return pack_dithered(format, pp.pack, pp.dither);
}

hipError_t launch_frames_pack_pcm_gain_dither(uint32_t format, const FramesPackPcmGainDitherParams &pp, hipStream_t) {
    const FramesPackPcmGainParams &g = pp.gain;
    if (!pcm_bytes(format)) return hipErrorInvalidValue;
    if (g.pack.n_frames == 0) return hipSuccess;
    if (!g.norm || !(g.target_peak > 0.0f) || !std::isfinite(g.target_peak)) return hipErrorInvalidValue;
    float peak;
    memcpy(&peak, &g.norm->peak_bits, 4);
    const float q = g.target_peak / peak, gain = (peak > 0.0f && std::isfinite(q)) ? q : 1.0f;
    if (g.store_gain) {
        g.norm->gain = gain;
        ++rc_stub_gain_stores;
    }
    return pack_dithered(format, g.pack, pp.dither);
}
}  // namespace rc
