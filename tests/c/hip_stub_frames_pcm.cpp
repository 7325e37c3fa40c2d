// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launcher of rocoder_amd/csrc/rc_frames.hip's PCM pack kernels for the host-only engine builds (tests/c/hip_stub.cpp
// and hip_stub_frames.cpp have the rest). It reads every planar sample of the range it is handed and writes exactly the
// bytes the real launcher may write: n_frames * channels * bytes from target + phase on, one at a time, and the
// counter. The stub's device memory is host memory, so a byte offset, a phase or a count that the engine's chunk
// arithmetic gets wrong is an AddressSanitizer finding. Each byte written says which sample it belongs to (the low bits
// of frame, channel and byte number), so that the driver can tell a chunk that landed in the wrong place.
#include <hip/hip_runtime_api.h>

#include "../../rocoder_amd/csrc/rc_frames.h"

namespace rc {
hipError_t launch_frames_pack_pcm(uint32_t format, const FramesPackPcmParams &p, hipStream_t) {
    const uint32_t B = pcm_bytes(format);
    if (!B) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.phase > 3 || ((uintptr_t)p.target & 3) || !p.clipped) return hipErrorInvalidValue;
    unsigned char *dst = p.target + p.phase;
    uint64_t beyond = 0;
    for (uint64_t f = 0; f < p.n_frames; ++f)
        for (uint32_t c = 0; c < p.channels; ++c) {
            const float x = p.planar[(uint64_t)c * p.stride + f];
            beyond += !(x >= -1.0f && x <= 1.0f);
            for (uint32_t b = 0; b < B; ++b) dst[(f * p.channels + c) * B + b] = (unsigned char)(0x80u | ((c & 7u) << 2) | b);
        }
    *p.clipped += beyond;
    return hipSuccess;
}
}  // namespace rc
