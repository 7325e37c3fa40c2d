// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launchers of rocoder_amd/csrc/rc_frames.hip for the host-only engine builds (tests/c/hip_stub.cpp has the rest).
// Unlike the other stubbed launchers these two touch memory: each reads every input byte and writes every output element
// of the range it is handed, and no other. The stub's device memory is host memory, so a byte offset or a count that the
// engine's chunk arithmetic gets wrong is an AddressSanitizer finding. (The kernels' reads of whole 16-byte groups
// around a tile are theirs alone: here the raw block is read to the byte.)
#include <hip/hip_runtime_api.h>

#include "../../rocoder_amd/csrc/rc_frames.h"

namespace rc {
hipError_t launch_frames_unpack(uint32_t format, const FramesUnpackParams &p, hipStream_t) {
    const uint32_t B = pcm_bytes(format);
    if (!B || p.phase > 3 || (p.raw_dwords & 3) || ((uintptr_t)p.raw & 15)) return hipErrorInvalidValue;
    const unsigned char *raw = (const unsigned char *)p.raw + p.phase;
    if (p.n_frames && p.phase + (p.frame0 + p.n_frames) * p.channels * B > p.raw_dwords * 4) return hipErrorInvalidValue;
    for (uint64_t f = p.frame0; f < p.frame0 + p.n_frames; ++f)
        for (uint32_t c = 0; c < p.channels; ++c) {
            uint32_t v = 0;
            for (uint32_t b = 0; b < B; ++b) v |= (uint32_t)raw[(f * p.channels + c) * B + b] << (8 * b);
            p.planar[(uint64_t)c * p.stride + f] = (float)v;
        }
    return hipSuccess;
}
hipError_t launch_frames_pack(const FramesPackParams &p, hipStream_t) {
    for (uint64_t f = 0; f < p.n_frames; ++f)
        for (uint32_t c = 0; c < p.channels; ++c) p.frames[f * p.channels + c] = p.planar[(uint64_t)c * p.stride + f];
    return hipSuccess;
}
}  // namespace rc
