// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launcher of rocoder_amd/csrc/rc_frames.hip's power kernel for the host-only engine builds (tests/c/hip_stub.cpp and
// the other hip_stub_frames*.cpp have the rest). The stub's device memory is host memory, so a pointer, a byte count or a
// frame range that the engine's chunk loop gets wrong is an AddressSanitizer finding.
//   - It reads every byte of the frames [frame0, frame0 + n_frames) from the raw block - and no other byte - and joins
//     the largest byte of each bin's part of the range to that bin's word, as the real launcher joins a maximum: a driver
//     that fills the block with known bytes finds in the bins what the uploads had brought when the launcher ran.
//   - It marks coverage: rc_stub_power_cover (the driver points it at n_frames bytes, or leaves it null) counts how often
//     each frame came through.
//   - It logs every launch (rc_stub_power_log, rc_stub_power_launches; the driver zeroes the count) and whether every
//     bin word it touched had been zeroed or written by an earlier launch of the job (the word's top bit is never set
//     by this stub: a word that was not zeroed in front of the first launch shows as rc_stub_power_dirty).
#include <hip/hip_runtime_api.h>

#include "../../rocoder_amd/csrc/rc_frames.h"

struct RcStubPowerLaunch {
    uint64_t frame0, n_frames, bin_frames, n_bins;
    uint32_t channels, phase, format;
};
RcStubPowerLaunch rc_stub_power_log[256];
uint32_t rc_stub_power_launches = 0;
unsigned char *rc_stub_power_cover = nullptr;
uint64_t rc_stub_power_dirty = 0;

namespace rc {
hipError_t launch_frames_power(uint32_t format, const FramesPowerParams &p, hipStream_t) {
    const uint32_t B = pcm_bytes(format);
    if (!B) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || p.phase > 3u || (p.raw_dwords & 3u) || ((uintptr_t)p.raw & 15u) || !p.bin_bits ||
        p.bin_frames == 0 || (p.frame0 + p.n_frames - 1) / p.bin_frames >= p.n_bins)
        return hipErrorInvalidValue;
    if (rc_stub_power_launches < 256)
        rc_stub_power_log[rc_stub_power_launches] = RcStubPowerLaunch{p.frame0, p.n_frames, p.bin_frames, p.n_bins, p.channels, p.phase, format};
    ++rc_stub_power_launches;
    const unsigned char *raw = (const unsigned char *)p.raw;
    const uint64_t fb = (uint64_t)p.channels * B;
    for (uint64_t f = p.frame0; f < p.frame0 + p.n_frames; ++f) {
        uint32_t m = 0;
        for (uint64_t i = 0; i < fb; ++i) m = raw[p.phase + f * fb + i] > m ? raw[p.phase + f * fb + i] : m;
        uint32_t &word = p.bin_bits[f / p.bin_frames];
        if (word & 0x80000000u) ++rc_stub_power_dirty;
        if (m > word) word = m;
        if (rc_stub_power_cover) ++rc_stub_power_cover[f];
    }
    return hipSuccess;
}
}  // namespace rc
