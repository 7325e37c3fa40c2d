// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launchers of rocoder_amd/csrc/rc_frames.hip's mapped unpack kernels and channel-peaks kernels for the host-only
// engine builds (tests/c/hip_stub.cpp and the other hip_stub_frames*.cpp have the rest). The stub's device memory is host
// memory, so a pointer, a byte count, a frame range or a table that the engine gets wrong is an AddressSanitizer finding.
//   launch_frames_unpack_map   reads `channels` words of the map, reads exactly the bytes of sample (f, map[c]) for its
//       frame range - and no other byte of the block - and writes exactly its rows, as tests/c/hip_stub_frames.cpp's
//       unmapped launcher does for sample (f, c). It counts its launches (rc_stub_map_launches), counts how often each
//       frame came through (rc_stub_map_cover: n_frames bytes of the driver's, or null) and keeps the first words of the
//       table it read (rc_stub_map_seen).
//   launch_frames_channel_peaks   reads every byte of the frames [frame0, frame0 + n_frames) - and no other byte - and
//       joins the largest byte of each channel's samples to that channel's word, as the real launcher joins a maximum.
//       It marks coverage (rc_stub_chan_cover: the driver points it at n_frames bytes, or leaves it null), logs every
//       launch (rc_stub_chan_log, rc_stub_chan_launches) and flags a word that was not zeroed in front of the first launch
//       (the top bit of a word is never set by this stub: rc_stub_chan_dirty).
#include <hip/hip_runtime_api.h>

#include "../../rocoder_amd/csrc/rc_frames.h"

struct RcStubChanLaunch {
    uint64_t frame0, n_frames;
    uint32_t channels, phase, format;
};
RcStubChanLaunch rc_stub_chan_log[256];
uint32_t rc_stub_chan_launches = 0;
unsigned char *rc_stub_chan_cover = nullptr;
uint64_t rc_stub_chan_dirty = 0;
uint32_t rc_stub_map_launches = 0;
unsigned char *rc_stub_map_cover = nullptr;
uint32_t rc_stub_map_seen[8];

namespace rc {
hipError_t launch_frames_unpack_map(uint32_t format, const FramesUnpackMapParams &pm, hipStream_t) {
    const FramesUnpackParams &p = pm.unpack;
    const uint32_t B = pcm_bytes(format);
    if (!B || p.phase > 3 || (p.raw_dwords & 3) || ((uintptr_t)p.raw & 15) || !pm.map) return hipErrorInvalidValue;
    const unsigned char *raw = (const unsigned char *)p.raw + p.phase;
    if (p.n_frames && p.phase + (p.frame0 + p.n_frames) * p.channels * B > p.raw_dwords * 4) return hipErrorInvalidValue;
    ++rc_stub_map_launches;
    for (uint32_t c = 0; c < p.channels; ++c)
        if (pm.map[c] >= p.channels) return hipErrorInvalidValue;
    for (uint32_t c = 0; c < p.channels && c < 8; ++c) rc_stub_map_seen[c] = pm.map[c];
    for (uint64_t f = p.frame0; f < p.frame0 + p.n_frames; ++f) {
        for (uint32_t c = 0; c < p.channels; ++c) {
            uint32_t v = 0;
            for (uint32_t b = 0; b < B; ++b) v |= (uint32_t)raw[(f * p.channels + pm.map[c]) * B + b] << (8 * b);
            p.planar[(uint64_t)c * p.stride + f] = (float)v;
        }
        if (rc_stub_map_cover) ++rc_stub_map_cover[f];
    }
    return hipSuccess;
}

hipError_t launch_frames_channel_peaks(uint32_t format, const FramesChannelPeaksParams &p, hipStream_t) {
    const uint32_t B = pcm_bytes(format);
    if (!B) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || p.phase > 3u || (p.raw_dwords & 3u) || ((uintptr_t)p.raw & 15u) || !p.chan_bits)
        return hipErrorInvalidValue;
    if (rc_stub_chan_launches < 256)
        rc_stub_chan_log[rc_stub_chan_launches] = RcStubChanLaunch{p.frame0, p.n_frames, p.channels, p.phase, format};
    ++rc_stub_chan_launches;
    const unsigned char *raw = (const unsigned char *)p.raw;
    const uint64_t fb = (uint64_t)p.channels * B;
    for (uint64_t f = p.frame0; f < p.frame0 + p.n_frames; ++f) {
        for (uint32_t c = 0; c < p.channels; ++c) {
            uint32_t m = 0;
            for (uint32_t b = 0; b < B; ++b) {
                const uint32_t v = raw[p.phase + f * fb + (uint64_t)c * B + b];
                m = v > m ? v : m;
            }
            uint32_t &word = p.chan_bits[c];
            if (word & 0x80000000u) ++rc_stub_chan_dirty;
            if (m > word) word = m;
        }
        if (rc_stub_chan_cover) ++rc_stub_chan_cover[f];
    }
    return hipSuccess;
}
}  // namespace rc
