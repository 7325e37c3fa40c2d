// Output warp (include/rocoder_hip_warp.h: rc_engine_set_output_warp): the resample stage whose step varies
// along the output. It belongs to no kernel family: it reads and writes planar rows behind the hops, and neither this
// header nor rc_frames_warp.hip enters rc_kernel_id().
#ifndef RC_WARP_H
#define RC_WARP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rocoder_hip.h"

namespace rc {

constexpr uint32_t kWarpTiers = 13, kWarpBlock = 64, kWarpRows = 257;
constexpr int64_t kWarpD[kWarpTiers] = {RC_WARP_D_LIST};
constexpr uint32_t kWarpW[kWarpTiers] = {RC_WARP_W_LIST};
constexpr int64_t kWarpDMin = (int64_t)1 << 35, kWarpDMax = (int64_t)1 << 41, kWarpMaxAnchor = (int64_t)1 << 62;
constexpr uint32_t kWarpNoTier = 0xFFFFFFFFu;

// the tier of a block step inside [kWarpDMin, kWarpDMax]: the smallest t with D <= kWarpD[t]
inline uint32_t warp_tier(int64_t D) {
    uint32_t t = 0;
    while (t + 1 < kWarpTiers && D > kWarpD[t]) ++t;
    return t;
}

// The definition is stated in include/rocoder_hip_warp.h: output frame m = 64 b + i reads P(m) = anchor[b] +
// ((anchor[b + 1] - anchor[b]) * i >> 6); q, p, a its integer part, phase of 256 and fraction of a phase; tier t of the
// block's step; y0 / y1 ONE fmaf chain each over the rows p / p + 1 of the tier's table from +0 with j ascending,
// y = a == 0 ? y0 : fmaf(a, y1 - y0, y0). x[c][k] is the job's row c, k in [0, n), zero outside.
// `src` is the sample of the first channel at absolute input frame src0, of which src_len frames are readable per row (rows
// `stride` floats apart); `dst` the sample of the first channel at output frame m0 (rows dst_stride apart). The launch
// writes the frames [m0, m1) of every channel and nothing else.
// `table` is the device copy of the tiers in use, TAP-MAJOR: the coefficient h_t[p][j] of rc_warp_table lies at
// table[tier_off[t] + j * 257 + p]; tier_off[t] == kWarpNoTier for a tier that was not uploaded. `anchor` is the DEVICE
// copy of the n_anchors anchors and `h_anchor` the host's, which the launcher reads: it refuses (hipErrorInvalidValue,
// nothing launched) m1 > 64 (n_anchors - 1), a block of the range whose step is out of range or whose tier was not
// uploaded, and a range one of whose taps lies inside [0, n) but outside [src0, src0 + src_len). Nothing is launched for
// m1 <= m0; more than 2^27 outputs go out as several launches.
struct FramesWarpParams {
    const float *src;
    uint64_t src0, src_len;
    uint64_t stride;
    uint32_t channels;
    uint64_t n;
    const float *table;
    uint32_t tier_off[kWarpTiers];
    const int64_t *anchor;
    const int64_t *h_anchor;
    uint64_t n_anchors;
    float *dst;
    uint64_t dst_stride;
    uint64_t m0, m1;
};

hipError_t launch_frames_warp(const FramesWarpParams &p, hipStream_t s);

}  // namespace rc

#endif
