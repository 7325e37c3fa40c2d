// Test-hook entry for launch_frames_warp (rc_warp.h): compiled into librocoder_hip_hooks.so only (`make hooks`), as
// rc_frames_hooks.hip is. The fields of the parameter block as plain scalars and pointers, a launch on the null stream, a
// synchronise, the hipError_t as an int. No logic, no clamping, no defaults and no allocation. tier_off: 13 host words.
#include "rc_warp.h"

extern "C" int rc_test_frames_warp(const float *src, uint64_t src0, uint64_t src_len, uint64_t stride, uint32_t channels, uint64_t n,
                                   const float *table, const uint32_t *tier_off, const int64_t *d_anchor, const int64_t *h_anchor,
                                   uint64_t n_anchors, float *dst, uint64_t dst_stride, uint64_t m0, uint64_t m1) {
    rc::FramesWarpParams p{src, src0, src_len, stride, channels, n, table, {}, d_anchor, h_anchor, n_anchors, dst, dst_stride, m0, m1};
    for (uint32_t t = 0; t < rc::kWarpTiers; ++t) p.tier_off[t] = tier_off[t];
    const hipError_t err = rc::launch_frames_warp(p, nullptr);
    return (int)(err != hipSuccess ? err : hipStreamSynchronize(nullptr));
}
