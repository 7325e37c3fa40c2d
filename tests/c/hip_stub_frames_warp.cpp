// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launcher of rocoder_amd/csrc/rc_frames_warp.hip for the host-only engine builds (tests/c/hip_stub.cpp and the other
// hip_stub_frames*.cpp have the rest). The stub's device memory is host memory, so a pointer, a stride or a range that the
// engine's lag bookkeeping gets wrong is an AddressSanitizer finding.
//   - It refuses what the real launcher refuses: m1 beyond the anchors' blocks, a block of the range whose step is out of
//     range or whose tier was not uploaded, a range one of whose taps lies inside [0, n) but outside [src0, src0 + src_len).
//   - It reads every tap of the range that lies inside [0, n), the device copy of every anchor of the range (which must
//     equal the host's) and the first and last float of every tier the range uses, and writes rc_stub_warp_mark over the
//     frames [m0, m1) of every channel of dst.
//   - It logs every launch (rc_stub_warp_log, rc_stub_warp_launches; the driver zeroes the count): [m0, m1), src0, src_len,
//     n, the strides, the rows that the launch's pointers imply and the last tap of the range, hi.
#include <hip/hip_runtime_api.h>

#include <algorithm>

#include "../../rocoder_amd/csrc/rc_warp.h"

struct RcStubWarpLaunch {
    uint64_t m0, m1, src0, src_len, n, stride, dst_stride, n_anchors, hi;
    uint32_t channels, tiers;      // tiers: a bit per tier the range uses
    uintptr_t src_row0, dst_row0;  // where frame 0 of the first channel lies, by this launch's pointers
};
RcStubWarpLaunch rc_stub_warp_log[256];
uint32_t rc_stub_warp_launches = 0;
float rc_stub_warp_mark = 0.375f;
float rc_stub_warp_sum = 0.0f;  // (what the launcher read: keeps the reads alive)

namespace rc {
hipError_t launch_frames_warp(const FramesWarpParams &p, hipStream_t) {
    if (p.m1 <= p.m0) return hipSuccess;
    if (!p.src || !p.dst || !p.table || !p.anchor || !p.h_anchor || p.channels == 0 || p.channels > 65535u || p.n_anchors < 2 ||
        p.m1 > (uint64_t)kWarpBlock * (p.n_anchors - 1))
        return hipErrorInvalidValue;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    uint32_t tiers = 0;
    for (uint64_t b = p.m0 >> 6; b < (p.m1 + 63) >> 6; ++b) {
        const int64_t A0 = p.h_anchor[b], D = p.h_anchor[b + 1] - A0;
        if (p.anchor[b] != A0 || p.anchor[b + 1] != A0 + D) return hipErrorInvalidValue;
        if (A0 < 0 || D < kWarpDMin || D > kWarpDMax) return hipErrorInvalidValue;
        const uint32_t t = warp_tier(D);
        if (p.tier_off[t] == kWarpNoTier) return hipErrorInvalidValue;
        tiers |= 1u << t;
        const int64_t W = (int64_t)kWarpW[t];
        const int64_t i0 = b * 64 < p.m0 ? (int64_t)(p.m0 - b * 64) : 0;
        const int64_t i1 = (b + 1) * 64 > p.m1 ? (int64_t)(p.m1 - b * 64) - 1 : 63;
        lo = std::min(lo, ((A0 + ((D * i0) >> 6)) >> 32) - (W - 1));
        hi = std::max(hi, ((A0 + ((D * i1) >> 6)) >> 32) + W + 1);
    }
    const uint64_t need_lo = lo < 0 ? 0 : (uint64_t)lo, need_hi = hi < 0 ? 0 : std::min((uint64_t)hi, p.n);
    if (need_lo < need_hi && (need_lo < p.src0 || need_hi > p.src0 + p.src_len)) return hipErrorInvalidValue;
    if (rc_stub_warp_launches < 256)
        rc_stub_warp_log[rc_stub_warp_launches] = RcStubWarpLaunch{
            p.m0, p.m1, p.src0, p.src_len, p.n, p.stride, p.dst_stride, p.n_anchors, (uint64_t)hi, p.channels, tiers,
            (uintptr_t)p.src - (uintptr_t)(p.src0 * sizeof(float)), (uintptr_t)p.dst - (uintptr_t)(p.m0 * sizeof(float))};
    ++rc_stub_warp_launches;
    for (uint32_t t = 0; t < kWarpTiers; ++t)
        if (tiers >> t & 1u) rc_stub_warp_sum += p.table[p.tier_off[t]] + p.table[p.tier_off[t] + (uint64_t)kWarpRows * 2 * kWarpW[t] - 1];
    for (uint32_t c = 0; c < p.channels; ++c) {
        for (uint64_t k = need_lo; k < need_hi; ++k) rc_stub_warp_sum += p.src[(uint64_t)c * p.stride + (k - p.src0)];
        for (uint64_t i = 0; i < p.m1 - p.m0; ++i) p.dst[(uint64_t)c * p.dst_stride + i] = rc_stub_warp_mark;
    }
    return hipSuccess;
}
}  // namespace rc
