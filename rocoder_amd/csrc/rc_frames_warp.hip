// Band-limited resampling of planar float rows by a step that varies along the output (rc_engine_set_output_warp; the
// definition is stated in include/rocoder_hip_warp.h and rc_warp.h): output frame m = 64 b + i reads the position
// P(m) = anchor[b] + ((anchor[b + 1] - anchor[b]) * i >> 6), q = P >> 32, p = (P >> 24) & 255, a = (P & 0xFFFFFF) * 2^-24,
// and y = a == 0 ? y0 : fmaf(a, y1 - y0, y0) with y0 / y1 the fmaf chains over rows p / p + 1 of the block's tier.
//
// Mapping. A workgroup takes kWarpTileBlocks = 16 blocks (1024 outputs) of one channel, counted from the block
// that holds m0, and stages the span of the row that their taps cover in LDS with coalesced loads, zeros where the span
// leaves [0, n): at most 1023 * 8 + 1 + 512 floats. A wave takes whole blocks, one after the other, a lane one output:
// tier, W, T and D_b are wave-uniform, so there is no divergence inside a wave but the store mask at the ends of [m0, m1).
// Nothing of the table is shared between outputs - every lane has its own (p, a) - so the table lies TAP-MAJOR on the
// device, h[j][257]: rows p and p + 1 are neighbours, and a wave's loads at one tap fall inside 1028 bytes (L1 / L2), where
// the row-major layout gives 64 lines 2 W floats apart.
// Every output's two chains run over j = 0 ... T - 1 from +0: the order depends on (t, p, a, j) alone, so a sample's bits
// do not depend on the tile, the launch or the range it was computed in.
#include "rc_frames.h"
#include "rc_warp.h"

namespace rc {
namespace {

constexpr uint32_t kWarpTileBlocks = 16;
constexpr uint64_t kMaxWarpPerLaunch = (uint64_t)1 << 27;  // outputs: a multiple of the tile
constexpr uint32_t kWarpSpan = 1023 * 8 + 1 + 2 * 256;     // floats of LDS: 34 KB

__device__ const int64_t kTierD[kWarpTiers] = {RC_WARP_D_LIST};
__device__ const uint32_t kTierW[kWarpTiers] = {RC_WARP_W_LIST};

__device__ __forceinline__ uint32_t tier_of(int64_t D) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k + 1 < kWarpTiers; ++k) t += D > kTierD[k] ? 1u : 0u;
    return t;
}

__global__ __launch_bounds__(kFramesThreads) void frames_warp_kernel(FramesWarpParams p) {
    __shared__ float span[kWarpSpan];
    const uint64_t b_first = (p.m0 >> 6) + (uint64_t)blockIdx.x * kWarpTileBlocks;
    const uint64_t b_all = (p.m1 + 63) >> 6;
    const uint64_t b_end = b_first + kWarpTileBlocks < b_all ? b_first + kWarpTileBlocks : b_all;
    const uint32_t c = blockIdx.y;
    // the span of the tile's taps: over its blocks, from the first tap of a block's first frame inside [m0, m1) to the last
    // tap of its last one (a lower tier behind a higher one may start further left than the tile's first frame does)
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    for (uint64_t b = b_first; b < b_end; ++b) {
        const int64_t A0 = p.anchor[b], D = p.anchor[b + 1] - A0;
        const int64_t W = (int64_t)kTierW[tier_of(D)];
        const int64_t i0 = b * 64 < p.m0 ? (int64_t)(p.m0 - b * 64) : 0;
        const int64_t i1 = (b + 1) * 64 > p.m1 ? (int64_t)(p.m1 - b * 64) - 1 : 63;
        const int64_t q0 = (A0 + ((D * i0) >> 6)) >> 32, q1 = (A0 + ((D * i1) >> 6)) >> 32;
        lo = q0 - (W - 1) < lo ? q0 - (W - 1) : lo;
        hi = q1 + W + 1 > hi ? q1 + W + 1 : hi;
    }
    // (the setter and the launcher hold every step inside [2^35, 2^41], which keeps the span inside the array; a table that
    // breaks that is not computed on)
    if (hi <= lo || hi - lo > (int64_t)kWarpSpan) return;
    const uint32_t span_len = (uint32_t)(hi - lo);
    const float *row = p.src + (uint64_t)c * p.stride;
    for (uint32_t s = threadIdx.x; s < span_len; s += kFramesThreads) {
        const int64_t a = lo + (int64_t)s;
        float v = 0.0f;
        // (the launcher has seen to it that a frame inside [0, n) is one of src; the second test keeps a wrong call in bounds)
        if (a >= 0 && (uint64_t)a < p.n && (uint64_t)a >= p.src0 && (uint64_t)a - p.src0 < p.src_len) v = row[(uint64_t)a - p.src0];
        span[s] = v;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float *out = p.dst + (uint64_t)c * p.dst_stride;
    for (uint64_t b = b_first + wave; b < b_end; b += kFramesThreads / 64) {
        const int64_t A0 = p.anchor[b], D = p.anchor[b + 1] - A0;
        const uint32_t t = tier_of(D);
        const uint32_t off = p.tier_off[t];
        if (off == kWarpNoTier) continue;
        const uint32_t W = kTierW[t], T = 2 * W;
        const uint64_t m = b * 64 + lane;
        const bool mine = m >= p.m0 && m < p.m1;
        const int64_t P = A0 + ((D * (int64_t)lane) >> 6);
        const int64_t k0 = (P >> 32) - (int64_t)(W - 1);
        const uint32_t ph = (uint32_t)(P >> 24) & 255u;
        const float a = (float)(uint32_t)(P & 0xFFFFFF) * 0x1p-24f;
        // a lane outside [m0, m1) computes on the span's first frames and stores nothing
        const uint32_t at = mine && k0 >= lo && k0 + (int64_t)T <= hi ? (uint32_t)(k0 - lo) : 0u;
        const float *h = p.table + off + ph;
        const float *x = span + at;
        float y0 = 0.0f, y1 = 0.0f;
#pragma unroll 4
        for (uint32_t j = 0; j < T; ++j) {
            const float xj = x[j];
            y0 = fmaf(h[0], xj, y0);
            y1 = fmaf(h[1], xj, y1);
            h += kWarpRows;
        }
        const float y = a == 0.0f ? y0 : fmaf(a, y1 - y0, y0);
        if (mine) out[m - p.m0] = y;
    }
}

}  // namespace

hipError_t launch_frames_warp(const FramesWarpParams &p, hipStream_t s) {
    if (p.m1 <= p.m0) return hipSuccess;
    if (!p.src || !p.dst || !p.table || !p.anchor || !p.h_anchor || p.channels == 0 || p.channels > 65535u || p.n_anchors < 2 ||
        p.m1 > (uint64_t)kWarpBlock * (p.n_anchors - 1) || p.src0 + p.src_len < p.src0)
        return hipErrorInvalidValue;
    // the taps of the range are the frames [lo, hi) of the row; those of them inside [0, n) must be frames of src
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    for (uint64_t b = p.m0 >> 6; b < (p.m1 + 63) >> 6; ++b) {
        const int64_t A0 = p.h_anchor[b], A1 = p.h_anchor[b + 1];
        if (A0 < 0 || A1 >= kWarpMaxAnchor || A1 < A0 || A1 - A0 < kWarpDMin || A1 - A0 > kWarpDMax) return hipErrorInvalidValue;
        const int64_t D = A1 - A0;
        const uint32_t t = warp_tier(D);
        if (p.tier_off[t] == kWarpNoTier) return hipErrorInvalidValue;
        const int64_t W = (int64_t)kWarpW[t];
        const int64_t i0 = b * 64 < p.m0 ? (int64_t)(p.m0 - b * 64) : 0;
        const int64_t i1 = (b + 1) * 64 > p.m1 ? (int64_t)(p.m1 - b * 64) - 1 : 63;
        lo = std::min(lo, ((A0 + ((D * i0) >> 6)) >> 32) - (W - 1));
        hi = std::max(hi, ((A0 + ((D * i1) >> 6)) >> 32) + W + 1);
    }
    const uint64_t need_lo = lo < 0 ? 0 : (uint64_t)lo, need_hi = hi < 0 ? 0 : std::min((uint64_t)hi, p.n);
    if (need_lo < need_hi && (need_lo < p.src0 || need_hi > p.src0 + p.src_len)) return hipErrorInvalidValue;
    for (uint64_t done = p.m0; done < p.m1; done += kMaxWarpPerLaunch) {
        FramesWarpParams q = p;
        q.dst = p.dst + (done - p.m0);
        q.m0 = done;
        q.m1 = p.m1 - done < kMaxWarpPerLaunch ? p.m1 : done + kMaxWarpPerLaunch;
        const uint64_t blocks = ((q.m1 + 63) >> 6) - (q.m0 >> 6);
        const uint32_t tiles = (uint32_t)((blocks + kWarpTileBlocks - 1) / kWarpTileBlocks);
        frames_warp_kernel<<<dim3(tiles, p.channels), dim3(kFramesThreads), 0, s>>>(q);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace rc
