// Band-limited resampling of planar float rows by a rational step (rc_engine_set_output_resample; the definition is stated
// in include/rocoder_hip.h): y[c][m] = sum_j table[p][j] * x[c][k0 + j], q = floor(m * num / den), p = (m * num) mod den,
// k0 = q - (W - 1), T = 2 W taps, x zero outside [0, n).
//
// Mapping. A workgroup takes kResampleTile consecutive outputs of one channel. Their taps lie in one span of
// the row, q(last) - q(first) + T floats (at most 1023 * 8 + 1 + 512), which the workgroup stages in LDS with coalesced
// loads, zeros where the span leaves [0, n). Outputs m and m + den share a table row, so the tile's outputs are dealt out
// by phase class: a work item is (class r, group g) and computes the outputs r + den * (g + G * k), k < kResampleAcc, of
// the tile in registers. Its row is read once from global memory (L2: den * T floats, 274 KB at 1069/1009) and every
// coefficient meets up to kResampleAcc samples from LDS. Lanes of a wave hold consecutive classes: their LDS addresses
// at one tap are num/den apart on average, conflict-free up to a step of 1 and num/den-way above it.
// Every output is one chain acc = fmaf(h[p][j], x[k0 + j], acc), j = 0 ... T - 1, from +0: the order depends on j alone,
// so a sample's bits do not depend on the tile, the launch or the range it was computed in.
#include "rc_frames.h"

namespace rc {
namespace {

constexpr uint32_t kResampleTile = 1024;
constexpr uint32_t kResampleAcc = 8;
constexpr uint32_t kResampleMaxW = 256;                                               // T = 2 W <= 512
constexpr uint64_t kMaxResamplePerLaunch = (uint64_t)1 << 27;                        // outputs: a multiple of the tile
constexpr uint32_t kResampleSpan = (kResampleTile - 1) * 8 + 1 + 2 * kResampleMaxW;  // floats of LDS: 34 KB

__global__ __launch_bounds__(kFramesThreads) void frames_resample_kernel(FramesResampleParams p) {
    __shared__ float span[kResampleSpan];
    const uint64_t mt = p.m0 + (uint64_t)blockIdx.x * kResampleTile;  // the tile's first output
    const uint32_t count = (uint32_t)(p.m1 - mt < kResampleTile ? p.m1 - mt : kResampleTile);
    const uint32_t c = blockIdx.y;
    const uint32_t W = p.W, T = 2 * W;
    const uint64_t num = p.num, den = p.den;
    const uint64_t q_first = mt * num / den, q_last = (mt + count - 1) * num / den;
    const int64_t span0 = (int64_t)q_first - (int64_t)(W - 1);  // absolute input frame of span[0]
    const uint32_t span_len = (uint32_t)(q_last - q_first) + T;
    const float *row = p.src + (uint64_t)c * p.stride;
    for (uint32_t s = threadIdx.x; s < span_len; s += kFramesThreads) {
        const int64_t a = span0 + (int64_t)s;
        float v = 0.0f;
        // (the launcher has seen to it that a frame inside [0, n) is one of src; the second test keeps a wrong call in bounds)
        if (a >= 0 && (uint64_t)a < p.n && (uint64_t)a >= p.src0 && (uint64_t)a - p.src0 < p.src_len) v = row[(uint64_t)a - p.src0];
        span[s] = v;
    }
    __syncthreads();
    // phase classes of the tile, and the groups that share a class's outputs where there are fewer classes than threads
    const uint32_t R = den < count ? (uint32_t)den : count;
    const uint32_t G = R >= kFramesThreads ? 1u : kFramesThreads / R;
    float *out = p.dst + (uint64_t)c * p.dst_stride + (mt - p.m0);
    for (uint32_t w = threadIdx.x; w < R * G; w += kFramesThreads) {
        const uint32_t r = w % R, g = w / R;
        const uint64_t i0 = (uint64_t)r + den * g, step = den * G;  // the item's outputs: i0 + step * k inside the tile
        if (i0 >= count) continue;
        const uint32_t ph = (uint32_t)(((mt + r) * num) % den);
        const float *h = p.table + (uint64_t)ph * T;
        uint32_t at[kResampleAcc];
        float acc[kResampleAcc];
#pragma unroll
        for (uint32_t k = 0; k < kResampleAcc; ++k) {
            const uint64_t i = i0 + step * k;
            // an output beyond the tile computes on the item's first one and is not stored
            at[k] = (uint32_t)((mt + (i < count ? i : i0)) * num / den - q_first);
            acc[k] = 0.0f;
        }
        for (uint32_t j = 0; j < T; j += 2) {  // (T is even and the table 8-byte aligned: two coefficients a load)
            const float2 hj = *(const float2 *)(h + j);
#pragma unroll
            for (uint32_t k = 0; k < kResampleAcc; ++k) {
                acc[k] = fmaf(hj.x, span[at[k] + j], acc[k]);
                acc[k] = fmaf(hj.y, span[at[k] + j + 1], acc[k]);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kResampleAcc; ++k) {
            const uint64_t i = i0 + step * k;
            if (i < count) out[i] = acc[k];
        }
    }
}

}  // namespace

hipError_t launch_frames_resample(const FramesResampleParams &p, hipStream_t s) {
    if (p.m1 <= p.m0) return hipSuccess;
    if (!p.src || !p.dst || !p.table || p.channels == 0 || p.channels > 65535u || p.num == 0 || p.den == 0 || p.den > 1024u ||
        p.num > 8u * p.den || p.den > 8u * p.num || p.W == 0 || p.W > kResampleMaxW || p.m1 > (UINT64_MAX >> 14) ||
        p.src0 + p.src_len < p.src0 || ((uintptr_t)p.table & 7u))
        return hipErrorInvalidValue;
    // the taps of the range are the frames [lo, hi) of the row; those of them inside [0, n) must be frames of src
    const int64_t lo = (int64_t)(p.m0 * p.num / p.den) - (int64_t)(p.W - 1);
    const uint64_t hi = (p.m1 - 1) * p.num / p.den + p.W + 1;
    const uint64_t need_lo = lo < 0 ? 0 : (uint64_t)lo, need_hi = hi < p.n ? hi : p.n;
    if (need_lo < need_hi && (need_lo < p.src0 || need_hi > p.src0 + p.src_len)) return hipErrorInvalidValue;
    for (uint64_t done = p.m0; done < p.m1; done += kMaxResamplePerLaunch) {
        FramesResampleParams q = p;
        q.dst = p.dst + (done - p.m0);
        q.m0 = done;
        q.m1 = p.m1 - done < kMaxResamplePerLaunch ? p.m1 : done + kMaxResamplePerLaunch;
        const uint32_t tiles = (uint32_t)((q.m1 - q.m0 + kResampleTile - 1) / kResampleTile);
        frames_resample_kernel<<<dim3(tiles, p.channels), dim3(kFramesThreads), 0, s>>>(q);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace rc
