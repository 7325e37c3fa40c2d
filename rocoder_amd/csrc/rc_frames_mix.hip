// The mix launch of rc_engine_mix_frames (include/rocoder_hip_mix.h; the definition is stated there and in rc_frames.h): a
// chunk of a layer's planar rows, under the layer's keyframed envelope and through its send, accumulated into the bus rows.
// No hop kernel family and no family hash (tools/kernel_id.py), as the other frames kernels.
//
// Memory-bound: per landed sample one row word in, one bus word in, one bus word out. The streaming shape: a thread takes
// one 16-byte group of BUS frames - the bus is the read-modify-write, so the alignment is taken there, and `offset` leaves
// the rows to fall as they do (16-byte loads at dword alignment) - forms amp(t) of its four frames once and uses it
// for every bus channel in a loop inside the thread; at most kMixMaxBlocks workgroups, a grid-stride for the rest. The
// first and the last group of the range may be ragged: those go word by word, so that no word outside
// [max(0, offset + t0), min(N, offset + t1)) of any row is read or written.
#include "rc_frames.h"

namespace rc {
namespace {

constexpr uint32_t kMixMaxBlocks = 2048;

// The last key at or in front of frame t, for key_frame[0] <= t < key_frame[K - 1], K >= 2: one binary search.
__device__ __forceinline__ uint32_t mix_segment(const uint64_t *key_frame, uint32_t K, uint64_t t) {
    uint32_t lo = 0, hi = K - 1;  // key_frame[lo] <= t < key_frame[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key_frame[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// math::sqrt_interp(a, b, r). One rounding per operation under this build (-ffp-contract=fast): the division and the
// square root as in rc_frames.hip's fade_gain (hipcc's correctly rounded divide / sqrt; sqrtf, not __fsqrt_rn); r * 2 is
// exact, so r * 2 - 1 gives the same bits fused or not, and the multiplication by +-1 is a change of sign. The one step
// the build would contract is |b - a| * fct + lo: the empty statement keeps the rounded product in a register of its own
// (the idiom of pcm_encode_dithered).
__device__ __forceinline__ float mix_sqrt_interp(float a, float b, float r) {
    const bool inc = a < b;
    const float c = __fsub_rn(__fmul_rn(r, 2.0f), 1.0f);
    const float fct = sqrtf(__fmul_rn(0.5f, __fadd_rn(1.0f, fmaxf(inc ? c : -c, -1.0f))));
    float prod = __fmul_rn(fabsf(__fsub_rn(b, a)), fct);
    float lo = inc ? a : b;
    asm volatile("" : "+v"(prod), "+v"(lo));
    return __fadd_rn(lo, prod);
}

// The segment a thread is in: the last key at or in front of its frame and the words of that pair of keys, loaded when
// the thread enters the segment and kept for the frames it stays there.
struct MixSegment {
    uint32_t i;
    bool loaded;
    uint64_t k0, k1;
    float a, b, den;
};

// amp(t); `sg` steps forward with t, never back
__device__ __forceinline__ float mix_amp(const FramesMixParams &p, uint64_t t, MixSegment *sg) {
    const uint32_t K = p.n_keys;
    if (K == 0) return 1.0f;
    if (K == 1 || t < p.key_frame[0]) return p.key_amp[0];
    if (t >= p.key_frame[K - 1]) return p.key_amp[K - 1];
    if (!sg->loaded || t >= sg->k1) {
        uint32_t i = sg->i;
        while (p.key_frame[i + 1] <= t) ++i;  // (t < key_frame[K - 1]: ends at K - 2 at the latest)
        sg->i = i;
        sg->k0 = p.key_frame[i];
        sg->k1 = p.key_frame[i + 1];
        sg->a = p.key_amp[i];
        sg->b = p.key_amp[i + 1];
        sg->den = __ull2float_rn(sg->k1 - sg->k0);
        sg->loaded = true;
    }
    const float r = __fdiv_rn(__ull2float_rn(t - sg->k0), sg->den);
    return mix_sqrt_interp(sg->a, sg->b, r);
}

// Four frames of a row from its first, which is 4-byte aligned and no more: one 16-byte load (global multi-dword loads
// need dword alignment only), so that a row that `offset` leaves misaligned against the bus costs no more instructions.
__device__ __forceinline__ float4 mix_load4(const float *x) {
    float4 v;
    __builtin_memcpy(&v, x, sizeof v);
    return v;
}

// s[cb][t] for one frame / for four: the row itself, or ONE fmaf chain per frame over the layer's channels from +0 with cl
// ascending (the one fused operation of the definition). x: the sample of layer channel 0 at frame t.
__device__ __forceinline__ float mix_send(const FramesMixParams &p, const float *x, uint32_t cb) {
    if (!p.send) return x[(uint64_t)cb * p.stride];
    const float *w = p.send + (uint64_t)cb * p.channels;
    float acc = 0.0f;
    for (uint32_t cl = 0; cl < p.channels; ++cl) acc = fmaf(w[cl], x[(uint64_t)cl * p.stride], acc);
    return acc;
}
__device__ __forceinline__ float4 mix_send4(const FramesMixParams &p, const float *x, uint32_t cb) {
    if (!p.send) return mix_load4(x + (uint64_t)cb * p.stride);
    const float *w = p.send + (uint64_t)cb * p.channels;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t cl = 0; cl < p.channels; ++cl) {
        const float4 v = mix_load4(x + (uint64_t)cl * p.stride);
        const float g = w[cl];
        acc.x = fmaf(g, v.x, acc.x);
        acc.y = fmaf(g, v.y, acc.y);
        acc.z = fmaf(g, v.z, acc.z);
        acc.w = fmaf(g, v.w, acc.w);
    }
    return acc;
}

// bus + s * amp: a multiplication, then an addition
__device__ __forceinline__ float mix_acc(float bus, float s, float amp) {
    float prod = __fmul_rn(s, amp);
    asm volatile("" : "+v"(prod), "+v"(bus));
    return __fadd_rn(bus, prod);
}

// u_lo, u_hi: the bus frames the launch lands on, 0 <= u_lo < u_hi <= N. Group g holds the bus frames [4 g, 4 g + 4).
__global__ __launch_bounds__(kFramesThreads) void frames_mix_kernel(FramesMixParams p, uint64_t u_lo, uint64_t u_hi) {
    const uint64_t g_lo = u_lo >> 2, g_hi = (u_hi + 3) >> 2;
    const uint64_t step = (uint64_t)gridDim.x * kFramesThreads;
    for (uint64_t g = g_lo + (uint64_t)blockIdx.x * kFramesThreads + threadIdx.x; g < g_hi; g += step) {
        const uint64_t u = g << 2;
        const uint64_t a = u < u_lo ? u_lo : u, b = u + 4 < u_hi ? u + 4 : u_hi;  // the group's frames of the range: [a, b)
        const uint64_t t_a = (uint64_t)((int64_t)a - p.offset);                  // layer frame of bus frame a (>= t0)
        const float *x = p.rows + (t_a - p.t0);
        MixSegment seg{0, false, 0, 0, 0.0f, 0.0f, 1.0f};
        if (p.n_keys >= 2 && t_a >= p.key_frame[0] && t_a < p.key_frame[p.n_keys - 1]) seg.i = mix_segment(p.key_frame, p.n_keys, t_a);
        if (b - a == 4) {
            float amp[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) amp[i] = mix_amp(p, t_a + i, &seg);
            for (uint32_t cb = 0; cb < p.bus_channels; ++cb) {
                float4 *q = (float4 *)(p.bus + (uint64_t)cb * p.bus_stride + u);
                const float4 sv = mix_send4(p, x, cb);
                float4 v = *q;
                v.x = mix_acc(v.x, sv.x, amp[0]);
                v.y = mix_acc(v.y, sv.y, amp[1]);
                v.z = mix_acc(v.z, sv.z, amp[2]);
                v.w = mix_acc(v.w, sv.w, amp[3]);
                *q = v;
            }
        } else {  // a ragged first or last group: word by word
            for (uint64_t f = a; f < b; ++f) {
                const float amp = mix_amp(p, t_a + (f - a), &seg);
                for (uint32_t cb = 0; cb < p.bus_channels; ++cb) {
                    float *q = p.bus + (uint64_t)cb * p.bus_stride + f;
                    *q = mix_acc(*q, mix_send(p, x + (f - a), cb), amp);
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_frames_mix(const FramesMixParams &p, hipStream_t s) {
    if (p.t1 < p.t0 || p.n_keys > kMixMaxKeys) return hipErrorInvalidValue;
    if (p.t1 == p.t0) return hipSuccess;
    if (!p.rows || !p.bus || (p.n_keys && (!p.key_frame || !p.key_amp)) || p.channels == 0 || p.bus_channels == 0 ||
        (!p.send && p.channels != p.bus_channels) || (p.bus_stride & 3u) || ((uintptr_t)p.bus & 15u) || p.bus_stride < p.bus_frames ||
        p.t1 > ((uint64_t)1 << 62) || p.offset > ((int64_t)1 << 62) || p.offset < -((int64_t)1 << 62) || p.bus_frames > ((uint64_t)1 << 62))
        return hipErrorInvalidValue;
    // the bus frames the range lands on, in signed 64 bits (every term is within +-2^62)
    const int64_t lo = p.offset + (int64_t)p.t0, hi = p.offset + (int64_t)p.t1;
    const int64_t u_lo = lo < 0 ? 0 : lo, u_hi = hi < (int64_t)p.bus_frames ? hi : (int64_t)p.bus_frames;
    if (u_hi <= u_lo) return hipSuccess;  // wholly outside the bus
    const uint64_t groups = (((uint64_t)u_hi + 3) >> 2) - ((uint64_t)u_lo >> 2);
    const uint64_t blocks = (groups + kFramesThreads - 1) / kFramesThreads;
    frames_mix_kernel<<<dim3((uint32_t)(blocks < kMixMaxBlocks ? blocks : kMixMaxBlocks)), dim3(kFramesThreads), 0, s>>>(p, (uint64_t)u_lo, (uint64_t)u_hi);
    return hipGetLastError();
}

}  // namespace rc
