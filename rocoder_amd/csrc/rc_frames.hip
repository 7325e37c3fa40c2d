// Interleaved PCM frames <-> planar float rows, on the device (rc_engine_stretch_frames).
//
// Both kernels are transposes between a frame-major block (sample (f, c) at f * channels + c) and channel-major rows.
// Read or written directly, one side would be touched with a per-lane stride of channels x bytes. Instead a tile goes
// through LDS: on the global side consecutive lanes always take consecutive dwords (the frame side in 16-byte groups
// where a tile is one contiguous range), and the strided access, the byte phase and the sub-dword samples are dealt
// with in LDS.
//   channels <= 8  a tile is 1024 whole frames: one contiguous byte range of the frame block
//   channels  > 8  a tile is 64 frames x 64 channels: one contiguous range of up to 256 bytes per frame, a wave per row
// A sample is taken from LDS as the two dwords it may straddle, shifted right by its byte phase (v_alignbit): the same
// code serves a 16-bit sample at an even offset and a 24-bit one across a dword boundary.
#include "rc_frames.h"

namespace rc {
namespace {

// the 32 bits that start `byte` bytes into `lds` (the dword behind the last sample of a tile exists and is never used:
// a sample that ends at a dword boundary takes nothing from it)
__device__ __forceinline__ uint32_t lds_bits(const uint32_t *lds, uint32_t byte) {
    const uint32_t w = byte >> 2, sh = (byte & 3u) * 8u;
    const uint64_t two = ((uint64_t)lds[w + 1] << 32) | lds[w];
    return (uint32_t)(two >> sh);
}

// the reader's formulas (host/rocoder_cli.cpp read_wav): (float)n / K, one IEEE division each
template <uint32_t FMT>
__device__ __forceinline__ float pcm_decode(uint32_t v) {
    if (FMT == PCM_U8) return (float)((int)(v & 0xffu) - 128) / 127.0f;
    if (FMT == PCM_I16) return (float)(int)(int16_t)(v & 0xffffu) / 32767.0f;
    if (FMT == PCM_I24) return (float)(((int32_t)(v << 8)) >> 8) / 8388608.0f;
    if (FMT == PCM_I32) return (float)(int32_t)v / 2147483647.0f;
    return __uint_as_float(v);
}

template <uint32_t FMT>
constexpr uint32_t fmt_bytes() {
    return FMT == PCM_U8 ? 1u : FMT == PCM_I16 ? 2u : FMT == PCM_I24 ? 3u : 4u;
}

// ---- channels <= kNarrowChannels --------------------------------------------------------------------------------
// LDS: the 16-byte groups that cover 1024 frames of 8 channels of 4 bytes from any byte on (2048 + 2), + the spare dword
constexpr uint32_t kNarrowLdsDwords = (kNarrowFrames * kNarrowChannels * 4 / 16 + 2) * 4 + 4;

template <uint32_t FMT>
__global__ __launch_bounds__(kFramesThreads) void frames_unpack_kernel(FramesUnpackParams p) {
    constexpr uint32_t B = fmt_bytes<FMT>();
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNarrowLdsDwords];
    const uint32_t C = p.channels, tid = threadIdx.x;
    const uint64_t f0 = p.frame0 + (uint64_t)blockIdx.x * kNarrowFrames, f_end = p.frame0 + p.n_frames;
    if (f0 >= f_end) return;
    const uint32_t tf = (uint32_t)(f_end - f0 < kNarrowFrames ? f_end - f0 : kNarrowFrames);
    const uint64_t b0 = p.phase + f0 * C * B, b1 = b0 + (uint64_t)tf * C * B;
    const uint64_t g0 = b0 >> 4, g1 = (b1 + 15) >> 4;  // 16-byte groups [g0, g1): at most 2050
    const uint4 *raw4 = (const uint4 *)p.raw;
    const uint64_t raw_groups = p.raw_dwords >> 2;
    for (uint32_t g = tid; g < (uint32_t)(g1 - g0); g += kFramesThreads) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g0 + g < raw_groups) v = raw4[g0 + g];
        ((uint4 *)lds)[g] = v;
    }
    __syncthreads();
    const uint32_t lead = (uint32_t)(b0 - (g0 << 4));  // bytes of the first group in front of the tile
    for (uint32_t c = 0; c < C; ++c) {
        float *row = p.planar + (uint64_t)c * p.stride + f0;
        for (uint32_t fl = tid; fl < tf; fl += kFramesThreads)
            row[fl] = pcm_decode<FMT>(lds_bits(lds, lead + (fl * C + c) * B));
    }
}

__global__ __launch_bounds__(kFramesThreads) void frames_pack_kernel(FramesPackParams p) {
    __shared__ __attribute__((aligned(16))) float lds[kNarrowFrames * kNarrowChannels];
    const uint32_t C = p.channels, tid = threadIdx.x;
    const uint64_t f0 = (uint64_t)blockIdx.x * kNarrowFrames;
    if (f0 >= p.n_frames) return;
    const uint32_t tf = (uint32_t)(p.n_frames - f0 < kNarrowFrames ? p.n_frames - f0 : kNarrowFrames);
    for (uint32_t c = 0; c < C; ++c) {
        const float *row = p.planar + (uint64_t)c * p.stride + f0;
        for (uint32_t fl = tid; fl < tf; fl += kFramesThreads) lds[fl * C + c] = row[fl];
    }
    __syncthreads();
    float *dst = p.frames + f0 * C;
    const uint32_t total = tf * C;
    uint32_t done = 0;
    if (((uintptr_t)dst & 15u) == 0) {  // (a tile starts 1024 x channels floats after the one before it: all or none)
        const uint32_t n4 = total >> 2;
        for (uint32_t k = tid; k < n4; k += kFramesThreads) ((float4 *)dst)[k] = ((const float4 *)lds)[k];
        done = n4 << 2;
    }
    for (uint32_t k = done + tid; k < total; k += kFramesThreads) dst[k] = lds[k];
}

// ---- any channel count: 64 frames x 64 channels ----------------------------------------------------------------------
// a row of the tile: the dwords that cover 64 samples of 4 bytes from any byte on (65) + the spare dword, made odd so
// that the lanes of a wave, one row each, fall on different banks
constexpr uint32_t kWidePitch = 67;
constexpr uint32_t kWaves = kFramesThreads / 64;

template <uint32_t FMT>
__global__ __launch_bounds__(kFramesThreads) void frames_unpack_wide_kernel(FramesUnpackParams p) {
    constexpr uint32_t B = fmt_bytes<FMT>();
    __shared__ uint32_t lds[kWideFrames * kWidePitch];
    const uint32_t C = p.channels, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t f0 = p.frame0 + (uint64_t)blockIdx.x * kWideFrames, f_end = p.frame0 + p.n_frames;
    const uint32_t c0 = blockIdx.y * kWideChannels;
    if (f0 >= f_end || c0 >= C) return;
    const uint32_t tf = (uint32_t)(f_end - f0 < kWideFrames ? f_end - f0 : kWideFrames);
    const uint32_t tc = C - c0 < kWideChannels ? C - c0 : kWideChannels;
    for (uint32_t r = wave; r < tf; r += kWaves) {
        const uint64_t s = p.phase + ((f0 + r) * C + c0) * B, d0 = s >> 2, d1 = (s + (uint64_t)tc * B + 3) >> 2;
        const uint32_t nd = (uint32_t)(d1 - d0);  // at most 65
        for (uint32_t j = lane; j < nd; j += 64) lds[r * kWidePitch + j] = d0 + j < p.raw_dwords ? p.raw[d0 + j] : 0u;
    }
    __syncthreads();
    if (lane < tf) {
        const uint32_t lead = (uint32_t)((p.phase + ((f0 + lane) * C + c0) * B) & 3u);
        const uint32_t *row = lds + lane * kWidePitch;
        for (uint32_t c = wave; c < tc; c += kWaves)
            p.planar[(uint64_t)(c0 + c) * p.stride + f0 + lane] = pcm_decode<FMT>(lds_bits(row, lead + c * B));
    }
}

__global__ __launch_bounds__(kFramesThreads) void frames_pack_wide_kernel(FramesPackParams p) {
    constexpr uint32_t kPitch = kWideChannels + 1;
    __shared__ float lds[kWideFrames * kPitch];
    const uint32_t C = p.channels, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t f0 = (uint64_t)blockIdx.x * kWideFrames;
    const uint32_t c0 = blockIdx.y * kWideChannels;
    if (f0 >= p.n_frames || c0 >= C) return;
    const uint32_t tf = (uint32_t)(p.n_frames - f0 < kWideFrames ? p.n_frames - f0 : kWideFrames);
    const uint32_t tc = C - c0 < kWideChannels ? C - c0 : kWideChannels;
    if (lane < tf)
        for (uint32_t c = wave; c < tc; c += kWaves) lds[lane * kPitch + c] = p.planar[(uint64_t)(c0 + c) * p.stride + f0 + lane];
    __syncthreads();
    if (lane < tc)
        for (uint32_t r = wave; r < tf; r += kWaves) p.frames[(f0 + r) * C + c0 + lane] = lds[r * kPitch + lane];
}

// ---- planar float rows -> integer (or float) PCM frames at any byte address (rc_engine_stretch_frames_pcm) ----------
// The mirror image of the unpack kernels. Samples are quantised on their way into LDS, one per dword in frame order;
// the target is then written as whole dwords assembled from them. With 1-, 2- and 3-byte samples and a byte phase the
// byte ranges of neighbouring tiles (and of neighbouring launches, whose downloads are in flight) meet inside a dword.
// No dword is read back and none is written twice: a dword belongs to the tile that holds its LAST byte, and that tile
// also quantises the up to three samples in front of its own range that the dword starts with. Only the first and the
// last dword of a launch can be partial; they are written byte by byte, the bytes of the launch's frames and no other.

// the definition in rc_frames.h / include/rocoder_hip.h: t = x * S (one IEEE multiplication), rint, NaN -> 0, clamp
template <uint32_t FMT>
__device__ __forceinline__ uint32_t pcm_encode(float x) {
    if (FMT == PCM_F32) return __float_as_uint(x);
    constexpr float S = FMT == PCM_U8 ? 127.0f : FMT == PCM_I16 ? 32767.0f : FMT == PCM_I24 ? 8388608.0f : 2147483648.0f;
    constexpr float LO = FMT == PCM_U8 ? -128.0f : FMT == PCM_I16 ? -32768.0f : FMT == PCM_I24 ? -8388608.0f : -2147483648.0f;
    constexpr float HI = FMT == PCM_U8 ? 127.0f : FMT == PCM_I16 ? 32767.0f : FMT == PCM_I24 ? 8388607.0f : 2147483648.0f;
    float r = rintf(__fmul_rn(x, S));
    if (r != r) r = 0.0f;
    r = fminf(fmaxf(r, LO), HI);
    // (I32: 2^31 - 1 is no float; what the clamp leaves at 2^31 saturates)
    const int32_t n = (FMT == PCM_I32 && r >= 2147483648.0f) ? 2147483647 : (int32_t)r;
    return FMT == PCM_U8 ? (uint32_t)(n + 128) : (uint32_t)n;
}

__device__ __forceinline__ uint32_t pcm_is_clipped(float x) { return !(fabsf(x) <= 1.0f) ? 1u : 0u; }

// pcm_encode with the dither d in front of rint (rc_engine_set_output_dither): t1 = x * S, t2 = t1 + d, one IEEE operation
// each and never one fma (see below). U8, I16 and I24 only: the other two formats take no dither.
template <uint32_t FMT>
__device__ __forceinline__ uint32_t pcm_encode_dithered(float x, float d) {
    static_assert(FMT == PCM_U8 || FMT == PCM_I16 || FMT == PCM_I24, "no dither on i32 and f32");
    constexpr float S = FMT == PCM_U8 ? 127.0f : FMT == PCM_I16 ? 32767.0f : 8388608.0f;
    constexpr float LO = FMT == PCM_U8 ? -128.0f : FMT == PCM_I16 ? -32768.0f : -8388608.0f;
    constexpr float HI = FMT == PCM_U8 ? 127.0f : FMT == PCM_I16 ? 32767.0f : 8388607.0f;
    float t1 = __fmul_rn(x, S);
    // (the build contracts a * b + c wherever it sees one, through __fmul_rn / __fadd_rn too: the empty statement keeps
    // the rounded product, and d = i * 2^-16, in registers of their own, so that the addition below is an addition)
    asm volatile("" : "+v"(t1), "+v"(d));
    float r = rintf(__fadd_rn(t1, d));
    if (r != r) r = 0.0f;
    r = fminf(fmaxf(r, LO), HI);
    const int32_t n = (int32_t)r;
    return FMT == PCM_U8 ? (uint32_t)(n + 128) : (uint32_t)n;
}

// rc_phase_hash's mixer (rc_engine.cpp; rc_dev.hpp phase_hash_x) on x = counter * mul + k0
__device__ __forceinline__ uint32_t dither_hash_x(uint32_t x) {
    x ^= x >> 16;
    x *= 0x21F0AAADu;
    x ^= x >> 15;
    x *= 0x735A2D97u;
    x ^= x >> 15;
    return x;
}

// `q` holds one encoded sample per dword. The byte `rel` bytes into the stream of their low B bytes each ...
template <uint32_t B>
__device__ __forceinline__ uint32_t stream_byte(const uint32_t *q, uint32_t rel) {
    const uint32_t s = rel / B, k = rel - s * B;
    return (q[s] >> (8u * k)) & 0xffu;
}
// ... and the four bytes from there on (every sample they belong to is in q)
template <uint32_t B>
__device__ __forceinline__ uint32_t stream_dword(const uint32_t *q, uint32_t rel) {
    if (B == 4) {
        const uint32_t s = rel >> 2, sh = (rel & 3u) * 8u, lo = q[s];
        return sh ? (lo >> sh) | (q[s + 1] << (32u - sh)) : lo;
    }
    uint32_t s = rel / B, k = rel - s * B;
    uint32_t v = q[s] >> (8u * k), w = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        w |= (v & 0xffu) << (8u * j);
        v >>= 8;
        if (j < 3 && ++k == B) {
            k = 0;
            v = q[++s];
        }
    }
    return w;
}

// bytes [lo, hi) of one dword, from stream byte `rel` of q on
template <uint32_t B>
__device__ __forceinline__ void store_bytes(const uint32_t *q, uint32_t rel, uintptr_t lo, uintptr_t hi) {
    for (uintptr_t a = lo; a < hi; ++a) *(unsigned char *)a = (unsigned char)stream_byte<B>(q, rel + (uint32_t)(a - lo));
}

// per-lane counts -> one atomic of the workgroup (none where nothing clipped). Holds a barrier: every lane calls it.
__device__ __forceinline__ void add_clipped(uint32_t n, uint32_t *block_sum, uint64_t *clipped) {
    for (uint32_t off = 32; off; off >>= 1) n += __shfl_down(n, off);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(block_sum, n);
    __syncthreads();
    if (threadIdx.x == 0 && *block_sum) atomicAdd((unsigned long long *)clipped, (unsigned long long)*block_sum);
}

// The pack kernels below are templates over their parameter block: FramesPackPcmParams (rc_engine_stretch_frames_pcm:
// the samples as they are) or FramesPackPcmGainParams (rc_engine_stretch_frames_norm: every sample times a gain that
// each lane forms from the peak word - one correctly rounded division, the definition in rc_frames.h). The first
// instantiation is the kernel it was before the second existed: NoGain is the identity and holds nothing.
struct NoGain {
    __device__ __forceinline__ float operator()(float x) const { return x; }
};
struct Gain {
    float g;
    // (an intrinsic: never contracted with the quantiser's multiplication by S)
    __device__ __forceinline__ float operator()(float x) const { return __fmul_rn(x, g); }
};
__host__ __device__ __forceinline__ const FramesPackPcmParams &pack_of(const FramesPackPcmParams &p) { return p; }
__host__ __device__ __forceinline__ const FramesPackPcmParams &pack_of(const FramesPackPcmGainParams &p) { return p.pack; }
__device__ __forceinline__ NoGain gain_of(const FramesPackPcmParams &) { return NoGain{}; }
__device__ __forceinline__ Gain gain_of(const FramesPackPcmGainParams &p) {
    const float peak = __uint_as_float(p.norm->peak_bits), q = __fdiv_rn(p.target_peak, peak);
    const float g = (peak > 0.0f && q < __builtin_inff()) ? q : 1.0f;
    if (p.store_gain && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.norm->gain = g;
    return Gain{g};
}

// The dither is a third policy, beside the gain: what turns a sample x of row c at frame f of the launch into its code.
// NoDither is pcm_encode and looks at neither c nor f: the undithered instantiations are the kernels they were. Dither
// adds d(c, t) of the sample's OWN job channel and absolute frame, whichever tile quantises it (a tile re-quantises the
// up to three samples in front of it that its first dword starts with): the bytes do not depend on the tiling.
struct NoDither {
    struct Row {
        template <uint32_t FMT>
        __device__ __forceinline__ uint32_t encode(float x, uint32_t) const { return pcm_encode<FMT>(x); }
    };
    __device__ __forceinline__ Row row(uint32_t) const { return Row{}; }
    __device__ __forceinline__ Row wave_row(uint32_t) const { return Row{}; }
};
struct Dither {
    const uint64_t *keys;  // of the launch's row 0 on
    uint32_t t0, hp;       // the launch's frame 0 mod 2^32 (the counter is t mod 2^32); TPDF_HP
    struct Row {
        uint32_t mul, x0, hp;  // the hash's x at the launch's frame f: f * mul + x0
        template <uint32_t FMT>
        __device__ __forceinline__ uint32_t encode(float x, uint32_t f) const {
            const uint32_t xt = f * mul + x0, h = dither_hash_x(xt);
            // TPDF_HP: the counter one back is x - mul, at t = 0 the counter 0xFFFFFFFF as well (all mod 2^32)
            const int i = hp ? (int)(h >> 16) - (int)(dither_hash_x(xt - mul) >> 16) : (int)(h >> 16) - (int)(h & 0xFFFFu);
            return pcm_encode_dithered<FMT>(x, (float)i * (1.0f / 65536.0f));
        }
    };
    __device__ __forceinline__ Row row(uint32_t c) const {
        const uint64_t k = keys[c];
        const uint32_t mul = (uint32_t)(k >> 32) | 1u;
        return Row{mul, t0 * mul + (uint32_t)k, hp};
    }
    // row(c) where c is the same in every lane of the wave (the wide kernel's main loop: a wave per channel): said so, the
    // key is one scalar load and mul and x0 are formed once per wave, not once per lane
    __device__ __forceinline__ Row wave_row(uint32_t c) const { return row(__builtin_amdgcn_readfirstlane(c)); }
};
__host__ __device__ __forceinline__ const FramesPackPcmParams &pack_of(const FramesPackPcmDitherParams &p) { return p.pack; }
__host__ __device__ __forceinline__ const FramesPackPcmParams &pack_of(const FramesPackPcmGainDitherParams &p) { return p.gain.pack; }
__device__ __forceinline__ NoGain gain_of(const FramesPackPcmDitherParams &) { return NoGain{}; }
__device__ __forceinline__ Gain gain_of(const FramesPackPcmGainDitherParams &p) { return gain_of(p.gain); }
__device__ __forceinline__ NoDither dither_of(const FramesPackPcmParams &) { return NoDither{}; }
__device__ __forceinline__ NoDither dither_of(const FramesPackPcmGainParams &) { return NoDither{}; }
__device__ __forceinline__ Dither dither_of(const FramesDitherParams &d) {
    return Dither{d.keys + d.channel0, (uint32_t)d.t0, d.mode == 2u ? 1u : 0u};
}
__device__ __forceinline__ Dither dither_of(const FramesPackPcmDitherParams &p) { return dither_of(p.dither); }
__device__ __forceinline__ Dither dither_of(const FramesPackPcmGainDitherParams &p) { return dither_of(p.dither); }

// LDS: 1024 frames of 8 channels + the frames in front that the first dword starts with (at most 3 bytes: 3 + channels
// samples at the most)
constexpr uint32_t kPcmLdsDwords = kNarrowFrames * kNarrowChannels + 16;

template <uint32_t FMT, class PP>
__global__ __launch_bounds__(kFramesThreads) void frames_pack_pcm_kernel(PP pp) {
    constexpr uint32_t B = fmt_bytes<FMT>();
    __shared__ __attribute__((aligned(16))) uint32_t lds[kPcmLdsDwords];
    __shared__ uint32_t clip_sum;
    const FramesPackPcmParams &p = pack_of(pp);
    const uint32_t C = p.channels, tid = threadIdx.x;
    const uint64_t f0 = (uint64_t)blockIdx.x * kNarrowFrames;
    if (f0 >= p.n_frames) return;
    const auto gain = gain_of(pp);
    const auto dither = dither_of(pp);
    if (tid == 0) clip_sum = 0;
    __syncthreads();
    const uint32_t tf = (uint32_t)(p.n_frames - f0 < kNarrowFrames ? p.n_frames - f0 : kNarrowFrames);
    const uintptr_t T = (uintptr_t)p.target + p.phase, END = T + p.n_frames * C * B;  // the launch's bytes
    const uintptr_t g0 = T + f0 * C * B, g1 = g0 + (uintptr_t)tf * C * B;              // the tile's
    const uintptr_t a0 = g0 & ~(uintptr_t)3;                                            // its first dword
    const uintptr_t first = a0 > T ? a0 : T;                                            // its first byte
    // whole frames in front of the tile that byte `first` reaches into (0 for the first tile: first == T == g0)
    const uint32_t lead = ((uint32_t)(g0 - first) + C * B - 1) / (C * B);
    const uintptr_t P = g0 - (uintptr_t)lead * C * B;  // where lds[0] lies in the target
    const uint32_t sf = lead + tf;
    uint32_t nclip = 0;
    for (uint32_t c = 0; c < C; ++c) {
        const float *row = p.planar + (uint64_t)c * p.stride + (f0 - lead);
        const auto enc = dither.row(c);
        const uint32_t fr = (uint32_t)f0 - lead;  // the launch's frame of lds[0] (a launch has at most 2^27)
        for (uint32_t fl = tid; fl < sf; fl += kFramesThreads) {
            const float x = gain(row[fl]);
            lds[fl * C + c] = enc.template encode<FMT>(x, fr + fl);
            if (fl >= lead) nclip += pcm_is_clipped(x);  // (a frame in front is counted by its own tile)
        }
    }
    add_clipped(nclip, &clip_sum, p.clipped);  // (its barrier stands between the LDS stores above and the loads below)
    // the launch's partial first and last dword, byte by byte (one and the same dword in a launch of under 4 bytes)
    const uintptr_t t0 = END & ~(uintptr_t)3;
    if (tid == 0 && a0 < T) store_bytes<B>(lds, 0, T, a0 + 4 < END ? a0 + 4 : END);
    if (tid == 64 && g1 == END && (END & 3u) && t0 >= T) store_bytes<B>(lds, (uint32_t)(t0 - P), t0, END);
    // whole dwords [d0, d1): 16-byte groups from the first aligned address on, single dwords around them
    const uintptr_t d0 = a0 < T ? a0 + 4 : a0, d1 = g1 & ~(uintptr_t)3;
    const uint32_t nd = d1 > d0 ? (uint32_t)((d1 - d0) >> 2) : 0u;
    const uint32_t pre_want = (uint32_t)((16u - (d0 & 15u)) & 15u) >> 2, pre = pre_want < nd ? pre_want : nd;
    const uint32_t n4 = (nd - pre) >> 2;
    const uint32_t rel0 = (uint32_t)(d0 - P);
    uint4 *dst4 = (uint4 *)(d0 + 4u * pre);
    for (uint32_t k = tid; k < n4; k += kFramesThreads) {
        const uint32_t rel = rel0 + 4u * pre + 16u * k;
        dst4[k] = make_uint4(stream_dword<B>(lds, rel), stream_dword<B>(lds, rel + 4), stream_dword<B>(lds, rel + 8),
                             stream_dword<B>(lds, rel + 12));
    }
    uint32_t *dst = (uint32_t *)d0;
    if (tid < pre) dst[tid] = stream_dword<B>(lds, rel0 + 4u * tid);
    const uint32_t i = pre + 4u * n4 + tid;
    if (i < nd) dst[i] = stream_dword<B>(lds, rel0 + 4u * i);
}

// a row of the wide tile: 3 samples in front of the row's segment + 64 + odd
constexpr uint32_t kPcmWidePitch = 69;

template <uint32_t FMT, class PP>
__global__ __launch_bounds__(kFramesThreads) void frames_pack_pcm_wide_kernel(PP pp) {
    constexpr uint32_t B = fmt_bytes<FMT>();
    __shared__ uint32_t lds[kWideFrames * kPcmWidePitch];
    __shared__ uint32_t clip_sum;
    const FramesPackPcmParams &p = pack_of(pp);
    const uint32_t C = p.channels, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t f0 = (uint64_t)blockIdx.x * kWideFrames;
    const uint32_t c0 = blockIdx.y * kWideChannels;
    if (f0 >= p.n_frames || c0 >= C) return;
    const auto gain = gain_of(pp);
    const auto dither = dither_of(pp);
    if (tid == 0) clip_sum = 0;
    __syncthreads();
    const uint32_t tf = (uint32_t)(p.n_frames - f0 < kWideFrames ? p.n_frames - f0 : kWideFrames);
    const uint32_t tc = C - c0 < kWideChannels ? C - c0 : kWideChannels;
    const uintptr_t T = (uintptr_t)p.target + p.phase, END = T + p.n_frames * C * B;
    uint32_t nclip = 0;
    if (lane < tf)
        for (uint32_t c = wave; c < tc; c += kWaves) {
            const float x = gain(p.planar[(uint64_t)(c0 + c) * p.stride + f0 + lane]);
            lds[lane * kPcmWidePitch + 3 + c] = dither.wave_row(c0 + c).template encode<FMT>(x, (uint32_t)f0 + lane);
            nclip += pcm_is_clipped(x);
        }
    // the samples in front of a row's segment that its first dword starts with: sample e back ends at g0 - (e - 1) B
    for (uint32_t i = tid; i < tf * 3u; i += kFramesThreads) {
        const uint32_t r = i / 3u, e = i - r * 3u + 1u;
        const uintptr_t g0 = T + ((f0 + r) * C + c0) * B, a0 = g0 & ~(uintptr_t)3, first = a0 > T ? a0 : T;
        if (g0 - (e - 1u) * B > first) {  // (then it is a sample of the launch: its last byte is at or behind T)
            const uint64_t f = c0 >= e ? f0 + r : f0 + r - 1;
            const uint32_t c = c0 >= e ? c0 - e : C + c0 - e;
            lds[r * kPcmWidePitch + 3 - e] = dither.row(c).template encode<FMT>(gain(p.planar[(uint64_t)c * p.stride + f]), (uint32_t)f);
        }
    }
    add_clipped(nclip, &clip_sum, p.clipped);
    for (uint32_t r = wave; r < tf; r += kWaves) {
        const uint32_t *row = lds + r * kPcmWidePitch;
        const uintptr_t g0 = T + ((f0 + r) * C + c0) * B, g1 = g0 + (uintptr_t)tc * B;
        const uintptr_t P = g0 - 3u * B;  // where row[0] would lie in the target
        const uintptr_t a0 = g0 & ~(uintptr_t)3, a1 = g1 == END ? (g1 + 3) & ~(uintptr_t)3 : g1 & ~(uintptr_t)3;
        for (uintptr_t a = a0 + 4u * lane; a < a1; a += 256) {  // at most 65 dwords
            if (a >= T && a + 4 <= END) {
                *(uint32_t *)a = stream_dword<B>(row, (uint32_t)(a - P));
            } else {
                const uintptr_t lo = a > T ? a : T, hi = a + 4 < END ? a + 4 : END;
                store_bytes<B>(row, (uint32_t)(lo - P), lo, hi);
            }
        }
    }
}

// ---- the peak of planar rows (rc_engine_stretch_frames_norm, phase 1) ---------------------------------------------------
// A workgroup takes kPeakSegment samples of one row (blockIdx.y: the channel): 16-byte loads from the segment's first
// aligned address on, single dwords at its ragged ends (rows start at any float: a chunk's range, a stride of any length).
constexpr uint32_t kPeakSegment = 8192;

// the bits of |x| for a finite x, 0 for NaN and +-inf (whose bits would sort above every finite value)
__device__ __forceinline__ uint32_t peak_bits_of(float x) {
    const uint32_t b = __float_as_uint(x) & 0x7fffffffu;
    return b < 0x7f800000u ? b : 0u;
}

__global__ __launch_bounds__(kFramesThreads) void frames_peak_kernel(FramesPeakParams p) {
    __shared__ uint32_t wave_max[kFramesThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t s0 = (uint64_t)blockIdx.x * kPeakSegment;
    if (s0 >= p.n_frames) return;  // (the whole workgroup)
    const uint32_t len = (uint32_t)(p.n_frames - s0 < kPeakSegment ? p.n_frames - s0 : kPeakSegment);
    const float *q = p.planar + (uint64_t)blockIdx.y * p.stride + s0;
    const uint32_t head_want = (uint32_t)((16u - ((uintptr_t)q & 15u)) & 15u) >> 2, head = head_want < len ? head_want : len;
    const uint32_t n4 = (len - head) >> 2;
    uint32_t m = 0;
    if (tid < head) m = peak_bits_of(q[tid]);
    const float4 *q4 = (const float4 *)(q + head);
    for (uint32_t k = tid; k < n4; k += kFramesThreads) {
        const float4 v = q4[k];
        m = max(max(m, peak_bits_of(v.x)), max(peak_bits_of(v.y), max(peak_bits_of(v.z), peak_bits_of(v.w))));
    }
    const uint32_t t = head + 4u * n4 + tid;  // (at most 3 behind the groups)
    if (t < len) m = max(m, peak_bits_of(q[t]));
    for (uint32_t off = 32; off; off >>= 1) m = max(m, (uint32_t)__shfl_down(m, off));
    if ((tid & 63u) == 0) wave_max[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < kFramesThreads / 64; ++w) m = max(m, wave_max[w]);
        if (m) atomicMax(&p.norm->peak_bits, m);
    }
}

// ---- the output fade, in place on planar rows (rc_engine_set_output_fade; the definition: rc_frames.h) -----------------
// The peak kernel's shape: a workgroup takes kFadeSegment samples of one row (blockIdx.y: the channel), 16-byte loads and
// stores from the segment's first aligned address on, single dwords at its ragged ends. No two lanes share a sample.
constexpr uint32_t kFadeSegment = 8192;

// Position p of a fade of d frames, p < d. What makes every step one correctly rounded operation under this build:
//   - the division and the square root by hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt (the v_div_scale /
//     v_div_fmas / v_div_fixup sequence, v_sqrt_f32 with its correction step). Building with
//     -fno-hip-fp32-correctly-rounded-divide-sqrt or fast-math breaks the definition.
//   - the __f*_rn intrinsics are NOT a guard: in this toolchain's headers they are the plain operators unless
//     OCML_BASIC_ROUNDED_OPERATIONS is defined (they state the intent, no more), and __fsqrt_rn is the hardware's 1-ulp
//     approximation there, which is why the square root is sqrtf. Under -ffp-contract=fast the one fusable step is
//     r * 2 - 1, and r * 2 is exact, so fused and unfused give the same bits; the additions and multiplications behind
//     it feed a maximum, a square root or a store, which nothing fuses with.
__device__ __forceinline__ float fade_gain(uint64_t p, uint64_t d, bool falling) {
    const float r = __fdiv_rn(__ull2float_rn(p), __ull2float_rn(d));
    const float b = __fsub_rn(__fmul_rn(r, 2.0f), 1.0f);
    return sqrtf(__fmul_rn(0.5f, __fadd_rn(1.0f, fmaxf(falling ? -b : b, -1.0f))));
}

__device__ __forceinline__ bool fade_is_tail(uint64_t t, const FramesFadeParams &p) {
    return t >= p.out_start && t - p.out_start >= p.out_len;
}

__device__ __forceinline__ float fade_sample(float x, uint64_t t, const FramesFadeParams &p) {
    if (t < p.in_len) x = __fmul_rn(x, fade_gain(t, p.in_len, false));
    if (t >= p.out_start) x = t - p.out_start < p.out_len ? __fmul_rn(x, fade_gain(t - p.out_start, p.out_len, true)) : 0.0f;
    return x;
}

__global__ __launch_bounds__(kFramesThreads) void frames_fade_kernel(FramesFadeParams p) {
    const uint32_t tid = threadIdx.x;
    const uint64_t n = p.t1 - p.t0, s0 = (uint64_t)blockIdx.x * kFadeSegment;
    if (s0 >= n) return;  // (the whole workgroup)
    const uint32_t len = (uint32_t)(n - s0 < kFadeSegment ? n - s0 : kFadeSegment);
    float *q = p.planar + (uint64_t)blockIdx.y * p.stride + s0;
    const uint64_t t = p.t0 + s0;  // the frame of q[0]
    const uint32_t head_want = (uint32_t)((16u - ((uintptr_t)q & 15u)) & 15u) >> 2, head = head_want < len ? head_want : len;
    const uint32_t n4 = (len - head) >> 2;
    if (tid < head) q[tid] = fade_sample(q[tid], t + tid, p);
    float4 *q4 = (float4 *)(q + head);
    for (uint32_t k = tid; k < n4; k += kFramesThreads) {
        const uint64_t tk = t + head + 4u * k;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!fade_is_tail(tk, p)) {  // (behind the fade-out nothing is read: the group's later frames lie there too)
            v = q4[k];
            v.x = fade_sample(v.x, tk, p);
            v.y = fade_sample(v.y, tk + 1, p);
            v.z = fade_sample(v.z, tk + 2, p);
            v.w = fade_sample(v.w, tk + 3, p);
        }
        q4[k] = v;
    }
    const uint32_t i = head + 4u * n4 + tid;  // (at most 3 behind the groups)
    if (i < len) q[i] = fade_sample(q[i], t + i, p);
}

// ---- the peak of every bin of a raw frame block (rc_engine_frames_power; the definition: include/rocoder_hip.h) ----------
// A bin of bin_frames whole frames, every channel, is one contiguous range of the block's samples, so the kernel works on
// the sample stream and never asks which channel a sample is: sample s of the job (s = frame * channels + channel) lies
// in bin s / (bin_frames * channels). A workgroup takes kPowerTileBytes of the stream, whatever the channel count, through
// LDS as the narrow unpack kernel does: 16-byte loads of the groups that cover the tile, a sample taken as the two dwords
// it may straddle. What is reduced is a key that orders as |x| does - the magnitude of the integer, the bits of |x| for
// f32 - and the float of the definition is formed once per partial result: n -> fl((float)|n| / K) is monotone, so the
// largest key gives the largest |x|, bit for bit.
//   a tile in one or two bins (a bin no shorter than the tile)   registers, __shfl_down, one atomicMax per bin
//   a tile over more bins                                        an LDS word per bin, flushed with global atomics; above
//                                                                kPowerLdsBins bins (bins of under a dozen samples) every
//                                                                sample goes to its bin's global word itself
constexpr uint32_t kPowerTileBytes = 12288;  // a multiple of every sample size
constexpr uint32_t kPowerLdsDwords = (kPowerTileBytes / 16 + 2) * 4 + 4;
constexpr uint32_t kPowerLdsBins = 1024;
constexpr uint64_t kPowerMaxSamplesPerLaunch = (uint64_t)1 << 30;

// orders as |x| does; 0 for a zero of either sign and for NaN (skipped). +-inf is kept: it sorts above every finite value.
template <uint32_t FMT>
__device__ __forceinline__ uint32_t power_key(uint32_t v) {
    if (FMT == PCM_F32) {
        const uint32_t b = v & 0x7fffffffu;
        return b <= 0x7f800000u ? b : 0u;
    }
    const int32_t n = FMT == PCM_U8 ? (int32_t)(v & 0xffu) - 128 : FMT == PCM_I16 ? (int32_t)(int16_t)(v & 0xffffu)
                    : FMT == PCM_I24 ? ((int32_t)(v << 8)) >> 8 : (int32_t)v;
    return n < 0 ? 0u - (uint32_t)n : (uint32_t)n;  // (INT32_MIN: 2^31)
}

// the bits of |x| of the sample with that key: |(float)n / K| = (float)|n| / K, conversion and division rounded to nearest
template <uint32_t FMT>
__device__ __forceinline__ uint32_t power_bits(uint32_t key) {
    if (FMT == PCM_F32) return key;
    constexpr float K = FMT == PCM_U8 ? 127.0f : FMT == PCM_I16 ? 32767.0f : FMT == PCM_I24 ? 8388608.0f : 2147483647.0f;
    return __float_as_uint(__uint2float_rn(key) / K);
}

template <uint32_t FMT>
__global__ __launch_bounds__(kFramesThreads) void frames_power_kernel(FramesPowerParams p) {
    constexpr uint32_t B = fmt_bytes<FMT>(), TS = kPowerTileBytes / B;
    __shared__ __attribute__((aligned(16))) uint32_t lds[kPowerLdsDwords];
    __shared__ uint32_t bins[kPowerLdsBins];
    __shared__ uint32_t wave_max[2][kWaves];
    const uint32_t tid = threadIdx.x;
    const uint64_t s_end = (p.frame0 + p.n_frames) * p.channels;
    const uint64_t s0 = p.frame0 * p.channels + (uint64_t)blockIdx.x * TS;
    if (s0 >= s_end) return;  // (the whole workgroup)
    const uint32_t ts = (uint32_t)(s_end - s0 < TS ? s_end - s0 : TS);
    const uint64_t b0 = p.phase + s0 * B, b1 = b0 + (uint64_t)ts * B;
    const uint64_t g0 = b0 >> 4, g1 = (b1 + 15) >> 4;  // 16-byte groups [g0, g1): at most 769
    const uint4 *raw4 = (const uint4 *)p.raw;
    const uint64_t raw_groups = p.raw_dwords >> 2;
    for (uint32_t g = tid; g < (uint32_t)(g1 - g0); g += kFramesThreads) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g0 + g < raw_groups) v = raw4[g0 + g];
        ((uint4 *)lds)[g] = v;
    }
    const uint32_t lead = (uint32_t)(b0 - (g0 << 4));  // bytes of the first group in front of the tile
    const uint64_t bs = p.bin_frames * p.channels;     // samples of a bin
    const uint64_t bin_a = s0 / bs, n_touched = (s0 + ts - 1) / bs - bin_a + 1;
    if (n_touched <= 2) {
        // samples [0, edge) of the tile lie in bin_a, the rest in the bin behind it
        const uint32_t edge = n_touched == 2 ? (uint32_t)((bin_a + 1) * bs - s0) : ts;
        __syncthreads();
        uint32_t m0 = 0, m1 = 0;
        for (uint32_t i = tid; i < ts; i += kFramesThreads) {
            const uint32_t k = power_key<FMT>(lds_bits(lds, lead + i * B));
            if (i < edge) m0 = max(m0, k);
            else m1 = max(m1, k);
        }
        for (uint32_t off = 32; off; off >>= 1) {
            m0 = max(m0, (uint32_t)__shfl_down(m0, off));
            m1 = max(m1, (uint32_t)__shfl_down(m1, off));
        }
        if ((tid & 63u) == 0) {
            wave_max[0][tid >> 6] = m0;
            wave_max[1][tid >> 6] = m1;
        }
        __syncthreads();
        if (tid < 2) {  // (thread 0: bin_a, thread 1: the bin behind it)
            uint32_t m = 0;
            for (uint32_t w = 0; w < kWaves; ++w) m = max(m, wave_max[tid][w]);
            if (m) atomicMax(&p.bin_bits[bin_a + tid], power_bits<FMT>(m));
        }
        return;
    }
    // more than two bins: a bin is shorter than the tile, so a bin's length and the tile's offset in bin_a are small
    const uint32_t nb = (uint32_t)n_touched, bs32 = (uint32_t)bs, r0 = (uint32_t)(s0 - bin_a * bs);
    const bool in_lds = nb <= kPowerLdsBins;
    if (in_lds)
        for (uint32_t i = tid; i < nb; i += kFramesThreads) bins[i] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < ts; i += kFramesThreads) {
        const uint32_t k = power_key<FMT>(lds_bits(lds, lead + i * B));
        if (!k) continue;
        const uint32_t rel = (r0 + i) / bs32;
        if (in_lds) atomicMax(&bins[rel], k);
        else atomicMax(&p.bin_bits[bin_a + rel], power_bits<FMT>(k));
    }
    if (!in_lds) return;
    __syncthreads();
    for (uint32_t i = tid; i < nb; i += kFramesThreads)
        if (bins[i]) atomicMax(&p.bin_bits[bin_a + i], power_bits<FMT>(bins[i]));
}

// ---- the unpack kernels with a channel map (rc_engine_set_channel_map; FramesUnpackMapParams) ------------------------------
// Row c is filled from channel map[c]. The global side is what it is without a map: whole tiles, consecutive lanes on
// consecutive dwords. Up to kNarrowChannels channels the tile holds whole frames, and the map is an index in the LDS read.
template <uint32_t FMT>
__global__ __launch_bounds__(kFramesThreads) void frames_unpack_map_kernel(FramesUnpackMapParams pm) {
    constexpr uint32_t B = fmt_bytes<FMT>();
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNarrowLdsDwords];
    const FramesUnpackParams &p = pm.unpack;
    const uint32_t C = p.channels, tid = threadIdx.x;
    const uint64_t f0 = p.frame0 + (uint64_t)blockIdx.x * kNarrowFrames, f_end = p.frame0 + p.n_frames;
    if (f0 >= f_end) return;
    const uint32_t tf = (uint32_t)(f_end - f0 < kNarrowFrames ? f_end - f0 : kNarrowFrames);
    const uint64_t b0 = p.phase + f0 * C * B, b1 = b0 + (uint64_t)tf * C * B;
    const uint64_t g0 = b0 >> 4, g1 = (b1 + 15) >> 4;  // 16-byte groups [g0, g1): at most 2050
    const uint4 *raw4 = (const uint4 *)p.raw;
    const uint64_t raw_groups = p.raw_dwords >> 2;
    for (uint32_t g = tid; g < (uint32_t)(g1 - g0); g += kFramesThreads) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g0 + g < raw_groups) v = raw4[g0 + g];
        ((uint4 *)lds)[g] = v;
    }
    __syncthreads();
    const uint32_t lead = (uint32_t)(b0 - (g0 << 4));  // bytes of the first group in front of the tile
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t m = min(pm.map[c], C - 1u);
        float *row = p.planar + (uint64_t)c * p.stride + f0;
        for (uint32_t fl = tid; fl < tf; fl += kFramesThreads)
            row[fl] = pcm_decode<FMT>(lds_bits(lds, lead + (fl * C + m) * B));
    }
}

// Above, a workgroup owns 64 frames of 64 ROWS (blockIdx.y: the row tile) and fetches, one after the other and each once,
// the 64-channel SOURCE tiles that hold a channel one of its rows reads, in rising order: the load of a source tile is the
// unmapped kernel's, and behind it the rows whose source lies in that tile are written, a wave per row. An identity-like
// map costs one source tile per row tile, as without a map; a map that scatters the 64 rows of a tile over 64 source
// tiles reads 64 tiles for it, every load still coalesced.
template <uint32_t FMT>
__global__ __launch_bounds__(kFramesThreads) void frames_unpack_map_wide_kernel(FramesUnpackMapParams pm) {
    constexpr uint32_t B = fmt_bytes<FMT>();
    __shared__ uint32_t lds[kWideFrames * kWidePitch];
    __shared__ uint32_t src[kWideChannels];
    const FramesUnpackParams &p = pm.unpack;
    const uint32_t C = p.channels, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t f0 = p.frame0 + (uint64_t)blockIdx.x * kWideFrames, f_end = p.frame0 + p.n_frames;
    const uint32_t c0 = blockIdx.y * kWideChannels;
    if (f0 >= f_end || c0 >= C) return;
    const uint32_t tf = (uint32_t)(f_end - f0 < kWideFrames ? f_end - f0 : kWideFrames);
    const uint32_t tc = C - c0 < kWideChannels ? C - c0 : kWideChannels;
    if (threadIdx.x < tc) src[threadIdx.x] = min(pm.map[c0 + threadIdx.x], C - 1u);
    __syncthreads();
    for (uint32_t next = 0;;) {
        // the lowest source tile from `next` on that a row of this workgroup reads (every lane finds the same)
        uint32_t t = UINT32_MAX;
        for (uint32_t c = 0; c < tc; ++c) {
            const uint32_t tc_of = src[c] / kWideChannels;
            if (tc_of >= next && tc_of < t) t = tc_of;
        }
        if (t == UINT32_MAX) break;
        const uint32_t s0 = t * kWideChannels, sc = C - s0 < kWideChannels ? C - s0 : kWideChannels;
        for (uint32_t r = wave; r < tf; r += kWaves) {
            const uint64_t s = p.phase + ((f0 + r) * C + s0) * B, d0 = s >> 2, d1 = (s + (uint64_t)sc * B + 3) >> 2;
            const uint32_t nd = (uint32_t)(d1 - d0);  // at most 65
            for (uint32_t j = lane; j < nd; j += 64) lds[r * kWidePitch + j] = d0 + j < p.raw_dwords ? p.raw[d0 + j] : 0u;
        }
        __syncthreads();
        if (lane < tf) {
            const uint32_t lead = (uint32_t)((p.phase + ((f0 + lane) * C + s0) * B) & 3u);
            const uint32_t *row = lds + lane * kWidePitch;
            for (uint32_t c = wave; c < tc; c += kWaves) {
                const uint32_t m = src[c];
                if (m / kWideChannels == t)
                    p.planar[(uint64_t)(c0 + c) * p.stride + f0 + lane] = pcm_decode<FMT>(lds_bits(row, lead + (m - s0) * B));
            }
        }
        next = t + 1;
        __syncthreads();  // (the next source tile goes into the same LDS)
    }
}

// ---- the peak of every channel of a raw frame block (rc_engine_frames_channel_peaks; FramesChannelPeaksParams) ------------
// frames_power_kernel's integer key, with NaN kept: the bits of |x| for f32 as they are (a NaN sorts above +inf, +inf
// above every finite magnitude), the magnitude of the integer otherwise; power_bits forms the float once per partial
// result. A workgroup walks several tiles of the unpack kernels' shapes and joins each channel with one atomicMax.
//   channels <= 8  kChanPeakNarrowTiles tiles of 1024 whole frames: a thread keeps one running maximum per channel in
//                  registers over its frames; they are reduced across the wave, then across the waves through LDS
//   channels  > 8  kChanPeakWideTiles tiles of 64 frames x 64 channels: a lane owns a channel of the tile (consecutive lanes
//                  read consecutive samples of an LDS row), a wave every fourth frame
constexpr uint32_t kChanPeakNarrowTiles = 4, kChanPeakWideTiles = 16;

template <uint32_t FMT>
__device__ __forceinline__ uint32_t chan_key(uint32_t v) {
    if (FMT == PCM_F32) return v & 0x7fffffffu;
    return power_key<FMT>(v);
}

template <uint32_t FMT>
__global__ __launch_bounds__(kFramesThreads) void frames_channel_peaks_kernel(FramesChannelPeaksParams p) {
    constexpr uint32_t B = fmt_bytes<FMT>();
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNarrowLdsDwords];
    __shared__ uint32_t wave_max[kNarrowChannels][kWaves];
    const uint32_t C = p.channels, tid = threadIdx.x;
    const uint64_t f_end = p.frame0 + p.n_frames;
    uint64_t f0 = p.frame0 + (uint64_t)blockIdx.x * (kChanPeakNarrowTiles * kNarrowFrames);
    if (f0 >= f_end) return;  // (the whole workgroup)
    const uint4 *raw4 = (const uint4 *)p.raw;
    const uint64_t raw_groups = p.raw_dwords >> 2;
    uint32_t m[kNarrowChannels];
#pragma unroll
    for (uint32_t c = 0; c < kNarrowChannels; ++c) m[c] = 0;
    for (uint32_t t = 0; t < kChanPeakNarrowTiles && f0 < f_end; ++t, f0 += kNarrowFrames) {
        const uint32_t tf = (uint32_t)(f_end - f0 < kNarrowFrames ? f_end - f0 : kNarrowFrames);
        const uint64_t b0 = p.phase + f0 * C * B, b1 = b0 + (uint64_t)tf * C * B;
        const uint64_t g0 = b0 >> 4, g1 = (b1 + 15) >> 4;  // 16-byte groups [g0, g1): at most 2050
        if (t) __syncthreads();  // (the tile before has been read)
        for (uint32_t g = tid; g < (uint32_t)(g1 - g0); g += kFramesThreads) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g0 + g < raw_groups) v = raw4[g0 + g];
            ((uint4 *)lds)[g] = v;
        }
        __syncthreads();
        const uint32_t lead = (uint32_t)(b0 - (g0 << 4));
        for (uint32_t fl = tid; fl < tf; fl += kFramesThreads) {
#pragma unroll
            for (uint32_t c = 0; c < kNarrowChannels; ++c)
                if (c < C) m[c] = max(m[c], chan_key<FMT>(lds_bits(lds, lead + (fl * C + c) * B)));
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < kNarrowChannels; ++c) {
        uint32_t v = m[c];
        for (uint32_t off = 32; off; off >>= 1) v = max(v, (uint32_t)__shfl_down(v, off));
        if ((tid & 63u) == 0) wave_max[c][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < C) {
        uint32_t v = 0;
        for (uint32_t w = 0; w < kWaves; ++w) v = max(v, wave_max[tid][w]);
        if (v) atomicMax(&p.chan_bits[tid], power_bits<FMT>(v));
    }
}

template <uint32_t FMT>
__global__ __launch_bounds__(kFramesThreads) void frames_channel_peaks_wide_kernel(FramesChannelPeaksParams p) {
    constexpr uint32_t B = fmt_bytes<FMT>();
    __shared__ uint32_t lds[kWideFrames * kWidePitch];
    __shared__ uint32_t wave_max[kWaves][kWideChannels];
    const uint32_t C = p.channels, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t f_end = p.frame0 + p.n_frames;
    uint64_t f0 = p.frame0 + (uint64_t)blockIdx.x * (kChanPeakWideTiles * kWideFrames);
    const uint32_t c0 = blockIdx.y * kWideChannels;
    if (f0 >= f_end || c0 >= C) return;  // (the whole workgroup)
    const uint32_t tc = C - c0 < kWideChannels ? C - c0 : kWideChannels;
    uint32_t m = 0;
    for (uint32_t t = 0; t < kChanPeakWideTiles && f0 < f_end; ++t, f0 += kWideFrames) {
        const uint32_t tf = (uint32_t)(f_end - f0 < kWideFrames ? f_end - f0 : kWideFrames);
        if (t) __syncthreads();  // (the tile before has been read)
        for (uint32_t r = wave; r < tf; r += kWaves) {
            const uint64_t s = p.phase + ((f0 + r) * C + c0) * B, d0 = s >> 2, d1 = (s + (uint64_t)tc * B + 3) >> 2;
            const uint32_t nd = (uint32_t)(d1 - d0);  // at most 65
            for (uint32_t j = lane; j < nd; j += 64) lds[r * kWidePitch + j] = d0 + j < p.raw_dwords ? p.raw[d0 + j] : 0u;
        }
        __syncthreads();
        if (lane < tc)
            for (uint32_t r = wave; r < tf; r += kWaves) {
                const uint32_t lead = (uint32_t)((p.phase + ((f0 + r) * C + c0) * B) & 3u);
                m = max(m, chan_key<FMT>(lds_bits(lds + r * kWidePitch, lead + lane * B)));
            }
    }
    wave_max[wave][lane] = m;
    __syncthreads();
    if (wave == 0 && lane < tc) {
        for (uint32_t w = 1; w < kWaves; ++w) m = max(m, wave_max[w][lane]);
        if (m) atomicMax(&p.chan_bits[c0 + lane], power_bits<FMT>(m));
    }
}

constexpr uint64_t kMaxFramesPerLaunch = (uint64_t)1 << 27;  // (a grid dimension times the block stays far below 2^32)

// the launches after the first of a job of more than kMaxFramesPerLaunch frames: the gain is stored once
inline FramesPackPcmParams &pack_of(FramesPackPcmParams &p) { return p; }
inline FramesPackPcmParams &pack_of(FramesPackPcmGainParams &p) { return p.pack; }
inline void next_launch(FramesPackPcmParams &) {}
inline void next_launch(FramesPackPcmGainParams &p) { p.store_gain = 0; }
inline FramesPackPcmParams &pack_of(FramesPackPcmDitherParams &p) { return p.pack; }
inline FramesPackPcmParams &pack_of(FramesPackPcmGainDitherParams &p) { return p.gain.pack; }
inline void next_launch(FramesPackPcmDitherParams &) {}
inline void next_launch(FramesPackPcmGainDitherParams &p) { p.gain.store_gain = 0; }
// a launch's absolute frame 0: the job's t0 + the frames of the launches in front of it (the dithered blocks only)
inline void launch_frame0(FramesPackPcmParams &, uint64_t) {}
inline void launch_frame0(FramesPackPcmGainParams &, uint64_t) {}
inline void launch_frame0(FramesPackPcmDitherParams &p, uint64_t t0) { p.dither.t0 = t0; }
inline void launch_frame0(FramesPackPcmGainDitherParams &p, uint64_t t0) { p.dither.t0 = t0; }
inline uint64_t frame0_of(const FramesPackPcmParams &) { return 0; }
inline uint64_t frame0_of(const FramesPackPcmGainParams &) { return 0; }
inline uint64_t frame0_of(const FramesPackPcmDitherParams &p) { return p.dither.t0; }
inline uint64_t frame0_of(const FramesPackPcmGainDitherParams &p) { return p.dither.t0; }

template <uint32_t FMT, class PP>
hipError_t pack_pcm_fmt(const PP &pp, hipStream_t s) {
    constexpr uint32_t B = fmt_bytes<FMT>();
    const FramesPackPcmParams &p = pack_of(pp);
    const bool narrow = p.channels <= kNarrowChannels;
    const uint32_t per = narrow ? kNarrowFrames : kWideFrames;
    PP qq = pp;
    for (uint64_t done = 0; done < p.n_frames; done += kMaxFramesPerLaunch) {
        FramesPackPcmParams &q = pack_of(qq);
        const uint64_t off = p.phase + done * p.channels * B;
        q.planar = p.planar + done;
        q.target = p.target + (off & ~(uint64_t)3);
        q.phase = (uint32_t)(off & 3u);
        q.n_frames = p.n_frames - done < kMaxFramesPerLaunch ? p.n_frames - done : kMaxFramesPerLaunch;
        if (done) next_launch(qq);
        launch_frame0(qq, frame0_of(pp) + done);
        const uint32_t tiles = (uint32_t)((q.n_frames + per - 1) / per);
        if (narrow) {
            frames_pack_pcm_kernel<FMT, PP><<<dim3(tiles), dim3(kFramesThreads), 0, s>>>(qq);
        } else {
            const uint32_t ct = (p.channels + kWideChannels - 1) / kWideChannels;
            frames_pack_pcm_wide_kernel<FMT, PP><<<dim3(tiles, ct), dim3(kFramesThreads), 0, s>>>(qq);
        }
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

template <uint32_t FMT>
hipError_t unpack_fmt(const FramesUnpackParams &p, hipStream_t s) {
    const bool narrow = p.channels <= kNarrowChannels;
    const uint32_t per = narrow ? kNarrowFrames : kWideFrames;
    for (uint64_t done = 0; done < p.n_frames; done += kMaxFramesPerLaunch) {
        FramesUnpackParams q = p;
        q.frame0 = p.frame0 + done;
        q.n_frames = p.n_frames - done < kMaxFramesPerLaunch ? p.n_frames - done : kMaxFramesPerLaunch;
        const uint32_t tiles = (uint32_t)((q.n_frames + per - 1) / per);
        if (narrow) {
            frames_unpack_kernel<FMT><<<dim3(tiles), dim3(kFramesThreads), 0, s>>>(q);
        } else {
            const uint32_t ct = (p.channels + kWideChannels - 1) / kWideChannels;
            frames_unpack_wide_kernel<FMT><<<dim3(tiles, ct), dim3(kFramesThreads), 0, s>>>(q);
        }
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

template <uint32_t FMT>
hipError_t power_fmt(const FramesPowerParams &p, hipStream_t s) {
    constexpr uint32_t TS = kPowerTileBytes / fmt_bytes<FMT>();
    // (a launch: at most 2^27 frames and at most 2^30 samples, whichever is fewer; at least one frame)
    const uint64_t by_samples = kPowerMaxSamplesPerLaunch / p.channels;
    const uint64_t per = by_samples < kMaxFramesPerLaunch ? (by_samples ? by_samples : 1) : kMaxFramesPerLaunch;
    for (uint64_t done = 0; done < p.n_frames; done += per) {
        FramesPowerParams q = p;
        q.frame0 = p.frame0 + done;
        q.n_frames = p.n_frames - done < per ? p.n_frames - done : per;
        const uint32_t tiles = (uint32_t)((q.n_frames * p.channels + TS - 1) / TS);
        frames_power_kernel<FMT><<<dim3(tiles), dim3(kFramesThreads), 0, s>>>(q);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

template <uint32_t FMT>
hipError_t unpack_map_fmt(const FramesUnpackMapParams &pm, hipStream_t s) {
    const FramesUnpackParams &p = pm.unpack;
    const bool narrow = p.channels <= kNarrowChannels;
    const uint32_t per = narrow ? kNarrowFrames : kWideFrames;
    for (uint64_t done = 0; done < p.n_frames; done += kMaxFramesPerLaunch) {
        FramesUnpackMapParams q = pm;
        q.unpack.frame0 = p.frame0 + done;
        q.unpack.n_frames = p.n_frames - done < kMaxFramesPerLaunch ? p.n_frames - done : kMaxFramesPerLaunch;
        const uint32_t tiles = (uint32_t)((q.unpack.n_frames + per - 1) / per);
        if (narrow) {
            frames_unpack_map_kernel<FMT><<<dim3(tiles), dim3(kFramesThreads), 0, s>>>(q);
        } else {
            const uint32_t ct = (p.channels + kWideChannels - 1) / kWideChannels;
            frames_unpack_map_wide_kernel<FMT><<<dim3(tiles, ct), dim3(kFramesThreads), 0, s>>>(q);
        }
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

template <uint32_t FMT>
hipError_t channel_peaks_fmt(const FramesChannelPeaksParams &p, hipStream_t s) {
    const bool narrow = p.channels <= kNarrowChannels;
    const uint32_t per = narrow ? kChanPeakNarrowTiles * kNarrowFrames : kChanPeakWideTiles * kWideFrames;
    for (uint64_t done = 0; done < p.n_frames; done += kMaxFramesPerLaunch) {
        FramesChannelPeaksParams q = p;
        q.frame0 = p.frame0 + done;
        q.n_frames = p.n_frames - done < kMaxFramesPerLaunch ? p.n_frames - done : kMaxFramesPerLaunch;
        const uint32_t groups = (uint32_t)((q.n_frames + per - 1) / per);
        if (narrow) {
            frames_channel_peaks_kernel<FMT><<<dim3(groups), dim3(kFramesThreads), 0, s>>>(q);
        } else {
            const uint32_t ct = (p.channels + kWideChannels - 1) / kWideChannels;
            frames_channel_peaks_wide_kernel<FMT><<<dim3(groups, ct), dim3(kFramesThreads), 0, s>>>(q);
        }
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_frames_unpack(uint32_t format, const FramesUnpackParams &p, hipStream_t s) {
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || p.phase > 3u || (p.raw_dwords & 3u) || ((uintptr_t)p.raw & 15u))
        return hipErrorInvalidValue;
    switch (format) {
    case PCM_U8: return unpack_fmt<PCM_U8>(p, s);
    case PCM_I16: return unpack_fmt<PCM_I16>(p, s);
    case PCM_I24: return unpack_fmt<PCM_I24>(p, s);
    case PCM_I32: return unpack_fmt<PCM_I32>(p, s);
    case PCM_F32: return unpack_fmt<PCM_F32>(p, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_frames_pack(const FramesPackParams &p, hipStream_t s) {
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u) return hipErrorInvalidValue;
    const bool narrow = p.channels <= kNarrowChannels;
    const uint32_t per = narrow ? kNarrowFrames : kWideFrames;
    for (uint64_t done = 0; done < p.n_frames; done += kMaxFramesPerLaunch) {
        FramesPackParams q = p;
        q.planar = p.planar + done;
        q.frames = p.frames + done * p.channels;
        q.n_frames = p.n_frames - done < kMaxFramesPerLaunch ? p.n_frames - done : kMaxFramesPerLaunch;
        const uint32_t tiles = (uint32_t)((q.n_frames + per - 1) / per);
        if (narrow) {
            frames_pack_kernel<<<dim3(tiles), dim3(kFramesThreads), 0, s>>>(q);
        } else {
            const uint32_t ct = (p.channels + kWideChannels - 1) / kWideChannels;
            frames_pack_wide_kernel<<<dim3(tiles, ct), dim3(kFramesThreads), 0, s>>>(q);
        }
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

hipError_t launch_frames_pack_pcm(uint32_t format, const FramesPackPcmParams &p, hipStream_t s) {
    if (!pcm_bytes(format)) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || p.phase > 3u || ((uintptr_t)p.target & 3u) || !p.clipped) return hipErrorInvalidValue;
    switch (format) {
    case PCM_U8: return pack_pcm_fmt<PCM_U8>(p, s);
    case PCM_I16: return pack_pcm_fmt<PCM_I16>(p, s);
    case PCM_I24: return pack_pcm_fmt<PCM_I24>(p, s);
    case PCM_I32: return pack_pcm_fmt<PCM_I32>(p, s);
    default: return pack_pcm_fmt<PCM_F32>(p, s);
    }
}

hipError_t launch_frames_peak(const FramesPeakParams &p, hipStream_t s) {
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || !p.norm) return hipErrorInvalidValue;
    for (uint64_t done = 0; done < p.n_frames; done += kMaxFramesPerLaunch) {
        FramesPeakParams q = p;
        q.planar = p.planar + done;
        q.n_frames = p.n_frames - done < kMaxFramesPerLaunch ? p.n_frames - done : kMaxFramesPerLaunch;
        const uint32_t segs = (uint32_t)((q.n_frames + kPeakSegment - 1) / kPeakSegment);
        frames_peak_kernel<<<dim3(segs, p.channels), dim3(kFramesThreads), 0, s>>>(q);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

hipError_t launch_frames_pack_pcm_gain(uint32_t format, const FramesPackPcmGainParams &pp, hipStream_t s) {
    const FramesPackPcmParams &p = pp.pack;
    if (!pcm_bytes(format)) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || p.phase > 3u || ((uintptr_t)p.target & 3u) || !p.clipped || !pp.norm ||
        !(pp.target_peak > 0.0f && pp.target_peak < __builtin_inff()))
        return hipErrorInvalidValue;
    switch (format) {
    case PCM_U8: return pack_pcm_fmt<PCM_U8>(pp, s);
    case PCM_I16: return pack_pcm_fmt<PCM_I16>(pp, s);
    case PCM_I24: return pack_pcm_fmt<PCM_I24>(pp, s);
    case PCM_I32: return pack_pcm_fmt<PCM_I32>(pp, s);
    default: return pack_pcm_fmt<PCM_F32>(pp, s);
    }
}

namespace {
bool dither_ok(uint32_t format, const FramesPackPcmParams &p, const FramesDitherParams &d) {
    return (d.mode == 1u || d.mode == 2u) && d.keys && (uint64_t)d.channel0 + p.channels <= 65535u &&
           (format == PCM_U8 || format == PCM_I16 || format == PCM_I24);
}
}  // namespace

hipError_t launch_frames_pack_pcm_dither(uint32_t format, const FramesPackPcmDitherParams &pp, hipStream_t s) {
    const FramesPackPcmParams &p = pp.pack;
    if (!pcm_bytes(format)) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || p.phase > 3u || ((uintptr_t)p.target & 3u) || !p.clipped || !dither_ok(format, p, pp.dither))
        return hipErrorInvalidValue;
    switch (format) {
    case PCM_U8: return pack_pcm_fmt<PCM_U8>(pp, s);
    case PCM_I16: return pack_pcm_fmt<PCM_I16>(pp, s);
    default: return pack_pcm_fmt<PCM_I24>(pp, s);
    }
}

hipError_t launch_frames_pack_pcm_gain_dither(uint32_t format, const FramesPackPcmGainDitherParams &pp, hipStream_t s) {
    const FramesPackPcmParams &p = pp.gain.pack;
    if (!pcm_bytes(format)) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || p.phase > 3u || ((uintptr_t)p.target & 3u) || !p.clipped || !pp.gain.norm ||
        !(pp.gain.target_peak > 0.0f && pp.gain.target_peak < __builtin_inff()) || !dither_ok(format, p, pp.dither))
        return hipErrorInvalidValue;
    switch (format) {
    case PCM_U8: return pack_pcm_fmt<PCM_U8>(pp, s);
    case PCM_I16: return pack_pcm_fmt<PCM_I16>(pp, s);
    default: return pack_pcm_fmt<PCM_I24>(pp, s);
    }
}

hipError_t launch_frames_fade(const FramesFadeParams &p, hipStream_t s) {
    if (p.t1 <= p.t0) return hipSuccess;
    if (!p.planar || p.channels == 0 || p.channels > 65535u || (p.out_start != UINT64_MAX && p.out_start + p.out_len < p.out_start))
        return hipErrorInvalidValue;
    for (uint64_t done = p.t0; done < p.t1; done += kMaxFramesPerLaunch) {
        FramesFadeParams q = p;
        q.planar = p.planar + (done - p.t0);
        q.t0 = done;
        q.t1 = p.t1 - done < kMaxFramesPerLaunch ? p.t1 : done + kMaxFramesPerLaunch;
        const uint32_t segs = (uint32_t)((q.t1 - q.t0 + kFadeSegment - 1) / kFadeSegment);
        frames_fade_kernel<<<dim3(segs, p.channels), dim3(kFramesThreads), 0, s>>>(q);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

hipError_t launch_frames_power(uint32_t format, const FramesPowerParams &pp, hipStream_t s) {
    if (!pcm_bytes(format)) return hipErrorInvalidValue;
    if (pp.n_frames == 0) return hipSuccess;
    if (pp.channels == 0 || pp.channels > 65535u || pp.phase > 3u || (pp.raw_dwords & 3u) || ((uintptr_t)pp.raw & 15u) || !pp.bin_bits ||
        pp.bin_frames == 0 || pp.frame0 + pp.n_frames < pp.frame0)
        return hipErrorInvalidValue;
    FramesPowerParams p = pp;
    // every frame of the range lies in front of frame0 + n_frames: a longer bin holds the same frames, and the kernel's
    // samples of a bin (bin_frames x channels) stay far inside 64 bits
    if (p.bin_frames > p.frame0 + p.n_frames) p.bin_frames = p.frame0 + p.n_frames;
    if ((p.frame0 + p.n_frames - 1) / p.bin_frames >= p.n_bins) return hipErrorInvalidValue;  // a bin behind bin_bits
    // the range's last byte lies inside raw
    if ((p.phase + (p.frame0 + p.n_frames) * p.channels * pcm_bytes(format) + 3) / 4 > p.raw_dwords) return hipErrorInvalidValue;
    switch (format) {
    case PCM_U8: return power_fmt<PCM_U8>(p, s);
    case PCM_I16: return power_fmt<PCM_I16>(p, s);
    case PCM_I24: return power_fmt<PCM_I24>(p, s);
    case PCM_I32: return power_fmt<PCM_I32>(p, s);
    default: return power_fmt<PCM_F32>(p, s);
    }
}

hipError_t launch_frames_unpack_map(uint32_t format, const FramesUnpackMapParams &pm, hipStream_t s) {
    const FramesUnpackParams &p = pm.unpack;
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || p.phase > 3u || (p.raw_dwords & 3u) || ((uintptr_t)p.raw & 15u) || !pm.map)
        return hipErrorInvalidValue;
    switch (format) {
    case PCM_U8: return unpack_map_fmt<PCM_U8>(pm, s);
    case PCM_I16: return unpack_map_fmt<PCM_I16>(pm, s);
    case PCM_I24: return unpack_map_fmt<PCM_I24>(pm, s);
    case PCM_I32: return unpack_map_fmt<PCM_I32>(pm, s);
    case PCM_F32: return unpack_map_fmt<PCM_F32>(pm, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_frames_channel_peaks(uint32_t format, const FramesChannelPeaksParams &p, hipStream_t s) {
    if (!pcm_bytes(format)) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    if (p.channels == 0 || p.channels > 65535u || p.phase > 3u || (p.raw_dwords & 3u) || ((uintptr_t)p.raw & 15u) || !p.chan_bits ||
        p.frame0 + p.n_frames < p.frame0)
        return hipErrorInvalidValue;
    // the range's last byte lies inside raw
    if ((p.phase + (p.frame0 + p.n_frames) * p.channels * pcm_bytes(format) + 3) / 4 > p.raw_dwords) return hipErrorInvalidValue;
    switch (format) {
    case PCM_U8: return channel_peaks_fmt<PCM_U8>(p, s);
    case PCM_I16: return channel_peaks_fmt<PCM_I16>(p, s);
    case PCM_I24: return channel_peaks_fmt<PCM_I24>(p, s);
    case PCM_I32: return channel_peaks_fmt<PCM_I32>(p, s);
    default: return channel_peaks_fmt<PCM_F32>(p, s);
    }
}

}  // namespace rc
