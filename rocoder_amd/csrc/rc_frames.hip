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

constexpr uint64_t kMaxFramesPerLaunch = (uint64_t)1 << 27;  // (a grid dimension times the block stays far below 2^32)

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

}  // namespace rc
