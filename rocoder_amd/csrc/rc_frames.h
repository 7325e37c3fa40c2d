// Interleaved PCM frames <-> the engine's planar float rows (rc_engine_stretch_frames): parameter blocks and launcher
// prototypes of rc_frames.hip. Kept apart from rc_kernels.h: these kernels move samples, they are no part of a hop
// kernel family and of no family hash (tools/kernel_id.py).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <stddef.h>
#include <stdint.h>

namespace rc {

// sample formats: the values of RC_PCM_* (include/rocoder_hip.h)
enum : uint32_t { PCM_U8 = 1, PCM_I16 = 2, PCM_I24 = 3, PCM_I32 = 4, PCM_F32 = 5 };

inline uint32_t pcm_bytes(uint32_t format) {
    return format == PCM_U8 ? 1u : format == PCM_I16 ? 2u : format == PCM_I24 ? 3u : (format == PCM_I32 || format == PCM_F32) ? 4u : 0u;
}

// Tiles. Up to kNarrowChannels channels a tile is kNarrowFrames whole frames: one contiguous byte range of the frame
// block. Above, a tile is kWideFrames frames x kWideChannels channels: one contiguous range per frame.
constexpr uint32_t kFramesThreads = 256;
constexpr uint32_t kNarrowChannels = 8, kNarrowFrames = 1024;
constexpr uint32_t kWideChannels = 64, kWideFrames = 64;

// frames [frame0, frame0 + n_frames) of a block of raw frames -> planar[c * stride + frame0 + i], every channel c.
// Sample (f, c) of the block starts at byte `phase + (f * channels + c) * bytes` of `raw`; raw is 16-byte aligned
// and holds raw_dwords (a multiple of 4) readable dwords, which cover every byte of the frames asked for. The kernel
// reads whole 16-byte groups around its tile: bytes of those groups that belong to no frame of the tile are loaded
// and never looked at.
struct FramesUnpackParams {
    const uint32_t *raw;
    uint64_t raw_dwords;
    uint32_t phase;  // 0 ... 3
    uint32_t channels;
    uint64_t frame0, n_frames;
    float *planar;
    uint64_t stride;  // floats between the rows of two channels
};

// planar[c * stride + i], i < n_frames, every channel c -> frames[(i) * channels + c]
struct FramesPackParams {
    const float *planar;
    uint64_t stride;
    float *frames;
    uint64_t n_frames;
    uint32_t channels;
};

// planar[c * stride + i], i < n_frames, every channel c -> sample (i, c) of a frame-major block of PCM samples of `format`,
// little endian, which starts at byte target + phase (target: 4-byte aligned; the block may start and end anywhere in a
// dword). Quantisation, bit for bit what include/rocoder_hip.h states (rc_engine_stretch_frames_pcm):
//   t = x * (float)S, ONE IEEE multiplication; r = rint(t), ties to even, NaN -> 0; n = r clamped to [LO, HI]
//   U8   S 127         [-128, 127]          the byte n + 128
//   I16  S 32767       [-32768, 32767]      2 bytes
//   I24  S 8388608     [-8388608, 8388607]  the low 3 bytes
//   I32  S 2147483647  [-2^31, 2^31 - 1]    4 bytes ((float)S is 2^31: clamped in float to +-2^31, then saturated)
//   F32  the bits as they are
// S is the reader's divisor, so decode(encode(.)) is the identity on what the reader gives for u8 / i16 / i24. These
// launchers add no dither: that is launch_frames_pack_pcm_dither / _gain_dither below. *clipped (device memory) grows by the number of samples with
// !(|x| <= 1) - beyond full scale or NaN, whatever the format - by one atomic per workgroup that saw any.
// The launch writes the n_frames * channels * bytes bytes of its frames and no other byte, each once and without
// reading the target: a launch for the frames in front or behind may run, or be downloaded, at the same time.
struct FramesPackPcmParams {
    const float *planar;
    uint64_t stride;
    unsigned char *target;
    uint32_t phase;  // 0 ... 3
    uint32_t channels;
    uint64_t n_frames;
    uint64_t *clipped;
};

// Peak normalisation (rc_engine_stretch_frames_norm): two device words of the engine, zeroed in front of a job.
//   peak_bits  the bits of the largest |x| among the finite samples seen so far (for non-negative floats the unsigned
//              order of the bits is the order of the values; NaN and +-inf are skipped: their bits sort above every
//              finite value). 0 where nothing finite and non-zero was seen.
//   gain       what the pack launches multiplied by, stored by the first of them for the host to read back
struct FramesNormWords {
    uint32_t peak_bits;
    float gain;
};

// planar[c * stride + i], i < n_frames, every channel c: norm->peak_bits = max(norm->peak_bits, bits of |x|) over the
// finite samples, by one atomicMax per workgroup that saw a non-zero one. A maximum does not depend on the order.
struct FramesPeakParams {
    const float *planar;
    uint64_t stride;
    uint64_t n_frames;
    uint32_t channels;
    FramesNormWords *norm;
};

// FramesPackPcmParams with a gain in front of the quantiser. Every lane forms the gain itself from the peak word:
//   peak = the float of norm->peak_bits;  gain = target_peak / peak, ONE IEEE division, where peak > 0 and the quotient
//   is finite, else 1;  z = x * gain, ONE IEEE multiplication (not contracted with the quantiser's x * S; denormals kept)
// and z takes the place of x in the encoding and in the count of clipped samples. With store_gain set, one thread of
// the first launch stores the gain to norm->gain.
struct FramesPackPcmGainParams {
    FramesPackPcmParams pack;
    FramesNormWords *norm;
    float target_peak;
    uint32_t store_gain;
};

// The dither in front of the quantiser (rc_engine_set_output_dither; the definition is stated in include/rocoder_hip.h).
// Row c of the launch is job channel channel0 + c, frame f of the launch is absolute output frame t = t0 + f, and
// keys[channel0 + c] is that channel's key K = rc_phase_key(seed, channel0 + c, 0xFFFFFFFFFF): `keys` is the JOB's device
// table, of which the launch reads the entries [channel0, channel0 + channels). With h(c, t) = rc_phase_hash(K(c), t mod 2^32):
//   mode 1 (TPDF)     i = (int)(h >> 16) - (int)(h & 0xFFFF)
//   mode 2 (TPDF_HP)  i = (int)(h(c, t) >> 16) - (int)(h(c, t - 1) >> 16)        (t - 1 mod 2^32: at t = 0 the counter 0xFFFFFFFF)
//   d = (float)i * 2^-16;  t1 = x * (float)S;  t2 = t1 + d, ONE IEEE addition, no fma;  r = rint(t2), NaN -> 0, clamped
// with S, LO, HI of FramesPackPcmParams and x behind the gain where there is one. *clipped counts on x, in front of the
// dither. U8, I16 and I24 only; any other format or mode is refused. A sample gets the d of its own (c, t) whichever
// workgroup or launch encodes it: the bytes do not depend on how a job is cut into tiles or launches.
struct FramesDitherParams {
    uint32_t mode;      // 1 or 2: RC_DITHER_TPDF, RC_DITHER_TPDF_HP
    uint32_t channel0;
    uint64_t t0;
    const uint64_t *keys;
};
struct FramesPackPcmDitherParams {
    FramesPackPcmParams pack;
    FramesDitherParams dither;
};
struct FramesPackPcmGainDitherParams {
    FramesPackPcmGainParams gain;
    FramesDitherParams dither;
};

// The output fade (rc_engine_set_output_fade; the definition is stated in include/rocoder_hip.h), in place on planar rows.
// `planar` is the sample of the first channel at absolute output frame t0; the launch covers the frames [t0, t1) of every
// channel, frame t of channel c at planar[c * stride + (t - t0)]. For each of them, with every operation ONE correctly
// rounded IEEE f32 operation and the frame counts converted to f32 with round to nearest even:
//   t < in_len                           x = x * up(t, in_len)
//   out_start <= t < out_start + out_len x = x * down(t - out_start, out_len)   (after the line above: two multiplications
//                                                                                 where the ranges overlap)
//   t >= out_start + out_len             x = +0.0f, assigned: whatever x was, NaN included; x is not read
//   up(p, d)   = sqrtf(0.5f * (1.0f + fmaxf( (p / d * 2.0f - 1.0f), -1.0f)))
//   down(p, d) = sqrtf(0.5f * (1.0f + fmaxf(-(p / d * 2.0f - 1.0f), -1.0f)))
// out_start == UINT64_MAX: no fade-out. out_start + out_len does not wrap (the engine's setter sees to it). A frame that
// none of the three lines names is written back as it was read: the host launches on the frames a fade changes, each in
// one launch only, so that every sample is read and written once.
struct FramesFadeParams {
    float *planar;
    uint64_t stride;
    uint32_t channels;
    uint64_t in_len, out_start, out_len;
    uint64_t t0, t1;
};

// The peak of every bin of a block of raw frames (rc_engine_frames_power; the definition is stated in
// include/rocoder_hip.h). The block is what FramesUnpackParams describes: raw, raw_dwords, phase, channels, and the same
// licence to load whole 16-byte groups around a range. The launch covers the job's frames [frame0, frame0 + n_frames),
// a range that may start and end inside a bin, and adds to the bins it touches only:
//   bin_bits[b] = max(bin_bits[b], bits of the largest |x| among the samples of the range in bin b), NaN skipped, +-inf
//   kept, x the reader's float of the sample; bin b holds the frames [b * bin_frames, (b + 1) * bin_frames), every channel.
// For non-negative floats the unsigned order of the bits is the order of the values, and a maximum does not depend on
// the order: workgroups and launches join a bin with atomicMax. bin_bits holds n_bins words, zeroed by the host in front
// of a job's first launch; the launcher refuses a range whose last frame lies in no bin of them.
struct FramesPowerParams {
    const uint32_t *raw;
    uint64_t raw_dwords;
    uint32_t phase;  // 0 ... 3
    uint32_t channels;
    uint64_t frame0, n_frames;
    uint64_t bin_frames;  // >= 1
    uint32_t *bin_bits;
    uint64_t n_bins;
};

// FramesUnpackParams with a channel map (rc_engine_set_channel_map): row c of planar is filled from channel map[c] of the
// block, planar[c * stride + frame0 + i] = sample (frame0 + i, map[c]). `map` is a device table of `channels` words, each
// below `channels` (the engine's setter sees to it; the kernels clamp an entry to channels - 1 rather than trust it). A
// source channel may feed several rows, or none. Every row gets every frame exactly once; nothing of the block is written.
struct FramesUnpackMapParams {
    FramesUnpackParams unpack;
    const uint32_t *map;
};

// The peak of every channel of a block of raw frames (rc_engine_frames_channel_peaks; the definition is stated in
// include/rocoder_hip.h). The block is what FramesUnpackParams describes, with the same licence to load whole 16-byte
// groups around a range. The launch covers the job's frames [frame0, frame0 + n_frames) and adds to every channel:
//   chan_bits[c] = max(chan_bits[c], bits of |x| with the sign bit cleared) over the range's samples of channel c, in the
//   unsigned order of the bits: a NaN wins over +inf, +inf over every finite magnitude; x the reader's float of the sample.
// Workgroups and launches join a channel with atomicMax, one per channel per workgroup that saw a non-zero sample.
// chan_bits holds `channels` words, zeroed by the host in front of a job's first launch.
struct FramesChannelPeaksParams {
    const uint32_t *raw;
    uint64_t raw_dwords;
    uint32_t phase;  // 0 ... 3
    uint32_t channels;
    uint64_t frame0, n_frames;
    uint32_t *chan_bits;
};

// Band-limited resampling of planar rows by the step num/den input frames per output frame (rc_engine_set_output_resample;
// the definition is stated in include/rocoder_hip.h; not the reference's `-p < 0` interpolation, which is ResampleParams /
// launch_resample_slower of rc_kernels.h). x[c][k] is the job's row c, k in [0, n), zero outside. For output frame m, in
// 64-bit integers: q = m * num / den, p = (m * num) mod den, k0 = q - (W - 1), and
//   y[c][m] = sum over j < 2 W of table[p * 2 W + j] * x[c][k0 + j]
// as ONE chain acc = fmaf(table[..j], x[k0 + j], acc) from acc = +0 with j ascending: a sample's bits do not depend on
// the tile, the launch or the range that computed it. `src` is the sample of the first channel at absolute input frame
// src0, of which src_len frames are readable per row (rows `stride` floats apart); `dst` the sample of the first channel
// at output frame m0 (rows dst_stride apart). The launch writes the frames [m0, m1) of every channel and nothing else.
// `table` is the device copy of rc_resample_table's den x 2 W floats (8-byte aligned), num/den reduced, W <= 256.
// The launcher refuses (hipErrorInvalidValue, nothing launched) a range one of whose taps lies inside [0, n) but outside
// [src0, src0 + src_len). Nothing is launched for m1 <= m0; more than 2^27 outputs go out as several launches.
struct FramesResampleParams {
    const float *src;
    uint64_t src0, src_len;
    uint64_t stride;
    uint32_t channels;
    uint64_t n;
    const float *table;
    uint32_t num, den, W;
    float *dst;
    uint64_t dst_stride;
    uint64_t m0, m1;
};

// The look-ahead peak limiter (rc_engine_set_output_limiter; the definition is stated in include/rocoder_hip.h), from planar
// rows to planar rows. x[c][t] is the job's row c, t in [0, n). With L the look-ahead, T = 2 L + 1, ONE = 2^24, every float
// step ONE correctly rounded IEEE f32 operation:
//   v = x * drive;  a[t] = the largest |v[c][t]| < inf over the channels (NaN, +-inf skipped; 0 where none);
//   r[t] = ceiling / a[t] where a[t] > ceiling, else 1;  rq[t] = (uint32_t)(r[t] * 2^24), ONE outside [0, n);
//   m[u] = min rq[t], |t - u| <= L;  S[t] = sum m[u], |u - t| <= L, in 64 bits;  g[t] = (float)S[t] / (float)(T * ONE);
//   y = v * g[t], clamped to [-ceiling, ceiling], a NaN kept.
// m and S are integers: a frame's g does not depend on the tile, the launch or the range that computed it. `src` is the
// sample of the first channel at absolute frame src0, of which src_len frames are readable per row (rows `stride` floats
// apart); `dst` the sample of the first channel at frame t0 (rows dst_stride apart). The launch writes the frames [t0, t1) of
// every channel of dst and nothing else; the halo of rq it needs, the frames [t0 - 2 L, t1 + 2 L), it recomputes from src.
// The launcher refuses (hipErrorInvalidValue, nothing launched) a range that needs a frame inside [0, n) but outside
// [src0, src0 + src_len). Nothing is launched for t1 <= t0; more than 2^27 frames go out as several launches.
// `scratch` / scratch_words: device words a launch may use between its passes. The fused kernel of rc_frames_limit.hip keeps
// rq, m and the prefix sums in LDS and needs none (frames_limit_scratch_words gives 0): null / 0 are accepted.
// stats: two device words of the engine, reset by the host in front of a job to {the bits of 1.0f, 0}:
//   min_gain_bits  the bits of the smallest g[t] so far, joined with atomicMin (g >= 0: the unsigned order of the bits is
//                  the order of the values), one per workgroup that saw a g below 1
//   limited        the number of frames with S[t] < T * ONE, one atomicAdd per workgroup that saw any. A frame is computed
//                  by exactly one launch.
struct FramesLimitWords {
    uint32_t min_gain_bits;
    uint32_t reserved;
    uint64_t limited;
};
constexpr uint32_t kLimitMaxLookahead = 2048;  // RC_LIMITER_MAX_LOOKAHEAD
struct FramesLimitParams {
    const float *src;
    uint64_t src0, src_len;
    uint64_t stride;
    uint32_t channels;
    uint64_t n;
    float drive, ceiling;
    uint32_t L;
    float *dst;
    uint64_t dst_stride;
    uint64_t t0, t1;
    uint32_t *scratch;
    uint64_t scratch_words;
    FramesLimitWords *stats;
};

// The two measurements of rc_engine_stretch_frames_loud (the definition is stated in include/rocoder_hip.h), on the finished
// planar rows of a job: y[c][t] at planar[c * stride + t], t in [0, n). Both read the rows and write nothing to them.
//
// K-weighted sub-block energies (rc_frames_loud.hip). The two biquads of BS.1770 as ONE linear system of four states in
// direct form II transposed, run in f64 on the device (the high-pass's poles lie 3e-4 from the unit circle at 768 kHz: an
// f32 recurrence loses what the gate is held to):
//   y1 = b0 x + s1;  s1' = b1 x - a1 y1 + s2;  s2' = b2 x - a2 y1          stage 1, coef[0 ... 4] = b0 b1 b2 a1 a2
//   y2 = c0 y1 + u1; u1' = c1 y1 - d1 y2 + u2; u2' = c2 y1 - d2 y2         stage 2, coef[5 ... 9] = c0 c1 c2 d1 d2
// step[k], k < 8, is A^(kLoudRun * 2^k), row-major 4 x 4 over (s1, s2, u1, u2), A the system's state-transition matrix:
// what 16, 32, ... 2048 frames of silence do to a state. The host forms them in f64 (frames_loud_energy_steps).
//   energy[c * e_stride + j] = (float)(sum of k[c][t]^2 over t in [j * sub, (j + 1) * sub)), j < nb, nb * sub <= n
// with k the f64 recurrence started from a zero state at frame max(0, (j0 - kLoudWarm) * sub), j0 the first sub-block of
// the workgroup's span (frames_loud_span sub-blocks): from frame 0 that is the definition itself, later it differs from it
// by what the filter has not forgotten in kLoudWarm sub-blocks (200 ms), a relative 1.6e-12 of a sub-block's energy. Every
// word is written once, by one workgroup, from sums of a fixed order: no atomics, and the span depends on (channels, nb)
// alone, so two launches on the same rows give the same words. The launcher refuses (hipErrorInvalidValue, nothing
// launched) sub < kLoudMinSub, nb * sub > n, e_stride < nb. Nothing is launched for nb == 0.
constexpr uint32_t kLoudRun = 16;       // frames of a lane's run
constexpr uint32_t kLoudWarm = 2;       // sub-blocks of warm-up in front of a span
constexpr uint32_t kLoudMinSub = 800;   // the sub-block of 8 kHz, the lowest rate of rc_engine_stretch_frames_loud
struct FramesLoudEnergyParams {
    const float *planar;
    uint64_t stride;
    uint64_t n;
    uint32_t channels;
    uint32_t sub;  // frames of a sub-block
    uint64_t nb;   // sub-blocks measured
    float *energy;
    uint64_t e_stride;
    double coef[10];
    double step[8][16];
};
// sub-blocks of a workgroup's span: enough workgroups to fill the device on a short job, little warm-up on a long one
inline uint32_t frames_loud_span(uint32_t channels, uint64_t nb) {
    const uint64_t s = (uint64_t)channels * nb / 2048u;
    return (uint32_t)(s < 4u ? 4u : s > 32u ? 32u : s);
}
// the ten f64 coefficients at the rate R, as include/rocoder_hip.h states them (rc_loudness_coeffs rounds these); host code
inline void frames_loud_coeffs(uint32_t R, double coef[10]) {
    const double kPi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(kPi * f0 / (double)R), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        coef[0] = (Vh + Vb * K / Q + K * K) / a0;
        coef[1] = 2.0 * (K * K - Vh) / a0;
        coef[2] = (Vh - Vb * K / Q + K * K) / a0;
        coef[3] = 2.0 * (K * K - 1.0) / a0;
        coef[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(kPi * f0 / (double)R), a0 = 1.0 + K / Q + K * K;
        coef[5] = 1.0;
        coef[6] = -2.0;
        coef[7] = 1.0;
        coef[8] = 2.0 * (K * K - 1.0) / a0;
        coef[9] = (1.0 - K / Q + K * K) / a0;
    }
}
// coef and step of a params block from the ten f64 coefficients (b0 b1 b2 a1 a2 of stage 1, then of stage 2); host code.
// With x = 0: s1' = -a1 s1 + s2; s2' = -a2 s1; u1' = (c1 - d1 c0) s1 - d1 u1 + u2; u2' = (c2 - d2 c0) s1 - d2 u1.
inline void frames_loud_energy_steps(const double coef[10], FramesLoudEnergyParams *p) {
    static_assert(kLoudRun == 16, "A^kLoudRun below is four squarings");
    const double a1 = coef[3], a2 = coef[4], c0 = coef[5], c1 = coef[6], c2 = coef[7], d1 = coef[8], d2 = coef[9];
    double m[16] = {-a1, 1, 0, 0, -a2, 0, 0, 0, c1 - d1 * c0, 0, -d1, 1, c2 - d2 * c0, 0, -d2, 0};
    auto square = [](double *a) {
        double r[16];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) r[4 * i + j] = a[4 * i] * a[j] + a[4 * i + 1] * a[4 + j] + a[4 * i + 2] * a[8 + j] + a[4 * i + 3] * a[12 + j];
        for (int i = 0; i < 16; ++i) a[i] = r[i];
    };
    for (int i = 0; i < 10; ++i) p->coef[i] = coef[i];
    for (int k = 0; k < 4; ++k) square(m);
    for (int k = 0; k < 8; ++k) {
        for (int i = 0; i < 16; ++i) p->step[k][i] = m[i];
        square(m);
    }
}

// True peak (rc_frames_loud.hip): the 4 x oversampled rows are what FramesResampleParams defines for num / den = 1 / 4 -
// u[c][m] = one chain acc = fmaf(table[(m % 4) * 64 + j], y[c][m / 4 - 31 + j], acc) from +0, j = 0 ... 63, y zero outside
// [0, n) - and are never stored:
//   norm->peak_bits = max(norm->peak_bits, bits of |v|) over every y[c][t] and u[c][m] with |v| < inf
// by one atomicMax per workgroup that saw a non-zero one. A maximum of order-fixed chains is order-free: bit for bit.
// `table`: the device copy of rc_resample_table(1, 4)'s 4 x 64 floats.
struct FramesTruePeakParams {
    const float *planar;
    uint64_t stride;
    uint64_t n;
    uint32_t channels;
    const float *table;
    FramesNormWords *norm;
};

// The mix launch (rc_engine_mix_frames; the definition is stated in include/rocoder_hip_mix.h), from a layer's planar rows
// into the bus rows. `rows` is the sample of the layer's first channel at layer frame t0 (rows `stride` floats apart,
// `channels` = CL of them); the launch covers the layer frames [t0, t1). `bus` is frame 0 of the first bus row (16-byte
// aligned; rows bus_stride floats apart, a multiple of 4; bus_channels = CB rows of bus_frames = N frames). For every t of
// the range with 0 <= u = offset + t < N and every cb:
//   bus[cb][u] = bus[cb][u] + s[cb][t] * amp(t)      one multiplication, then one addition, never one fma
//   s[cb][t]   = x[cb][t] where send is null (CL == CB), else ONE chain acc = fmaf(send[cb * CL + cl], x[cl][t], acc) from +0
//   amp(t)     = the envelope of the keys (key_frame, key_amp: device tables of n_keys entries) on the layer's clock
// and no other word of the bus is read or written; frames that fall outside the bus are dropped, and nothing is launched
// for a range that falls wholly outside. A sample's bits do not depend on the launch, the tile or the range. The launcher
// refuses (hipErrorInvalidValue, nothing launched) t1 < t0, n_keys > kMixMaxKeys, and with a non-empty range a null
// pointer (send may be null), a null send with CL != CB, a bus that is not aligned as stated, |offset|, t1 or N above 2^62.
constexpr uint32_t kMixMaxKeys = 4096;  // RC_MIX_MAX_KEYS
struct FramesMixParams {
    const float *rows;
    uint64_t stride;
    uint32_t channels;
    uint64_t t0, t1;
    float *bus;
    uint64_t bus_stride;
    uint32_t bus_channels;
    uint64_t bus_frames;
    int64_t offset;
    const uint64_t *key_frame;
    const float *key_amp;
    uint32_t n_keys;
    const float *send;
};
// nullptr where the keys are what rc_engine_mix_frames accepts, else what is wrong with them (rc_mix_envelope.cpp; host code)
const char *mix_check_keys(const uint64_t *key_frame, const float *key_amp, size_t n_keys);

// (all: nothing is launched for n_frames == 0; a job of more than 2^27 frames goes out as several launches)
hipError_t launch_frames_unpack(uint32_t format, const FramesUnpackParams &p, hipStream_t s);
hipError_t launch_frames_pack(const FramesPackParams &p, hipStream_t s);
hipError_t launch_frames_pack_pcm(uint32_t format, const FramesPackPcmParams &p, hipStream_t s);
hipError_t launch_frames_peak(const FramesPeakParams &p, hipStream_t s);
hipError_t launch_frames_pack_pcm_gain(uint32_t format, const FramesPackPcmGainParams &p, hipStream_t s);
hipError_t launch_frames_pack_pcm_dither(uint32_t format, const FramesPackPcmDitherParams &p, hipStream_t s);
hipError_t launch_frames_pack_pcm_gain_dither(uint32_t format, const FramesPackPcmGainDitherParams &p, hipStream_t s);
hipError_t launch_frames_fade(const FramesFadeParams &p, hipStream_t s);  // (nothing is launched for t1 <= t0)
hipError_t launch_frames_power(uint32_t format, const FramesPowerParams &p, hipStream_t s);
hipError_t launch_frames_unpack_map(uint32_t format, const FramesUnpackMapParams &p, hipStream_t s);
hipError_t launch_frames_channel_peaks(uint32_t format, const FramesChannelPeaksParams &p, hipStream_t s);
hipError_t launch_frames_resample(const FramesResampleParams &p, hipStream_t s);  // (rc_frames_resample.hip)
hipError_t launch_frames_limit(const FramesLimitParams &p, hipStream_t s);        // (rc_frames_limit.hip)
inline uint64_t frames_limit_scratch_words(uint64_t /*frames*/, uint32_t /*L*/) { return 0; }
hipError_t launch_frames_loud_energy(const FramesLoudEnergyParams &p, hipStream_t s);  // (rc_frames_loud.hip)
hipError_t launch_frames_true_peak(const FramesTruePeakParams &p, hipStream_t s);      // (rc_frames_loud.hip)
hipError_t launch_frames_mix(const FramesMixParams &p, hipStream_t s);                 // (rc_frames_mix.hip; one launch whatever the range)

}  // namespace rc
