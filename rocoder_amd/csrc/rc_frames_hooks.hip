// Test-hook entries for the launchers of rc_frames.h: compiled into librocoder_hip_hooks.so only (`make hooks`), never
// into the product library. One wrapper per launcher: the fields of its parameter block as plain scalars and device
// pointers, a launch on the null stream, a synchronise, the hipError_t as an int. No logic, no clamping, no defaults and
// no allocation: what a launcher does with a set of arguments is what the test sees (tests/frameskernelutil.py sizes
// every buffer and asserts the sizes before a call).
#include "rc_frames.h"

namespace {
int finish(hipError_t err) { return (int)(err != hipSuccess ? err : hipStreamSynchronize(nullptr)); }
}  // namespace

extern "C" {

int rc_test_frames_unpack(uint32_t format, const uint32_t *raw, uint64_t raw_dwords, uint32_t phase, uint32_t channels,
                          uint64_t frame0, uint64_t n_frames, float *planar, uint64_t stride) {
    return finish(rc::launch_frames_unpack(format, rc::FramesUnpackParams{raw, raw_dwords, phase, channels, frame0, n_frames, planar, stride},
                                           nullptr));
}

int rc_test_frames_unpack_map(uint32_t format, const uint32_t *raw, uint64_t raw_dwords, uint32_t phase, uint32_t channels,
                              uint64_t frame0, uint64_t n_frames, float *planar, uint64_t stride, const uint32_t *map) {
    return finish(rc::launch_frames_unpack_map(
        format, rc::FramesUnpackMapParams{rc::FramesUnpackParams{raw, raw_dwords, phase, channels, frame0, n_frames, planar, stride}, map},
        nullptr));
}

int rc_test_frames_pack(const float *planar, uint64_t stride, float *frames, uint64_t n_frames, uint32_t channels) {
    return finish(rc::launch_frames_pack(rc::FramesPackParams{planar, stride, frames, n_frames, channels}, nullptr));
}

int rc_test_frames_pack_pcm(uint32_t format, const float *planar, uint64_t stride, unsigned char *target, uint32_t phase,
                            uint32_t channels, uint64_t n_frames, uint64_t *clipped) {
    return finish(rc::launch_frames_pack_pcm(format, rc::FramesPackPcmParams{planar, stride, target, phase, channels, n_frames, clipped},
                                             nullptr));
}

int rc_test_frames_pack_pcm_gain(uint32_t format, const float *planar, uint64_t stride, unsigned char *target, uint32_t phase,
                                 uint32_t channels, uint64_t n_frames, uint64_t *clipped, rc::FramesNormWords *norm,
                                 float target_peak, uint32_t store_gain) {
    return finish(rc::launch_frames_pack_pcm_gain(
        format,
        rc::FramesPackPcmGainParams{rc::FramesPackPcmParams{planar, stride, target, phase, channels, n_frames, clipped}, norm, target_peak,
                                    store_gain},
        nullptr));
}

// (norm null: launch_frames_pack_pcm_dither; else launch_frames_pack_pcm_gain_dither)
int rc_test_frames_pack_pcm_dither(uint32_t format, const float *planar, uint64_t stride, unsigned char *target, uint32_t phase,
                                   uint32_t channels, uint64_t n_frames, uint64_t *clipped, rc::FramesNormWords *norm, float target_peak,
                                   uint32_t store_gain, uint32_t mode, uint64_t t0, uint32_t channel0, const uint64_t *keys) {
    const rc::FramesPackPcmParams pk{planar, stride, target, phase, channels, n_frames, clipped};
    const rc::FramesDitherParams di{mode, channel0, t0, keys};
    return finish(norm ? rc::launch_frames_pack_pcm_gain_dither(
                             format, rc::FramesPackPcmGainDitherParams{rc::FramesPackPcmGainParams{pk, norm, target_peak, store_gain}, di}, nullptr)
                       : rc::launch_frames_pack_pcm_dither(format, rc::FramesPackPcmDitherParams{pk, di}, nullptr));
}

int rc_test_frames_peak(const float *planar, uint64_t stride, uint64_t n_frames, uint32_t channels, rc::FramesNormWords *norm) {
    return finish(rc::launch_frames_peak(rc::FramesPeakParams{planar, stride, n_frames, channels, norm}, nullptr));
}

int rc_test_frames_fade(float *planar, uint64_t stride, uint32_t channels, uint64_t in_len, uint64_t out_start, uint64_t out_len,
                        uint64_t t0, uint64_t t1) {
    return finish(rc::launch_frames_fade(rc::FramesFadeParams{planar, stride, channels, in_len, out_start, out_len, t0, t1}, nullptr));
}

int rc_test_frames_resample(const float *src, uint64_t src0, uint64_t src_len, uint64_t stride, uint32_t channels, uint64_t n,
                            const float *table, uint32_t num, uint32_t den, uint32_t W, float *dst, uint64_t dst_stride, uint64_t m0,
                            uint64_t m1) {
    return finish(rc::launch_frames_resample(
        rc::FramesResampleParams{src, src0, src_len, stride, channels, n, table, num, den, W, dst, dst_stride, m0, m1}, nullptr));
}

int rc_test_frames_limit(const float *src, uint64_t src0, uint64_t src_len, uint64_t stride, uint32_t channels, uint64_t n, float drive,
                         float ceiling, uint32_t L, float *dst, uint64_t dst_stride, uint64_t t0, uint64_t t1, uint32_t *scratch,
                         uint64_t scratch_words, rc::FramesLimitWords *stats) {
    return finish(rc::launch_frames_limit(
        rc::FramesLimitParams{src, src0, src_len, stride, channels, n, drive, ceiling, L, dst, dst_stride, t0, t1, scratch, scratch_words, stats},
        nullptr));
}

// (the coefficients and the matrix powers of sample_rate, as the engine forms them: frames_loud_coeffs / _energy_steps)
int rc_test_frames_kweight_energy(const float *planar, uint64_t stride, uint64_t n, uint32_t channels, uint32_t sample_rate, uint32_t sub,
                                  uint64_t nb, float *energy, uint64_t e_stride) {
    rc::FramesLoudEnergyParams p{planar, stride, n, channels, sub, nb, energy, e_stride, {}, {}};
    double coef[10];
    rc::frames_loud_coeffs(sample_rate, coef);
    rc::frames_loud_energy_steps(coef, &p);
    return finish(rc::launch_frames_loud_energy(p, nullptr));
}

uint32_t rc_test_frames_loud_span(uint32_t channels, uint64_t nb) { return rc::frames_loud_span(channels, nb); }

int rc_test_frames_true_peak(const float *planar, uint64_t stride, uint64_t n, uint32_t channels, const float *table,
                             rc::FramesNormWords *norm) {
    return finish(rc::launch_frames_true_peak(rc::FramesTruePeakParams{planar, stride, n, channels, table, norm}, nullptr));
}

}  // extern "C"
