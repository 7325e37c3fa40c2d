// TEST INFRASTRUCTURE: rc_engine_stretch_frames_loud and its host helpers over the HIP stub (tests/c/hip_stub.cpp: device
// memory is host memory, the hop kernels compute nothing; tests/c/hip_stub_frames_loud.cpp: the two measuring launchers read
// what the real ones read and give fixed answers; tests/c/hip_stub_frames_norm.cpp: the pack launcher forms and stores the
// gain from the peak word) under ASan + UBSan (rocoder_amd/csrc/host/sanitize.mk: engine_frames_loud_asan). What runs for
// real is the host side of the entry: phase 1 without a peak launch, the middle - which rows are measured, the readback of
// channels x nb words and the peak word, the gate, the gain, the 1.0f written over the peak word - phase 2's pack ranges and
// downloads, and the error paths. The output buffer is exactly as long as the call says; every byte of it is checked.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/rocoder_hip.h"

struct RcStubLoudLaunch {
    uint64_t n, nb, stride, e_stride;
    uint32_t sub, channels;
    float first;
    double coef0, step_last;
};
extern RcStubLoudLaunch rc_stub_loud_energy_log[16], rc_stub_loud_peak_log[16];  // tests/c/hip_stub_frames_loud.cpp
extern uint32_t rc_stub_loud_energy_launches, rc_stub_loud_peak_launches;
extern uint64_t rc_stub_loud_energy_frames, rc_stub_loud_peak_frames;
extern float rc_stub_loud_level, rc_stub_loud_peak;
extern uint64_t rc_stub_peak_samples, rc_stub_gain_stores;  // tests/c/hip_stub_frames_norm.cpp
extern float rc_stub_limit_mark, rc_stub_resample_mark;     // tests/c/hip_stub_frames_limit.cpp, hip_stub_frames_resample.cpp

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rc_last_error()); \
            exit(2);                                                             \
        }                                                                        \
    } while (0)

static rc_config config(uint32_t N, float f, uint32_t ch, uint32_t rate) {
    rc_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.window_len = N;
    c.factor = f;
    c.amplitude = 1.0f;
    c.pitch_multiple = 1;
    c.sample_rate = rate;
    c.channels = ch;
    c.buffer_secs = 1.0f;
    c.seed = 7;
    return c;
}

static int ok_kernel(uint64_t, const float *in, float *out, size_t n, void *) {
    memcpy(out, in, n * 2 * sizeof(float));
    return 0;
}

static uint32_t bytes_of(uint32_t format) { return format == RC_PCM_U8 ? 1 : format == RC_PCM_I16 ? 2 : format == RC_PCM_I24 ? 3 : 4; }

// the header's gain from the reported values
static float gain_of(float lufs, float tp, float target, float ceiling) {
    const float gl = std::isinf(lufs) ? 1.0f : (float)pow(10.0, ((double)target - (double)lufs) / 20.0);
    const float gc = ceiling > 0.0f && tp > 0.0f ? ceiling / tp : INFINITY;
    const float g = gl < gc ? gl : gc;
    return std::isfinite(g) && g > 0.0f ? g : 1.0f;
}

enum { PLAIN, LIMITER, RESAMPLE, BOTH };

// one job: i16 frames in, `out_format` out, at the engine's rate (sample_rate 0) or an explicit one
static void job(uint32_t N, float f, uint32_t ch, uint32_t out_format, size_t L, size_t misalign, uint32_t cfg_rate, uint32_t rate, int state = PLAIN,
                bool host_kernel = false) {
    rc_config c = config(N, f, ch, cfg_rate);
    if (host_kernel) {
        c.kernel = ok_kernel;
        c.kernel_time_ms = 1;
    }
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&c, &e) == RC_OK);
    if (state == LIMITER || state == BOTH) CHECK(rc_engine_set_output_limiter(e, 1.0f, 0.9f, 32) == RC_OK);
    if (state == RESAMPLE || state == BOTH) CHECK(rc_engine_set_output_resample(e, 160, 147) == RC_OK);
    const uint32_t OB = bytes_of(out_format), R = rate ? rate : cfg_rate, sub = (R + 5) / 10;
    const size_t n_rows = rc_offline_output_len(&c, L), n_out = state == RESAMPLE || state == BOTH ? rc_resample_len(n_rows, 160, 147) : n_rows;
    const size_t out_bytes = n_out * ch * OB, nb = n_out / sub;
    CHECK(rc_loudness_sub_blocks(n_out, R) == nb);
    int16_t *in = (int16_t *)calloc(L * ch + 1, sizeof(int16_t));
    unsigned char *block = (unsigned char *)malloc(out_bytes + misalign);
    CHECK(in != nullptr && block != nullptr);
    unsigned char *out = block + misalign;
    const float want_lufs = nb >= 4 ? (float)(-0.691 + 10.0 * log10((double)ch * (double)rc_stub_loud_level)) : -INFINITY;
    const float want_tp = n_out ? rc_stub_loud_peak : 0.0f;
    for (int rep = 0; rep < 3; ++rep) {  // the later calls find the engine's buffers reserved; the last one has a ceiling that binds
        const float target = rep == 2 ? 20.0f : -23.0f, ceiling = rep == 2 ? 0.125f : 0.0f;
        memset(block, 0x11, out_bytes + misalign);
        size_t got = 0;
        uint64_t clipped = 99;
        float lufs = 1.0f, tp = -1.0f, gain = -1.0f;
        rc_stub_peak_samples = rc_stub_gain_stores = 0;
        rc_stub_loud_energy_launches = rc_stub_loud_peak_launches = 0;
        rc_stub_loud_energy_frames = rc_stub_loud_peak_frames = 0;
        CHECK(rc_engine_stretch_frames_loud(e, in, L, RC_PCM_I16, out, n_out, out_format, rate, target, ceiling, &got, &lufs, &tp, &gain, &clipped) ==
                  RC_OK && got == n_out);
        // no launch of the normaliser's peak kernel; each measurement once, over the whole finished rows, whichever they are
        CHECK(rc_stub_peak_samples == 0 && rc_stub_gain_stores == (n_out ? 1u : 0u));
        CHECK(rc_stub_loud_energy_launches == (nb ? 1u : 0u) && rc_stub_loud_peak_launches == (n_out ? 1u : 0u));
        CHECK(rc_stub_loud_energy_frames == (uint64_t)nb * sub * ch && rc_stub_loud_peak_frames == (uint64_t)n_out * ch);
        if (nb) {
            const RcStubLoudLaunch &l = rc_stub_loud_energy_log[0];
            float cf[10];
            CHECK(rc_loudness_coeffs(R, cf) == RC_OK);
            CHECK(l.n == n_out && l.nb == nb && l.sub == sub && l.channels == ch && l.stride >= n_out && l.e_stride >= nb && (float)l.coef0 == cf[0]);
            CHECK(std::isfinite(l.step_last) && fabs(l.step_last) < 1.0);  // 2048 frames of silence shrink a state
        }
        if (n_out) {
            const RcStubLoudLaunch &l = rc_stub_loud_peak_log[0];
            const float mark = state == LIMITER || state == BOTH ? rc_stub_limit_mark : state == RESAMPLE ? rc_stub_resample_mark : 0.0f;
            CHECK(l.n == n_out && l.channels == ch && l.stride >= n_out && l.first == mark);
            if (nb) CHECK(rc_stub_loud_energy_log[0].first == mark);
        }
        CHECK(lufs == want_lufs && tp == want_tp && gain == gain_of(lufs, tp, target, ceiling) && clipped == 0);
        if (rep == 2 && n_out) CHECK(gain == 0.125f / 0.5f);
        for (size_t i = 0; i < misalign; ++i) CHECK(block[i] == 0x11);
        for (size_t i = 0; i < out_bytes; ++i) {
            const size_t s = i / OB;
            if (out[i] != (unsigned char)(0x80u | (((s % ch) & 7u) << 2) | (i % OB))) {
                fprintf(stderr, "FAIL: byte %zu of %zu is %02x (format %u, %u channels, misalign %zu)\n", i, out_bytes, out[i], out_format, ch, misalign);
                exit(2);
            }
        }
    }
    // the entries around it on the same engine: the new middle leaves nothing behind
    {
        memset(block, 0x11, out_bytes + misalign);
        uint64_t clipped = 99;
        float peak = -1.0f, gain = -1.0f;
        CHECK(rc_engine_stretch_frames_pcm(e, in, L, RC_PCM_I16, out, n_out, out_format, nullptr, &clipped) == RC_OK && clipped == 0);
        for (size_t i = 0; i < out_bytes; ++i) CHECK(out[i] == (unsigned char)(0x80u | ((((i / OB) % ch) & 7u) << 2) | (i % OB)));
        rc_stub_peak_samples = rc_stub_gain_stores = 0;
        CHECK(rc_engine_stretch_frames_norm(e, in, L, RC_PCM_I16, out, n_out, out_format, 0.5f, nullptr, &peak, &gain, &clipped) == RC_OK);
        CHECK(rc_stub_peak_samples == (uint64_t)n_out * ch && (n_out == 0 || peak >= (float)(1 + (uint64_t)n_out * ch)));
    }
    CHECK(rc_engine_stretch_frames_loud(e, in, L, RC_PCM_I16, out, n_out, out_format, rate, -14.0f, 1.0f, nullptr, nullptr, nullptr, nullptr, nullptr) == RC_OK);
    CHECK(rc_engine_stretch_frames_loud(e, nullptr, L, RC_PCM_I16, out, n_out, out_format, rate, -14.0f, 1.0f, nullptr, nullptr, nullptr, nullptr, nullptr) ==
          (L ? RC_EINVAL : RC_OK));
    size_t got = 7;
    uint64_t clipped = 5;
    float lufs = 2.0f, tp = 3.0f, gain = 4.0f;
    memset(block, 0x11, out_bytes + misalign);
#define LOUD(fmt_in, dst, cap, fmt_out, r, target, ceil) \
    rc_engine_stretch_frames_loud(e, in, L, fmt_in, dst, cap, fmt_out, r, target, ceil, &got, &lufs, &tp, &gain, &clipped)
    if (n_out) CHECK(LOUD(RC_PCM_I16, out, n_out - 1, out_format, rate, -23.0f, 0.0f) == RC_ECAPACITY);
    for (float bad : {(float)NAN, (float)INFINITY, -(float)INFINITY}) CHECK(LOUD(RC_PCM_I16, out, n_out, out_format, rate, bad, 0.0f) == RC_EINVAL);
    for (float bad : {(float)NAN, -1.0f, -(float)INFINITY}) CHECK(LOUD(RC_PCM_I16, out, n_out, out_format, rate, -23.0f, bad) == RC_EINVAL);
    for (uint32_t bad : {1u, 7999u, 768001u, 0xFFFFFFFFu}) CHECK(LOUD(RC_PCM_I16, out, n_out, out_format, bad, -23.0f, 0.0f) == RC_EINVAL);
    CHECK(LOUD(0, out, n_out, out_format, rate, -23.0f, 0.0f) == RC_EINVAL);
    CHECK(LOUD(6, out, n_out, out_format, rate, -23.0f, 0.0f) == RC_EINVAL);
    CHECK(LOUD(RC_PCM_I16, out, n_out, 0, rate, -23.0f, 0.0f) == RC_EINVAL);
    CHECK(LOUD(RC_PCM_I16, out, n_out, 6, rate, -23.0f, 0.0f) == RC_EINVAL);
    CHECK(LOUD(RC_PCM_I16, nullptr, n_out, out_format, rate, -23.0f, 0.0f) == RC_EINVAL);
    CHECK(rc_engine_stretch_frames_loud(nullptr, in, L, RC_PCM_I16, out, n_out, out_format, rate, -23.0f, 0.0f, &got, &lufs, &tp, &gain, &clipped) == RC_EINVAL);
    CHECK(LOUD(RC_PCM_I16, out, n_out, out_format, rate, -23.0f, (float)INFINITY) == RC_OK);  // (+inf: a ceiling that never binds)
    CHECK(got == n_out && gain == gain_of(lufs, tp, -23.0f, INFINITY));
    got = 7, clipped = 5, lufs = 2.0f, tp = 3.0f, gain = 4.0f;
    memset(block, 0x11, out_bytes + misalign);
    CHECK(LOUD(RC_PCM_I16, out, n_out, out_format, 5, -23.0f, 0.0f) == RC_EINVAL);
    // on any error nothing behind the out-pointers was written
    CHECK(got == 7 && clipped == 5 && lufs == 2.0f && tp == 3.0f && gain == 4.0f);
    for (size_t i = 0; i < out_bytes + misalign; ++i) CHECK(block[i] == 0x11);
    free(block);
    free(in);
    rc_engine_destroy(e);
}

// the host helpers, with no engine: exact-size buffers under ASan
static void helpers() {
    float cf[10];
    CHECK(rc_loudness_coeffs(48000, cf) == RC_OK && cf[5] == 1.0f && cf[6] == -2.0f && cf[7] == 1.0f && fabsf(cf[0] - 1.5351249f) < 1e-6f);
    CHECK(rc_loudness_coeffs(48000, nullptr) == RC_EINVAL && rc_loudness_coeffs(7999, cf) == RC_EINVAL && rc_loudness_coeffs(768001, cf) == RC_EINVAL);
    CHECK(rc_loudness_sub_blocks(4799, 48000) == 0 && rc_loudness_sub_blocks(4800, 48000) == 1 && rc_loudness_sub_blocks(100, 0) == 0);
    for (size_t nb : {(size_t)0, (size_t)3, (size_t)4, (size_t)5, (size_t)1000}) {
        for (uint32_t ch : {1u, 3u}) {
            const size_t stride = nb + 2;
            std::vector<float> e(nb ? (ch - 1) * stride + nb : 0);  // exactly the words the call may read
            for (uint32_t c = 0; c < ch; ++c)
                for (size_t j = 0; j < nb; ++j) e[c * stride + j] = 800.0f * (j % 7 == 0 ? 1e-9f : 0.01f * (float)(1 + j % 3));
            float lufs = 5.0f;
            CHECK(rc_loudness_integrated(nb ? e.data() : nullptr, ch, nb, stride, 8000, &lufs) == RC_OK);
            CHECK(nb < 4 ? lufs == -INFINITY : (std::isfinite(lufs) && lufs < 0.0f && lufs > -30.0f));
            float keep = 5.0f;
            CHECK(rc_loudness_integrated(e.data(), 0, nb, stride, 8000, &keep) == RC_EINVAL);
            CHECK(rc_loudness_integrated(e.data(), ch, nb, stride, 7000, &keep) == RC_EINVAL);
            CHECK(rc_loudness_integrated(e.data(), ch, nb + 3, stride, 8000, &keep) == RC_EINVAL);  // stride < n_sub
            CHECK(rc_loudness_integrated(e.data(), ch, nb, stride, 8000, nullptr) == RC_EINVAL && keep == 5.0f);
        }
    }
    // silence and a programme below the absolute gate: -inf
    std::vector<float> z(40, 0.0f), q(40, 800.0f * 1e-8f);
    float lufs = 0.0f;
    CHECK(rc_loudness_integrated(z.data(), 2, 20, 20, 8000, &lufs) == RC_OK && lufs == -INFINITY);
    CHECK(rc_loudness_integrated(q.data(), 1, 40, 40, 8000, &lufs) == RC_OK && lufs == -INFINITY);
}

int main() {
    helpers();
    // several pipeline chunks (9.6 M output samples per channel, 4 M per staging slot), 9-byte frames off a dword
    job(1024, 8.0f, 3, RC_PCM_I24, 1200001, 1, 44100, 0);
    job(1024, 8.0f, 3, RC_PCM_I24, 1200001, 3, 44100, 48000, BOTH);
    job(1024, 2.0f, 1, RC_PCM_U8, 30001, 3, 8000, 0);
    job(1024, 2.0f, 2, RC_PCM_I16, 30001, 1, 44100, 8000, LIMITER);
    job(1024, 2.0f, 2, RC_PCM_I16, 30001, 0, 44100, 8000, RESAMPLE);
    job(1024, 2.0f, 5, RC_PCM_I32, 30001, 2, 48000, 0);
    job(1024, 2.0f, 2, RC_PCM_F32, 30001, 1, 44100, 768000);  // 60002 frames at 768 kHz: no whole sub-block
    job(256, 2.0f, 67, RC_PCM_I24, 3000, 1, 8000, 0);      // beyond the frames-only tile
    job(1024, 2.0f, 2, RC_PCM_I16, 30001, 1, 8000, 0, PLAIN, true);  // a host kernel: one pack, one download
    job(1024, 2.0f, 2, RC_PCM_I16, 30001, 1, 8000, 0, BOTH, true);
    for (size_t L : {(size_t)0, (size_t)1, (size_t)1023, (size_t)1024, (size_t)1600}) {  // none, and fewer than four sub-blocks
        job(1024, 2.0f, 3, RC_PCM_I24, L, 1, 8000, 0);
        job(1024, 2.0f, 1, RC_PCM_U8, L, 0, 44100, 8000);
    }
    printf("engine_host_driver_frames_loud: ok\n");
    return 0;
}
