// TEST INFRASTRUCTURE: rc_engine_set_output_dither over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory,
// the hop kernels compute nothing; tests/c/hip_stub_frames_dither.cpp: the dithered pack launchers write exactly the
// bytes they may write, each marked with the low bits of its sample's absolute frame and job channel, the mode and the
// byte number, and log every launch's exact t0, frame count and channel0; the undithered launchers of
// hip_stub_frames_pcm.cpp write marks of another form) under ASan + UBSan
// (rocoder_amd/csrc/host/sanitize.mk: engine_frames_dither_asan). What runs for real is the engine's side of the feature:
// which launcher a job takes, the t0 and channel0 each chunk's launch is handed, the key table's upload, the byte ranges.
// The output buffer is exactly as long as the call says and starts `misalign` bytes into its allocation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rocoder_hip.h"

struct RcStubDitherLaunch {  // tests/c/hip_stub_frames_dither.cpp
    uint64_t t0, n_frames;
    uint32_t channel0, channels, mode;
};
extern RcStubDitherLaunch rc_stub_dither_log[256];
extern uint64_t rc_stub_dither_launches;
extern uint64_t rc_stub_dither_key_sum;
unsigned char rc_stub_dither_mark(uint64_t t, uint32_t channel, uint32_t mode, uint32_t byte);
extern uint64_t rc_stub_gain_stores;      // tests/c/hip_stub_frames_norm.cpp
extern uint64_t rc_stub_peak_samples;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rc_last_error()); \
            exit(2);                                                             \
        }                                                                        \
    } while (0)

static rc_config config(uint32_t N, float f, int p, uint32_t ch) {
    rc_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.window_len = N;
    c.factor = f;
    c.amplitude = 1.0f;
    c.pitch_multiple = p;
    c.sample_rate = 44100;
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
static bool dithers(uint32_t format) { return format == RC_PCM_U8 || format == RC_PCM_I16 || format == RC_PCM_I24; }

// the mark of byte i of the output: the dithered launcher's where mode and format dither, else the undithered one's
static unsigned char want(size_t i, uint32_t ch, uint32_t OB, uint32_t mode, uint32_t out_format) {
    const size_t s = i / OB;
    if (mode != RC_DITHER_NONE && dithers(out_format)) return rc_stub_dither_mark(s / ch, (uint32_t)(s % ch), mode, (uint32_t)(i % OB));
    return (unsigned char)(0x80u | (((s % ch) & 7u) << 2) | (i % OB));
}

// one job: i16 frames in, `out_format` out through the pcm entry or (norm) the normalised one, with `mode` set; brief: the
// one call alone (the long jobs)
static void job(uint32_t N, float f, int p, uint32_t ch, uint32_t out_format, size_t L, size_t misalign, uint32_t mode, bool norm,
                bool host_kernel = false, bool brief = false) {
    rc_config c = config(N, f, p, ch);
    if (host_kernel) {
        c.kernel = ok_kernel;
        c.kernel_time_ms = 1;
    }
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&c, &e) == RC_OK);
    const uint32_t OB = bytes_of(out_format);
    const size_t n_out = rc_offline_output_len(&c, L), out_bytes = n_out * ch * OB;
    int16_t *in = (int16_t *)calloc(L * ch + 1, sizeof(int16_t));
    unsigned char *block = (unsigned char *)malloc(out_bytes + misalign);
    CHECK(in != nullptr && block != nullptr);
    unsigned char *out = block + misalign;
    uint64_t key_sum = 0;
    for (uint32_t k = 0; k < ch; ++k) key_sum += rc_phase_key(11, k, 0xFFFFFFFFFFull);
    auto run = [&](uint32_t set_mode) {
        memset(block, 0x11, out_bytes + misalign);
        rc_stub_dither_launches = rc_stub_dither_key_sum = rc_stub_gain_stores = rc_stub_peak_samples = 0;
        size_t got = 0;
        uint64_t clipped = 99;
        float peak = -1.0f, gain = -1.0f;
        if (norm)
            CHECK(rc_engine_stretch_frames_norm(e, in, L, RC_PCM_I16, out, n_out, out_format, 0.5f, &got, &peak, &gain, &clipped) == RC_OK);
        else
            CHECK(rc_engine_stretch_frames_pcm(e, in, L, RC_PCM_I16, out, n_out, out_format, &got, &clipped) == RC_OK);
        CHECK(got == n_out && clipped == 0);
        const bool on = set_mode != RC_DITHER_NONE && dithers(out_format);
        CHECK((rc_stub_dither_launches != 0) == (on && n_out != 0));
        // every launch read the keys of seed 11, all channels (a frames job is one piece of all of them)
        CHECK(rc_stub_dither_key_sum == rc_stub_dither_launches * key_sum);
        // the launches cover the job's frames in order, each handed exactly the absolute frame it starts at
        CHECK(rc_stub_dither_launches <= 256);
        uint64_t at = 0;
        for (uint64_t k = 0; k < rc_stub_dither_launches; ++k) {
            const RcStubDitherLaunch &l = rc_stub_dither_log[k];
            if (l.t0 != at || l.channel0 != 0 || l.channels != ch || l.mode != set_mode || l.n_frames == 0) {
                fprintf(stderr, "FAIL: launch %llu of %llu: t0 %llu (the frames in front: %llu), %llu frames, channel0 %u, %u channels, mode %u\n",
                        (unsigned long long)k, (unsigned long long)rc_stub_dither_launches, (unsigned long long)l.t0, (unsigned long long)at,
                        (unsigned long long)l.n_frames, l.channel0, l.channels, l.mode);
                exit(2);
            }
            at += l.n_frames;
        }
        if (on) CHECK(at == n_out);
        if (norm && n_out) CHECK(rc_stub_gain_stores == 1 && gain == 0.5f / (float)(1 + n_out * ch));
        for (size_t i = 0; i < misalign; ++i) CHECK(block[i] == 0x11);
        for (size_t i = 0; i < out_bytes; ++i)
            if (out[i] != want(i, ch, OB, set_mode, out_format)) {
                fprintf(stderr, "FAIL: byte %zu of %zu is %02x, not %02x (format %u, %u channels, misalign %zu, mode %u, norm %d)\n", i,
                        out_bytes, out[i], want(i, ch, OB, set_mode, out_format), out_format, ch, misalign, set_mode, (int)norm);
                exit(2);
            }
    };
    CHECK(rc_engine_set_output_dither(e, mode, 11) == RC_OK);
    run(mode);
    if (brief) {
        free(block);
        free(in);
        rc_engine_destroy(e);
        return;
    }
    run(mode);  // the second call finds the key table on the device
    // the setter's errors leave the state as it was
    CHECK(rc_engine_set_output_dither(e, 3, 5) == RC_EINVAL);
    CHECK(rc_engine_set_output_dither(e, 0xFFFFFFFFu, 5) == RC_EINVAL);
    CHECK(rc_engine_set_output_dither(nullptr, mode, 5) == RC_EINVAL);
    run(mode);
    // the other mode, then none again: the undithered launchers
    const uint32_t other = mode == RC_DITHER_TPDF ? RC_DITHER_TPDF_HP : RC_DITHER_TPDF;
    CHECK(rc_engine_set_output_dither(e, other, 11) == RC_OK);
    run(other);
    CHECK(rc_engine_set_output_dither(e, RC_DITHER_NONE, 11) == RC_OK);
    run(RC_DITHER_NONE);
    // the f32 entry takes no dither
    if (n_out) {
        CHECK(rc_engine_set_output_dither(e, mode, 11) == RC_OK);
        std::vector<float> y(n_out * ch);
        size_t got = 0;
        rc_stub_dither_launches = 0;
        CHECK(rc_engine_stretch_frames(e, in, L, RC_PCM_I16, y.data(), n_out, &got) == RC_OK && got == n_out);
        CHECK(rc_stub_dither_launches == 0);
    }
    free(block);
    free(in);
    rc_engine_destroy(e);
}

int main() {
    // several pipeline chunks (9.6 M output samples per channel, 4 M per staging slot), 9-byte frames to every phase: the
    // log holds every chunk's exact t0, so a chunk handed the wrong one fails
    for (size_t mis = 0; mis < 4; ++mis) job(1024, 8.0f, 1, 3, RC_PCM_I24, 1200001, mis, mis & 1 ? RC_DITHER_TPDF : RC_DITHER_TPDF_HP, false, false, true);
    job(1024, 8.0f, 1, 3, RC_PCM_U8, 1200001, 3, RC_DITHER_TPDF, true, false, true);
    // a negative pitch multiple: window_out_len 1023, so the chunks start at frames that are no multiple of 8 and a wrong
    // t0 shows in the marks of the bytes as well; the chunk edges lie inside a dword
    job(1024, 8.0f, -3, 3, RC_PCM_I24, 1200001, 1, RC_DITHER_TPDF_HP, false, false, true);
    job(1024, 8.0f, -3, 1, RC_PCM_U8, 1200001, 2, RC_DITHER_TPDF, true, false, true);  // the normalised entry: two runs over the chunks
    for (size_t mis = 0; mis < 4; ++mis) {
        job(1024, 2.0f, 1, 1, RC_PCM_U8, 30001, mis, RC_DITHER_TPDF, false);
        job(1024, 2.0f, 1, 2, RC_PCM_I16, 30001, mis, RC_DITHER_TPDF_HP, true);
    }
    // formats that take no dither: the undithered launchers, mode set or not
    job(1024, 2.0f, 1, 5, RC_PCM_I32, 30001, 2, RC_DITHER_TPDF, false);
    job(1024, 2.0f, 1, 2, RC_PCM_F32, 30001, 1, RC_DITHER_TPDF_HP, false);
    job(1024, 2.0f, 1, 2, RC_PCM_I32, 30001, 1, RC_DITHER_TPDF, true);
    job(256, 2.0f, 1, 67, RC_PCM_I24, 3000, 1, RC_DITHER_TPDF, false);          // beyond the frames-only tile
    job(1024, 2.0f, 1, 2, RC_PCM_I16, 30001, 1, RC_DITHER_TPDF, false, true);   // a host kernel: one pack, one download
    job(1024, 2.0f, 1, 2, RC_PCM_I16, 30001, 3, RC_DITHER_TPDF_HP, true, true);
    for (size_t L : {(size_t)0, (size_t)1}) {  // jobs of 0 and 1 input frames
        job(1024, 2.0f, 1, 3, RC_PCM_I24, L, 1, RC_DITHER_TPDF, false);
        job(1024, 2.0f, 1, 1, RC_PCM_U8, L, 0, RC_DITHER_TPDF_HP, true);
    }
    printf("engine_host_driver_frames_dither: ok\n");
    return 0;
}
