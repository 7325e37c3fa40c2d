// TEST INFRASTRUCTURE: rc_engine_stretch_frames_norm over the HIP stub (tests/c/hip_stub.cpp: device memory is host
// memory, the hop kernels compute nothing; tests/c/hip_stub_frames_norm.cpp: the peak launcher reads its range and counts
// the samples it covered, the pack launcher forms and stores the gain and writes the marks of hip_stub_frames_pcm.cpp)
// under ASan + UBSan (rocoder_amd/csrc/host/sanitize.mk: engine_frames_norm_asan). What runs for real is the two-phase
// bookkeeping: phase 1's uploads and peak ranges, phase 2's pack ranges and downloads through the staging slots, the
// one readback of counter, peak word and gain, and the error paths. The output buffer is exactly as long as the call
// says and starts `misalign` bytes into its allocation; every byte of it is checked.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../include/rocoder_hip.h"

extern uint64_t rc_stub_peak_samples, rc_stub_gain_stores;  // tests/c/hip_stub_frames_norm.cpp

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

// one job: i16 frames in, `out_format` out; the target starts `misalign` bytes into its allocation and ends with it
static void job(uint32_t N, float f, int p, uint32_t ch, uint32_t out_format, size_t L, size_t misalign, bool host_kernel = false) {
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
    const float target = 0.5f, want_peak = (float)(1 + (uint64_t)n_out * ch);
    for (int rep = 0; rep < 2; ++rep) {  // the second call finds the engine's buffers reserved
        memset(block, 0x11, out_bytes + misalign);
        size_t got = 0;
        uint64_t clipped = 99;
        float peak = -1.0f, gain = -1.0f;
        rc_stub_peak_samples = rc_stub_gain_stores = 0;
        CHECK(rc_engine_stretch_frames_norm(e, in, L, RC_PCM_I16, out, n_out, out_format, target, &got, &peak, &gain, &clipped) == RC_OK &&
              got == n_out);
        // every output sample went through the peak launcher once, all of them in front of the first pack launch, which
        // alone stored the gain; the rows are zeros, so nothing is beyond full scale
        CHECK(rc_stub_peak_samples == (uint64_t)n_out * ch && rc_stub_gain_stores == 1);
        CHECK(peak == want_peak && gain == target / want_peak && clipped == 0);
        for (size_t i = 0; i < misalign; ++i) CHECK(block[i] == 0x11);
        for (size_t i = 0; i < out_bytes; ++i) {
            const size_t s = i / OB;
            if (out[i] != (unsigned char)(0x80u | (((s % ch) & 7u) << 2) | (i % OB))) {
                fprintf(stderr, "FAIL: byte %zu of %zu is %02x (format %u, %u channels, misalign %zu)\n", i, out_bytes, out[i],
                        out_format, ch, misalign);
                exit(2);
            }
        }
    }
    // a plain PCM call on the same engine behind a normalised one: the new phase leaves nothing behind
    {
        memset(block, 0x11, out_bytes + misalign);
        uint64_t clipped = 99;
        CHECK(rc_engine_stretch_frames_pcm(e, in, L, RC_PCM_I16, out, n_out, out_format, nullptr, &clipped) == RC_OK && clipped == 0);
        for (size_t i = 0; i < out_bytes; ++i) CHECK(out[i] == (unsigned char)(0x80u | ((((i / OB) % ch) & 7u) << 2) | (i % OB)));
    }
    CHECK(rc_engine_stretch_frames_norm(e, in, L, RC_PCM_I16, out, n_out, out_format, target, nullptr, nullptr, nullptr, nullptr) == RC_OK);
    CHECK(rc_engine_stretch_frames_norm(e, nullptr, L, RC_PCM_I16, out, n_out, out_format, target, nullptr, nullptr, nullptr, nullptr) ==
          (L ? RC_EINVAL : RC_OK));
    size_t got = 7;
    uint64_t clipped = 5;
    float peak = 3.0f, gain = 4.0f;
    memset(block, 0x11, out_bytes + misalign);
    if (n_out) CHECK(rc_engine_stretch_frames_norm(e, in, L, RC_PCM_I16, out, n_out - 1, out_format, target, &got, &peak, &gain, &clipped) == RC_ECAPACITY);
    for (float bad : {0.0f, -1.0f, (float)NAN, (float)INFINITY, -(float)INFINITY})
        CHECK(rc_engine_stretch_frames_norm(e, in, L, RC_PCM_I16, out, n_out, out_format, bad, &got, &peak, &gain, &clipped) == RC_EINVAL);
    CHECK(rc_engine_stretch_frames_norm(e, in, L, 0, out, n_out, out_format, target, &got, &peak, &gain, &clipped) == RC_EINVAL);
    CHECK(rc_engine_stretch_frames_norm(e, in, L, 6, out, n_out, out_format, target, &got, &peak, &gain, &clipped) == RC_EINVAL);
    CHECK(rc_engine_stretch_frames_norm(e, in, L, RC_PCM_I16, out, n_out, 0, target, &got, &peak, &gain, &clipped) == RC_EINVAL);
    CHECK(rc_engine_stretch_frames_norm(e, in, L, RC_PCM_I16, out, n_out, 6, target, &got, &peak, &gain, &clipped) == RC_EINVAL);
    CHECK(rc_engine_stretch_frames_norm(e, in, L, RC_PCM_I16, nullptr, n_out, out_format, target, &got, &peak, &gain, &clipped) == RC_EINVAL);
    CHECK(rc_engine_stretch_frames_norm(nullptr, in, L, RC_PCM_I16, out, n_out, out_format, target, &got, &peak, &gain, &clipped) == RC_EINVAL);
    // on any error nothing behind the out-pointers was written
    CHECK(got == 7 && clipped == 5 && peak == 3.0f && gain == 4.0f);
    for (size_t i = 0; i < out_bytes + misalign; ++i) CHECK(block[i] == 0x11);
    free(block);
    free(in);
    rc_engine_destroy(e);
}

int main() {
    // several pipeline chunks (9.6 M output samples per channel, 4 M per staging slot), 9-byte frames to every phase
    for (size_t mis = 0; mis < 4; ++mis) job(1024, 8.0f, 1, 3, RC_PCM_I24, 1200001, mis);
    job(1024, 8.0f, 1, 3, RC_PCM_U8, 1200001, 3);
    // window_out_len x channels x bytes no multiple of 4 (a negative pitch multiple): chunk edges inside a dword
    job(1024, 8.0f, -3, 3, RC_PCM_I24, 1200001, 1);
    job(1024, 2.0f, 1, 1, RC_PCM_U8, 30001, 3);
    job(1024, 2.0f, 1, 2, RC_PCM_I16, 30001, 1);
    job(1024, 2.0f, 1, 5, RC_PCM_I32, 30001, 2);
    job(1024, 2.0f, 1, 2, RC_PCM_F32, 30001, 1);
    job(256, 2.0f, 1, 67, RC_PCM_I24, 3000, 1);            // beyond the frames-only tile
    job(1024, 2.0f, 1, 2, RC_PCM_I16, 30001, 1, true);     // a host kernel: the peak kernel, one pack, one download
    for (size_t L : {(size_t)0, (size_t)1, (size_t)1023, (size_t)1024}) {
        job(1024, 2.0f, 1, 3, RC_PCM_I24, L, 1);
        job(1024, 2.0f, 1, 1, RC_PCM_U8, L, 0);
    }
    printf("engine_host_driver_frames_norm: ok\n");
    return 0;
}
