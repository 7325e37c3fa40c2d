// TEST INFRASTRUCTURE: rc_engine_stretch_frames over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory,
// the hop kernels compute nothing; tests/c/hip_stub_frames.cpp: the two frame launchers read and write exactly the
// ranges they are handed) under ASan + UBSan (rocoder_amd/csrc/host/sanitize.mk: engine_frames_asan). What runs for real
// is the engine's arithmetic on the raw frame block: the byte ranges of the uploads, the frames each chunk unpacks, the
// frame ranges packed and downloaded. Every buffer is exactly as long as the call says, so an early start or a late end
// is a finding.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rocoder_hip.h"

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

// one job; the source starts `misalign` bytes into its allocation and ends with it
static void job(uint32_t N, float f, int p, uint32_t ch, uint32_t format, uint32_t bytes, size_t L, size_t misalign,
                bool host_kernel = false) {
    rc_config c = config(N, f, p, ch);
    if (host_kernel) {
        c.kernel = ok_kernel;
        c.kernel_time_ms = 1;
    }
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&c, &e) == RC_OK);
    const size_t n_out = rc_offline_output_len(&c, L);
    unsigned char *block = (unsigned char *)malloc(L * ch * bytes + misalign);
    CHECK(block != nullptr);
    memset(block, 0x5a, L * ch * bytes + misalign);
    float *out = (float *)malloc(n_out * ch * sizeof(float));
    CHECK(out != nullptr);
    for (int rep = 0; rep < 2; ++rep) {  // the second call finds the engine's buffers reserved
        size_t got = 0;
        CHECK(rc_engine_stretch_frames(e, block + misalign, L, format, out, n_out, &got) == RC_OK && got == n_out);
    }
    if (n_out) {
        size_t got = 7;
        CHECK(rc_engine_stretch_frames(e, block + misalign, L, format, out, n_out - 1, &got) == RC_ECAPACITY && got == 7);
    }
    CHECK(rc_engine_stretch_frames(e, block + misalign, L, 0, out, n_out, nullptr) == RC_EINVAL);
    CHECK(rc_engine_stretch_frames(e, block + misalign, L, 6, out, n_out, nullptr) == RC_EINVAL);
    CHECK(rc_engine_stretch_frames(e, nullptr, L, format, out, n_out, nullptr) == (L ? RC_EINVAL : RC_OK));
    CHECK(rc_engine_stretch_frames(e, block + misalign, L, format, nullptr, n_out, nullptr) == RC_EINVAL);
    CHECK(rc_engine_stretch_frames(nullptr, block + misalign, L, format, out, n_out, nullptr) == RC_EINVAL);
    free(out);
    free(block);
    rc_engine_destroy(e);
}

int main() {
    // several pipeline chunks (9.6 M output samples per channel, 4 M per staging slot), 9-byte frames from an odd address
    job(1024, 8.0f, 1, 3, RC_PCM_I24, 3, 1200001, 1);
    job(1024, 8.0f, 1, 3, RC_PCM_I24, 3, 1200001, 0);
    job(1024, 2.0f, 1, 1, RC_PCM_U8, 1, 30001, 3);
    job(1024, 2.0f, 1, 1, RC_PCM_U8, 1, 30001, 2);
    job(4096, 0.3f, 1, 2, RC_PCM_I16, 2, 3000000, 1);   // more input than output: uploads of more than one slot per chunk
    job(256, 2.0f, 1, 67, RC_PCM_I24, 3, 3000, 1);      // beyond the frames-only tile
    job(2048, 2.0f, -2, 2, RC_PCM_I32, 4, 50001, 1);
    job(65536, 8.0f, 1, 2, RC_PCM_F32, 4, 300000, 2);
    job(1024, 2.0f, 1, 2, RC_PCM_I16, 2, 30001, 1, true);  // a host kernel: whole input up, whole output down
    for (size_t L : {(size_t)0, (size_t)1, (size_t)1023, (size_t)1024}) {
        job(1024, 2.0f, 1, 3, RC_PCM_I24, 3, L, 1);
        job(1024, 2.0f, 1, 1, RC_PCM_U8, 1, L, 0);
    }
    printf("engine_host_driver_frames: ok\n");
    return 0;
}
