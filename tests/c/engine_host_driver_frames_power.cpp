// TEST INFRASTRUCTURE: rc_engine_frames_power over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory;
// tests/c/hip_stub_frames_power.cpp: the launcher reads every byte of its frame range, joins the largest byte of each bin,
// logs the range and counts how often each frame came through) under ASan + UBSan (rocoder_amd/csrc/host/sanitize.mk:
// engine_frames_power_asan). What runs for real is the engine's chunk loop: the uploads of a block at any byte phase from
// pageable memory through the staging slots or from page-locked memory itself, the frame range of every launch, the zeroed
// bins in front of the first, the one readback behind the last, and the error paths. The same program holds
// rc_autocrop_points and rc_frames_power_bins, which need no engine, to their status codes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/rocoder_hip.h"

struct RcStubPowerLaunch {  // tests/c/hip_stub_frames_power.cpp
    uint64_t frame0, n_frames, bin_frames, n_bins;
    uint32_t channels, phase, format;
};
extern RcStubPowerLaunch rc_stub_power_log[256];
extern uint32_t rc_stub_power_launches;
extern unsigned char *rc_stub_power_cover;
extern uint64_t rc_stub_power_dirty;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rc_last_error()); \
            exit(2);                                                             \
        }                                                                        \
    } while (0)

static rc_config config(uint32_t ch) {
    rc_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.window_len = 1024;
    c.factor = 2.0f;
    c.amplitude = 1.0f;
    c.pitch_multiple = 1;
    c.sample_rate = 44100;
    c.channels = ch;
    c.buffer_secs = 1.0f;
    c.seed = 7;
    return c;
}

static uint32_t bytes_of(uint32_t format) { return format == RC_PCM_U8 ? 1 : format == RC_PCM_I16 ? 2 : format == RC_PCM_I24 ? 3 : 4; }

// the byte the driver puts at byte i of frame f: below 0x80, and the largest of a bin depends on where the bin's edges fall
static unsigned char fill(size_t f, size_t i) { return (unsigned char)(((f * 2654435761u) >> 7) % 120u + (i & 7u)); }

// one job; the block is exactly as long as the call says and starts `misalign` bytes into its allocation
static void job(uint32_t ch, uint32_t format, size_t L, uint64_t bin_frames, size_t misalign, bool pinned) {
    rc_config c = config(ch);
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&c, &e) == RC_OK);
    const size_t fb = (size_t)ch * bytes_of(format), bytes = L * fb;
    void *alloc = nullptr;
    if (pinned) CHECK(rc_host_alloc(bytes + misalign + 1, &alloc) == RC_OK);
    else alloc = malloc(bytes + misalign + 1);
    CHECK(alloc != nullptr);
    unsigned char *in = (unsigned char *)alloc + misalign;
    for (size_t f = 0; f < L; ++f)
        for (size_t i = 0; i < fb; ++i) in[f * fb + i] = fill(f, i);
    const size_t n_bins = rc_frames_power_bins(L, bin_frames);
    CHECK(n_bins == (size_t)((L + bin_frames - 1) / bin_frames));
    std::vector<uint32_t> want(n_bins, 0);
    for (size_t f = 0; f < L; ++f)
        for (size_t i = 0; i < fb; ++i) want[f / bin_frames] = fill(f, i) > want[f / bin_frames] ? fill(f, i) : want[f / bin_frames];
    // the bins: guard words on both sides, a pattern the stub would report as not zeroed
    std::vector<uint32_t> block(n_bins + 2);
    std::vector<unsigned char> cover(L + 1, 0);
    for (int rep = 0; rep < 2; ++rep) {  // the second call finds the engine's buffers reserved and the bins of the first in them
        std::fill(block.begin(), block.end(), 0xdeadbeefu);
        std::fill(cover.begin(), cover.end(), (unsigned char)0);
        rc_stub_power_cover = cover.data();
        rc_stub_power_launches = 0;
        rc_stub_power_dirty = 0;
        size_t got = 99;
        CHECK(rc_engine_frames_power(e, L ? in : nullptr, L, format, bin_frames, (float *)(block.data() + 1), n_bins, &got) == RC_OK);
        rc_stub_power_cover = nullptr;
        CHECK(got == n_bins);
        // every frame went through the launcher exactly once, in launches that follow each other without a gap
        for (size_t f = 0; f < L; ++f) CHECK(cover[f] == 1);
        CHECK(cover[L] == 0);
        uint64_t at = 0;
        CHECK(rc_stub_power_launches <= 256);
        for (uint32_t k = 0; k < rc_stub_power_launches; ++k) {
            const RcStubPowerLaunch &q = rc_stub_power_log[k];
            CHECK(q.frame0 == at && q.n_frames > 0 && q.bin_frames == bin_frames && q.n_bins == n_bins && q.channels == ch &&
                  q.format == format && q.phase == (uint32_t)((uintptr_t)in & 3u));
            at += q.n_frames;
        }
        CHECK(at == L && (L == 0) == (rc_stub_power_launches == 0));
        // a job of more than one staging slot (16 MiB) went out as more than one chunk
        if (bytes > ((size_t)16 << 20)) CHECK(rc_stub_power_launches >= 2);
        // the bins were zeroed in front of the first launch (the second call finds the first call's values there), the
        // uploads had brought every byte a launch read, and one readback brought exactly n_bins words
        CHECK(rc_stub_power_dirty == 0);
        CHECK(block[0] == 0xdeadbeefu && block[n_bins + 1] == 0xdeadbeefu);
        for (size_t b = 0; b < n_bins; ++b) CHECK(block[1 + b] == want[b]);
        // (the second pass: other bytes, so that a stale bin of the first pass would show)
        for (size_t f = 0; f < L; ++f)
            for (size_t i = 0; i < fb; ++i) in[f * fb + i] = (unsigned char)(fill(f, i) / 2);
        for (size_t b = 0; b < n_bins; ++b) want[b] = 0;
        for (size_t f = 0; f < L; ++f)
            for (size_t i = 0; i < fb; ++i) {
                const uint32_t v = (unsigned char)(fill(f, i) / 2);
                if (v > want[f / bin_frames]) want[f / bin_frames] = v;
            }
    }
    // errors: nothing behind bin_peak is written, *n_bins is set where the arguments in front of it are valid
    std::fill(block.begin(), block.end(), 0xdeadbeefu);
    float *peak = (float *)(block.data() + 1);
    size_t got = 77;
    CHECK(rc_engine_frames_power(nullptr, in, L, format, bin_frames, peak, n_bins, &got) == RC_EINVAL && got == 77);
    CHECK(rc_engine_frames_power(e, in, L, format, bin_frames, nullptr, n_bins, &got) == RC_EINVAL && got == 77);
    CHECK(rc_engine_frames_power(e, in, L, format, bin_frames, peak, n_bins, nullptr) == RC_EINVAL);
    CHECK(rc_engine_frames_power(e, nullptr, L, format, bin_frames, peak, n_bins, &got) == (L ? RC_EINVAL : RC_OK));
    got = 77;
    CHECK(rc_engine_frames_power(e, in, L, 0, bin_frames, peak, n_bins, &got) == RC_EINVAL && got == 77);
    CHECK(rc_engine_frames_power(e, in, L, 6, bin_frames, peak, n_bins, &got) == RC_EINVAL && got == 77);
    CHECK(rc_engine_frames_power(e, in, L, format, 0, peak, n_bins, &got) == RC_EINVAL && got == 77);
    if (n_bins) {
        rc_stub_power_launches = 0;
        CHECK(rc_engine_frames_power(e, in, L, format, bin_frames, peak, n_bins - 1, &got) == RC_ECAPACITY && got == n_bins);
        CHECK(rc_stub_power_launches == 0);
    }
    for (uint32_t w : block) CHECK(w == 0xdeadbeefu);
    // a stretch call behind it finds the engine as it was
    {
        const size_t Ls = 3000, n_out = rc_offline_output_len(&c, Ls);
        std::vector<int16_t> s(Ls * ch + 1, 0);
        std::vector<float> out(n_out * ch + 1, 0.0f);
        size_t n = 0;
        CHECK(rc_engine_stretch_frames(e, s.data(), Ls, RC_PCM_I16, out.data(), n_out, &n) == RC_OK && n == n_out);
    }
    if (pinned) CHECK(rc_host_free(alloc) == RC_OK);
    else free(alloc);
    rc_engine_destroy(e);
}

static void autocrop_codes() {
    CHECK(rc_frames_power_bins(0, 5) == 0 && rc_frames_power_bins(1, 5) == 1 && rc_frames_power_bins(5, 5) == 1 &&
          rc_frames_power_bins(6, 5) == 2 && rc_frames_power_bins(4, 5) == 1 && rc_frames_power_bins(10, 5) == 2 &&
          rc_frames_power_bins(7, 0) == 0 && rc_frames_power_bins(7, UINT64_MAX) == 1);
    const float peaks[8] = {0.0f, 0.1f, 1.0f, 0.4f, 0.8f, 1.0f, 0.1f, 0.0f};
    uint64_t a = 11, b = 12;
    int found = 13;
    CHECK(rc_autocrop_points(peaks, 8, 1, 8, 25, &a, &b, &found) == RC_OK && a == 2 && b == 6 && found == 1);
    CHECK(rc_autocrop_points(peaks, 8, 10, 75, 25, &a, &b, &found) == RC_OK && a == 20 && b == 60 && found == 1);
    const float zeros[3] = {0.0f, 0.0f, 0.0f};
    CHECK(rc_autocrop_points(zeros, 3, 4, 10, 10, &a, &b, &found) == RC_OK && a == 0 && b == 10 && found == 0);
    const float last[3] = {0.0f, 0.5f, 1.0f};  // the quirk: the last bin above the threshold is the job's last
    CHECK(rc_autocrop_points(last, 3, 4, 10, 0, &a, &b, &found) == RC_OK && a == 4 && b == 8 && found == 1);
    a = 11, b = 12, found = 13;
    CHECK(rc_autocrop_points(nullptr, 8, 1, 8, 25, &a, &b, &found) == RC_EINVAL);
    CHECK(rc_autocrop_points(peaks, 8, 1, 8, 25, nullptr, &b, &found) == RC_EINVAL);
    CHECK(rc_autocrop_points(peaks, 8, 1, 8, 25, &a, nullptr, &found) == RC_EINVAL);
    CHECK(rc_autocrop_points(peaks, 8, 1, 8, 25, &a, &b, nullptr) == RC_EINVAL);
    CHECK(rc_autocrop_points(peaks, 0, 1, 0, 25, &a, &b, &found) == RC_EINVAL);
    CHECK(rc_autocrop_points(peaks, 8, 1, 8, 100, &a, &b, &found) == RC_EINVAL);
    CHECK(rc_autocrop_points(peaks, 8, 1, 8, 4000000000u, &a, &b, &found) == RC_EINVAL);
    CHECK(rc_autocrop_points(peaks, 8, 0, 8, 25, &a, &b, &found) == RC_EINVAL);
    CHECK(rc_autocrop_points(peaks, 8, 1, 9, 25, &a, &b, &found) == RC_EINVAL);
    CHECK(rc_autocrop_points(peaks, 8, 2, 8, 25, &a, &b, &found) == RC_EINVAL);
    const float with_nan[3] = {0.0f, (float)NAN, 1.0f};
    CHECK(rc_autocrop_points(with_nan, 3, 4, 10, 10, &a, &b, &found) == RC_EINVAL);
    CHECK(a == 11 && b == 12 && found == 13);
    const float with_inf[3] = {0.25f, (float)INFINITY, 0.0f};
    CHECK(rc_autocrop_points(with_inf, 3, 4, 10, 40, &a, &b, &found) == RC_OK && a == 4 && b == 8 && found == 1);
}

int main() {
    autocrop_codes();
    // several chunks (9-byte frames: 16 MiB is no whole number of them), every byte phase, pageable and page-locked
    for (size_t mis = 0; mis < 4; ++mis) job(3, RC_PCM_I24, 4000001, 4410, mis, false);
    for (size_t mis : {(size_t)0, (size_t)1}) job(3, RC_PCM_I24, 4000001, 4410, mis, true);
    job(1, RC_PCM_U8, 40000003, 4096, 1, true);
    job(2, RC_PCM_I16, 5000001, 50000, 2, false);
    job(2, RC_PCM_F32, 30001, 7, 1, false);
    job(5, RC_PCM_I32, 30001, 1, 3, true);
    job(67, RC_PCM_I24, 3000, 4410, 1, false);  // one bin, longer than the job
    for (size_t L : {(size_t)0, (size_t)1, (size_t)6, (size_t)7, (size_t)8})
        for (bool pinned : {false, true}) {
            job(3, RC_PCM_I24, L, 7, 1, pinned);
            job(1, RC_PCM_U8, L, 7, 0, pinned);
        }
    printf("engine_host_driver_frames_power: ok\n");
    return 0;
}
