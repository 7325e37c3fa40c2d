// TEST INFRASTRUCTURE: rc_engine_set_output_fade over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory,
// streams run at enqueue time, the hop kernels compute nothing; tests/c/hip_stub_frames_fade.cpp: the fade launcher logs
// its launch and writes a mark over every sample of its range) under ASan + UBSan (rocoder_amd/csrc/host/sanitize.mk:
// engine_frames_fade_asan). What runs for real is the engine's bookkeeping: the cut of every pipeline chunk with the
// fade ranges, the pointers and strides of the launches, their place in front of the peak launch, the pack launch or the
// download of the chunk, and the error paths. Held to, for all four whole-job host-form entries:
//   1. every output sample that a fade range covers passes through the fade launcher exactly once,
//   2. in front of the peak launch and of the pack launch / download that read it,
//   3. no sample outside the ranges passes through it,
//   4. nothing happens on an error.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/rocoder_hip.h"

struct RcStubFadeLaunch {  // tests/c/hip_stub_frames_fade.cpp
    uint64_t t0, t1, in_len, out_start, out_len, stride, peak_samples_before;
    uint32_t channels;
    uintptr_t row0;
};
extern RcStubFadeLaunch rc_stub_fade_log[256];
extern uint32_t rc_stub_fade_launches;
extern float rc_stub_fade_mark;
extern uint64_t rc_stub_peak_samples;  // tests/c/hip_stub_frames_norm.cpp

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rc_last_error()); \
            exit(2);                                                             \
        }                                                                        \
    } while (0)

static rc_config config(uint32_t N, float f, uint32_t ch) {
    rc_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.window_len = N;
    c.factor = f;
    c.amplitude = 1.0f;
    c.pitch_multiple = 1;
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

struct Fade {
    uint64_t in_len, out_start, out_len;
};

// frame t of a job of T frames lies in a range the fade changes
static bool covered(const Fade &f, uint64_t t) { return t < f.in_len || (f.out_start != RC_FADE_NONE && t >= f.out_start); }

static uint64_t covered_frames(const Fade &f, uint64_t T) {
    const uint64_t in = std::min<uint64_t>(f.in_len, T);
    if (f.out_start == RC_FADE_NONE || f.out_start >= T) return in;
    return f.out_start <= in ? T : in + (T - f.out_start);
}

// the log of one call: the launches are disjoint, cover exactly the frames the fade changes, carry the fade as set, all
// point into the same rows, and none came behind the peak launch that read its first frame
static void check_log(const Fade &f, uint64_t T, uint32_t C) {
    CHECK(rc_stub_fade_launches <= 256);
    std::vector<RcStubFadeLaunch> l(rc_stub_fade_log, rc_stub_fade_log + rc_stub_fade_launches);
    std::sort(l.begin(), l.end(), [](const RcStubFadeLaunch &a, const RcStubFadeLaunch &b) { return a.t0 < b.t0; });
    uint64_t frames = 0, end = 0;
    for (size_t i = 0; i < l.size(); ++i) {
        CHECK(l[i].t0 < l[i].t1 && l[i].t1 <= T && l[i].t0 >= end);
        // 3. wholly inside the fade-in's frames or the fade-out's, or the two meet and leave no frame between them
        CHECK(l[i].t1 <= f.in_len || (f.out_start != RC_FADE_NONE && (l[i].t0 >= f.out_start || f.out_start <= f.in_len)));
        frames += l[i].t1 - l[i].t0;
        end = l[i].t1;
        CHECK(l[i].channels == C && l[i].stride >= T && l[i].row0 == l[0].row0);
        CHECK(l[i].in_len == f.in_len && l[i].out_start == f.out_start && l[i].out_len == f.out_len);
        CHECK(l[i].peak_samples_before <= (uint64_t)C * l[i].t0);
    }
    CHECK(frames == covered_frames(f, T));
}

enum Entry { HOST, FRAMES, PCM, NORM };

// one call of `entry` on a fresh engine with the fade `f` set: the log, and the marks in what came back
static void call(Entry entry, uint32_t N, float fac, uint32_t ch, size_t L, const Fade &f, bool host_kernel, float mark) {
    rc_config c = config(N, fac, ch);
    if (host_kernel) {
        c.kernel = ok_kernel;
        c.kernel_time_ms = 1;
    }
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&c, &e) == RC_OK);
    const size_t T = rc_offline_output_len(&c, L);
    int16_t *in = (int16_t *)calloc(L * ch + 1, sizeof(int16_t));
    float *rows_in = (float *)calloc(L * ch + 1, sizeof(float));
    float *out = (float *)malloc((T * ch + 1) * sizeof(float));
    CHECK(in && rows_in && out);
    std::vector<const float *> in_rows(ch);
    std::vector<float *> out_rows(ch);
    for (uint32_t k = 0; k < ch; ++k) {
        in_rows[k] = rows_in + (size_t)k * L;
        out_rows[k] = out + (size_t)k * T;
    }
    auto run = [&](size_t *got, float *peak, uint64_t *clipped) {
        switch (entry) {
        case HOST: return rc_engine_stretch_host(e, in_rows.data(), L, out_rows.data(), T, got);
        case FRAMES: return rc_engine_stretch_frames(e, in, L, RC_PCM_I16, out, T, got);
        case PCM: return rc_engine_stretch_frames_pcm(e, in, L, RC_PCM_I16, out, T, RC_PCM_F32, got, clipped);
        default: return rc_engine_stretch_frames_norm(e, in, L, RC_PCM_I16, out, T, RC_PCM_F32, 0.5f, got, peak, nullptr, clipped);
        }
    };
    const bool fits = f.in_len <= T && (f.out_start == RC_FADE_NONE || f.out_start + f.out_len <= T);
    CHECK(rc_engine_set_output_fade(e, f.in_len, f.out_start, f.out_len) == RC_OK);
    memset(out, 0x11, (T * ch + 1) * sizeof(float));
    size_t got = 7;
    float peak = 3.0f;
    uint64_t clipped = 5;
    rc_stub_fade_launches = 0;
    rc_stub_peak_samples = 0;
    rc_stub_fade_mark = mark;
    const int rc = run(&got, &peak, &clipped);
    if (!fits) {  // 4. the status, and nothing else: no launch, no byte of the output, no word behind an out-pointer
        CHECK(rc == RC_EINVAL && rc_stub_fade_launches == 0 && rc_stub_peak_samples == 0);
        CHECK(got == 7 && peak == 3.0f && clipped == 5);
        for (size_t i = 0; i < (T * ch + 1) * sizeof(float); ++i) CHECK(((unsigned char *)out)[i] == 0x11);
    } else {
        CHECK(rc == RC_OK && got == T);
        check_log(f, T, ch);
        // 1. - 3. in the result: the mark on exactly the samples of the covered frames (the rows of a fresh engine hold
        // zeros). The PCM pack stub writes byte marks, not the samples: it counts the marks it read as clipped instead.
        const uint64_t n_cov = covered_frames(f, T);
        if (entry == HOST || entry == FRAMES) {
            for (size_t t = 0; t < T; ++t)
                for (uint32_t k = 0; k < ch; ++k) {
                    const float x = entry == HOST ? out[(size_t)k * T + t] : out[t * ch + k];
                    if (x != (covered(f, t) ? mark : 0.0f)) {
                        fprintf(stderr, "FAIL: frame %zu of %zu channel %u is %g (entry %d, fade %llu %llu %llu)\n", t, T, k, (double)x,
                                (int)entry, (unsigned long long)f.in_len, (unsigned long long)f.out_start, (unsigned long long)f.out_len);
                        exit(2);
                    }
                }
        } else {
            CHECK(clipped == n_cov * ch);
        }
        if (entry == NORM) {  // every sample through the peak launcher once, and it saw the marks (each above its own count)
            CHECK(rc_stub_peak_samples == (uint64_t)T * ch);
            CHECK(peak == (n_cov ? mark : T ? (float)(1 + (uint64_t)T * ch) : 0.0f));
        }
        // cleared: no launch, and what the entry gave before this fade was set
        CHECK(rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 0) == RC_OK);
        rc_stub_fade_launches = 0;
        CHECK(run(&got, &peak, &clipped) == RC_OK && rc_stub_fade_launches == 0);
    }
    free(out);
    free(rows_in);
    free(in);
    rc_engine_destroy(e);
}

static void all_entries(uint32_t N, float fac, uint32_t ch, size_t L, const Fade &f, bool host_kernel = false) {
    // (a mark above every count the peak stub folds in, and beyond full scale)
    for (Entry en : {HOST, FRAMES, PCM, NORM}) call(en, N, fac, ch, L, f, host_kernel, 1e30f);
}

int main() {
    {  // the setter
        rc_config c = config(1024, 2.0f, 1);
        rc_engine *e = nullptr;
        CHECK(rc_engine_create(&c, &e) == RC_OK);
        CHECK(rc_engine_set_output_fade(nullptr, 0, RC_FADE_NONE, 0) == RC_EINVAL);
        CHECK(rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 0) == RC_OK);
        CHECK(rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 1) == RC_EINVAL);
        CHECK(rc_engine_set_output_fade(e, 0, RC_FADE_NONE - 1, 2) == RC_EINVAL);
        CHECK(rc_engine_set_output_fade(e, RC_FADE_NONE, RC_FADE_NONE - 1, 1) == RC_OK);
        CHECK(rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 0) == RC_OK);
        // (for tests/test_frames_fade_host.py, which has no engine without a device: the codes as they came back)
        printf("setter: clear %d, wrap %d, none with a length %d, null engine %d\n", rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 0),
               rc_engine_set_output_fade(e, 0, RC_FADE_NONE - 1, 2), rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 1),
               rc_engine_set_output_fade(nullptr, 0, RC_FADE_NONE, 0));
        rc_engine_destroy(e);
    }
    {
        // several pipeline chunks (9.6 M output frames per channel, 4 M floats per staging slot): a fade-in across the
        // first chunk edge, a fade-out from inside the second chunk to 7 frames in front of the end, both ranges
        // overlapping, and a fade-out that starts where a chunk may end
        rc_config c = config(1024, 8.0f, 3);
        const uint64_t T = rc_offline_output_len(&c, 1200001);
        CHECK(T > (uint64_t)(16 << 20) / 4);
        all_entries(1024, 8.0f, 3, 1200001, Fade{5000001, 6000001, T - 6000001 - 7});
        all_entries(1024, 8.0f, 3, 1200001, Fade{5000001, 4500000, 3000001});
        call(FRAMES, 1024, 8.0f, 3, 1200001, Fade{0, (uint64_t)(16 << 20) / 4, 1}, false, 3.0f);
        call(NORM, 1024, 8.0f, 3, 1200001, Fade{T, RC_FADE_NONE, 0}, false, 1e30f);
    }
    {
        rc_config c = config(256, 2.0f, 2);
        const uint64_t T = rc_offline_output_len(&c, 5001);
        for (const Fade &f : {Fade{1, RC_FADE_NONE, 0}, Fade{3, RC_FADE_NONE, 0}, Fade{1001, RC_FADE_NONE, 0}, Fade{T, RC_FADE_NONE, 0},
                              Fade{0, 5, 0}, Fade{0, 7, T - 7}, Fade{0, T, 0}, Fade{1001, T - 1502, 1499}, Fade{2000, 1000, 3001},
                              Fade{0, 0, 0},
                              // 4. a fade that does not lie inside the job
                              Fade{T + 1, RC_FADE_NONE, 0}, Fade{0, T - 1, 2}, Fade{0, T + 1, 0}, Fade{T + 1, 0, T}})
            all_entries(256, 2.0f, 2, 5001, f);
        all_entries(256, 2.0f, 67, 3000, Fade{1001, 2000, 999});  // beyond the frames-only tile
        // a host frequency kernel: the simple order - the whole job, one fade launch per range, one pack, one download
        rc_config ck = config(1024, 2.0f, 2);
        const uint64_t Tk = rc_offline_output_len(&ck, 30001);
        all_entries(1024, 2.0f, 2, 30001, Fade{1001, Tk - 1506, 1499}, true);
        all_entries(1024, 2.0f, 2, 30001, Fade{1001, Tk, 1}, true);
    }
    {  // no input frames: whatever output length that gives, the same rules hold
        rc_config c = config(1024, 2.0f, 2);
        const uint64_t T = rc_offline_output_len(&c, 0);
        all_entries(1024, 2.0f, 2, 0, Fade{0, 0, 0});
        all_entries(1024, 2.0f, 2, 0, Fade{T, T, 0});
        all_entries(1024, 2.0f, 2, 0, Fade{T + 1, RC_FADE_NONE, 0});
        all_entries(1024, 2.0f, 2, 0, Fade{0, T, 1});
    }
    printf("engine_host_driver_frames_fade: ok\n");
    return 0;
}
