// TEST INFRASTRUCTURE: rc_engine_set_output_resample over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory,
// streams run at enqueue time, the hop kernels compute nothing; tests/c/hip_stub_frames_resample.cpp: the resample launcher
// logs its launch, reads every tap it may and writes a mark over its range) under ASan + UBSan
// (rocoder_amd/csrc/host/sanitize.mk: engine_frames_resample_asan). What runs for real is the engine's bookkeeping: the
// lag of the stage behind the pipeline's chunks, the pointers and strides of the launches, the ranges of the fade, pack
// and download behind it. Held to, for several ratios and multi-chunk jobs, on all four whole-job host-form entries:
//   1. the ranges of a job tile [0, n_rs) exactly once, in order,
//   2. no launch reads a row frame its chunk has not finished (every tap below src_len, src_len never beyond the job),
//   3. the fade, pack and download ranges are the resampled ones,
//   4. with the state cleared, the logged operations and the bytes equal those of an engine that never set it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rocoder_hip.h"

struct RcStubResampleLaunch {  // tests/c/hip_stub_frames_resample.cpp
    uint64_t m0, m1, src0, src_len, n, stride, dst_stride;
    uint32_t num, den, W, channels;
    uintptr_t src_row0, dst_row0;
};
extern RcStubResampleLaunch rc_stub_resample_log[256];
extern uint32_t rc_stub_resample_launches;
extern float rc_stub_resample_mark;
struct RcStubFadeLaunch {  // tests/c/hip_stub_frames_fade.cpp
    uint64_t t0, t1, in_len, out_start, out_len, stride, peak_samples_before;
    uint32_t channels;
    uintptr_t row0;
};
extern RcStubFadeLaunch rc_stub_fade_log[256];
extern uint32_t rc_stub_fade_launches;
extern float rc_stub_fade_mark;
struct RcStubDitherLaunch {  // tests/c/hip_stub_frames_dither.cpp
    uint64_t t0, n_frames;
    uint32_t channel0, channels, mode;
};
extern RcStubDitherLaunch rc_stub_dither_log[256];
extern uint64_t rc_stub_dither_launches;
extern uint64_t rc_stub_peak_samples;  // tests/c/hip_stub_frames_norm.cpp

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rc_last_error()); \
            exit(2);                                                             \
        }                                                                        \
    } while (0)

static rc_config config(uint32_t N, float f, int32_t pitch, uint32_t ch) {
    rc_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.window_len = N;
    c.factor = f;
    c.amplitude = 1.0f;
    c.pitch_multiple = pitch;
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

static uint32_t gcd(uint32_t a, uint32_t b) { return b ? gcd(b, a % b) : a; }

static void reset_logs() { rc_stub_resample_launches = rc_stub_fade_launches = 0, rc_stub_dither_launches = rc_stub_peak_samples = 0; }

// 1. and 2. on the log of one run over the chunks of a job of n row frames
static void check_resample_log(uint32_t num, uint32_t den, uint64_t n, uint64_t n_rs, uint32_t C, bool whole_job) {
    CHECK(rc_stub_resample_launches <= 256);
    CHECK((rc_stub_resample_launches != 0) == (n_rs != 0));
    if (whole_job && n_rs) CHECK(rc_stub_resample_launches == 1);
    const uint32_t g = gcd(num, den);
    num /= g, den /= g;
    const uint64_t W = num <= den ? 32 : ((uint64_t)32 * num + den - 1) / den;
    uint64_t at = 0, finished = 0;
    for (uint32_t k = 0; k < rc_stub_resample_launches; ++k) {
        const RcStubResampleLaunch &l = rc_stub_resample_log[k];
        CHECK(l.m0 == at && l.m1 > l.m0 && l.m1 <= n_rs);
        CHECK(l.num == num && l.den == den && l.W == W && l.channels == C && l.n == n);
        CHECK(l.src0 == 0 && l.src_len <= n && l.src_len >= finished);
        CHECK(l.stride == std::max<uint64_t>(n, 1) && l.dst_stride == std::max<uint64_t>(n_rs, 1));
        CHECK(l.src_row0 == rc_stub_resample_log[0].src_row0 && l.dst_row0 == rc_stub_resample_log[0].dst_row0);
        // the last tap of the range lies in what the chunk has finished, or behind the job's end (zeros)
        const uint64_t last_tap = (l.m1 - 1) * num / den + W;
        CHECK(last_tap < l.src_len || l.src_len == n);
        // and the launch did not wait: the next output needs a frame that is not there yet
        if (l.src_len < n) CHECK(l.m1 * num / den + W >= l.src_len);
        finished = l.src_len;
        at = l.m1;
    }
    CHECK(at == n_rs);
}

// one engine, one input, all four entries under the step num / den
static void job(uint32_t N, float f, int32_t pitch, uint32_t ch, size_t L, uint32_t num, uint32_t den, bool host_kernel) {
    rc_config cfg = config(N, f, pitch, ch);
    if (host_kernel) cfg.kernel = ok_kernel;
    rc_engine *e = nullptr, *fresh = nullptr;
    CHECK(rc_engine_create(&cfg, &e) == RC_OK && rc_engine_create(&cfg, &fresh) == RC_OK);
    const size_t n = rc_offline_output_len(&cfg, L), n_rs = rc_resample_len(n, num, den);
    CHECK(n_rs == (n ? ((unsigned __int128)n * den - 1) / num + 1 : 0));
    std::vector<int16_t> in(std::max<size_t>(L * ch, 1), 0);
    const float kSentinel = -7.0f;
    CHECK(rc_engine_set_output_resample(e, num, den) == RC_OK);

    // --- rc_engine_stretch_frames, a fade-in over the whole resampled job: every frame is faded once, packed and downloaded
    CHECK(rc_engine_set_output_fade(e, n_rs, RC_FADE_NONE, 0) == RC_OK);
    {
        std::vector<float> out((n_rs + 3) * ch, kSentinel);
        size_t got = 99;
        reset_logs();
        if (n_rs) {
            CHECK(rc_engine_stretch_frames(e, in.data(), L, RC_PCM_I16, out.data(), n_rs - 1, &got) == RC_ECAPACITY);
            CHECK(rc_stub_resample_launches == 0 && got == 99 && out[0] == kSentinel);
        }
        CHECK(rc_engine_stretch_frames(e, in.data(), L, RC_PCM_I16, out.data(), n_rs + 3, &got) == RC_OK && got == n_rs);
        check_resample_log(num, den, n, n_rs, ch, host_kernel);
        if (!host_kernel && n > ((size_t)4 << 20)) CHECK(rc_stub_resample_launches >= 2);  // (more than a staging slot: chunks)
        // 3. the fade launches are the resample launches' ranges, on the resampled rows
        CHECK(rc_stub_fade_launches == rc_stub_resample_launches);
        for (uint32_t k = 0; k < rc_stub_fade_launches; ++k) {
            const RcStubFadeLaunch &fl = rc_stub_fade_log[k];
            const RcStubResampleLaunch &rl = rc_stub_resample_log[k];
            CHECK(fl.t0 == rl.m0 && fl.t1 == rl.m1 && fl.stride == rl.dst_stride && fl.row0 == rl.dst_row0 && fl.channels == ch);
        }
        for (size_t i = 0; i < out.size(); ++i) CHECK(out[i] == (i < n_rs * ch ? rc_stub_fade_mark : kSentinel));
        // a fade beyond n_rs, though inside the unresampled n
        if (n > n_rs) {
            CHECK(rc_engine_set_output_fade(e, n_rs + 1, RC_FADE_NONE, 0) == RC_OK);
            reset_logs();
            CHECK(rc_engine_stretch_frames(e, in.data(), L, RC_PCM_I16, out.data(), n_rs + 3, &got) == RC_EINVAL);
            CHECK(rc_stub_resample_launches == 0);
        }
    }
    CHECK(rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 0) == RC_OK);

    // --- rc_engine_stretch_host: rows of n_rs resampled frames, each the resample launcher's mark
    {
        std::vector<std::vector<float>> xin(ch, std::vector<float>(std::max<size_t>(L, 1), 0.0f)), rows(ch, std::vector<float>(n_rs + 2, kSentinel));
        std::vector<const float *> ip(ch);
        std::vector<float *> op(ch);
        for (uint32_t c = 0; c < ch; ++c) ip[c] = xin[c].data(), op[c] = rows[c].data();
        size_t got = 99;
        reset_logs();
        CHECK(rc_engine_stretch_host(e, ip.data(), L, op.data(), n_rs + 2, &got) == RC_OK && got == n_rs);
        check_resample_log(num, den, n, n_rs, ch, host_kernel);
        for (uint32_t c = 0; c < ch; ++c)
            for (size_t i = 0; i < n_rs + 2; ++i) CHECK(rows[c][i] == (i < n_rs ? rc_stub_resample_mark : kSentinel));
        if (n_rs) CHECK(rc_engine_stretch_host(e, ip.data(), L, op.data(), n_rs - 1, &got) == RC_ECAPACITY);
    }

    // --- _pcm and _norm with a dither: the pack launches count resampled frames and tile [0, n_rs)
    CHECK(rc_engine_set_output_dither(e, RC_DITHER_TPDF, 3) == RC_OK);
    for (int norm = 0; norm < 2; ++norm) {
        std::vector<unsigned char> out((n_rs + 2) * ch * 2 + 1, 0x11);
        size_t got = 99;
        uint64_t clipped = 99;
        float peak = -1.0f, gain = -1.0f;
        reset_logs();
        if (norm)
            CHECK(rc_engine_stretch_frames_norm(e, in.data(), L, RC_PCM_I16, out.data() + 1, n_rs, RC_PCM_I16, 0.5f, &got, &peak, &gain, &clipped) == RC_OK);
        else
            CHECK(rc_engine_stretch_frames_pcm(e, in.data(), L, RC_PCM_I16, out.data() + 1, n_rs, RC_PCM_I16, &got, &clipped) == RC_OK);
        CHECK(got == n_rs);
        check_resample_log(num, den, n, n_rs, ch, host_kernel);  // (the normalised job resamples in its first run only)
        if (norm) CHECK(rc_stub_peak_samples == n_rs * ch);
        uint64_t at = 0;
        std::vector<std::pair<uint64_t, uint64_t>> packs;
        for (uint64_t k = 0; k < rc_stub_dither_launches; ++k) {
            const RcStubDitherLaunch &l = rc_stub_dither_log[k];
            CHECK(l.t0 == at && l.channel0 == 0 && l.channels == ch && l.n_frames != 0);
            packs.push_back({l.t0, l.t0 + l.n_frames});
            at += l.n_frames;
        }
        CHECK(at == n_rs && packs.size() == rc_stub_resample_launches);
        for (size_t k = 0; k < packs.size(); ++k) CHECK(packs[k].first == rc_stub_resample_log[k].m0 && packs[k].second == rc_stub_resample_log[k].m1);
        CHECK(out[0] == 0x11);
        for (size_t i = 1 + n_rs * ch * 2; i < out.size(); ++i) CHECK(out[i] == 0x11);
    }

    // --- setter errors leave the state; cleared, the job is that of an engine that never set it
    CHECK(rc_engine_set_output_resample(e, 0, 3) == RC_EINVAL && rc_engine_set_output_resample(e, 3, 0) == RC_EINVAL);
    CHECK(rc_engine_set_output_resample(e, 9, 1) == RC_EINVAL && rc_engine_set_output_resample(e, 1, 9) == RC_EINVAL);
    CHECK(rc_engine_set_output_resample(e, 1026, 1025) == RC_EINVAL && rc_engine_set_output_resample(nullptr, 3, 2) == RC_EINVAL);
    {
        std::vector<float> out(std::max<size_t>(n_rs * ch, 1));
        size_t got = 0;
        reset_logs();
        CHECK(rc_engine_stretch_frames(e, in.data(), L, RC_PCM_I16, out.data(), n_rs, &got) == RC_OK && got == n_rs);
        check_resample_log(num, den, n, n_rs, ch, host_kernel);
    }
    CHECK(rc_engine_set_output_fade(e, std::min<size_t>(n, 100), RC_FADE_NONE, 0) == RC_OK);
    CHECK(rc_engine_set_output_fade(fresh, std::min<size_t>(n, 100), RC_FADE_NONE, 0) == RC_OK);
    CHECK(rc_engine_set_output_dither(fresh, RC_DITHER_TPDF, 3) == RC_OK);
    for (int clear = 0; clear < 2; ++clear) {
        CHECK(rc_engine_set_output_resample(e, clear ? 0 : 5, clear ? 0 : 5) == RC_OK);
        std::vector<unsigned char> a(std::max<size_t>(n * ch * 2, 1), 0x11), b(a);
        std::vector<RcStubFadeLaunch> fa;
        std::vector<RcStubDitherLaunch> da;
        size_t got = 0;
        uint64_t clipped = 0;
        reset_logs();
        CHECK(rc_engine_stretch_frames_pcm(e, in.data(), L, RC_PCM_I16, a.data(), n, RC_PCM_I16, &got, &clipped) == RC_OK && got == n);
        CHECK(rc_stub_resample_launches == 0);
        fa.assign(rc_stub_fade_log, rc_stub_fade_log + rc_stub_fade_launches);
        da.assign(rc_stub_dither_log, rc_stub_dither_log + rc_stub_dither_launches);
        reset_logs();
        CHECK(rc_engine_stretch_frames_pcm(fresh, in.data(), L, RC_PCM_I16, b.data(), n, RC_PCM_I16, &got, &clipped) == RC_OK && got == n);
        CHECK(fa.size() == rc_stub_fade_launches && da.size() == rc_stub_dither_launches && a == b);
        for (size_t k = 0; k < fa.size(); ++k)
            CHECK(fa[k].t0 == rc_stub_fade_log[k].t0 && fa[k].t1 == rc_stub_fade_log[k].t1 && fa[k].stride == rc_stub_fade_log[k].stride);
        for (size_t k = 0; k < da.size(); ++k) CHECK(da[k].t0 == rc_stub_dither_log[k].t0 && da[k].n_frames == rc_stub_dither_log[k].n_frames);
    }
    rc_engine_destroy(fresh);
    rc_engine_destroy(e);
}

int main() {
    // several pipeline chunks (9.6 M row frames per channel, 4 M per staging slot) under steps on both sides of 1
    job(1024, 8.0f, 1, 3, 1200001, 160, 147, false);
    job(1024, 8.0f, 1, 2, 1200001, 2, 3, false);
    job(1024, 8.0f, -3, 1, 1200001, 1069, 1009, false);  // window_out_len 1023: chunk edges at no multiple of anything
    job(1024, 8.0f, 1, 1, 1200001, 8, 1, false);
    job(1024, 8.0f, 1, 1, 600001, 1, 8, false);
    job(1024, 2.0f, 1, 2, 30001, 3, 2, false);
    job(1024, 2.0f, 1, 2, 30001, 147, 160, true);  // a host frequency kernel: the whole-job order, one launch
    job(256, 2.0f, 1, 67, 3000, 6, 4, false);      // beyond the frames-only tile; a step the setter reduces
    for (size_t L : {(size_t)0, (size_t)1, (size_t)40}) {  // jobs of no frames and shorter than the filter
        job(1024, 2.0f, 1, 2, L, 160, 147, false);
        job(1024, 2.0f, 1, 1, L, 2, 3, true);
    }
    printf("engine_host_driver_frames_resample: ok\n");
    return 0;
}
