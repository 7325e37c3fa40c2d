// TEST INFRASTRUCTURE: rc_engine_set_output_limiter over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory,
// streams run at enqueue time, the hop kernels compute nothing; tests/c/hip_stub_frames_limit.cpp: the limit launcher logs
// its launch, refuses what the real one refuses, reads every frame of its halo and writes a mark over its range) under
// ASan + UBSan (rocoder_amd/csrc/host/sanitize.mk: engine_frames_limit_asan). What runs for real is the engine's
// bookkeeping: the lag of the stage behind the pipeline's chunks, alone and behind the resampler's, the pointers and strides
// of the launches, the ranges of the fade in front of it and of the peak, pack and download behind it. Held to, on
// multi-chunk jobs with and without a resample step and a fade, on all four whole-job host-form entries:
//   1. the limit launches tile [0, n) exactly once, in order,
//   2. none reads an input frame its chunk has not finished (the stub refuses such a range as the real launcher does),
//   3. none waits longer than 2 L frames,
//   4. the fade launches precede the limit launch that reads their frames,
//   5. the peak, pack and download ranges are the limit launches' ranges,
//   6. a rejected setter leaves the previous state,
//   7. with the state cleared, the logged operations and the bytes equal those of an engine that never set a limiter.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rocoder_hip.h"

struct RcStubLimitLaunch {  // tests/c/hip_stub_frames_limit.cpp
    uint64_t t0, t1, src0, src_len, n, stride, dst_stride;
    uint32_t L, channels;
    float drive, ceiling;
    uintptr_t src_row0, dst_row0;
    float in_first, in_last;
};
extern RcStubLimitLaunch rc_stub_limit_log[256];
extern uint32_t rc_stub_limit_launches, rc_stub_limit_refused;
extern float rc_stub_limit_mark;
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

static void reset_logs() {
    rc_stub_limit_launches = rc_stub_limit_refused = rc_stub_resample_launches = rc_stub_fade_launches = 0;
    rc_stub_dither_launches = rc_stub_peak_samples = 0;
}

static const float kDrive = 1.5f, kCeiling = 0.75f;

// 1., 2. and 3. on the log of one run over the chunks of a job of n frames of the limiter's input
static void check_limit_log(uint32_t L, uint64_t n, uint32_t C, bool whole_job) {
    CHECK(rc_stub_limit_launches <= 256 && rc_stub_limit_refused == 0);
    CHECK((rc_stub_limit_launches != 0) == (n != 0));
    if (whole_job && n) CHECK(rc_stub_limit_launches == 1);
    uint64_t at = 0, finished = 0;
    for (uint32_t k = 0; k < rc_stub_limit_launches; ++k) {
        const RcStubLimitLaunch &l = rc_stub_limit_log[k];
        CHECK(l.t0 == at && l.t1 > l.t0 && l.t1 <= n);
        CHECK(l.L == L && l.channels == C && l.n == n && l.drive == kDrive && l.ceiling == kCeiling);
        CHECK(l.src0 == 0 && l.src_len <= n && l.src_len >= finished);
        CHECK(l.stride == std::max<uint64_t>(n, 1) && l.dst_stride == std::max<uint64_t>(n, 1));
        CHECK(l.src_row0 == rc_stub_limit_log[0].src_row0 && l.dst_row0 == rc_stub_limit_log[0].dst_row0 && l.src_row0 != l.dst_row0);
        // the halo of the range lies in what the chunk has finished, or behind the job's end
        CHECK(std::min<uint64_t>(l.t1 + 2 * (uint64_t)L, n) <= l.src_len);
        // and the launch did not wait: the next frame's halo needs a frame that is not there yet
        if (l.src_len < n) CHECK(l.t1 + 2 * (uint64_t)L == l.src_len);
        else CHECK(l.t1 == n);
        finished = l.src_len;
        at = l.t1;
    }
    CHECK(at == n);
}

// one engine, one input, all four entries under the limiter, with the resample step num / den where num != den
static void job(uint32_t N, float f, int32_t pitch, uint32_t ch, size_t len, uint32_t L, uint32_t num, uint32_t den, bool host_kernel) {
    rc_config cfg = config(N, f, pitch, ch);
    if (host_kernel) cfg.kernel = ok_kernel;
    rc_engine *e = nullptr, *fresh = nullptr;
    CHECK(rc_engine_create(&cfg, &e) == RC_OK && rc_engine_create(&cfg, &fresh) == RC_OK);
    const bool rs = num != den;
    const size_t n_rows = rc_offline_output_len(&cfg, len), n = rs ? rc_resample_len(n_rows, num, den) : n_rows;
    std::vector<int16_t> in(std::max<size_t>(len * ch, 1), 0);
    const float kSentinel = -7.0f;
    float g = -1.0f;
    uint64_t lf = 99;
    CHECK(rc_engine_last_limiter_stats(e, &g, &lf) == RC_OK && g == 1.0f && lf == 0);  // no such call has run
    CHECK(rc_engine_set_output_resample(e, num, den) == RC_OK);
    CHECK(rc_engine_set_output_limiter(e, kDrive, kCeiling, L) == RC_OK);

    // --- rc_engine_stretch_frames, a fade-in over the whole job: every input frame of the limiter is faded once in front of
    // the launch that reads it, every output frame limited once, packed and downloaded
    CHECK(rc_engine_set_output_fade(e, n, RC_FADE_NONE, 0) == RC_OK);
    {
        std::vector<float> out((n + 3) * ch, kSentinel);
        size_t got = 99;
        reset_logs();
        if (n) {
            CHECK(rc_engine_stretch_frames(e, in.data(), len, RC_PCM_I16, out.data(), n - 1, &got) == RC_ECAPACITY);
            CHECK(rc_stub_limit_launches == 0 && got == 99 && out[0] == kSentinel);
        }
        CHECK(rc_engine_stretch_frames(e, in.data(), len, RC_PCM_I16, out.data(), n + 3, &got) == RC_OK && got == n);
        check_limit_log(L, n, ch, host_kernel);
        if (!host_kernel && n > ((size_t)4 << 20)) CHECK(rc_stub_limit_launches >= 2);  // (more than a staging slot: chunks)
        // 4. a chunk's fade launch covers the frames its limit launch newly reads, on the limiter's input rows, and ran first:
        // the first and the last frame of the halo hold the fade's mark when the limit launch reads them
        uint64_t faded = 0;
        uint32_t fk = 0;
        for (uint32_t k = 0; k < rc_stub_limit_launches; ++k) {
            const RcStubLimitLaunch &ll = rc_stub_limit_log[k];
            while (fk < rc_stub_fade_launches && faded < ll.src_len) {
                const RcStubFadeLaunch &fl = rc_stub_fade_log[fk++];
                CHECK(fl.t0 == faded && fl.stride == ll.stride && fl.row0 == ll.src_row0 && fl.channels == ch);
                faded = fl.t1;
            }
            CHECK(faded == ll.src_len);
            CHECK(ll.in_first == rc_stub_fade_mark && ll.in_last == rc_stub_fade_mark);
        }
        CHECK(fk == rc_stub_fade_launches && faded == n);
        if (rs) {  // both lags: a chunk's limit launch reads what its resample launch produced, no more
            uint64_t made = 0;
            uint32_t rk = 0;
            for (uint32_t k = 0; k < rc_stub_limit_launches; ++k) {
                while (rk < rc_stub_resample_launches && made < rc_stub_limit_log[k].src_len) made = rc_stub_resample_log[rk++].m1;
                CHECK(made == rc_stub_limit_log[k].src_len && rc_stub_resample_log[0].dst_row0 == rc_stub_limit_log[k].src_row0);
            }
        } else
            CHECK(rc_stub_resample_launches == 0);
        // 5. the download: every frame of the output is the limit launcher's mark
        for (size_t i = 0; i < out.size(); ++i) CHECK(out[i] == (i < n * ch ? rc_stub_limit_mark : kSentinel));
        CHECK(rc_engine_last_limiter_stats(e, &g, &lf) == RC_OK && g == 1.0f && lf == n);  // (the stub counts every frame)
        CHECK(rc_engine_last_limiter_stats(e, nullptr, nullptr) == RC_OK);
    }
    CHECK(rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 0) == RC_OK);

    // --- rc_engine_stretch_host: rows of n limited frames, each the limit launcher's mark
    {
        std::vector<std::vector<float>> xin(ch, std::vector<float>(std::max<size_t>(len, 1), 0.0f)), rows(ch, std::vector<float>(n + 2, kSentinel));
        std::vector<const float *> ip(ch);
        std::vector<float *> op(ch);
        for (uint32_t c = 0; c < ch; ++c) ip[c] = xin[c].data(), op[c] = rows[c].data();
        size_t got = 99;
        reset_logs();
        CHECK(rc_engine_stretch_host(e, ip.data(), len, op.data(), n + 2, &got) == RC_OK && got == n);
        check_limit_log(L, n, ch, host_kernel);
        CHECK(rc_stub_fade_launches == 0);
        for (uint32_t c = 0; c < ch; ++c)
            for (size_t i = 0; i < n + 2; ++i) CHECK(rows[c][i] == (i < n ? rc_stub_limit_mark : kSentinel));
        CHECK(rc_engine_last_limiter_stats(e, &g, &lf) == RC_OK && lf == n);  // (reset in front of the job: not 2 n)
        if (n) CHECK(rc_engine_stretch_host(e, ip.data(), len, op.data(), n - 1, &got) == RC_ECAPACITY);
    }

    // --- _pcm and _norm with a dither: the peak covers the limited frames, the pack launches are the limit launches' ranges
    CHECK(rc_engine_set_output_dither(e, RC_DITHER_TPDF, 3) == RC_OK);
    for (int norm = 0; norm < 2; ++norm) {
        std::vector<unsigned char> out((n + 2) * ch * 2 + 1, 0x11);
        size_t got = 99;
        uint64_t clipped = 99;
        float peak = -1.0f, gain = -1.0f;
        reset_logs();
        if (norm)
            CHECK(rc_engine_stretch_frames_norm(e, in.data(), len, RC_PCM_I16, out.data() + 1, n, RC_PCM_I16, 0.5f, &got, &peak, &gain, &clipped) == RC_OK);
        else
            CHECK(rc_engine_stretch_frames_pcm(e, in.data(), len, RC_PCM_I16, out.data() + 1, n, RC_PCM_I16, &got, &clipped) == RC_OK);
        CHECK(got == n);
        check_limit_log(L, n, ch, host_kernel);  // (the normalised job limits in its first run only)
        if (norm) CHECK(rc_stub_peak_samples == n * ch);
        uint64_t at = 0;
        std::vector<std::pair<uint64_t, uint64_t>> packs;
        for (uint64_t k = 0; k < rc_stub_dither_launches; ++k) {
            const RcStubDitherLaunch &l = rc_stub_dither_log[k];
            CHECK(l.t0 == at && l.channel0 == 0 && l.channels == ch && l.n_frames != 0);
            packs.push_back({l.t0, l.t0 + l.n_frames});
            at += l.n_frames;
        }
        CHECK(at == n && packs.size() == rc_stub_limit_launches);
        for (size_t k = 0; k < packs.size(); ++k) CHECK(packs[k].first == rc_stub_limit_log[k].t0 && packs[k].second == rc_stub_limit_log[k].t1);
        CHECK(out[0] == 0x11);
        for (size_t i = 1 + n * ch * 2; i < out.size(); ++i) CHECK(out[i] == 0x11);
        CHECK(rc_engine_last_limiter_stats(e, &g, &lf) == RC_OK && lf == n);
    }

    // --- 6. setter errors leave the state
    CHECK(rc_engine_set_output_limiter(nullptr, 1.0f, 1.0f, 0) == RC_EINVAL && rc_engine_last_limiter_stats(nullptr, &g, &lf) == RC_EINVAL);
    CHECK(rc_engine_set_output_limiter(e, 0.0f, 1.0f, 0) == RC_EINVAL && rc_engine_set_output_limiter(e, -1.0f, 1.0f, 0) == RC_EINVAL);
    CHECK(rc_engine_set_output_limiter(e, NAN, 1.0f, 0) == RC_EINVAL && rc_engine_set_output_limiter(e, INFINITY, 1.0f, 0) == RC_EINVAL);
    CHECK(rc_engine_set_output_limiter(e, 1.0f, -1.0f, 0) == RC_EINVAL && rc_engine_set_output_limiter(e, 1.0f, NAN, 0) == RC_EINVAL);
    CHECK(rc_engine_set_output_limiter(e, 1.0f, INFINITY, 0) == RC_EINVAL);
    CHECK(rc_engine_set_output_limiter(e, 1.0f, 1.0f, RC_LIMITER_MAX_LOOKAHEAD + 1) == RC_EINVAL);
    {
        std::vector<float> out(std::max<size_t>(n * ch, 1));
        size_t got = 0;
        reset_logs();
        CHECK(rc_engine_stretch_frames(e, in.data(), len, RC_PCM_I16, out.data(), n, &got) == RC_OK && got == n);
        check_limit_log(L, n, ch, host_kernel);
    }

    // --- 7. cleared (whatever the other arguments are), the job is that of an engine that never set a limiter
    CHECK(rc_engine_set_output_resample(e, 0, 0) == RC_OK);
    CHECK(rc_engine_set_output_fade(e, std::min<size_t>(n_rows, 100), RC_FADE_NONE, 0) == RC_OK);
    CHECK(rc_engine_set_output_fade(fresh, std::min<size_t>(n_rows, 100), RC_FADE_NONE, 0) == RC_OK);
    CHECK(rc_engine_set_output_dither(fresh, RC_DITHER_TPDF, 3) == RC_OK);
    CHECK(rc_engine_set_output_limiter(e, NAN, 0.0f, 99999) == RC_OK);
    {
        std::vector<unsigned char> a(std::max<size_t>(n_rows * ch * 2, 1), 0x11), b(a);
        std::vector<RcStubFadeLaunch> fa;
        std::vector<RcStubDitherLaunch> da;
        size_t got = 0;
        uint64_t clipped = 0;
        reset_logs();
        CHECK(rc_engine_stretch_frames_pcm(e, in.data(), len, RC_PCM_I16, a.data(), n_rows, RC_PCM_I16, &got, &clipped) == RC_OK && got == n_rows);
        CHECK(rc_stub_limit_launches == 0);
        fa.assign(rc_stub_fade_log, rc_stub_fade_log + rc_stub_fade_launches);
        da.assign(rc_stub_dither_log, rc_stub_dither_log + rc_stub_dither_launches);
        reset_logs();
        CHECK(rc_engine_stretch_frames_pcm(fresh, in.data(), len, RC_PCM_I16, b.data(), n_rows, RC_PCM_I16, &got, &clipped) == RC_OK && got == n_rows);
        CHECK(fa.size() == rc_stub_fade_launches && da.size() == rc_stub_dither_launches && a == b);
        for (size_t k = 0; k < fa.size(); ++k)
            CHECK(fa[k].t0 == rc_stub_fade_log[k].t0 && fa[k].t1 == rc_stub_fade_log[k].t1 && fa[k].stride == rc_stub_fade_log[k].stride);
        for (size_t k = 0; k < da.size(); ++k) CHECK(da[k].t0 == rc_stub_dither_log[k].t0 && da[k].n_frames == rc_stub_dither_log[k].n_frames);
    }
    rc_engine_destroy(fresh);
    rc_engine_destroy(e);
}

int main() {
    // several pipeline chunks (9.6 M row frames per channel, 4 M per staging slot), without and with a resample step
    job(1024, 8.0f, 1, 3, 1200001, 2048, 1, 1, false);
    job(1024, 8.0f, 1, 2, 1200001, 64, 3, 2, false);
    job(1024, 8.0f, -3, 1, 1200001, 2048, 147, 160, false);  // window_out_len 1023: chunk edges at no multiple of anything
    job(1024, 8.0f, 1, 1, 1200001, 0, 1, 1, false);          // no look-ahead: no lag
    job(1024, 2.0f, 1, 2, 30001, 5, 1, 1, false);
    job(1024, 2.0f, 1, 2, 30001, 700, 160, 147, true);  // a host frequency kernel: the whole-job order, one launch
    job(256, 2.0f, 1, 67, 3000, 2048, 1, 1, false);      // beyond the frames-only tile; a job shorter than the halo
    for (size_t len : {(size_t)0, (size_t)1, (size_t)40}) {  // the shortest jobs
        job(1024, 2.0f, 1, 2, len, 2048, 1, 1, false);
        job(1024, 2.0f, 1, 1, len, 7, 2, 3, true);
    }
    printf("engine_host_driver_frames_limit: ok\n");
    return 0;
}
