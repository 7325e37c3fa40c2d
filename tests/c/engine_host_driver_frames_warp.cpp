// TEST INFRASTRUCTURE: rc_engine_set_output_warp over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory,
// streams run at enqueue time, the hop kernels compute nothing; tests/c/hip_stub_frames_warp.cpp: the warp launcher logs its
// launch, holds the device anchors to the host's, reads every tap it may and writes a mark over its range) under ASan + UBSan
// and under TSan (rocoder_amd/csrc/host/sanitize.mk: engine_frames_warp_asan / _tsan). What runs for real is the engine's
// bookkeeping: the block-wise lag of the stage behind the pipeline's chunks, the pointers and strides of the launches, the
// ranges of the fade, pack and download behind it. Held to, on all four whole-job host-form entries:
//   1. the ranges of a job tile [0, n_out) exactly once, in order,
//   2. no launch reads a row frame its chunk has not finished, and none waits for a frame it does not need: its end is
//      64 times the leading blocks whose need[] - recomputed here - lies inside what is finished,
//   3. a tier that drops between two blocks at a chunk's edge holds the later blocks back (need[] is a prefix maximum):
//      the first launch of that job ends at a block written out by hand,
//   4. the fade, pack and download ranges are the warp launches' ranges,
//   5. the setter's validation, and with the state cleared the logged operations and the bytes of an engine that never set it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rocoder_hip.h"

struct RcStubWarpLaunch {  // tests/c/hip_stub_frames_warp.cpp
    uint64_t m0, m1, src0, src_len, n, stride, dst_stride, n_anchors, hi;
    uint32_t channels, tiers;
    uintptr_t src_row0, dst_row0;
};
extern RcStubWarpLaunch rc_stub_warp_log[256];
extern uint32_t rc_stub_warp_launches;
extern float rc_stub_warp_mark;
struct RcStubResampleLaunch;  // tests/c/hip_stub_frames_resample.cpp
extern uint32_t rc_stub_resample_launches;
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

static const int64_t kD[RC_WARP_TIERS] = {RC_WARP_D_LIST};
static const uint64_t kW[RC_WARP_TIERS] = {RC_WARP_W_LIST};
static const int64_t kOne = (int64_t)1 << 32;  // one row frame

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
    rc_stub_warp_launches = rc_stub_fade_launches = rc_stub_resample_launches = 0, rc_stub_dither_launches = rc_stub_peak_samples = 0;
}

// need[b], written out again: the prefix maximum of (P(frame 63 of b') >> 32) + W[t_b'] + 1
static std::vector<uint64_t> need_of(const std::vector<int64_t> &a) {
    std::vector<uint64_t> need(a.size() - 1);
    uint64_t reach = 0;
    for (size_t b = 0; b + 1 < a.size(); ++b) {
        const int64_t D = a[b + 1] - a[b];
        uint32_t t = 0;
        while (D > kD[t]) ++t;
        reach = std::max<uint64_t>(reach, (uint64_t)((a[b] + ((D * 63) >> 6)) >> 32) + kW[t] + 1);
        need[b] = reach;
    }
    return need;
}

// 1. and 2. on the log of one run over the chunks of a job of n row frames
static void check_warp_log(const std::vector<int64_t> &a, uint64_t n, uint64_t n_out, uint32_t C, bool whole_job) {
    CHECK(rc_stub_warp_launches <= 256 && rc_stub_resample_launches == 0);
    CHECK((rc_stub_warp_launches != 0) == (n_out != 0));
    if (whole_job && n_out) CHECK(rc_stub_warp_launches == 1);
    const std::vector<uint64_t> need = need_of(a);
    uint64_t at = 0, finished = 0;
    for (uint32_t k = 0; k < rc_stub_warp_launches; ++k) {
        const RcStubWarpLaunch &l = rc_stub_warp_log[k];
        CHECK(l.m0 == at && l.m1 > l.m0 && l.m1 <= n_out);
        CHECK(l.channels == C && l.n == n && l.n_anchors == a.size());
        CHECK(l.src0 == 0 && l.src_len <= n && l.src_len >= finished);
        CHECK(l.stride == std::max<uint64_t>(n, 1) && l.dst_stride == std::max<uint64_t>(n_out, 1));
        CHECK(l.src_row0 == rc_stub_warp_log[0].src_row0 && l.dst_row0 == rc_stub_warp_log[0].dst_row0);
        // the last tap of the range lies in what the chunk has finished, or behind the job's end (zeros)
        CHECK(l.hi <= l.src_len || l.src_len == n);
        // and the launch ends at the block the lag names: the leading blocks with need[b] <= src_len
        if (l.src_len < n) {
            uint64_t blocks = 0;
            while (blocks < need.size() && need[blocks] <= l.src_len) ++blocks;
            CHECK(l.m1 == std::min<uint64_t>(n_out, 64 * blocks));
        } else
            CHECK(l.m1 == n_out);
        finished = l.src_len;
        at = l.m1;
    }
    CHECK(at == n_out);
}

// the anchors of a curve over the engine's grid, by the two-call idiom
static std::vector<int64_t> curve(const rc_config &cfg, size_t L, size_t n, std::vector<double> at, std::vector<double> ratio, size_t *n_out) {
    rc_params par;
    CHECK(rc_derive_params(&cfg, &par) == RC_OK);
    const size_t n_hops = std::max<size_t>(1, n / par.window_out_len * par.hops_per_window);
    size_t A = 0, got = 0;
    (void)L;
    CHECK(rc_warp_curve(&cfg, nullptr, n_hops, at.data(), ratio.data(), at.size(), n, nullptr, 0, &A, n_out) == (A ? RC_ECAPACITY : RC_OK));
    CHECK(A >= 1);
    std::vector<int64_t> a(A, -1);
    if (A > 1) CHECK(rc_warp_curve(&cfg, nullptr, n_hops, at.data(), ratio.data(), at.size(), n, a.data(), A - 1, &got, n_out) == RC_ECAPACITY && a[0] == -1);
    CHECK(rc_warp_curve(&cfg, nullptr, n_hops, at.data(), ratio.data(), at.size(), n, a.data(), A, &got, n_out) == RC_OK && got == A);
    CHECK(a[0] == 0 && (uint64_t)(a[A - 1] >> 32) >= n && *n_out <= 64 * (A - 1));
    return a;
}

// one engine, one input, all four entries under the warp `a`
static void job(const rc_config &cfg, size_t L, const std::vector<int64_t> &a, size_t n_out, int64_t first_m1) {
    const bool host_kernel = cfg.kernel != nullptr;
    const uint32_t ch = cfg.channels;
    rc_engine *e = nullptr, *fresh = nullptr;
    CHECK(rc_engine_create(&cfg, &e) == RC_OK && rc_engine_create(&cfg, &fresh) == RC_OK);
    const size_t n = rc_offline_output_len(&cfg, L);
    std::vector<int16_t> in(std::max<size_t>(L * ch, 1), 0);
    const float kSentinel = -7.0f;
    CHECK(rc_engine_set_output_warp(e, a.data(), a.size(), n_out) == RC_OK);

    // --- rc_engine_stretch_frames, a fade-in over the whole warped job: every frame is faded once, packed and downloaded
    CHECK(rc_engine_set_output_fade(e, n_out, RC_FADE_NONE, 0) == RC_OK);
    {
        std::vector<float> out((n_out + 3) * ch, kSentinel);
        size_t got = 99;
        reset_logs();
        if (n_out) {
            CHECK(rc_engine_stretch_frames(e, in.data(), L, RC_PCM_I16, out.data(), n_out - 1, &got) == RC_ECAPACITY);
            CHECK(rc_stub_warp_launches == 0 && got == 99 && out[0] == kSentinel);
        }
        CHECK(rc_engine_stretch_frames(e, in.data(), L, RC_PCM_I16, out.data(), n_out + 3, &got) == RC_OK && got == n_out);
        check_warp_log(a, n, n_out, ch, host_kernel);
        if (!host_kernel && n > ((size_t)4 << 20)) CHECK(rc_stub_warp_launches >= 2);  // (more than a staging slot: chunks)
        if (first_m1 >= 0) CHECK(rc_stub_warp_log[0].m1 == (uint64_t)first_m1);         // 3.
        // 4. the fade launches are the warp launches' ranges, on the warped rows
        CHECK(rc_stub_fade_launches == rc_stub_warp_launches);
        for (uint32_t k = 0; k < rc_stub_fade_launches; ++k) {
            const RcStubFadeLaunch &fl = rc_stub_fade_log[k];
            const RcStubWarpLaunch &wl = rc_stub_warp_log[k];
            CHECK(fl.t0 == wl.m0 && fl.t1 == wl.m1 && fl.stride == wl.dst_stride && fl.row0 == wl.dst_row0 && fl.channels == ch);
        }
        for (size_t i = 0; i < out.size(); ++i) CHECK(out[i] == (i < n_out * ch ? rc_stub_fade_mark : kSentinel));
        // a fade beyond n_out
        CHECK(rc_engine_set_output_fade(e, n_out + 1, RC_FADE_NONE, 0) == RC_OK);
        reset_logs();
        CHECK(rc_engine_stretch_frames(e, in.data(), L, RC_PCM_I16, out.data(), n_out + 3, &got) == RC_EINVAL);
        CHECK(rc_stub_warp_launches == 0);
    }
    CHECK(rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 0) == RC_OK);

    // --- rc_engine_stretch_host: rows of n_out warped frames, each the warp launcher's mark
    {
        std::vector<std::vector<float>> xin(ch, std::vector<float>(std::max<size_t>(L, 1), 0.0f)), rows(ch, std::vector<float>(n_out + 2, kSentinel));
        std::vector<const float *> ip(ch);
        std::vector<float *> op(ch);
        for (uint32_t c = 0; c < ch; ++c) ip[c] = xin[c].data(), op[c] = rows[c].data();
        size_t got = 99;
        reset_logs();
        CHECK(rc_engine_stretch_host(e, ip.data(), L, op.data(), n_out + 2, &got) == RC_OK && got == n_out);
        check_warp_log(a, n, n_out, ch, host_kernel);
        for (uint32_t c = 0; c < ch; ++c)
            for (size_t i = 0; i < n_out + 2; ++i) CHECK(rows[c][i] == (i < n_out ? rc_stub_warp_mark : kSentinel));
        if (n_out) CHECK(rc_engine_stretch_host(e, ip.data(), L, op.data(), n_out - 1, &got) == RC_ECAPACITY);
    }

    // --- _pcm and _norm with a dither: the pack launches count warped frames and tile [0, n_out)
    CHECK(rc_engine_set_output_dither(e, RC_DITHER_TPDF, 3) == RC_OK);
    for (int norm = 0; norm < 2; ++norm) {
        std::vector<unsigned char> out((n_out + 2) * ch * 2 + 1, 0x11);
        size_t got = 99;
        uint64_t clipped = 99;
        float peak = -1.0f, gain = -1.0f;
        reset_logs();
        if (norm)
            CHECK(rc_engine_stretch_frames_norm(e, in.data(), L, RC_PCM_I16, out.data() + 1, n_out, RC_PCM_I16, 0.5f, &got, &peak, &gain, &clipped) == RC_OK);
        else
            CHECK(rc_engine_stretch_frames_pcm(e, in.data(), L, RC_PCM_I16, out.data() + 1, n_out, RC_PCM_I16, &got, &clipped) == RC_OK);
        CHECK(got == n_out);
        check_warp_log(a, n, n_out, ch, host_kernel);  // (the normalised job warps in its first run only)
        if (norm) CHECK(rc_stub_peak_samples == n_out * ch);
        uint64_t at = 0;
        CHECK(rc_stub_dither_launches == rc_stub_warp_launches);
        for (uint64_t k = 0; k < rc_stub_dither_launches; ++k) {
            const RcStubDitherLaunch &l = rc_stub_dither_log[k];
            CHECK(l.t0 == at && l.channel0 == 0 && l.channels == ch && l.n_frames != 0);
            CHECK(l.t0 == rc_stub_warp_log[k].m0 && l.t0 + l.n_frames == rc_stub_warp_log[k].m1);
            at += l.n_frames;
        }
        CHECK(at == n_out && out[0] == 0x11);
        for (size_t i = 1 + n_out * ch * 2; i < out.size(); ++i) CHECK(out[i] == 0x11);
    }

    // --- the setter's validation: each refusal leaves the warp as it is
    {
        std::vector<int64_t> bad;
        CHECK(rc_engine_set_output_warp(nullptr, a.data(), a.size(), n_out) == RC_EINVAL);
        CHECK(rc_engine_set_output_warp(e, a.data(), 1, 0) == RC_EINVAL);
        CHECK(rc_engine_set_output_warp(e, a.data(), a.size(), 64 * (a.size() - 1) + 1) == RC_EINVAL);
        bad = a, bad[0] = -1;
        CHECK(rc_engine_set_output_warp(e, bad.data(), bad.size(), n_out) == RC_EINVAL);
        bad = a, bad.back() = (int64_t)1 << 62;
        CHECK(rc_engine_set_output_warp(e, bad.data(), bad.size(), n_out) == RC_EINVAL);
        for (int64_t d : {((int64_t)1 << 35) - 1, ((int64_t)1 << 41) + 1, (int64_t)0, (int64_t)-9}) {
            bad = {0, kOne * 64, kOne * 64 + d, kOne * 64 + d + kOne * 64};
            CHECK(rc_engine_set_output_warp(e, bad.data(), bad.size(), 1) == RC_EINVAL);
        }
        CHECK(rc_engine_set_output_resample(e, 3, 2) == RC_EINVAL);  // the two are alternatives
        CHECK(rc_engine_set_output_resample(e, 0, 0) == RC_OK);
        std::vector<float> out(std::max<size_t>(n_out * ch, 1));
        size_t got = 0;
        reset_logs();
        CHECK(rc_engine_stretch_frames(e, in.data(), L, RC_PCM_I16, out.data(), n_out, &got) == RC_OK && got == n_out);
        check_warp_log(a, n, n_out, ch, host_kernel);
    }
    // the other way round: a step set refuses a warp and stays
    CHECK(rc_engine_set_output_warp(e, nullptr, 0, 0) == RC_OK && rc_engine_set_output_resample(e, 3, 2) == RC_OK);
    CHECK(rc_engine_set_output_warp(e, a.data(), a.size(), n_out) == RC_EINVAL);
    {
        const size_t n_rs = rc_resample_len(n, 3, 2);
        std::vector<float> out(std::max<size_t>(n_rs * ch, 1));
        size_t got = 0;
        reset_logs();
        CHECK(rc_engine_stretch_frames(e, in.data(), L, RC_PCM_I16, out.data(), n_rs, &got) == RC_OK && got == n_rs);
        CHECK(rc_stub_warp_launches == 0 && (rc_stub_resample_launches != 0) == (n_rs != 0));
    }
    CHECK(rc_engine_set_output_resample(e, 0, 0) == RC_OK && rc_engine_set_output_warp(e, a.data(), a.size(), n_out) == RC_OK);

    // --- cleared, the job is that of an engine that never set it
    CHECK(rc_engine_set_output_warp(e, a.data(), 0, 0) == RC_OK);
    CHECK(rc_engine_set_output_fade(e, std::min<size_t>(n, 100), RC_FADE_NONE, 0) == RC_OK);
    CHECK(rc_engine_set_output_fade(fresh, std::min<size_t>(n, 100), RC_FADE_NONE, 0) == RC_OK);
    CHECK(rc_engine_set_output_dither(fresh, RC_DITHER_TPDF, 3) == RC_OK);
    {
        std::vector<unsigned char> x(std::max<size_t>(n * ch * 2, 1), 0x11), y(x);
        std::vector<RcStubFadeLaunch> fa;
        std::vector<RcStubDitherLaunch> da;
        size_t got = 0;
        uint64_t clipped = 0;
        reset_logs();
        CHECK(rc_engine_stretch_frames_pcm(e, in.data(), L, RC_PCM_I16, x.data(), n, RC_PCM_I16, &got, &clipped) == RC_OK && got == n);
        CHECK(rc_stub_warp_launches == 0 && rc_stub_resample_launches == 0);
        fa.assign(rc_stub_fade_log, rc_stub_fade_log + rc_stub_fade_launches);
        da.assign(rc_stub_dither_log, rc_stub_dither_log + rc_stub_dither_launches);
        reset_logs();
        CHECK(rc_engine_stretch_frames_pcm(fresh, in.data(), L, RC_PCM_I16, y.data(), n, RC_PCM_I16, &got, &clipped) == RC_OK && got == n);
        CHECK(fa.size() == rc_stub_fade_launches && da.size() == rc_stub_dither_launches && x == y);
        for (size_t k = 0; k < fa.size(); ++k)
            CHECK(fa[k].t0 == rc_stub_fade_log[k].t0 && fa[k].t1 == rc_stub_fade_log[k].t1 && fa[k].stride == rc_stub_fade_log[k].stride);
        for (size_t k = 0; k < da.size(); ++k) CHECK(da[k].t0 == rc_stub_dither_log[k].t0 && da[k].n_frames == rc_stub_dither_log[k].n_frames);
    }
    rc_engine_destroy(fresh);
    rc_engine_destroy(e);
}

static void curve_job(uint32_t N, float f, int32_t pitch, uint32_t ch, size_t L, std::vector<double> at, std::vector<double> ratio, bool host_kernel) {
    rc_config cfg = config(N, f, pitch, ch);
    if (host_kernel) cfg.kernel = ok_kernel;
    const size_t n = rc_offline_output_len(&cfg, L);
    size_t n_out = 0;
    const std::vector<int64_t> a = curve(cfg, L, n, at, ratio, &n_out);
    if (a.size() < 2) {  // a job of no rows: one anchor, nothing to set - a warp of one block of no frames stands in
        CHECK(n == 0 && n_out == 0);
        return job(cfg, L, {0, kOne * 64}, 0, -1);
    }
    job(cfg, L, a, n_out, -1);
}

int main() {
    // need[] by hand: a block at a step of 8 (tier 12, W = 256) in front of blocks at a step of 1/8 (tier 0, W = 32)
    {
        const std::vector<uint64_t> need = need_of({0, kOne * 512, kOne * 520, kOne * 528});
        CHECK(need[0] == 504 + 256 + 1 && need[1] == 761 && need[2] == 761);  // (their own reach: 519 + 33, 527 + 33)
        const std::vector<uint64_t> up = need_of({0, kOne * 8, kOne * 16, kOne * 528});
        CHECK(up[0] == 7 + 33 && up[1] == 15 + 33 && up[2] == 16 + 504 + 257);
    }
    // 3. a tier drop at the first chunk's edge. N = 1024, f = 8: window_out_len frames a window, chunks of one staging
    // slot (4 Mi floats a channel), so the first chunk finishes o1 row frames. Blocks at a step of 1 up to o1 - 552 (a last
    // one of 8 ... 71 frames), ONE block of 512 frames - its last tap is frame o1 - 48 + 256 > o1 - and blocks of 8 frames
    // behind it: the first of them ends at tap o1 - 40 + 7 + 32 < o1, but waits for the block in front of it.
    {
        const rc_config cfg = config(1024, 8.0f, 1, 2);
        rc_params par;
        CHECK(rc_derive_params(&cfg, &par) == RC_OK);
        const size_t L = 1200001, n = rc_offline_output_len(&cfg, L);
        const uint64_t o1 = ((uint64_t)(4 << 20) / par.window_out_len) * par.window_out_len;
        CHECK(n > 2 * o1);
        std::vector<int64_t> a{0};
        const uint64_t target = o1 - 552, ones = (target - 8) / 64;
        for (uint64_t b = 0; b < ones; ++b) a.push_back(a.back() + kOne * 64);
        a.push_back(kOne * (int64_t)target);
        CHECK(a.back() - a[a.size() - 2] >= kOne * 8 && a.back() - a[a.size() - 2] < kOne * 72);
        const uint64_t big = a.size() - 1;  // the block of 512 frames
        a.push_back(a.back() + kOne * 512);
        for (int b = 0; b < 40; ++b) a.push_back(a.back() + kOne * 8);
        while ((uint64_t)(a.back() >> 32) < n) a.push_back(a.back() + kOne * 64 + 12345);  // (fractions of a frame from here on)
        const std::vector<uint64_t> need = need_of(a);
        CHECK(need[big - 1] <= o1 && need[big] == o1 - 48 + 257 && need[big + 1] == need[big]);
        CHECK((uint64_t)((a[big + 1] + ((kOne * 8 * 63) >> 6)) >> 32) + 33 <= o1);
        size_t n_out = 64 * (a.size() - 1);
        while ((uint64_t)((a[(n_out - 1) / 64] + (((a[(n_out - 1) / 64 + 1] - a[(n_out - 1) / 64]) * (int64_t)((n_out - 1) % 64)) >> 6)) >> 32) >= n) --n_out;
        job(cfg, L, a, n_out, (int64_t)(64 * big));
    }
    // several pipeline chunks under a glide up and down again: tiers rise and drop along the job
    curve_job(1024, 8.0f, 1, 3, 1200001, {0.0, 500000.0, 1200000.0}, {0.5, 2.5, 0.7}, false);
    curve_job(1024, 8.0f, -3, 1, 600001, {0.0, 600000.0}, {8.0, 0.125}, false);  // window_out_len 1023; both ends of the range
    curve_job(1024, 2.0f, 1, 2, 30001, {0.0, 30000.0}, {0.5, 2.0}, false);
    curve_job(1024, 2.0f, 1, 2, 30001, {1000.0}, {1.3}, true);   // a host frequency kernel: the whole-job order, one launch
    curve_job(256, 2.0f, 1, 67, 3000, {0.0, 3000.0}, {2.0, 0.5}, false);  // beyond the frames-only tile
    for (size_t L : {(size_t)0, (size_t)1, (size_t)40}) {        // jobs of no frames and shorter than the filter
        curve_job(1024, 2.0f, 1, 2, L, {0.0}, {1.5}, false);
        curve_job(1024, 2.0f, 1, 1, L, {0.0}, {0.75}, true);
    }
    printf("engine_host_driver_frames_warp: ok\n");
    return 0;
}
