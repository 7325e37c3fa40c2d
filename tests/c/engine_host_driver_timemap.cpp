// TEST INFRASTRUCTURE: rc_engine_set_time_map over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory,
// streams run at enqueue time, the hop kernels compute nothing; tests/c/hip_stub_timemap.cpp: the gather launcher really
// gathers on the CPU, refuses what the real one refuses and logs its launches) under ASan + UBSan and under TSan
// (rocoder_amd/csrc/host/sanitize.mk: engine_timemap_asan, engine_timemap_tsan; the engine is built with -DRC_TEST_HOOKS=1
// for rc_test_time_map_chunk_windows). What runs for real is the engine's bookkeeping: the chunks of a map job, the hops
// each chunk gathers in front of its own (the recomputed hop, a history kernel's halo), the rows and strides it hands
// on, the upload bound of the host pipeline, the refusals, and the way back to the plain launches. The expected
// launches below are written out by hand.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rocoder_hip.h"

struct RcStubTmLaunch {  // tests/c/hip_stub_timemap.cpp
    uint64_t hop_first, hop_count, in_len, in_stride, v_stride;
    uint32_t channels, N;
    uintptr_t x, v, table;
    double sum;
};
extern RcStubTmLaunch rc_stub_tm_log[256];
extern uint32_t rc_stub_tm_launches;
// tests/c/hip_stub_timemap_hops.cpp: this program is linked with --wrap, so the engine's calls of rc::launch_hop,
// rc::launch_prep and hipMemcpyAsync are logged on their way to the stub
struct RcStubHopLaunch {
    int mode;  // 0 fused, 1 forward, 2 resynthesis
    int64_t in_origin, in_len, hop_first, hop_count, tail_hop_first;
    uint64_t in_stride;
    uint32_t step, pitch, ch_first, n_channels;
    uintptr_t x;
};
struct RcStubPrepLaunch {
    uint64_t tail_len, real;
    int has_tail;
};
struct RcStubH2D {
    uintptr_t dst;
    uint64_t bytes;
};
extern RcStubHopLaunch rc_stub_hop_log[256];
extern uint32_t rc_stub_hop_launches;
extern RcStubPrepLaunch rc_stub_prep_log[256];
extern uint32_t rc_stub_prep_launches;
extern RcStubH2D rc_stub_h2d_log[1024];
extern uint32_t rc_stub_h2d_copies;
extern "C" int rc_test_time_map_chunk_windows(rc_engine *e, uint64_t n);
extern "C" int hipMalloc(void **, size_t);
extern "C" int hipFree(void *);

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

static float sample(uint32_t c, size_t i) { return (float)(c * 1000 + i + 1); }  // never 0, exact in f32

// the sum the stub forms for hops [h0, h0 + hc) of `ch` channels: the definition, on the driver's own input
static double gathered_sum(const std::vector<int64_t> &pos, uint64_t h0, uint64_t hc, uint32_t ch, uint32_t N, size_t L) {
    double s = 0.0;
    for (uint32_t c = 0; c < ch; ++c)
        for (uint64_t h = h0; h < h0 + hc; ++h)
            for (uint32_t n = 0; n < N; ++n) {
                const int64_t j = pos[h] + n;
                if (j >= 0 && j < (int64_t)L) s += (double)sample(c, (size_t)j);
            }
    return s;
}

struct Want {
    uint64_t hop_first, hop_count;
};

static void check_log(const std::vector<Want> &want, const std::vector<int64_t> &pos, uint32_t ch, uint32_t N, size_t L, bool sums = true) {
    CHECK(rc_stub_tm_launches == want.size());
    for (size_t i = 0; i < want.size(); ++i) {
        const RcStubTmLaunch &l = rc_stub_tm_log[i];
        if (l.hop_first != want[i].hop_first || l.hop_count != want[i].hop_count) {
            fprintf(stderr, "FAIL: gather %zu covers hops [%llu, +%llu), expected [%llu, +%llu)\n", i, (unsigned long long)l.hop_first,
                    (unsigned long long)l.hop_count, (unsigned long long)want[i].hop_first, (unsigned long long)want[i].hop_count);
            exit(2);
        }
        // the rows run_hops is handed: hop_count windows of N samples, a stride of exactly that, every channel
        CHECK(l.channels == ch && l.N == N && l.in_len == L && l.v_stride == l.hop_count * N);
        CHECK(l.table == rc_stub_tm_log[0].table && l.x == rc_stub_tm_log[0].x);
        if (sums) CHECK(l.sum == gathered_sum(pos, l.hop_first, l.hop_count, ch, N, L));
    }
}

// What run_hops hands the hop launchers for a chunk of a map job, typed in per launch: the mode, in_origin, in_len, the hops,
// and which gather launch wrote the rows it reads. Every launch of a map job reads those rows at a step of N and a stride of
// exactly in_len, with no padded tail: tail_hop_first INT64_MAX, and the prep launches ask for no tail copy.
struct WantHop {
    int mode;
    int64_t in_origin, in_len, hop_first, hop_count;
    uint32_t gather;
};
enum { FUSED = 0, FORWARD = 1, RESYNTH = 2 };

static void reset_logs() { rc_stub_tm_launches = rc_stub_hop_launches = rc_stub_prep_launches = rc_stub_h2d_copies = 0; }

static void check_hops(const std::vector<WantHop> &want, uint32_t ch, uint32_t N, uint32_t pitch, uint32_t preps) {
    if (rc_stub_hop_launches != want.size()) {
        fprintf(stderr, "FAIL: %u hop launches, expected %zu\n", rc_stub_hop_launches, want.size());
        exit(2);
    }
    for (size_t i = 0; i < want.size(); ++i) {
        const RcStubHopLaunch &l = rc_stub_hop_log[i];
        const WantHop &w = want[i];
        if (l.mode != w.mode || l.in_origin != w.in_origin || l.in_len != w.in_len || l.hop_first != w.hop_first || l.hop_count != w.hop_count) {
            fprintf(stderr, "FAIL: hop launch %zu is mode %d in_origin %lld in_len %lld hops [%lld, +%lld), expected %d %lld %lld [%lld, +%lld)\n", i,
                    l.mode, (long long)l.in_origin, (long long)l.in_len, (long long)l.hop_first, (long long)l.hop_count, w.mode,
                    (long long)w.in_origin, (long long)w.in_len, (long long)w.hop_first, (long long)w.hop_count);
            exit(2);
        }
        CHECK(l.step == N && l.tail_hop_first == INT64_MAX && l.in_stride == (uint64_t)l.in_len);
        CHECK(l.pitch == pitch && l.ch_first == 0 && l.n_channels == ch);
        CHECK(w.gather < rc_stub_tm_launches && l.x == rc_stub_tm_log[w.gather].v);
        // the rows are the gather's: they start at its first hop and hold its hops
        CHECK(l.in_origin == (int64_t)(rc_stub_tm_log[w.gather].hop_first * N) && l.in_len == (int64_t)(rc_stub_tm_log[w.gather].hop_count * N));
    }
    CHECK(rc_stub_prep_launches == preps);
    for (uint32_t i = 0; i < preps; ++i) CHECK(!rc_stub_prep_log[i].has_tail && rc_stub_prep_log[i].tail_len == 0);
}

// device rows of `ch` channels of L samples (stride L + 3: odd), filled with sample()
static float *device_input(uint32_t ch, size_t L, size_t *stride) {
    *stride = L + 3;
    void *p = nullptr;
    CHECK(hipMalloc(&p, ch * *stride * sizeof(float) + 4) == 0);
    float *x = (float *)p;
    for (uint32_t c = 0; c < ch; ++c)
        for (size_t i = 0; i < L; ++i) x[c * *stride + i] = sample(c, i);
    return x;
}

// ELF64 / EM_AMDGPU / gfx950 that carries what the loader's check reads: rc_user_dk, and rc_user_dk_history of hist_size bytes
static void put(std::string &b, size_t off, uint64_t v, size_t n) {
    for (size_t i = 0; i < n; ++i) b[off + i] = (char)(v >> (8 * i));
}
static std::string fake_code_object(uint64_t hist_size) {
    const std::string strtab = std::string("\0rc_user_dk\0rc_user_dk_history\0", 31);
    const size_t n_sym = 3, str_off = 64, sym_off = 96, sh_off = sym_off + 24 * 3;
    std::string b(sh_off + 3 * 64, '\0');
    memcpy(&b[0], "\x7f" "ELF", 4);
    b[4] = 2;
    b[5] = 1;
    put(b, 18, 224, 2);
    put(b, 48, 0x4f, 4);
    put(b, 40, sh_off, 8);
    put(b, 58, 64, 2);
    put(b, 60, 3, 2);
    memcpy(&b[str_off], strtab.data(), strtab.size());
    put(b, sym_off + 24, 1, 4);
    put(b, sym_off + 48, 12, 4);
    put(b, sym_off + 48 + 16, hist_size, 8);
    const size_t s1 = sh_off + 64, s2 = sh_off + 128;
    put(b, s1 + 4, 3, 4);
    put(b, s1 + 24, str_off, 8);
    put(b, s1 + 32, strtab.size(), 8);
    put(b, s2 + 4, 2, 4);
    put(b, s2 + 24, sym_off, 8);
    put(b, s2 + 32, 24 * n_sym, 8);
    put(b, s2 + 40, 1, 4);
    put(b, s2 + 56, 24, 8);
    return b;
}

int main() {
    const uint32_t N = 64, CH = 2;
    const size_t L = 300;
    rc_config c = config(N, 2.0f, 1, CH);  // hops_per_window 2, window_out_len 64
    rc_params par;
    CHECK(rc_derive_params(&c, &par) == RC_OK && par.hops_per_window == 2 && par.window_out_len == 64);
    {  // the pure host helpers
        CHECK(rc_time_map_output_len(&c, 8) == 256 && rc_time_map_output_len(&c, 7) == 0 && rc_time_map_output_len(nullptr, 8) == 0);
        // one point, f = 2: step 64 / 4 = 16 exactly; in_len 100: hops 0, 16, 32 fit, hop 3 at 48 runs out (48 + 64 > 100):
        // kd = 3, K = 2 * (3 / 2 + 1) = 4
        const double at[1] = {0.0}, fac[1] = {2.0};
        size_t K = 99;
        CHECK(rc_time_map_curve(&c, 100, at, fac, 1, nullptr, 0, &K) == RC_ECAPACITY && K == 4);
        int64_t pos[5] = {-1, -1, -1, -1, -1};
        CHECK(rc_time_map_curve(&c, 100, at, fac, 1, pos, 3, &K) == RC_ECAPACITY && K == 4 && pos[0] == -1);
        CHECK(rc_time_map_curve(&c, 100, at, fac, 1, pos, 4, &K) == RC_OK && K == 4);
        CHECK(pos[0] == 0 && pos[1] == 16 && pos[2] == 32 && pos[3] == 48 && pos[4] == -1);
        const double bad_at[2] = {5.0, 5.0}, two[2] = {2.0, 2.0}, huge[1] = {2097152.0};
        CHECK(rc_time_map_curve(&c, 100, bad_at, two, 2, nullptr, 0, &K) == RC_EINVAL);
        CHECK(rc_time_map_curve(&c, 100, at, huge, 1, nullptr, 0, &K) == RC_EINVAL);
        CHECK(rc_time_map_curve(&c, 100, at, fac, 0, nullptr, 0, &K) == RC_EINVAL);
        CHECK(rc_time_map_curve(&c, 100, at, fac, 1, nullptr, 0, nullptr) == RC_EINVAL);
    }
    size_t stride = 0;
    float *x = device_input(CH, L, &stride);
    void *outp = nullptr;
    CHECK(hipMalloc(&outp, CH * 4096 * sizeof(float)) == 0);
    float *out = (float *)outp;
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&c, &e) == RC_OK);
    {  // the setter's validation: none of it needs a device
        const int64_t ok[4] = {0, -((int64_t)1 << 48), (int64_t)1 << 48, 5}, far[2] = {0, ((int64_t)1 << 48) + 1},
                      near[2] = {-((int64_t)1 << 48) - 1, 0};
        CHECK(rc_engine_set_time_map(nullptr, ok, 4) == RC_EINVAL);
        CHECK(rc_engine_set_time_map(e, ok, 3) == RC_EINVAL);  // not a multiple of hops_per_window
        CHECK(rc_engine_set_time_map(e, far, 2) == RC_EINVAL && rc_engine_set_time_map(e, near, 2) == RC_EINVAL);
        CHECK(rc_engine_set_time_map(e, ok, 4) == RC_OK);
        CHECK(rc_engine_set_time_map(e, far, 2) == RC_EINVAL);  // the previous map stays: 4 hops, 2 windows
        size_t got = 0;
        CHECK(rc_engine_stretch_device(e, x, stride, L, out, 4096, 4096, &got, nullptr) == RC_OK && got == 128);
        CHECK(rc_engine_set_time_map(e, nullptr, 4) == RC_OK && rc_engine_set_time_map(e, ok, 0) == RC_OK);
    }
    const std::vector<int64_t> fwd = {0, 40, 80, 120, 160, 200, 240, 280};  // the last two windows end past the input
    {  // device form, chunks of one window: every chunk gathers the hop in front of it again
        CHECK(rc_engine_set_time_map(e, fwd.data(), fwd.size()) == RC_OK);
        CHECK(rc_test_time_map_chunk_windows(e, 1) == RC_OK);
        size_t got = 0;
        reset_logs();
        CHECK(rc_engine_stretch_device(e, x, stride, L, out, 4096, 4096, &got, nullptr) == RC_OK && got == 256);
        check_log({{0, 2}, {1, 3}, {3, 3}, {5, 3}}, fwd, CH, N, L);
        // one fused launch per chunk: its own two hops, on rows that start one hop earlier (none in front of hop 0)
        check_hops({{FUSED, 0, 128, 0, 2, 0}, {FUSED, 64, 192, 2, 2, 1}, {FUSED, 192, 192, 4, 2, 2}, {FUSED, 320, 192, 6, 2, 3}}, CH, N, 1, 4);
        CHECK(rc_stub_tm_log[0].in_stride == stride && rc_stub_tm_log[0].x == (uintptr_t)x);
        // chunks of three windows; then the 256 MiB bound: one chunk
        CHECK(rc_test_time_map_chunk_windows(e, 3) == RC_OK);
        rc_stub_tm_launches = 0;
        CHECK(rc_engine_stretch_device(e, x, stride, L, out, 4096, 4096, &got, nullptr) == RC_OK && got == 256);
        check_log({{0, 6}, {5, 3}}, fwd, CH, N, L);
        CHECK(rc_test_time_map_chunk_windows(e, 0) == RC_OK);
        rc_stub_tm_launches = 0;
        CHECK(rc_engine_stretch_device(e, x, stride, L, out, 4096, 4096, &got, nullptr) == RC_OK && got == 256);
        check_log({{0, 8}}, fwd, CH, N, L);
        // the capacity is the map's
        got = 77;
        rc_stub_tm_launches = 0;
        CHECK(rc_engine_stretch_device(e, x, stride, L, out, 4096, 255, &got, nullptr) == RC_ECAPACITY && got == 77 && rc_stub_tm_launches == 0);
        // no input at all is valid: silence everywhere
        CHECK(rc_engine_stretch_device(e, nullptr, 0, 0, out, 4096, 4096, &got, nullptr) == RC_OK && got == 256);
        CHECK(rc_stub_tm_launches == 1 && rc_stub_tm_log[0].sum == 0.0 && rc_stub_tm_log[0].x == 0);
    }
    {  // the refusals while a map is set: each names the map, and nothing is launched
        rc_stub_tm_launches = 0;
        float w[64];
        const float *view = nullptr;
        size_t n = 0;
        CHECK(rc_engine_stretch_device_range(e, x, stride, L, 0, CH, 0, 1, out, 4096, 4096, nullptr) == RC_EINVAL);
        CHECK(strstr(rc_last_error(), "time map") && strstr(rc_last_error(), "rc_engine_stretch_device_range"));
        CHECK(rc_engine_push_input(e, 0, w, 0) == RC_EINVAL && strstr(rc_last_error(), "time map"));
        CHECK(rc_engine_next_window(e, 0, w, 64, &n) == RC_EINVAL && strstr(rc_last_error(), "time map"));
        CHECK(rc_engine_next_window_view(e, 0, &view, &n) == RC_EINVAL && strstr(rc_last_error(), "time map") && view == nullptr);
        CHECK(rc_stub_tm_launches == 0);
    }
    {  // host-form entries: the job's length is the map's, through the one host job
        std::vector<float> rows(CH * L), res(CH * 256, 5.0f);
        std::vector<int16_t> frames(CH * L, 3);
        for (uint32_t k = 0; k < CH; ++k)
            for (size_t i = 0; i < L; ++i) rows[k * L + i] = sample(k, i);
        const float *in_rows[2] = {rows.data(), rows.data() + L};
        float *out_rows[2] = {res.data(), res.data() + 256};
        size_t got = 0;
        CHECK(rc_test_time_map_chunk_windows(e, 2) == RC_OK);
        rc_stub_tm_launches = 0;
        CHECK(rc_engine_stretch_host(e, in_rows, L, out_rows, 256, &got) == RC_OK && got == 256);
        check_log({{0, 4}, {3, 5}}, fwd, CH, N, L);  // (the whole input was up in front of the first gather: the sums)
        CHECK(rc_engine_stretch_host(e, in_rows, L, out_rows, 255, &got) == RC_ECAPACITY);
        rc_stub_tm_launches = 0;
        CHECK(rc_engine_stretch_frames(e, frames.data(), L, RC_PCM_I16, res.data(), 256, &got) == RC_OK && got == 256);
        check_log({{0, 4}, {3, 5}}, fwd, CH, N, L, false);
        uint64_t clipped = 0;
        float peak = 0.0f, gain = 0.0f, lufs = 0.0f, tp = 0.0f;
        rc_stub_tm_launches = 0;
        CHECK(rc_engine_stretch_frames_pcm(e, frames.data(), L, RC_PCM_I16, res.data(), 256, RC_PCM_I16, &got, &clipped) == RC_OK && got == 256);
        CHECK(rc_stub_tm_launches == 2);
        rc_stub_tm_launches = 0;  // two runs over the plan, the hops in the first alone
        CHECK(rc_engine_stretch_frames_norm(e, frames.data(), L, RC_PCM_I16, res.data(), 256, RC_PCM_I16, 0.5f, &got, &peak, &gain, &clipped) == RC_OK && got == 256);
        CHECK(rc_stub_tm_launches == 2);
        rc_stub_tm_launches = 0;
        CHECK(rc_engine_stretch_frames_loud(e, frames.data(), L, RC_PCM_I16, res.data(), 256, RC_PCM_I16, 0, -23.0f, 0.0f, &got, &lufs, &tp, &gain, &clipped) == RC_OK && got == 256);
        CHECK(rc_stub_tm_launches == 2);
        CHECK(rc_engine_stretch_frames(e, frames.data(), L, RC_PCM_I16, res.data(), 255, &got) == RC_ECAPACITY);
        // under the other output stages: a resample step of 3 / 2 and a fade inside the resampled length
        CHECK(rc_engine_set_output_resample(e, 3, 2) == RC_OK && rc_engine_set_output_fade(e, 10, 150, 20) == RC_OK);
        rc_stub_tm_launches = 0;
        CHECK(rc_engine_stretch_host(e, in_rows, L, out_rows, 256, &got) == RC_OK && got == rc_resample_len(256, 3, 2));
        check_log({{0, 4}, {3, 5}}, fwd, CH, N, L);
        CHECK(rc_engine_set_output_resample(e, 0, 0) == RC_OK && rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 0) == RC_OK);
    }
    {  // cleared: the plain launches again - no gather, the plain job's length, the streaming seam open
        CHECK(rc_engine_set_time_map(e, nullptr, 0) == RC_OK);
        size_t got = 0;
        reset_logs();
        CHECK(rc_engine_stretch_device(e, x, stride, L, out, 4096, 4096, &got, nullptr) == RC_OK && got == rc_offline_output_len(&c, L));
        // the plain launch again, from the caller's rows: step 64 / (2 * 2) = 16; hop 15 at 240 is the first whose window runs
        // past 300, so kd = 15, 15 / 2 + 1 = 8 windows, 16 hops; hop 15 reads the padded tail: 64 samples, 300 - 240 = 60 real
        CHECK(got == 8 * 64 && rc_stub_hop_launches == 1 && rc_stub_prep_launches == 1);
        {
            const RcStubHopLaunch &l = rc_stub_hop_log[0];
            CHECK(l.mode == FUSED && l.in_origin == 0 && l.in_len == 300 && l.hop_first == 0 && l.hop_count == 16 && l.step == 16);
            CHECK(l.x == (uintptr_t)x && l.in_stride == stride && l.tail_hop_first == 15 && l.pitch == 1 && l.n_channels == CH);
            CHECK(rc_stub_prep_log[0].has_tail && rc_stub_prep_log[0].tail_len == 64 && rc_stub_prep_log[0].real == 60);
        }
        CHECK(rc_engine_stretch_device_range(e, x, stride, L, 0, CH, 0, 1, out, 4096, 4096, nullptr) == RC_OK);
        float w[8] = {0};
        CHECK(rc_engine_push_input(e, 0, w, 8) == RC_OK);
        CHECK(rc_stub_tm_launches == 0);
    }
    rc_engine_destroy(e);
    {  // a history kernel (RC_HISTORY 3): every chunk gathers 1 + 3 hops in front of its own
        rc_engine *h = nullptr;
        CHECK(rc_engine_create(&c, &h) == RC_OK);
        const std::string code = fake_code_object(4);
        CHECK(rc_engine_load_device_kernel(h, code.data(), code.size()) == RC_OK);
        const std::vector<int64_t> pos = {250, 200, 150, 100, 50, 0, -50, -100, 0, 0, 0, 290};  // reversed, a hold, the end
        CHECK(rc_engine_set_time_map(h, pos.data(), pos.size()) == RC_OK);
        CHECK(rc_test_time_map_chunk_windows(h, 2) == RC_OK);
        size_t got = 0;
        reset_logs();
        CHECK(rc_engine_stretch_device(h, x, stride, L, out, 4096, 4096, &got, nullptr) == RC_OK && got == 384);
        check_log({{0, 4}, {0, 8}, {4, 8}}, pos, CH, N, L);
        // unfused: a forward launch that carries the halo of up to 3 hops and a resynthesis of the hops themselves. From the
        // second chunk on, the hop in front of the chunk runs first, for its tail, with a halo of its own.
        check_hops({{FORWARD, 0, 256, 0, 4, 0}, {RESYNTH, 0, 256, 0, 4, 0},
                    {FORWARD, 0, 512, 0, 4, 1}, {RESYNTH, 0, 512, 3, 1, 1}, {FORWARD, 0, 512, 1, 7, 1}, {RESYNTH, 0, 512, 4, 4, 1},
                    {FORWARD, 256, 512, 4, 4, 2}, {RESYNTH, 256, 512, 7, 1, 2}, {FORWARD, 256, 512, 5, 7, 2}, {RESYNTH, 256, 512, 8, 4, 2}},
                   CH, N, 1, 3);
        rc_engine_destroy(h);
    }
    {  // a host frequency kernel carries its tail: no hop is gathered twice
        rc_config ck = config(N, 2.0f, 1, CH);
        ck.kernel = ok_kernel;
        ck.kernel_time_ms = 1;
        rc_engine *h = nullptr;
        CHECK(rc_engine_create(&ck, &h) == RC_OK);
        CHECK(rc_engine_set_time_map(h, fwd.data(), fwd.size()) == RC_OK);
        CHECK(rc_test_time_map_chunk_windows(h, 1) == RC_OK);
        size_t got = 0;
        reset_logs();
        CHECK(rc_engine_stretch_device(h, x, stride, L, out, 4096, 4096, &got, nullptr) == RC_OK && got == 256);
        check_log({{0, 2}, {2, 2}, {4, 2}, {6, 2}}, fwd, CH, N, L);
        // the rows start at the chunk's own first hop: nothing is recomputed, the tail is carried
        check_hops({{FORWARD, 0, 128, 0, 2, 0}, {RESYNTH, 0, 128, 0, 2, 0}, {FORWARD, 128, 128, 2, 2, 1}, {RESYNTH, 128, 128, 2, 2, 1},
                    {FORWARD, 256, 128, 4, 2, 2}, {RESYNTH, 256, 128, 4, 2, 2}, {FORWARD, 384, 128, 6, 2, 3}, {RESYNTH, 384, 128, 6, 2, 3}},
                   CH, N, 1, 4);
        std::vector<float> rows(CH * L), res(CH * 256);
        for (uint32_t k = 0; k < CH; ++k)
            for (size_t i = 0; i < L; ++i) rows[k * L + i] = sample(k, i);
        const float *in_rows[2] = {rows.data(), rows.data() + L};
        float *out_rows[2] = {res.data(), res.data() + 256};
        rc_stub_tm_launches = 0;
        CHECK(rc_engine_stretch_host(h, in_rows, L, out_rows, 256, &got) == RC_OK && got == 256);
        check_log({{0, 2}, {2, 2}, {4, 2}, {6, 2}}, fwd, CH, N, L);
        rc_engine_destroy(h);
    }
    {  // negative pitch (one hop per window; the fused kernels at pitch 1 into scratch): the inner passes keep the step of N
        rc_config cn = config(N, 2.0f, -2, CH);
        rc_engine *h = nullptr;
        CHECK(rc_engine_create(&cn, &h) == RC_OK);
        rc_params pn;
        CHECK(rc_engine_get_params(h, &pn) == RC_OK && pn.hops_per_window == 1);
        const std::vector<int64_t> pos = {0, 100, 50, 280, -70};
        CHECK(rc_engine_set_time_map(h, pos.data(), pos.size()) == RC_OK);
        CHECK(rc_test_time_map_chunk_windows(h, 2) == RC_OK);
        size_t got = 0;
        reset_logs();
        CHECK(rc_engine_stretch_device(h, x, stride, L, out, 4096, 4096, &got, nullptr) == RC_OK && got == 5u * pn.window_out_len);
        check_log({{0, 2}, {1, 3}, {3, 2}}, pos, CH, N, L);
        // the inner pass of every chunk: the fused kernel at pitch 1, still at a step of N = 64 (sample_step_len is 32 here)
        CHECK(pn.sample_step_len == 32);
        check_hops({{FUSED, 0, 128, 0, 2, 0}, {FUSED, 64, 192, 2, 2, 1}, {FUSED, 192, 128, 4, 1, 2}}, CH, N, 1, 3);
        rc_engine_destroy(h);
    }
    hipFree(x);
    {
        // The upload bound of the host pipeline. 3 pipeline chunks: a chunk is one staging slot of output per channel, 4 Mi
        // floats = 65536 windows = 131072 hops here. Forward map, hop k at 2 k: chunk i gathers in front of everything
        // behind input sample 2 (131072 (i + 1) - 1) + 64 being up - its sums hold only if the bound reached that far.
        // Reversed map: the first chunk reads the end of the input, so everything is up in front of it.
        const size_t K = 3 * 131072, LL = 1000000;
        std::vector<float> rows(CH * LL), res(CH * (K / 2) * 64);
        for (uint32_t k = 0; k < CH; ++k)
            for (size_t i = 0; i < LL; ++i) rows[k * LL + i] = sample(k, i);
        const float *in_rows[2] = {rows.data(), rows.data() + LL};
        float *out_rows[2] = {res.data(), res.data() + (K / 2) * 64};
        std::vector<int64_t> pos(K);
        for (int dir = 0; dir < 2; ++dir) {
            for (size_t k = 0; k < K; ++k) pos[k] = dir == 0 ? (int64_t)(2 * k) : (int64_t)(LL - 64 - 2 * k);
            rc_engine *h = nullptr;
            CHECK(rc_engine_create(&c, &h) == RC_OK);
            CHECK(rc_engine_set_time_map(h, pos.data(), K) == RC_OK);
            size_t got = 0;
            reset_logs();
            CHECK(rc_engine_stretch_host(h, in_rows, LL, out_rows, (K / 2) * 64, &got) == RC_OK && got == (K / 2) * 64);
            check_log({{0, 131072}, {131071, 131073}, {262143, 131073}}, pos, CH, N, LL);
            // the plan's uploads themselves, per channel row (a staging slot holds 4 Mi floats: no cut inside a chunk's share).
            // Forward: chunk i brings the input up to 2 (131072 (i + 1) - 1) + 64 - 262206, 524350 - and the last chunk the
            // rest, so the later shares still go up under the compute. Reversed: one upload of the whole row.
            const std::vector<std::pair<uint64_t, uint64_t>> shares =
                dir == 0 ? std::vector<std::pair<uint64_t, uint64_t>>{{0, 262206}, {262206, 524350}, {524350, 1000000}}
                         : std::vector<std::pair<uint64_t, uint64_t>>{{0, 1000000}};
            const uintptr_t d_in = rc_stub_tm_log[0].x;
            for (uint32_t ch = 0; ch < CH; ++ch) {
                std::vector<std::pair<uint64_t, uint64_t>> seen;
                CHECK(rc_stub_h2d_copies <= 1024);
                for (uint32_t i = 0; i < rc_stub_h2d_copies; ++i) {
                    const uintptr_t lo = d_in + (uintptr_t)ch * LL * sizeof(float), d = rc_stub_h2d_log[i].dst;
                    if (d >= lo && d < lo + LL * sizeof(float)) seen.push_back({(d - lo) / sizeof(float), (d - lo + rc_stub_h2d_log[i].bytes) / sizeof(float)});
                }
                std::sort(seen.begin(), seen.end());
                CHECK(seen == shares);
            }
            rc_engine_destroy(h);
        }
    }
    hipFree(out);
    printf("engine_host_driver_timemap: ok\n");
    return 0;
}
