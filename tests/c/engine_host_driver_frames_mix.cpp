// TEST INFRASTRUCTURE: rc_engine_mix_frames and rc_engine_bus_frames over the HIP stub (tests/c/hip_stub.cpp: device memory is
// host memory, streams run at enqueue time, the hop kernels compute nothing; tests/c/hip_stub_frames_mix.cpp: the mix
// launcher logs its launch, reads what the real one reads and adds 1.0f to every bus word its range lands on) under ASan +
// UBSan and under TSan (rocoder_amd/csrc/host/sanitize.mk: engine_frames_mix_asan / _tsan; this program alone is linked with
// --wrap=hipMemcpyAsync, so that the copies the engine asks for are counted by kind). What runs for real is the engine's
// bookkeeping. Held to, against numbers written out by hand:
//   1. the mix launches of a multi-chunk job tile [0, n) exactly once and in order, every bus word of the landing range
//      was covered once and no other, and the job asks for no device-to-host copy,
//   2. under a limiter and a resampler the launches end where the two lags say,
//   3. rc_engine_bus_frames leaves the bus words as they were, with a fade (the copy) and a limiter set,
//   4. every refusal, with the bus untouched,
//   5. create / destroy of bus and engine in both orders.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rocoder_hip.h"

struct RcStubMixLaunch {  // tests/c/hip_stub_frames_mix.cpp
    uint64_t t0, t1, stride, bus_stride, bus_frames;
    int64_t offset;
    uint32_t channels, bus_channels, n_keys, has_send;
    uintptr_t row0, bus0;
};
extern RcStubMixLaunch rc_stub_mix_log[256];
extern uint32_t rc_stub_mix_launches;

static std::atomic<uint64_t> g_d2h_copies{0}, g_d2h_bytes{0};
extern "C" hipError_t __real_hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s);
extern "C" hipError_t __wrap_hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    if (kind == hipMemcpyDeviceToHost) {
        ++g_d2h_copies;
        g_d2h_bytes += bytes;
    }
    return __real_hipMemcpyAsync(dst, src, bytes, kind, s);
}

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

static const float *bus_words(rc_bus *b, size_t *stride) {
    float *d = nullptr;
    CHECK(rc_bus_device_rows(b, &d, stride) == RC_OK && d && *stride % 4 == 0 && (uintptr_t)d % 16 == 0);
    return d;  // (the stub's device memory is host memory)
}

// every word of the bus rows: 1.0f on [lo, hi), +0.0f elsewhere
static void check_cover(rc_bus *b, uint32_t CB, uint64_t N, uint64_t lo, uint64_t hi, float inside) {
    size_t stride = 0;
    const float *d = bus_words(b, &stride);
    for (uint32_t c = 0; c < CB; ++c)
        for (uint64_t u = 0; u < N; ++u) CHECK(d[c * stride + u] == (u >= lo && u < hi ? inside : 0.0f));
}

int main() {
    // window 1024, factor 8: written out by hand - 128 input frames a step, 8192 output frames a window, and a chunk of
    // the pipeline is 4 Mi floats / 8192 = 512 windows = 4194304 frames
    const rc_config cfg = config(1024, 8.0f, 2);
    rc_params par;
    CHECK(rc_derive_params(&cfg, &par) == RC_OK);
    const uint64_t wout = par.window_out_len, chunk = ((uint64_t)4 << 20) / wout * wout;
    const size_t L = 1300000;
    const uint64_t n = rc_offline_output_len(&cfg, L);
    CHECK(n > 2 * chunk && n < 3 * chunk);  // three chunks
    std::vector<int16_t> in(L * 2, 0);
    rc_engine *e = nullptr;
    rc_bus *bus = nullptr;
    CHECK(rc_engine_create(&cfg, &e) == RC_OK);
    const uint64_t N = n + 100;
    CHECK(rc_bus_create(0, 2, N, &bus) == RC_OK);
    uint32_t ch = 0, layers = 9;
    uint64_t frames = 0;
    CHECK(rc_bus_info(bus, &ch, &frames, &layers) == RC_OK && ch == 2 && frames == N && layers == 0);
    check_cover(bus, 2, N, 0, 0, 1.0f);
    const uint64_t kf[3] = {5, chunk, chunk + 1};
    const float ka[3] = {0.0f, 1.0f, 0.5f};

    // 1. three chunks, offset 37: the launches tile [0, n) and end on the chunks' ends; no copy to the host
    {
        uint64_t mixed = 0;
        rc_stub_mix_launches = 0;
        g_d2h_copies = 0;
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, 37, kf, ka, 3, nullptr, &mixed) == RC_OK && mixed == n);
        CHECK(g_d2h_copies == 0);
        CHECK(rc_stub_mix_launches == 3);
        uint64_t at = 0;
        for (uint32_t k = 0; k < 3; ++k) {
            const RcStubMixLaunch &l = rc_stub_mix_log[k];
            CHECK(l.t0 == at && l.t1 == std::min<uint64_t>(n, (k + 1) * chunk) && l.offset == 37 && l.n_keys == 3 && !l.has_send);
            CHECK(l.channels == 2 && l.bus_channels == 2 && l.bus_frames == N && l.stride == n && l.bus_stride % 4 == 0);
            CHECK(l.row0 == rc_stub_mix_log[0].row0 && l.bus0 == rc_stub_mix_log[0].bus0);
            at = l.t1;
        }
        CHECK(at == n);
        check_cover(bus, 2, N, 37, 37 + n, 1.0f);
        CHECK(rc_bus_info(bus, nullptr, nullptr, &layers) == RC_OK && layers == 1);
        // a second layer that starts in front of the bus and a third behind its end: dropped frames, counted
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, -(int64_t)n + 10, nullptr, nullptr, 0, nullptr, &mixed) == RC_OK && mixed == 10);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, (int64_t)N - 3, nullptr, nullptr, 0, nullptr, &mixed) == RC_OK && mixed == 3);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, (int64_t)N, nullptr, nullptr, 0, nullptr, &mixed) == RC_OK && mixed == 0);
        CHECK(rc_bus_info(bus, nullptr, nullptr, &layers) == RC_OK && layers == 4);
        CHECK(rc_bus_clear(bus) == RC_OK && rc_bus_info(bus, nullptr, nullptr, &layers) == RC_OK && layers == 0);
        check_cover(bus, 2, N, 0, 0, 1.0f);
    }

    // 2. a resampler at 3/2 (W = 48 row frames a side) and a limiter of look-ahead 100 in front of the mix: with the rows
    // final up to o, the resampled rows are final up to rs(o) = ceil((o - 48) * 2 / 3) and the limited rows up to
    // rs(o) - 200; behind the last chunk all of them
    {
        CHECK(rc_engine_set_output_resample(e, 3, 2) == RC_OK && rc_engine_set_output_limiter(e, 1.0f, 0.5f, 100) == RC_OK);
        const uint64_t n_rs = rc_resample_len(n, 3, 2);
        CHECK(n_rs == (n * 2 + 2) / 3);
        uint64_t mixed = 0;
        rc_stub_mix_launches = 0;
        g_d2h_copies = g_d2h_bytes = 0;
        const float send[4] = {1.0f, 0.0f, 0.5f, 0.5f};
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, 0, kf, ka, 3, send, &mixed) == RC_OK && mixed == n_rs);
        CHECK(g_d2h_copies == 1 && g_d2h_bytes == 16);  // the limiter's two stats words, nothing else
        CHECK(rc_stub_mix_launches == 3);
        uint64_t at = 0;
        for (uint32_t k = 0; k < 3; ++k) {
            const RcStubMixLaunch &l = rc_stub_mix_log[k];
            const uint64_t o = (k + 1) * chunk;
            const uint64_t want = o >= n ? n_rs : ((o - 48) * 2 + 2) / 3 - 200;
            CHECK(l.t0 == at && l.t1 == want && l.has_send && l.stride == n_rs);
            at = l.t1;
        }
        CHECK(at == n_rs);
        check_cover(bus, 2, N, 0, n_rs, 1.0f);
        CHECK(rc_engine_set_output_resample(e, 0, 0) == RC_OK);
    }

    // 3. the master with a fade and the limiter still set: the bus words stay, twice
    {
        CHECK(rc_engine_set_output_fade(e, 1000, N - 2000, 2000) == RC_OK);
        size_t stride = 0;
        const float *d = bus_words(bus, &stride);
        const std::vector<float> before(d, d + 2 * stride);
        std::vector<unsigned char> out(N * 2 * 2 + 3, 0x11);
        for (int pass = 0; pass < 2; ++pass) {
            size_t got = 0;
            float peak = -1.0f, gain = -1.0f;
            uint64_t clipped = 99;
            CHECK(rc_engine_bus_frames(e, bus, out.data() + 1, N, RC_PCM_I16, pass ? 0.5f : 0.0f, &got, &peak, &gain, &clipped) == RC_OK && got == N);
            CHECK(memcmp(before.data(), d, before.size() * sizeof(float)) == 0);
            CHECK(out[0] == 0x11 && out[1 + N * 4] == 0x11 && out[2 + N * 4] == 0x11);
            if (!pass) CHECK(gain == 1.0f);
        }
        // 4. the master's refusals write nothing behind the out-pointers
        size_t got = 99;
        float peak = 99.0f;
        rc_bus *bus3 = nullptr;
        CHECK(rc_bus_create(0, 3, 16, &bus3) == RC_OK);
        CHECK(rc_engine_bus_frames(nullptr, bus, out.data(), N, RC_PCM_I16, 0.0f, &got, &peak, nullptr, nullptr) == RC_EINVAL);
        CHECK(rc_engine_bus_frames(e, nullptr, out.data(), N, RC_PCM_I16, 0.0f, &got, &peak, nullptr, nullptr) == RC_EINVAL);
        CHECK(rc_engine_bus_frames(e, bus, nullptr, N, RC_PCM_I16, 0.0f, &got, &peak, nullptr, nullptr) == RC_EINVAL);
        CHECK(rc_engine_bus_frames(e, bus3, out.data(), N, RC_PCM_I16, 0.0f, &got, &peak, nullptr, nullptr) == RC_EINVAL);
        CHECK(rc_engine_bus_frames(e, bus, out.data(), N, 0, 0.0f, &got, &peak, nullptr, nullptr) == RC_EINVAL);
        CHECK(rc_engine_bus_frames(e, bus, out.data(), N, 6, 0.0f, &got, &peak, nullptr, nullptr) == RC_EINVAL);
        CHECK(rc_engine_bus_frames(e, bus, out.data(), N, RC_PCM_I16, -1.0f, &got, &peak, nullptr, nullptr) == RC_EINVAL);
        CHECK(rc_engine_bus_frames(e, bus, out.data(), N, RC_PCM_I16, HUGE_VALF, &got, &peak, nullptr, nullptr) == RC_EINVAL);
        CHECK(rc_engine_bus_frames(e, bus, out.data(), N - 1, RC_PCM_I16, 0.0f, &got, &peak, nullptr, nullptr) == RC_ECAPACITY);
        CHECK(rc_engine_set_output_fade(e, N + 1, RC_FADE_NONE, 0) == RC_OK);
        CHECK(rc_engine_bus_frames(e, bus, out.data(), N, RC_PCM_I16, 0.0f, &got, &peak, nullptr, nullptr) == RC_EINVAL);
        CHECK(got == 99 && peak == 99.0f);
        CHECK(rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 0) == RC_OK && rc_engine_set_output_limiter(e, 1.0f, 0.0f, 0) == RC_OK);

        // 4. the layer's refusals: nothing launched, the bus untouched, no layer counted
        uint64_t mixed = 99;
        uint32_t before_layers = 0;
        CHECK(rc_bus_info(bus, nullptr, nullptr, &before_layers) == RC_OK);
        rc_stub_mix_launches = 0;
        const uint64_t same[2] = {4, 4}, back[2] = {4, 3};
        const float nan_amp[2] = {0.5f, NAN}, inf_send[4] = {1.0f, 0.0f, HUGE_VALF, 1.0f};
        std::vector<uint64_t> many(RC_MIX_MAX_KEYS + 1);
        std::vector<float> many_amp(many.size(), 1.0f);
        for (size_t i = 0; i < many.size(); ++i) many[i] = i;
        CHECK(rc_engine_mix_frames(nullptr, in.data(), L, RC_PCM_I16, bus, 0, kf, ka, 3, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, nullptr, 0, kf, ka, 3, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, nullptr, L, RC_PCM_I16, bus, 0, kf, ka, 3, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, in.data(), L, 0, bus, 0, kf, ka, 3, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus3, 0, kf, ka, 3, nullptr, &mixed) == RC_EINVAL);  // no send, 2 into 3
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, 0, same, ka, 2, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, 0, back, ka, 2, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, 0, kf, nan_amp, 2, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, 0, nullptr, ka, 2, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, 0, many.data(), many_amp.data(), many.size(), nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, 0, kf, ka, 3, inf_send, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, ((int64_t)1 << 62) + 1, kf, ka, 3, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, -((int64_t)1 << 62) - 1, kf, ka, 3, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_set_output_fade(e, n + 1, RC_FADE_NONE, 0) == RC_OK);  // what rc_engine_stretch_frames rejects
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, 0, kf, ka, 3, nullptr, &mixed) == RC_EINVAL);
        CHECK(rc_engine_set_output_fade(e, 0, RC_FADE_NONE, 0) == RC_OK);
        CHECK(mixed == 99 && rc_stub_mix_launches == 0 && memcmp(before.data(), d, before.size() * sizeof(float)) == 0);
        CHECK(rc_bus_info(bus, nullptr, nullptr, &layers) == RC_OK && layers == before_layers);
        // the most keys, and no frames: valid, a layer
        CHECK(rc_engine_mix_frames(e, in.data(), L, RC_PCM_I16, bus, 0, many.data(), many_amp.data(), RC_MIX_MAX_KEYS, nullptr, &mixed) == RC_OK && mixed == n);
        CHECK(rc_engine_mix_frames(e, nullptr, 0, RC_PCM_I16, bus, 0, nullptr, nullptr, 0, nullptr, &mixed) == RC_OK);
        CHECK(rc_bus_info(bus, nullptr, nullptr, &layers) == RC_OK && layers == before_layers + 2);
        rc_bus_destroy(bus3);
    }

    // the bus's own refusals, and a bus of no frames
    {
        rc_bus *b = nullptr;
        CHECK(rc_bus_create(0, 0, 16, &b) == RC_EINVAL && !b && rc_bus_create(0, 33, 16, &b) == RC_EINVAL && !b);
        CHECK(rc_bus_create(0, 2, 16, nullptr) == RC_EINVAL && rc_bus_clear(nullptr) == RC_EINVAL);
        CHECK(rc_bus_info(nullptr, nullptr, nullptr, nullptr) == RC_EINVAL && rc_bus_device_rows(nullptr, nullptr, nullptr) == RC_EINVAL);
        rc_bus_destroy(nullptr);
        CHECK(rc_bus_create(0, 2, 0, &b) == RC_OK && b);
        uint64_t mixed = 99;
        CHECK(rc_engine_mix_frames(e, in.data(), 3000, RC_PCM_I16, b, 0, nullptr, nullptr, 0, nullptr, &mixed) == RC_OK && mixed == 0);
        unsigned char none[4];
        size_t got = 99;
        float gain = 0.0f;
        CHECK(rc_engine_bus_frames(e, b, none, 0, RC_PCM_I24, 0.7f, &got, nullptr, &gain, nullptr) == RC_OK && got == 0 && gain == 1.0f);
        rc_bus_destroy(b);
    }

    // 5. both orders: the engine first, then the bus it mixed into - and a bus first, then the engine that mixed into it
    rc_engine_destroy(e);
    rc_bus_destroy(bus);
    CHECK(rc_engine_create(&cfg, &e) == RC_OK && rc_bus_create(0, 2, 9000, &bus) == RC_OK);
    CHECK(rc_engine_mix_frames(e, in.data(), 1000, RC_PCM_I16, bus, 0, nullptr, nullptr, 0, nullptr, nullptr) == RC_OK);
    rc_bus_destroy(bus);
    rc_engine_destroy(e);
    printf("engine_host_driver_frames_mix: ok\n");
    return 0;
}
