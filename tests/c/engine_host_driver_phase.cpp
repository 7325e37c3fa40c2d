// TEST INFRASTRUCTURE: rc_engine_set_phase_mode over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory,
// streams run at enqueue time, the hop kernels compute nothing; tests/c/hip_stub_phase.cpp: the launchers of rc_phase.h log
// their launches, prep makes every hop add 1 to theta, scan and walk compose for real) under ASan + UBSan and under TSan
// (rocoder_amd/csrc/host/sanitize.mk: engine_phase_asan / _tsan, over an engine built with -DRC_TEST_HOOKS=1 for
// rc_test_phase_chunk_hops; this program alone is linked with --wrap for rc::launch_hop and rc::launch_ola, whose calls are
// logged here, in the stub's log, and handed on). What runs for real is the engine's bookkeeping. Held to, against numbers
// written out by hand:
//   1. the launch order of every chunk of a three-chunk job: analysis with the halo hop, prep, scan, walk, apply, the
//      phase-keeping synthesis, the overlap-add,
//   2. theta zeroed at hop 0 and carried from chunk to chunk, in both modes and call after call,
//   3. the overlap-add envelope and amplitude: the coherent table under a mode, the reference's bits again behind RANDOM,
//   4. every refusal, in both orders of the two calls, with the mode left as it was,
//   5. rc_test_phase_tap: the rows and the chunk table of the three-chunk job in arrays of exactly their size, the same
//      launches and the same output with the tap set, a job refused whole when any array is one element short.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rocoder_hip.h"
#include "../../rocoder_amd/csrc/rc_kernels.h"

struct RcStubPhaseLaunch {  // tests/c/hip_stub_phase.cpp
    int kind;
    int64_t hop_first, hop_count;
    uint32_t halo, n_channels, locked, step, block;
    uint32_t theta_in, theta_out;
};
extern RcStubPhaseLaunch rc_stub_phase_log[1024];
extern uint32_t rc_stub_phase_launches;
void rc_stub_phase_note(const RcStubPhaseLaunch &l);
extern "C" int rc_test_phase_chunk_hops(rc_engine *e, uint64_t n);  // (the engine of this program is the test-hook build)
extern "C" int rc_test_phase_tap(rc_engine *e, float *spec, size_t spec_cap, uint32_t *qs, size_t qs_cap, uint32_t *base, size_t base_cap,
                                 float *z, size_t z_cap, float *y, size_t y_cap, int64_t *chunks, size_t chunk_cap, uint64_t *n_chunks);

// the stub's own functions under the names --wrap gives them, and what the engine's calls resolve to
hipError_t real_launch_hop(int, rc::HopMode, const rc::HopParams &, hipStream_t) __asm__("__real__ZN2rc10launch_hopEiNS_7HopModeERKNS_9HopParamsEP12ihipStream_t");
hipError_t real_launch_ola(const rc::OlaParams &, hipStream_t, bool) __asm__("__real__ZN2rc10launch_olaERKNS_9OlaParamsEP12ihipStream_tb");
hipError_t wrap_launch_hop(int, rc::HopMode, const rc::HopParams &, hipStream_t) __asm__("__wrap__ZN2rc10launch_hopEiNS_7HopModeERKNS_9HopParamsEP12ihipStream_t");
hipError_t wrap_launch_ola(const rc::OlaParams &, hipStream_t, bool) __asm__("__wrap__ZN2rc10launch_olaERKNS_9OlaParamsEP12ihipStream_tb");

static const float *g_env = nullptr;  // of the last hop launch, and of the last overlap-add
static float g_amp = 0.0f, g_ola_amp = 0.0f;
static const float *g_ola_env = nullptr;
static int g_last_mode = -1;

hipError_t wrap_launch_hop(int log2n, rc::HopMode mode, const rc::HopParams &p, hipStream_t s) {
    g_env = p.env;
    g_amp = p.amp;
    g_last_mode = (int)mode;
    if (mode == rc::MODE_FORWARD) {
        rc_stub_phase_note(RcStubPhaseLaunch{10, p.hop_first, p.hop_count, 0, p.n_channels, 0, p.step, 0, 0, 0});
        // the stub's kernels compute nothing: mark every analysis row with (hop, channel) in bin 0 for the tap's check
        for (uint32_t c = 0; p.spec && c < p.n_channels; ++c)
            for (int64_t r = 0; r < p.hop_count; ++r)
                p.spec[((size_t)c * p.hop_count + r) << log2n] = make_float2((float)(p.hop_first + r), (float)c);
    }
    return real_launch_hop(log2n, mode, p, s);
}
hipError_t wrap_launch_ola(const rc::OlaParams &p, hipStream_t s, bool tail_only) {
    g_ola_env = p.env;
    g_ola_amp = p.amp;
    rc_stub_phase_note(RcStubPhaseLaunch{11, p.hop_first, p.hop_count, tail_only ? 1u : 0u, p.n_channels, 0, 0, 0, 0, 0});
    return real_launch_ola(p, s, tail_only);
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rc_last_error()); \
            exit(2);                                                             \
        }                                                                        \
    } while (0)

static rc_config config(uint32_t N, float f, int p, uint32_t ch, float amplitude = 1.0f) {
    rc_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.window_len = N;
    c.factor = f;
    c.amplitude = amplitude;
    c.pitch_multiple = p;
    c.sample_rate = 44100;
    c.channels = ch;
    c.buffer_secs = 1.0f;
    c.seed = 7;
    return c;
}

static bool names(const char *word) { return strstr(rc_last_error(), word) != nullptr; }

static void put(std::string &b, size_t off, uint64_t v, size_t n) {
    for (size_t i = 0; i < n; ++i) b[off + i] = (char)(v >> (8 * i));
}
// ELF64 / EM_AMDGPU / gfx950 with a string table and a symbol table that holds rc_user_dk: what the stub's loader takes
static std::string fake_code_object() {
    const std::string strtab = std::string("\0rc_user_dk\0", 12);
    const size_t str_off = 64, sym_off = 96, sh_off = sym_off + 24 * 3;
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
    const size_t s1 = sh_off + 64, s2 = sh_off + 128;
    put(b, s1 + 4, 3, 4);
    put(b, s1 + 24, str_off, 8);
    put(b, s1 + 32, strtab.size(), 8);
    put(b, s2 + 4, 2, 4);
    put(b, s2 + 24, sym_off, 8);
    put(b, s2 + 32, 24 * 2, 8);
    put(b, s2 + 40, 1, 4);
    put(b, s2 + 56, 24, 8);
    return b;
}

static int a_kernel(uint64_t, const float *in, float *out, size_t n, void *) {
    memcpy(out, in, 2 * n * sizeof(float));
    return 0;
}

int main() {
    // window 64, factor 2, by hand: psf 2, step 64 / 4 = 16, H 32, two hops a window of 64 output frames. L = 64 + 16 * 19:
    // the first hop past the input is hop 20, so 20 / 2 + 1 = 11 windows, 22 hops, 704 frames.
    const uint32_t N = 64, H = 32, CH = 2;
    const size_t L = 64 + 16 * 19, n_out = 704;
    const rc_config cfg = config(N, 2.0f, 1, CH, 0.5f);
    rc_params par;
    CHECK(rc_derive_params(&cfg, &par) == RC_OK && par.sample_step_len == 16 && par.hops_per_window == 2 && par.window_out_len == 64);
    CHECK(rc_offline_output_len(&cfg, L) == n_out);
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&cfg, &e) == RC_OK);
    float *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc((void **)&d_in, CH * L * sizeof(float)) == hipSuccess && hipMalloc((void **)&d_out, CH * n_out * sizeof(float)) == hipSuccess);
    for (size_t i = 0; i < CH * L; ++i) d_in[i] = 0.25f;  // (the stub's device memory is host memory)
    size_t got = 0;
    uint32_t mode = 9;
    CHECK(rc_engine_get_phase_mode(e, &mode) == RC_OK && mode == RC_PHASE_RANDOM);

    // 3a. RANDOM first: the fused kernel with the reference's envelope and max(4, psf / 4) * amplitude
    CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && got == n_out);
    CHECK(g_last_mode == (int)rc::MODE_FUSED && g_amp == 2.0f && g_env);
    std::vector<float> env_ref(g_env, g_env + H), env_c(H), window(N);
    const float *const env_table = g_env;
    for (uint32_t i = 0; i < N; ++i) window[i] = 0.5f - cosf(((float)i * (3.14159274101257324219f * 2.0f)) / (float)(N - 1)) * 0.5f;
    CHECK(rc_phase_envelope(window.data(), N, env_c.data()) == RC_OK);
    CHECK(memcmp(env_ref.data(), env_c.data(), H * sizeof(float)) != 0);

    // 1 + 2. both modes, chunks of 8 hops: (8, no halo), (8, halo), (6, halo); twice: every call restarts at hop 0
    CHECK(rc_test_phase_chunk_hops(e, 8) == RC_OK);
    for (uint32_t m : {(uint32_t)RC_PHASE_LOCKED, (uint32_t)RC_PHASE_PROPAGATE}) {
        CHECK(rc_engine_set_phase_mode(e, m) == RC_OK);
        CHECK(rc_engine_get_phase_mode(e, &mode) == RC_OK && mode == m);
        for (int call = 0; call < 2; ++call) {
            rc_stub_phase_launches = 0;
            CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && got == n_out);
            CHECK(rc_engine_synchronize(e) == RC_OK);
            const struct { int64_t k0, kc; uint32_t halo, th_in, th_out; } want[3] = {{0, 8, 0, 0, 7}, {8, 8, 1, 7, 15}, {16, 6, 1, 15, 21}};
            CHECK(rc_stub_phase_launches == 3 * 7);
            for (int c = 0; c < 3; ++c) {
                const RcStubPhaseLaunch *l = rc_stub_phase_log + 7 * c;
                const auto &w = want[c];
                CHECK(l[0].kind == 10 && l[0].hop_first == w.k0 - w.halo && l[0].hop_count == w.kc + w.halo && l[0].n_channels == CH && l[0].step == 16);
                CHECK(l[1].kind == 0 && l[1].hop_count == w.kc && l[1].halo == w.halo && l[1].n_channels == CH && l[1].step == 16 &&
                      l[1].locked == (m == RC_PHASE_LOCKED ? 1u : 0u));
                CHECK(l[2].kind == 1 && l[2].hop_count == w.kc && l[2].n_channels == CH && l[2].block >= 1);
                CHECK(l[3].kind == 2 && l[3].hop_count == w.kc && l[3].block == l[2].block && l[3].theta_in == w.th_in && l[3].theta_out == w.th_out);
                CHECK(l[4].kind == 3 && l[4].hop_count == w.kc && l[4].halo == w.halo && l[4].block == l[2].block);
                CHECK(l[5].kind == 4 && l[5].hop_first == w.k0 && l[5].hop_count == w.kc && l[5].n_channels == CH);
                CHECK(l[6].kind == 11 && l[6].hop_first == w.k0 && l[6].hop_count == w.kc && l[6].halo == 0 && l[6].n_channels == CH);
            }
            // 3b. the coherent table and the plain amplitude, in the table the engine has always handed out
            CHECK(g_ola_env == env_table && g_env == env_table && g_ola_amp == 0.5f && g_amp == 0.5f);
            CHECK(memcmp(env_table, env_c.data(), H * sizeof(float)) == 0);
        }
    }
    // one chunk for the whole job gives the same last state
    CHECK(rc_test_phase_chunk_hops(e, 0) == RC_OK);
    rc_stub_phase_launches = 0;
    CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK);
    CHECK(rc_stub_phase_launches == 7 && rc_stub_phase_log[3].kind == 2 && rc_stub_phase_log[3].theta_in == 0 && rc_stub_phase_log[3].theta_out == 21);

    // 5. the tap: arrays of exactly the job's size (one element more anywhere is an AddressSanitizer finding), chunks of 8
    // hops again. The stub's rows by hand: apply leaves theta - the hop's index - in the real part of every bin, the
    // synthesis in every sample; scan leaves Q = the identity and s = the hops since the chunk began; base is the carried
    // state 0, 7, 15.
    {
        const size_t nb = H + 1, hops = 22;
        const size_t n_spec = CH * (8 + 9 + 7) * N * 2, n_qs = CH * hops * 2 * nb, n_base = CH * 3 * nb, n_z = CH * hops * N * 2, n_y = CH * hops * N;
        std::vector<float> spec(n_spec, -1.0f), z(n_z, -1.0f), y(n_y, -1.0f), plain(CH * n_out), tapped(CH * n_out);
        std::vector<uint32_t> qs(n_qs, 0xA5A5A5A5u), base(n_base, 0xA5A5A5A5u);
        std::vector<int64_t> table(3 * 11, -1);
        uint64_t n_chunks = 99;
        CHECK(rc_test_phase_chunk_hops(e, 8) == RC_OK);
        CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && rc_engine_synchronize(e) == RC_OK);
        memcpy(plain.data(), d_out, plain.size() * sizeof(float));
        CHECK(rc_test_phase_tap(nullptr, spec.data(), n_spec, qs.data(), n_qs, base.data(), n_base, z.data(), n_z, y.data(), n_y, table.data(), 3, &n_chunks) == RC_EINVAL);
        CHECK(rc_test_phase_tap(e, spec.data(), n_spec, nullptr, n_qs, base.data(), n_base, z.data(), n_z, y.data(), n_y, table.data(), 3, &n_chunks) == RC_EINVAL);
        CHECK(rc_test_phase_tap(e, spec.data(), n_spec, qs.data(), n_qs, base.data(), n_base, z.data(), n_z, y.data(), n_y, table.data(), 3, &n_chunks) == RC_OK);
        CHECK(n_chunks == 0);
        rc_stub_phase_launches = 0;
        CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && rc_engine_synchronize(e) == RC_OK);
        CHECK(rc_stub_phase_launches == 3 * 7 && n_chunks == 3);  // (no launch more than without it)
        memcpy(tapped.data(), d_out, tapped.size() * sizeof(float));
        CHECK(memcmp(plain.data(), tapped.data(), plain.size() * sizeof(float)) == 0);
        const int64_t want[3][11] = {{0, 8, 16, 0, CH, 0, 0, 0, 0, 0, 0},
                                     {8, 8, 16, 0, CH, 1, (int64_t)(CH * 8 * N * 2), (int64_t)(CH * 8 * 2 * nb), (int64_t)(CH * nb), (int64_t)(CH * 8 * N * 2), (int64_t)(CH * 8 * N)},
                                     {16, 6, 16, 0, CH, 1, (int64_t)(CH * 17 * N * 2), (int64_t)(CH * 16 * 2 * nb), (int64_t)(2 * CH * nb), (int64_t)(CH * 16 * N * 2), (int64_t)(CH * 16 * N)}};
        CHECK(memcmp(table.data(), want, sizeof want) == 0);
        for (int c = 0; c < 3; ++c) {
            const int64_t k0 = want[c][0], kc = want[c][1], halo = want[c][5];
            for (uint32_t ch = 0; ch < CH; ++ch) {
                for (size_t j = 0; j < nb; ++j) CHECK(base[(size_t)want[c][8] + ch * nb + j] == (c == 0 ? 0u : c == 1 ? 7u : 15u));
                for (int64_t r = 0; r < kc; ++r) {
                    const uint32_t hop = (uint32_t)(k0 + r), since = (uint32_t)(k0 == 0 ? r : r + 1);  // (hop 0 adds nothing)
                    const uint32_t *row = qs.data() + want[c][7] + ((size_t)ch * kc + r) * 2 * nb;
                    for (size_t j = 0; j < nb; ++j) CHECK(row[j] == j && row[nb + j] == since);
                    const float *zr = z.data() + want[c][9] + ((size_t)ch * kc + r) * N * 2, *yr = y.data() + want[c][10] + ((size_t)ch * kc + r) * N;
                    for (size_t j = 0; j < nb; ++j) CHECK(zr[2 * j] == (float)hop && zr[2 * j + 1] == 0.0f);
                    for (size_t i = 0; i < N; ++i) CHECK(yr[i] == (float)hop);
                }
                // the analysis rows, the halo hop in front: bin 0 holds (hop, channel) (wrap_launch_hop), the rest zeros
                for (int64_t r = 0; r < kc + halo; ++r) {
                    const float *xr = spec.data() + want[c][6] + ((size_t)ch * (kc + halo) + r) * N * 2;
                    CHECK(xr[0] == (float)(k0 - halo + r) && xr[1] == (float)ch);
                    for (size_t i = 2; i < 2 * N; ++i) CHECK(xr[i] == 0.0f);
                }
            }
        }
        // one element short, in every array in turn: refused before any of the job's hops runs, nothing cut short
        const size_t caps[6] = {n_spec, n_qs, n_base, n_z, n_y, 3};
        for (int short_one = 0; short_one < 6; ++short_one) {
            size_t c6[6];
            for (int i = 0; i < 6; ++i) c6[i] = caps[i] - (i == short_one ? 1 : 0);
            CHECK(rc_test_phase_tap(e, spec.data(), c6[0], qs.data(), c6[1], base.data(), c6[2], z.data(), c6[3], y.data(), c6[4], table.data(), c6[5], &n_chunks) == RC_OK);
            rc_stub_phase_launches = 0;
            CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_EINVAL && names("rc_test_phase_tap"));
            CHECK(rc_stub_phase_launches == 0 && n_chunks == 0);
        }
        // the tap removed: the job runs as before and the arrays stay as they are
        CHECK(rc_test_phase_tap(e, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) == RC_OK);
        n_chunks = 42;
        CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && rc_engine_synchronize(e) == RC_OK);
        CHECK(n_chunks == 42 && memcmp(plain.data(), d_out, plain.size() * sizeof(float)) == 0);
        CHECK(rc_test_phase_chunk_hops(e, 0) == RC_OK);
    }

    // 4a. the mode first: the seam, the range entry and the single hop are unsupported and say which mode is set
    {
        std::vector<float> x(L, 0.0f), w(par.window_out_len), one(N);
        const float *view = nullptr;
        size_t n = 0;
        CHECK(rc_engine_push_input(e, 0, x.data(), L) == RC_EUNSUPPORTED && names("propagate"));
        CHECK(rc_engine_next_window(e, 0, w.data(), w.size(), &n) == RC_EUNSUPPORTED && names("propagate"));
        CHECK(rc_engine_next_window_view(e, 0, &view, &n) == RC_EUNSUPPORTED && names("propagate"));
        CHECK(rc_engine_stretch_device_range(e, d_in, L, L, 0, CH, 0, 1, d_out, n_out, n_out, nullptr) == RC_EUNSUPPORTED && names("propagate"));
        CHECK(rc_engine_resynth(e, 0, 0, x.data(), one.data()) == RC_EUNSUPPORTED && names("propagate"));
        // ... a kernel, a map and a warp are invalid
        const std::string code = fake_code_object();
        CHECK(rc_engine_load_device_kernel(e, code.data(), code.size()) == RC_EINVAL && names("propagate"));
        CHECK(rc_engine_load_device_kernel(e, nullptr, 0) == RC_OK);  // (clearing is no kernel)
        std::vector<int64_t> pos(4);
        for (size_t k = 0; k < pos.size(); ++k) pos[k] = (int64_t)k * 16;
        CHECK(rc_engine_set_time_map(e, pos.data(), pos.size()) == RC_EINVAL && names("propagate"));
        CHECK(rc_engine_set_time_map(e, nullptr, 0) == RC_OK);
        const int64_t anchor[3] = {0, (int64_t)64 << 32, (int64_t)128 << 32};
        CHECK(rc_engine_set_output_warp(e, anchor, 3, 100) == RC_EINVAL && names("propagate"));
        CHECK(rc_engine_set_output_warp(e, nullptr, 0, 0) == RC_OK);
        CHECK(rc_engine_set_phase_mode(e, 3) == RC_EINVAL && rc_engine_set_phase_mode(nullptr, 0) == RC_EINVAL);
        CHECK(rc_engine_get_phase_mode(e, nullptr) == RC_EINVAL && rc_engine_get_phase_mode(nullptr, &mode) == RC_EINVAL);
        CHECK(rc_engine_get_phase_mode(e, &mode) == RC_OK && mode == RC_PHASE_PROPAGATE);

        // 3c. RANDOM again: the reference's bits and amplitude are back, the refused entries run
        CHECK(rc_engine_set_phase_mode(e, RC_PHASE_RANDOM) == RC_OK);
        CHECK(memcmp(env_table, env_ref.data(), H * sizeof(float)) == 0);
        CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK);
        CHECK(g_last_mode == (int)rc::MODE_FUSED && g_amp == 2.0f && g_env == env_table);
        CHECK(rc_engine_stretch_device_range(e, d_in, L, L, 0, CH, 0, 1, d_out, n_out, n_out, nullptr) == RC_OK);
        CHECK(rc_engine_resynth(e, 0, 0, x.data(), one.data()) == RC_OK);

        // 4b. ... and the mode second
        CHECK(rc_engine_load_device_kernel(e, code.data(), code.size()) == RC_OK);
        CHECK(rc_engine_set_phase_mode(e, RC_PHASE_LOCKED) == RC_EINVAL && names("locked") && names("user device"));
        CHECK(rc_engine_load_device_kernel(e, nullptr, 0) == RC_OK);
        CHECK(rc_engine_set_time_map(e, pos.data(), pos.size()) == RC_OK);
        CHECK(rc_engine_set_phase_mode(e, RC_PHASE_LOCKED) == RC_EINVAL && names("time map"));
        CHECK(rc_engine_set_time_map(e, nullptr, 0) == RC_OK);
        CHECK(rc_engine_set_output_warp(e, anchor, 3, 100) == RC_OK);
        CHECK(rc_engine_set_phase_mode(e, RC_PHASE_PROPAGATE) == RC_EINVAL && names("warp"));
        CHECK(rc_engine_set_output_warp(e, nullptr, 0, 0) == RC_OK);
        CHECK(rc_engine_get_phase_mode(e, &mode) == RC_OK && mode == RC_PHASE_RANDOM);
        CHECK(memcmp(env_table, env_ref.data(), H * sizeof(float)) == 0);  // a refused setter wrote nothing
        CHECK(rc_engine_set_phase_mode(e, RC_PHASE_LOCKED) == RC_OK);
    }
    rc_engine_destroy(e);  // (with a mode set)

    // 4c. engines that can take no mode: a host kernel, the curated kernels, windows off the hop path, a window without
    // an inverse envelope - and a negative pitch multiple, which can
    {
        rc_config k = cfg;
        k.kernel = a_kernel;
        CHECK(rc_engine_create(&k, &e) == RC_OK);
        CHECK(rc_engine_set_phase_mode(e, RC_PHASE_LOCKED) == RC_EINVAL && names("host frequency"));
        rc_engine_destroy(e);
        for (uint32_t dk : {(uint32_t)RC_DK_GAIN, (uint32_t)RC_DK_BAND, (uint32_t)RC_DK_SHIFT}) {
            k = cfg;
            k.device_kernel = dk;
            k.dk_gain = k.dk_gain_outside = 1.0f;
            k.dk_hi_bin = 8;
            k.dk_shift_bins = 1;
            CHECK(rc_engine_create(&k, &e) == RC_OK);
            CHECK(rc_engine_set_phase_mode(e, RC_PHASE_PROPAGATE) == RC_EINVAL && names("curated"));
            CHECK(rc_engine_set_phase_mode(e, RC_PHASE_RANDOM) == RC_OK);
            rc_engine_destroy(e);
        }
        for (uint32_t n : {1000u, 32768u, 65536u, 131072u}) {
            k = config(n, 2.0f, 1, 1);
            CHECK(rc_engine_create(&k, &e) == RC_OK);
            CHECK(rc_engine_set_phase_mode(e, RC_PHASE_LOCKED) == RC_EUNSUPPORTED && names("locked") && names("power of two"));
            CHECK(rc_engine_get_phase_mode(e, &mode) == RC_OK && mode == RC_PHASE_RANDOM);
            rc_engine_destroy(e);
        }
        std::vector<float> w(N, 1.0f);
        w[5] = w[5 + H] = 0.0f;
        k = cfg;
        k.window = w.data();
        CHECK(rc_engine_create(&k, &e) == RC_OK);
        CHECK(rc_engine_set_phase_mode(e, RC_PHASE_LOCKED) == RC_EINVAL && names("2^-10"));
        rc_engine_destroy(e);
        // p = -2, factor 4: psf 2, one hop a window: the spectrum path with the interpolating overlap-add, not the fused pass
        k = config(N, 4.0f, -2, CH);
        CHECK(rc_engine_create(&k, &e) == RC_OK);
        CHECK(rc_engine_set_phase_mode(e, RC_PHASE_LOCKED) == RC_OK);
        const size_t n2 = rc_offline_output_len(&k, L);
        float *d_out2 = nullptr;
        CHECK(n2 > 0 && hipMalloc((void **)&d_out2, CH * n2 * sizeof(float)) == hipSuccess);
        rc_stub_phase_launches = 0;
        CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out2, n2, n2, &got, nullptr) == RC_OK && got == n2);
        CHECK(rc_stub_phase_launches == 7 && rc_stub_phase_log[0].kind == 10 && rc_stub_phase_log[5].kind == 4 && rc_stub_phase_log[6].kind == 11);
        CHECK(rc_stub_phase_log[3].theta_in == 0 && rc_stub_phase_log[3].theta_out == (uint32_t)rc_stub_phase_log[3].hop_count - 1);
        CHECK(hipFree(d_out2) == hipSuccess);
        rc_engine_destroy(e);
    }
    // the host helper, without an engine
    {
        float w[4] = {1.0f, 2.0f, 3.0f, 0.5f}, env[2] = {0, 0};
        CHECK(rc_phase_envelope(w, 4, env) == RC_OK && env[0] == 1.0f / 10.0f && env[1] == 1.0f / 4.25f);
        CHECK(rc_phase_envelope(w, 3, env) == RC_EINVAL && rc_phase_envelope(nullptr, 4, env) == RC_EINVAL && rc_phase_envelope(w, 4, nullptr) == RC_EINVAL);
    }
    CHECK(hipFree(d_in) == hipSuccess && hipFree(d_out) == hipSuccess);
    printf("engine_host_driver_phase: ok\n");
    return 0;
}
