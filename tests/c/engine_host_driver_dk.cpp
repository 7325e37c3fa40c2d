// TEST INFRASTRUCTURE: the engine's host code with a user device kernel that declares a history (RC_HISTORY 3) loaded,
// over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory, kernels compute nothing) under ASan + UBSan
// (rocoder_amd/csrc/host/sanitize.mk: engine_dk_asan). What runs for real is the bookkeeping around the halo: chunk
// sizes and reserves, the input spans of ranges, streaming batches and rc_multi shards and the copies they size. The
// code object is a hand-made ELF that carries only what the loader's check reads: the machine, and the two symbols.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rocoder_hip.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rc_last_error()); \
            exit(2);                                                             \
        }                                                                        \
    } while (0)

extern "C" int hipSetDevice(int);
extern "C" int hipMalloc(void **, size_t);
extern "C" int hipFree(void *);

static void put(std::string &b, size_t off, uint64_t v, size_t n) {
    for (size_t i = 0; i < n; ++i) b[off + i] = (char)(v >> (8 * i));
}
// ELF64 / EM_AMDGPU / gfx950 with a string table and a symbol table: rc_user_dk, and rc_user_dk_history of
// `hist_size` bytes (0: no such symbol, a code object from before the history contract)
static std::string fake_code_object(uint64_t hist_size) {
    const std::string strtab = std::string("\0rc_user_dk\0rc_user_dk_history\0", 31);
    const size_t n_sym = hist_size ? 3 : 2, str_off = 64, sym_off = 96, sh_off = sym_off + 24 * 3;
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
    put(b, sym_off + 24, 1, 4);  // symbol 1: rc_user_dk
    if (hist_size) {
        put(b, sym_off + 48, 12, 4);  // symbol 2: rc_user_dk_history
        put(b, sym_off + 48 + 16, hist_size, 8);
    }
    const size_t s1 = sh_off + 64, s2 = sh_off + 128;
    put(b, s1 + 4, 3, 4);  // SHT_STRTAB
    put(b, s1 + 24, str_off, 8);
    put(b, s1 + 32, strtab.size(), 8);
    put(b, s2 + 4, 2, 4);  // SHT_SYMTAB
    put(b, s2 + 24, sym_off, 8);
    put(b, s2 + 32, 24 * n_sym, 8);
    put(b, s2 + 40, 1, 4);
    put(b, s2 + 56, 24, 8);
    return b;
}

static rc_config config(uint32_t N, float f, int p, uint32_t ch, uint32_t batch = 0) {
    rc_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.window_len = N;
    c.factor = f;
    c.amplitude = 1.0f;
    c.pitch_multiple = p;
    c.sample_rate = 44100;
    c.channels = (uint16_t)ch;
    c.buffer_secs = 1.0f;
    c.seed = 7;
    c.max_batch_hops = batch;
    return c;
}

// offline host call, three uneven device ranges, and the streaming seam (closed first / open) on one engine
static void engine_paths(uint32_t N, float f, int p, uint32_t ch, size_t L, const std::string &code) {
    rc_config c = config(N, f, p, ch, 1);  // batches of one window
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&c, &e) == RC_OK);
    CHECK(rc_engine_load_device_kernel(e, code.data(), code.size()) == RC_OK);
    const float w[4] = {0.4f, 0.3f, 0.2f, 0.1f};
    CHECK(rc_engine_set_device_kernel_params(e, w, 4) == RC_OK);
    rc_params P;
    CHECK(rc_engine_get_params(e, &P) == RC_OK);
    // every buffer exactly as long as the call says: a span that starts too early or ends too late is a finding
    std::vector<std::vector<float>> x(ch, std::vector<float>(L, 0.25f));
    const size_t n_out = rc_offline_output_len(&c, L);
    std::vector<std::vector<float>> y(ch, std::vector<float>(n_out));
    std::vector<const float *> in;
    std::vector<float *> out;
    for (uint32_t i = 0; i < ch; ++i) {
        in.push_back(x[i].data());
        out.push_back(y[i].data());
    }
    size_t got = 0;
    CHECK(rc_engine_stretch_host(e, in.data(), L, out.data(), n_out, &got) == RC_OK && got == n_out);
    uint32_t launches_hist = 0, launches_plain = 0;
    float *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc((void **)&d_in, (size_t)ch * L * sizeof(float)) == 0);
    CHECK(hipMalloc((void **)&d_out, (size_t)ch * n_out * sizeof(float)) == 0);
    CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && got == n_out);
    CHECK(rc_engine_last_kernel_stats(e, nullptr, nullptr, &launches_hist) == RC_OK);
    const uint64_t wins = n_out / P.window_out_len;
    const uint64_t cut[4] = {0, wins / 5, wins / 5 + 1 + wins / 2, wins};
    for (int r = 0; r < 3; ++r)
        if (cut[r + 1] > cut[r] && cut[r + 1] <= wins)
            CHECK(rc_engine_stretch_device_range(e, d_in, L, L, 0, ch, cut[r], cut[r + 1] - cut[r],
                                                 d_out + cut[r] * P.window_out_len, n_out,
                                                 (size_t)((cut[r + 1] - cut[r]) * P.window_out_len), nullptr) == RC_OK);
    // the same call without history reports the same number of launches: the halo rides in the analysis launches
    const std::string plain = fake_code_object(0);
    CHECK(rc_engine_load_device_kernel(e, plain.data(), plain.size()) == RC_OK);
    CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK);
    CHECK(rc_engine_last_kernel_stats(e, nullptr, nullptr, &launches_plain) == RC_OK);
    CHECK(launches_hist == launches_plain);
    CHECK(rc_engine_synchronize(e) == RC_OK);
    hipFree(d_in);
    hipFree(d_out);
    rc_engine_destroy(e);
    for (int open = 0; open < 2; ++open) {  // the seam; the open stream swaps depth 0 -> 3 -> 0 while it runs
        CHECK(rc_engine_create(&c, &e) == RC_OK);
        const std::string &first = open ? plain : code;
        CHECK(rc_engine_load_device_kernel(e, first.data(), first.size()) == RC_OK);
        for (uint32_t i = 0; i < ch; ++i) {
            CHECK(rc_engine_push_input(e, i, x[i].data(), L) == RC_OK);
            if (!open) CHECK(rc_engine_close_input(e, i) == RC_OK);
        }
        std::vector<float> win(P.window_out_len);
        size_t total = 0, n = 0, handed = 0;
        std::vector<bool> done(ch, false);
        for (bool any = true; any;) {
            any = false;
            for (uint32_t i = 0; i < ch; ++i) {
                if (done[i]) continue;
                any = true;
                const int rc = rc_engine_next_window(e, i, win.data(), win.size(), &n);
                if (rc == RC_WOULD_BLOCK) {
                    CHECK(open);
                    CHECK(rc_engine_close_input(e, i) == RC_OK);
                    continue;
                }
                CHECK(rc == RC_OK);
                total += n;
                done[i] = rc_engine_is_done(e, i) == 1;
                if (open && ++handed == 6 * ch) CHECK(rc_engine_load_device_kernel(e, code.data(), code.size()) == RC_OK);
                if (open && handed == 11 * ch) CHECK(rc_engine_load_device_kernel(e, plain.data(), plain.size()) == RC_OK);
            }
        }
        CHECK(total == (size_t)ch * n_out);
        rc_engine_destroy(e);
    }
}

static void multi(const std::vector<int32_t> &devs, uint32_t N, float f, uint32_t ch, size_t L, const std::string &code) {
    rc_config c = config(N, f, 1, ch);
    rc_multi *m = nullptr;
    CHECK(rc_multi_create(&c, devs.data(), (uint32_t)devs.size(), &m) == RC_OK);
    CHECK(rc_multi_load_device_kernel(m, code.data(), code.size()) == RC_OK);
    std::vector<std::vector<float>> x(ch, std::vector<float>(L, 0.25f));
    const size_t n_out = rc_offline_output_len(&c, L);
    std::vector<std::vector<float>> y(ch, std::vector<float>(n_out));
    std::vector<const float *> in;
    std::vector<float *> out;
    for (uint32_t i = 0; i < ch; ++i) {
        in.push_back(x[i].data());
        out.push_back(y[i].data());
    }
    size_t got = 0;
    CHECK(rc_multi_stretch_host(m, in.data(), L, out.data(), n_out, &got) == RC_OK && got == n_out);
    rc_engine *probe = nullptr;
    rc_config c1 = c;
    c1.device = devs[0];
    CHECK(rc_engine_create(&c1, &probe) == RC_OK);
    hipSetDevice(devs[0]);
    float *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc((void **)&d_in, (size_t)ch * L * sizeof(float)) == 0);
    CHECK(hipMalloc((void **)&d_out, (size_t)ch * n_out * sizeof(float)) == 0);
    for (int staged = 0; staged < 2; ++staged) {
        CHECK(rc_multi_set_staging(m, staged) == RC_OK);
        CHECK(rc_multi_stretch_device(m, 0, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && got == n_out);
    }
    CHECK(rc_multi_load_device_kernel(m, nullptr, 0) == RC_OK);  // and without a kernel again: today's spans
    CHECK(rc_multi_stretch_device(m, 0, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && got == n_out);
    hipFree(d_in);
    hipFree(d_out);
    rc_engine_destroy(probe);
    rc_multi_destroy(m);
}

int main() {
    const std::string code = fake_code_object(4);  // RC_HISTORY 3
    {  // the loader's check: a depth above the maximum and a marker of no bytes are refused, and nothing is loaded
        rc_config c = config(1024, 4.0f, 1, 1);
        rc_engine *e = nullptr;
        CHECK(rc_engine_create(&c, &e) == RC_OK);
        const std::string deep = fake_code_object(10), cut = code.substr(0, code.size() - 40);
        CHECK(rc_engine_load_device_kernel(e, deep.data(), deep.size()) == RC_EINVAL);
        CHECK(rc_engine_load_device_kernel(e, cut.data(), cut.size()) == RC_EINVAL);
        const std::string max = fake_code_object(9);
        CHECK(rc_engine_load_device_kernel(e, max.data(), max.size()) == RC_OK);
        rc_engine_destroy(e);
    }
    engine_paths(1024, 4.0f, 1, 2, 40 * 1024 + 77, code);    // Hop
    engine_paths(1024, 4.0f, -2, 2, 20 * 1024 + 5, code);    // negative pitch: one hop per window
    engine_paths(12288, 4.0f, 3, 1, 12 * 12288 + 1, code);   // Gen
    // Long path, stereo: a chunk holds about 170 hops, so this job (step 16384, ~400 hops) crosses two chunk boundaries
    engine_paths(131072, 4.0f, 1, 2, (size_t)400 * 16384 + 131072, code);
    multi({0, 0}, 4096, 4.0f, 2, 30 * 4096, code);
    multi({0, 1, 2}, 2048, 2.0f, 3, 50 * 2048 + 3, code);
    printf("engine_host_driver_dk: ok\n");
    return 0;
}
