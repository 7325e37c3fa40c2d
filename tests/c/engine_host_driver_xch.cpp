// TEST INFRASTRUCTURE: the engine's host code with a user device kernel that declares RC_CROSS_CHANNEL (and RC_HISTORY 2)
// loaded, over the HIP stub (tests/c/hip_stub.cpp: device memory is host memory, kernels compute nothing) under ASan +
// UBSan (rocoder_amd/csrc/host/sanitize.mk: engine_xch_asan). What runs for real is the bookkeeping around the block of
// all channels: chunk sizes and reserves, the input spans of channel-subset ranges, streaming batches (every channel's
// span, zero padded) and rc_multi shards, and the stream rules. The code object is a hand-made ELF that carries only
// what the loader's check reads: the machine, and the symbols.
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
// ELF64 / EM_AMDGPU / gfx950 with a string table and a symbol table: rc_user_dk, rc_user_dk_history of `hist_size`
// bytes, and, when `cross`, rc_user_dk_channels
static std::string fake_code_object(uint64_t hist_size, bool cross) {
    const std::string strtab = std::string("\0rc_user_dk\0rc_user_dk_history\0rc_user_dk_channels\0", 51);
    const size_t n_sym = cross ? 4 : 3, str_off = 64, sym_off = 128, sh_off = sym_off + 24 * 4;
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
    put(b, sym_off + 48, 12, 4);  // symbol 2: rc_user_dk_history
    put(b, sym_off + 48 + 16, hist_size, 8);
    if (cross) {
        put(b, sym_off + 72, 31, 4);  // symbol 3: rc_user_dk_channels
        put(b, sym_off + 72 + 16, 1, 8);
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

// offline host and device calls, every channel on its own through the range form (and a window cut), and the seam
static void engine_paths(uint32_t N, float f, int p, uint32_t ch, size_t L, const std::string &code, const std::string &plain) {
    rc_config c = config(N, f, p, ch, 1);  // batches of one window
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&c, &e) == RC_OK);
    CHECK(rc_engine_load_device_kernel(e, code.data(), code.size()) == RC_OK);
    const float w[2] = {1.0f, 0.5f};
    CHECK(rc_engine_set_device_kernel_params(e, w, 2) == RC_OK);
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
    float *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc((void **)&d_in, (size_t)ch * L * sizeof(float)) == 0);
    CHECK(hipMalloc((void **)&d_out, (size_t)ch * n_out * sizeof(float)) == 0);
    CHECK(rc_engine_stretch_device(e, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && got == n_out);
    const uint64_t wins = n_out / P.window_out_len;
    const uint64_t cut[3] = {0, wins / 3 + 1, wins};
    for (uint32_t i = 0; i < ch; ++i)  // one channel of the job at a time: the analysis still reads all of d_in
        for (int r = 0; r < 2; ++r)
            if (cut[r + 1] > cut[r] && cut[r + 1] <= wins)
                CHECK(rc_engine_stretch_device_range(e, d_in, L, L, i, 1, cut[r], cut[r + 1] - cut[r],
                                                     d_out + (size_t)i * n_out + cut[r] * P.window_out_len, n_out,
                                                     (size_t)((cut[r + 1] - cut[r]) * P.window_out_len), nullptr) == RC_OK);
    CHECK(rc_engine_synchronize(e) == RC_OK);
    hipFree(d_in);
    hipFree(d_out);
    rc_engine_destroy(e);
    // the seam: channel 0 is shorter than the others by a few hops. Closed first, or open and closed at the shortfall.
    const size_t L0 = L - std::min<size_t>(L / 2, 3 * (size_t)P.sample_step_len + 11);
    for (int open = 0; open < 2; ++open) {
        CHECK(rc_engine_create(&c, &e) == RC_OK);
        CHECK(rc_engine_load_device_kernel(e, code.data(), code.size()) == RC_OK);
        std::vector<float> win(P.window_out_len);
        size_t n = 0;
        if (open && ch > 1) {
            // the sibling lacks input: channel 0 alone holds enough for its first window and still has to wait
            CHECK(rc_engine_push_input(e, 0, x[0].data(), L0) == RC_OK);
            CHECK(rc_engine_next_window(e, 0, win.data(), win.size(), &n) == RC_WOULD_BLOCK);
            for (uint32_t i = 1; i < ch; ++i) CHECK(rc_engine_push_input(e, i, x[i].data(), L) == RC_OK);
        } else {
            for (uint32_t i = 0; i < ch; ++i) {
                CHECK(rc_engine_push_input(e, i, x[i].data(), i == 0 ? L0 : L) == RC_OK);
                if (!open) CHECK(rc_engine_close_input(e, i) == RC_OK);
            }
        }
        size_t handed = 0;
        std::vector<size_t> total(ch, 0);
        std::vector<bool> done(ch, false);
        for (bool any = true; any;) {
            any = false;
            for (uint32_t i = 0; i < ch; ++i) {
                if (done[i]) continue;
                any = true;
                const int rc = rc_engine_next_window(e, i, win.data(), win.size(), &n);
                if (rc == RC_WOULD_BLOCK) {
                    CHECK(open);
                    // nothing more comes: the channel that has run out is closed; a channel that waits for an open
                    // sibling goes on once that one is closed
                    for (uint32_t j = 0; j < ch; ++j) CHECK(rc_engine_close_input(e, j) == RC_OK);
                    continue;
                }
                CHECK(rc == RC_OK);
                total[i] += n;
                done[i] = rc_engine_is_done(e, i) == 1;
                ++handed;
                if (ch > 1 && handed == 1) {
                    // channel 0 is one window ahead of the others: a kernel that reads them cannot be loaded now, the
                    // loaded one stays; one that does not can
                    CHECK(rc_engine_load_device_kernel(e, code.data(), code.size()) == RC_EINVAL);
                    CHECK(rc_engine_load_device_kernel(e, plain.data(), plain.size()) == RC_OK);
                }
                if (handed == ch) CHECK(rc_engine_load_device_kernel(e, code.data(), code.size()) == RC_OK);  // between rounds
            }
        }
        CHECK(total[0] == rc_offline_output_len(&c, L0));
        for (uint32_t i = 1; i < ch; ++i) CHECK(total[i] == n_out);
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
    hipSetDevice(devs[0]);
    float *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc((void **)&d_in, (size_t)ch * L * sizeof(float)) == 0);
    CHECK(hipMalloc((void **)&d_out, (size_t)ch * n_out * sizeof(float)) == 0);
    for (int staged = 0; staged < 2; ++staged) {
        CHECK(rc_multi_set_staging(m, staged) == RC_OK);
        CHECK(rc_multi_stretch_device(m, 0, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && got == n_out);
    }
    CHECK(rc_multi_load_device_kernel(m, nullptr, 0) == RC_OK);  // and without a kernel again: the shards' own channels
    CHECK(rc_multi_stretch_device(m, 0, d_in, L, L, d_out, n_out, n_out, &got, nullptr) == RC_OK && got == n_out);
    hipFree(d_in);
    hipFree(d_out);
    rc_multi_destroy(m);
}

int main() {
    const std::string code = fake_code_object(3, true);    // RC_CROSS_CHANNEL 1, RC_HISTORY 2
    const std::string plain = fake_code_object(1, false);  // neither
    const std::vector<int32_t> four = {0, 1, 2, 3};
    engine_paths(1024, 4.0f, 1, 2, 40 * 1024 + 77, code, plain);    // Hop
    engine_paths(1024, 4.0f, -2, 3, 20 * 1024 + 5, code, plain);    // negative pitch: one hop per window, three channels
    engine_paths(65536, 8.0f, 1, 2, 5 * 65536 + 333, code, plain);  // Big
    engine_paths(12288, 4.0f, 3, 2, 12 * 12288 + 1, code, plain);   // Gen
    engine_paths(131072, 4.0f, 1, 2, 5 * 131072 + 333, code, plain);  // Long
    multi(four, 1024, 4.0f, 2, 40 * 1024 + 77, code);    // shards: parts of ONE channel, all channels' input
    multi(four, 65536, 8.0f, 2, 5 * 65536 + 333, code);
    multi(four, 12288, 4.0f, 3, 12 * 12288 + 1, code);
    multi(four, 131072, 4.0f, 2, 5 * 131072 + 333, code);
    multi({0, 0}, 4096, 4.0f, 8, 30 * 4096, code);       // blocks of WHOLE channels
    printf("engine_host_driver_xch: ok\n");
    return 0;
}
