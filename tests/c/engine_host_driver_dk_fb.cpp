// TEST INFRASTRUCTURE: the engine's host code with a user device kernel that declares RC_FEEDBACK loaded, over the HIP
// stub (tests/c/hip_stub.cpp; tests/c/hip_stub_rtc_fb.cpp logs every module lookup and launch and walks the ring rows of
// every launch) under ASan + UBSan (rocoder_amd/csrc/host/sanitize.mk: engine_dk_fb_asan). Checked: the launches of a
// chunk in both shapes, the size of the state, the four ways a call may start (restart, continue, first call after a
// load, anything else), that a refused call enqueues nothing and leaves the ring as it was, that rc_multi refuses such a
// kernel, and that a rejected code object leaves the loaded kernel running. The stub's overlap-add computes nothing, so
// the tail itself is held by the GPU tests; here a refusal is shown to return before any launch or memset. The code
// object is a hand-made ELF that carries only what the loader's check reads: the machine, and the symbols.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rocoder_hip.h"
#include "hip_stub_rtc_fb.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rc_last_error()); \
            exit(2);                                                             \
        }                                                                        \
    } while (0)

static void put(std::string &b, size_t off, uint64_t v, size_t n) {
    for (size_t i = 0; i < n; ++i) b[off + i] = (char)(v >> (8 * i));
}
// ELF64 / EM_AMDGPU / gfx950 with a string table and a symbol table of the given (name, size) symbols
static std::string fake_code_object(const std::vector<std::pair<std::string, uint64_t>> &syms) {
    std::string strtab(1, '\0');
    std::vector<size_t> name_at;
    for (const auto &s : syms) {
        name_at.push_back(strtab.size());
        strtab += s.first;
        strtab += '\0';
    }
    const size_t n_sym = syms.size() + 1, str_off = 64, sym_off = (str_off + strtab.size() + 7) / 8 * 8;
    const size_t sh_off = sym_off + 24 * n_sym;
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
    for (size_t i = 0; i < syms.size(); ++i) {
        put(b, sym_off + 24 * (i + 1), name_at[i], 4);
        put(b, sym_off + 24 * (i + 1) + 16, syms[i].second, 8);
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
// a kernel with RC_FEEDBACK `fb` (0: no marker), RC_HISTORY `hist`, RC_CROSS_CHANNEL `cross` and RC_SUMS `sums`
static std::string kernel_object(uint32_t fb, uint32_t hist = 0, bool cross = false, uint32_t sums = 0) {
    std::vector<std::pair<std::string, uint64_t>> s = {{"rc_user_dk", 0}, {"rc_user_dk_history", hist + 1}};
    if (cross) s.push_back({"rc_user_dk_channels", 1});
    if (sums) {
        s.push_back({"rc_user_dk_sums", sums + 1});
        s.push_back({"rc_user_dk_sums_pass", 0});
    }
    if (fb) s.push_back({"rc_user_dk_feedback", fb + 1});
    return fake_code_object(s);
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

struct Job {
    rc_config c;
    rc_engine *e = nullptr;
    rc_params P;
    std::vector<std::vector<float>> x, y;
    std::vector<const float *> in;
    std::vector<float *> out;
    size_t L, n_out;
    float *d_in = nullptr, *d_out = nullptr;
    Job(uint32_t N, float f, int p, uint32_t ch, size_t len, uint32_t batch = 0) : c(config(N, f, p, ch, batch)), L(len) {
        CHECK(rc_engine_create(&c, &e) == RC_OK);
        CHECK(rc_engine_get_params(e, &P) == RC_OK);
        n_out = rc_offline_output_len(&c, L);
        x.assign(ch, std::vector<float>(L, 0.25f));
        y.assign(ch, std::vector<float>(n_out));
        for (uint32_t i = 0; i < ch; ++i) {
            in.push_back(x[i].data());
            out.push_back(y[i].data());
        }
        CHECK(hipMalloc((void **)&d_in, (size_t)ch * L * sizeof(float)) == hipSuccess);
        CHECK(hipMalloc((void **)&d_out, (size_t)ch * n_out * sizeof(float)) == hipSuccess);
    }
    ~Job() {
        rc_engine_destroy(e);
        (void)hipFree(d_in);
        (void)hipFree(d_out);
    }
    void load(const std::string &code) { CHECK(rc_engine_load_device_kernel(e, code.data(), code.size()) == RC_OK); }
    void host() {
        size_t got = 0;
        CHECK(rc_engine_stretch_host(e, in.data(), L, out.data(), n_out, &got) == RC_OK && got == n_out);
    }
    uint64_t wins() const { return n_out / P.window_out_len; }
    int range(uint32_t ch_first, uint32_t ch_count, uint64_t w0, uint64_t w1) {
        const int rc = rc_engine_stretch_device_range(e, d_in, L, L, ch_first, ch_count, w0, w1 - w0,
                                                      d_out + (size_t)ch_first * n_out + w0 * P.window_out_len, n_out,
                                                      (size_t)((w1 - w0) * P.window_out_len), nullptr);
        if (rc == RC_OK) CHECK(rc_engine_synchronize(e) == RC_OK);
        return rc;
    }
};

// The kernel launches of a log, chunk by chunk, in hop order: in the loop shape a chunk is one launch of grid (1, channels)
// over all its hops, in the per-hop shape one launch of grid (ceil(n / 256), channels) per hop, ascending. Returns the hops
// [first, last] the log covers for its channels, which must be consecutive; every launch carries the same state of
// channels x (F + 1) x N bins.
struct Span {
    int64_t first = -1, next = -1;
    size_t launches = 0, chunks = 0;
    const float2 *state = nullptr;
};
static Span verify(const std::vector<RtcFbLaunch> &log, uint32_t F, uint32_t N, uint32_t channels, bool per_hop) {
    Span sp;
    for (const RtcFbLaunch &l : log) {
        if (l.pass) continue;  // (a sums pass in front of a chunk)
        const rc::UserDkArgs &a = l.a;
        CHECK(a.state != nullptr && a.feedback == F && a.n == N && a.channels == channels);
        CHECK(l.state_bytes == (size_t)channels * (F + 1) * N * sizeof(float2));  // exactly what the load reserved
        CHECK(sp.state == nullptr || sp.state == a.state);
        sp.state = a.state;
        CHECK(l.bx == 256 && l.gz == 1 && l.gy >= 1 && a.ch_first + a.row_first + l.gy <= channels);
        if (per_hop) CHECK(l.gx == (N + 255) / 256 && a.fb_hop_count == 1);
        else CHECK(l.gx == 1 && a.fb_hop_first == 0 && a.fb_hop_count == a.hop_count);
        const int64_t k = a.hop_first + (int64_t)a.fb_hop_first;
        if (sp.first < 0) sp.first = k;
        else CHECK(k == sp.next);  // hop order, nothing skipped, nothing run twice
        sp.next = k + a.fb_hop_count;
        if (a.fb_hop_first == 0) ++sp.chunks;
        ++sp.launches;
    }
    return sp;
}

// the ring's first bins, as the stub left them
static std::vector<float> ring_marks(const Span &sp, uint32_t F, uint32_t N, uint32_t channels) {
    std::vector<float> v;
    for (size_t r = 0; r < (size_t)channels * (F + 1); ++r) v.push_back(sp.state[r * N].x);
    return v;
}

static void paths(uint32_t N, float f, int p, uint32_t ch, size_t L, uint32_t F, uint32_t hist, bool cross, uint32_t sums) {
    const bool per_hop = N > rc::kFeedbackLoopMaxN;
    const std::string code = kernel_object(F, hist, cross, sums);
    Job j(N, f, p, ch, L);
    (void)rtc_fb_stub_take_lookups();
    j.load(code);
    CHECK(rtc_fb_stub_take_lookups().size() == (sums ? 2u : 1u));
    const uint64_t hops = j.wins() * j.P.hops_per_window;
    // a whole job through the host pipeline: restart at 0, then its chunks continue
    (void)rtc_fb_stub_take_launches();
    j.host();
    Span s = verify(rtc_fb_stub_take_launches(), F, N, ch, per_hop);
    CHECK(s.first == 0 && s.next == (int64_t)hops && s.chunks >= 1);
    CHECK(s.launches == (per_hop ? hops : s.chunks));
    // the device entry: the launch statistics count the launches actually made
    (void)rtc_fb_stub_take_launches();
    CHECK(j.range(0, ch, 0, j.wins()) == RC_OK);
    std::vector<RtcFbLaunch> log = rtc_fb_stub_take_launches();
    s = verify(log, F, N, ch, per_hop);
    CHECK(s.first == 0 && s.next == (int64_t)hops);
    uint32_t launches = 0;
    CHECK(rc_engine_last_kernel_stats(j.e, nullptr, nullptr, &launches) == RC_OK);
    CHECK(launches >= log.size() + 3 * s.chunks);  // analysis, synthesis and the overlap-add's two per chunk beside them
    // restart, continue, continue; every cut starts at its own first hop (hop k0 - 1 is not run again)
    const uint64_t w = j.wins(), cut[4] = {0, 1, w / 3 + 2, w};
    for (int r = 0; r < 3; ++r) {
        (void)rtc_fb_stub_take_launches();
        CHECK(j.range(0, ch, cut[r], cut[r + 1]) == RC_OK);
        s = verify(rtc_fb_stub_take_launches(), F, N, ch, per_hop);
        CHECK(s.first == (int64_t)(cut[r] * j.P.hops_per_window) && s.next == (int64_t)(cut[r + 1] * j.P.hops_per_window));
    }
    // anything else: refused with the hop expected, nothing enqueued, the ring as it was; then the in-order call runs
    CHECK(j.range(0, ch, 0, 2) == RC_OK);
    s = verify(rtc_fb_stub_take_launches(), F, N, ch, per_hop);
    const std::vector<float> before = ring_marks(s, F, N, ch);
    const std::string want = "hop " + std::to_string(2 * j.P.hops_per_window) + " ";
    for (uint64_t w0 : {(uint64_t)3, (uint64_t)1, w - 1}) {
        CHECK(j.range(0, ch, w0, w0 + 1) == RC_EINVAL);
        CHECK(std::string(rc_last_error()).find(want) != std::string::npos);
        CHECK(rtc_fb_stub_take_launches().empty());
        CHECK(ring_marks(s, F, N, ch) == before);
    }
    if (ch > 1) {  // channels in different cases: channel 0 alone moves on, then both are asked for
        CHECK(j.range(0, 1, 2, 3) == RC_OK);
        (void)rtc_fb_stub_take_launches();
        CHECK(j.range(0, ch, 3, 4) == RC_EINVAL);
        CHECK(j.range(0, ch, 2, 3) == RC_EINVAL);
        CHECK(rtc_fb_stub_take_launches().empty());
        CHECK(j.range(1, ch - 1, 2, 3) == RC_OK);  // the others catch up
    } else {
        CHECK(j.range(0, 1, 2, 3) == RC_OK);
    }
    (void)rtc_fb_stub_take_launches();
    CHECK(j.range(0, ch, 3, w) == RC_OK);
    s = verify(rtc_fb_stub_take_launches(), F, N, ch, per_hop);
    CHECK(s.first == (int64_t)(3 * j.P.hops_per_window) && s.next == (int64_t)hops);
    // the first call after a load, with k0 > 0: hop k0 - 1 runs once, alone, in front (for its tail; its output enters
    // the state), into a zeroed ring
    j.load(code);
    (void)rtc_fb_stub_take_launches();
    CHECK(j.range(0, ch, 2, 4) == RC_OK);
    log = rtc_fb_stub_take_launches();
    s = verify(log, F, N, ch, per_hop);
    const int64_t k0 = 2 * j.P.hops_per_window;
    CHECK(s.first == k0 - 1 && s.next == (int64_t)(4 * j.P.hops_per_window));
    for (const RtcFbLaunch &l : log)
        if (!l.pass) {
            CHECK(l.a.hop_first == k0 - 1 && l.a.hop_count == 1);
            break;
        }
    {   // the ring holds the marks of the hops this kernel ran and zeros elsewhere
        const std::vector<float> m = ring_marks(s, F, N, ch);
        for (uint32_t c = 0; c < ch; ++c)
            for (uint32_t slot = 0; slot <= F; ++slot) {
                float newest = 0.f;  // the latest hop in [k0 - 1, next) that maps to this slot
                for (int64_t k = k0 - 1; k < s.next; ++k)
                    if ((uint64_t)k % (F + 1) == slot) newest = (float)k;
                CHECK(m[c * (F + 1) + slot] == newest);
            }
    }
    // a single frame carries no state and does not move the books
    std::vector<float> frame(N, 0.5f), back(N);
    (void)rtc_fb_stub_take_launches();
    CHECK(rc_engine_resynth(j.e, ch - 1, 9, frame.data(), back.data()) == RC_OK);
    log = rtc_fb_stub_take_launches();
    CHECK(!log.empty() && log.back().pass == 0 && log.back().a.state == nullptr && log.back().a.feedback == 0);
    CHECK(log.back().a.fb_hop_count == 1 && log.back().gy == 1);
    CHECK(j.range(0, ch, 4, 5) == RC_OK);
}

// the seam, batches of one window, closed first: every channel's hops in order from 0
static void seam(uint32_t N, float f, uint32_t ch, size_t L, uint32_t F) {
    Job j(N, f, 1, ch, L, 1);
    j.load(kernel_object(F));
    (void)rtc_fb_stub_take_launches();
    for (uint32_t i = 0; i < ch; ++i) {
        CHECK(rc_engine_push_input(j.e, i, j.x[i].data(), L) == RC_OK);
        CHECK(rc_engine_close_input(j.e, i) == RC_OK);
    }
    std::vector<float> win(j.P.window_out_len);
    std::vector<size_t> total(ch, 0);
    for (bool any = true; any;) {
        any = false;
        for (uint32_t i = 0; i < ch; ++i) {
            if (rc_engine_is_done(j.e, i) == 1) continue;
            any = true;
            size_t n = 0;
            CHECK(rc_engine_next_window(j.e, i, win.data(), win.size(), &n) == RC_OK);
            total[i] += n;
        }
    }
    for (uint32_t i = 0; i < ch; ++i) CHECK(total[i] == j.n_out);
    const Span s = verify(rtc_fb_stub_take_launches(), F, N, ch, N > rc::kFeedbackLoopMaxN);
    CHECK(s.first == 0 && s.chunks >= 2);
}

int main() {
    paths(1024, 4.0f, 1, 2, 40 * 1024 + 77, 1, 0, false, 0);      // the loop shape
    paths(1024, 4.0f, -2, 3, 20 * 1024 + 5, 4, 2, true, 2);       // with a halo, cross-channel blocks and a sums pass
    paths(1000, 4.0f, 1, 1, 30 * 1000, 2, 0, false, 0);           // Gen, one channel
    paths(8192, 4.0f, 1, 2, 20 * 8192 + 9, 2, 1, false, 0);       // the per-hop shape
    paths(65536, 8.0f, 1, 2, 12 * 65536 + 333, 3, 0, false, 1);    // Big
    paths(131072, 4.0f, 1, 2, 12 * 131072 + 333, 4, 0, true, 0);   // Long
    seam(1024, 4.0f, 2, 40 * 1024 + 77, 2);
    seam(8192, 4.0f, 2, 12 * 8192, 1);
    {
        // rc_multi refuses such a kernel and keeps the one it runs
        rc_config c = config(1024, 4.0f, 1, 2);
        const int32_t devs[2] = {0, 0};
        rc_multi *m = nullptr;
        CHECK(rc_multi_create(&c, devs, 2, &m) == RC_OK);
        const std::string plain = kernel_object(0, 1), fb = kernel_object(2, 1);
        CHECK(rc_multi_load_device_kernel(m, plain.data(), plain.size()) == RC_OK);
        (void)rtc_fb_stub_take_lookups();
        CHECK(rc_multi_load_device_kernel(m, fb.data(), fb.size()) == RC_EUNSUPPORTED);
        CHECK(std::string(rc_last_error()).find("in order") != std::string::npos);
        CHECK(rtc_fb_stub_take_lookups().empty());  // (never reached the runtime)
        const size_t L = 40 * 1024, n_out = rc_offline_output_len(&c, L);
        std::vector<std::vector<float>> x(2, std::vector<float>(L, 0.25f)), y(2, std::vector<float>(n_out));
        const float *in[2] = {x[0].data(), x[1].data()};
        float *out[2] = {y[0].data(), y[1].data()};
        size_t got = 0;
        (void)rtc_fb_stub_take_launches();
        CHECK(rc_multi_stretch_host(m, in, L, out, n_out, &got) == RC_OK && got == n_out);
        const std::vector<RtcFbLaunch> log = rtc_fb_stub_take_launches();
        CHECK(!log.empty());
        for (const RtcFbLaunch &l : log) CHECK(l.pass == 0 && l.a.state == nullptr && l.a.feedback == 0);
        rc_multi_destroy(m);
    }
    {
        // every rejected code object leaves the loaded kernel (F = 2) and its books in place
        Job j(1024, 4.0f, 1, 2, 40 * 1024 + 77);
        j.load(kernel_object(2));
        CHECK(j.range(0, 2, 0, 2) == RC_OK);
        std::vector<std::string> bad;
        bad.push_back(fake_code_object({{"rc_user_dk", 0}, {"rc_user_dk_feedback", 6}}));  // F = 5
        bad.push_back(fake_code_object({{"rc_user_dk", 0}, {"rc_user_dk_feedback", 1}}));  // a marker of one byte
        bad.push_back(fake_code_object({{"rc_user_dk", 0}, {"rc_user_dk_feedback", 0}}));
        bad.push_back(fake_code_object({{"rc_user_dk_feedback", 3}}));                     // no kernel
        bad.push_back(std::string(200, '\0'));
        bad.push_back(kernel_object(2).substr(0, 100));  // cut short
        (void)rtc_fb_stub_take_lookups();
        uint64_t w = 2;
        for (const std::string &b : bad) {
            CHECK(rc_engine_load_device_kernel(j.e, b.data(), b.size()) == RC_EINVAL);
            CHECK(rtc_fb_stub_take_lookups().empty());
            (void)rtc_fb_stub_take_launches();
            CHECK(j.range(0, 2, w, w + 1) == RC_OK);  // still in order: the books were not reset
            const Span s = verify(rtc_fb_stub_take_launches(), 2, 1024, 2, false);
            CHECK(s.first == (int64_t)(w * j.P.hops_per_window));
            ++w;
        }
        // an undeclared kernel takes the feedback kernel's place: no state, any order
        j.load(kernel_object(0));
        (void)rtc_fb_stub_take_launches();
        CHECK(j.range(0, 2, 5, 6) == RC_OK && j.range(0, 2, 1, 2) == RC_OK);
        for (const RtcFbLaunch &l : rtc_fb_stub_take_launches()) CHECK(l.a.state == nullptr && l.a.feedback == 0);
    }
    printf("engine_host_driver_dk_fb: ok\n");
    return 0;
}
