// TEST INFRASTRUCTURE: the engine's host code with a user device kernel that declares RC_SUMS loaded, over the HIP stub
// (tests/c/hip_stub.cpp; tests/c/hip_stub_rtc_sums.cpp logs every module lookup and launch and lets the pass write its
// rows) under ASan + UBSan (rocoder_amd/csrc/host/sanitize.mk: engine_dk_sums_asan). Checked: the size of the sums
// scratch, the row count and the grid chunks of the pass for jobs with a halo, with cross-channel blocks and with more
// than 32768 rows, that the pass precedes the kernel on the same stream, that an undeclared module causes no second
// lookup and gets no sums, and that every rejected code object leaves the previous kernel loaded. The code object is a
// hand-made ELF that carries only what the loader's check reads: the machine, and the symbols.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rocoder_hip.h"
#include "hip_stub_rtc_sums.h"

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
// a kernel with RC_HISTORY `hist`, RC_CROSS_CHANNEL `cross` and RC_SUMS `sums` (0: no marker and no pass)
static std::string kernel_object(uint32_t hist, bool cross, uint32_t sums) {
    std::vector<std::pair<std::string, uint64_t>> s = {{"rc_user_dk", 0}, {"rc_user_dk_history", hist + 1}};
    if (cross) s.push_back({"rc_user_dk_channels", 1});
    if (sums) {
        s.push_back({"rc_user_dk_sums", sums + 1});
        s.push_back({"rc_user_dk_sums_pass", 0});
    }
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

struct Seen {
    size_t groups = 0;      // pass + kernel pairs
    uint64_t max_rows = 0;  // the largest pass
    uint64_t pass_launches = 0;
};

// The log of one or more jobs of a kernel with S sums, history `hist` and, when `cross`, all `channels` in the block:
// groups of [pass chunks][kernel chunks]. Every pass covers in_ch_count * (halo + hop_count) rows in chunks of at most
// 32768 from row 0 on, writes into an allocation that holds them, and is followed at once by its kernel on the same
// stream with the same block.
// *running_max (when given) carries the largest pass of the engine's earlier jobs, whose scratch the engine still holds.
static Seen verify(const std::vector<RtcSumsLaunch> &log, uint32_t S, uint32_t hist, bool cross, uint32_t channels,
                   uint64_t *running_max = nullptr) {
    Seen seen;
    size_t i = 0;
    uint64_t max_bytes = running_max ? *running_max : 0;
    std::vector<size_t> allocated;
    while (i < log.size()) {
        const RtcSumsLaunch &first = log[i];
        CHECK(first.pass == 1);  // a kernel never runs without its pass in front
        const rc::UserDkArgs &a = first.a;
        CHECK(a.sums != nullptr && a.n_sums == S);
        CHECK(a.in_rows == a.halo + a.hop_count && a.halo <= hist);
        CHECK(a.halo == (uint32_t)std::min<int64_t>(hist, a.hop_first));
        CHECK(cross ? (a.in_ch_first == 0 && a.in_ch_count == channels) : a.in_ch_first == a.ch_first);
        const uint64_t rows = (uint64_t)a.in_ch_count * a.in_rows;
        uint64_t at = 0;
        for (; i < log.size() && log[i].pass == 1 && (at == 0 || log[i].a.row_first != 0); ++i) {
            const RtcSumsLaunch &l = log[i];
            CHECK(l.gx == 1 && l.gz == 1 && l.bx == 256 && l.gy >= 1 && l.gy <= 32768);
            CHECK(l.a.row_first == at && l.stream == first.stream);
            CHECK(l.a.sums == a.sums && l.a.in == a.in && l.a.in_rows == a.in_rows && l.a.halo == a.halo);
            CHECK(at + l.gy == rows || l.gy == 32768);  // only the last chunk is short
            at += l.gy;
            ++seen.pass_launches;
        }
        CHECK(at == rows);
        // the scratch: one allocation that starts at the first halo row's sums and holds every row's
        const size_t have = first.scratch_bytes;
        CHECK(have >= rows * S * sizeof(float));
        allocated.push_back(have);
        max_bytes = std::max<uint64_t>(max_bytes, rows * S * sizeof(float));
        // the kernel: at once, on the same stream, on the same block
        CHECK(i < log.size() && log[i].pass == 0);
        uint64_t out_at = 0;
        for (; i < log.size() && log[i].pass == 0; ++i) {
            const RtcSumsLaunch &l = log[i];
            CHECK(l.stream == first.stream && l.a.sums == a.sums && l.a.n_sums == S && l.a.in == a.in && l.a.out != nullptr);
            CHECK(l.a.hop_first == a.hop_first && l.a.hop_count == a.hop_count && l.a.in_rows == a.in_rows);
            CHECK(l.gx == (a.n + 255) / 256 && l.bx == 256 && l.gy <= 32768 && l.a.row_first == out_at);
            out_at += l.gy;
        }
        CHECK(out_at % a.hop_count == 0 && out_at / a.hop_count >= 1 && out_at / a.hop_count <= a.in_ch_count);
        seen.max_rows = std::max(seen.max_rows, rows);
        ++seen.groups;
    }
    for (size_t have : allocated) CHECK(have <= max_bytes + max_bytes / 4);  // (DevBuf::reserve keeps a quarter of slack)
    if (running_max) *running_max = max_bytes;
    return seen;
}

struct Job {
    rc_config c;
    rc_engine *e = nullptr;
    rc_params P;
    std::vector<std::vector<float>> x, y;
    std::vector<const float *> in;
    std::vector<float *> out;
    size_t L, n_out;
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
    }
    ~Job() { rc_engine_destroy(e); }
    void load(const std::string &code) { CHECK(rc_engine_load_device_kernel(e, code.data(), code.size()) == RC_OK); }
    void host() {
        size_t got = 0;
        CHECK(rc_engine_stretch_host(e, in.data(), L, out.data(), n_out, &got) == RC_OK && got == n_out);
    }
};

// whole jobs, ranges of one channel, a single frame and the seam, for one declaration
static void engine_paths(uint32_t N, float f, int p, uint32_t ch, size_t L, uint32_t S, uint32_t hist, bool cross) {
    const std::string code = kernel_object(hist, cross, S);
    {
        Job j(N, f, p, ch, L);
        (void)rtc_sums_stub_take_lookups();
        j.load(code);
        CHECK((rtc_sums_stub_take_lookups() == std::vector<std::string>{std::string("rc_user_dk"), std::string("rc_user_dk_sums_pass")}));
        (void)rtc_sums_stub_take_launches();
        j.host();
        uint64_t held = 0;
        Seen s = verify(rtc_sums_stub_take_launches(), S, hist, cross, ch, &held);
        CHECK(s.groups >= 1);
        uint32_t launches = 0;
        CHECK(rc_engine_last_kernel_stats(j.e, nullptr, nullptr, &launches) == RC_OK);
        CHECK(launches >= 2 * s.groups);  // the pass is counted
        // one channel at a time, two cuts: with RC_CROSS_CHANNEL the pass still covers every channel's rows
        float *d_in = nullptr, *d_out = nullptr;
        CHECK(hipMalloc((void **)&d_in, (size_t)ch * L * sizeof(float)) == hipSuccess);
        CHECK(hipMalloc((void **)&d_out, (size_t)ch * j.n_out * sizeof(float)) == hipSuccess);
        const uint64_t wins = j.n_out / j.P.window_out_len;
        const uint64_t cut[3] = {0, wins / 3 + 1, wins};
        for (uint32_t i = 0; i < ch; ++i)
            for (int r = 0; r < 2; ++r)
                if (cut[r + 1] > cut[r] && cut[r + 1] <= wins)
                    CHECK(rc_engine_stretch_device_range(j.e, d_in, L, L, i, 1, cut[r], cut[r + 1] - cut[r],
                                                         d_out + (size_t)i * j.n_out + cut[r] * j.P.window_out_len, j.n_out,
                                                         (size_t)((cut[r + 1] - cut[r]) * j.P.window_out_len), nullptr) == RC_OK);
        CHECK(rc_engine_synchronize(j.e) == RC_OK);
        (void)hipFree(d_in);
        (void)hipFree(d_out);
        s = verify(rtc_sums_stub_take_launches(), S, hist, cross, ch, &held);
        CHECK(s.groups >= ch);
    }
    {
        // a single frame: one row, whatever the kernel declares
        Job j(N, f, p, ch, L);
        j.load(code);
        std::vector<float> frame(N, 0.5f), back(N);
        (void)rtc_sums_stub_take_launches();
        CHECK(rc_engine_resynth(j.e, ch - 1, 9, frame.data(), back.data()) == RC_OK);
        const std::vector<RtcSumsLaunch> log = rtc_sums_stub_take_launches();
        CHECK(log.size() == 2 && log[0].pass == 1 && log[0].gy == 1 && log[0].a.row_first == 0 && log[1].pass == 0);
        CHECK(log[0].a.in_ch_count == 1 && log[0].a.in_rows == 1 && log[0].a.halo == 0 && log[0].a.hop_first == 9);
        CHECK(log[0].stream == log[1].stream && log[0].a.sums == log[1].a.sums && log[0].a.sums != nullptr);
        CHECK(log[0].scratch_bytes >= S * sizeof(float));
    }
    {
        // the seam, batches of one window, closed first
        Job j(N, f, p, ch, L, 1);
        j.load(code);
        (void)rtc_sums_stub_take_launches();
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
        const Seen s = verify(rtc_sums_stub_take_launches(), S, hist, cross, ch);
        CHECK(s.groups >= 2);
    }
}

static void multi(const std::vector<int32_t> &devs, uint32_t N, float f, uint32_t ch, size_t L, uint32_t S, uint32_t hist, bool cross) {
    const std::string code = kernel_object(hist, cross, S);
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
    (void)rtc_sums_stub_take_launches();
    CHECK(rc_multi_stretch_host(m, in.data(), L, out.data(), n_out, &got) == RC_OK && got == n_out);
    rc_multi_destroy(m);
    // the shards run on threads of their own: their groups interleave in the log, so sort them out by stream first
    std::vector<RtcSumsLaunch> log = rtc_sums_stub_take_launches();
    std::stable_sort(log.begin(), log.end(), [](const RtcSumsLaunch &a, const RtcSumsLaunch &b) { return a.stream < b.stream; });
    const Seen s = verify(log, S, hist, cross, ch);
    CHECK(s.groups >= devs.size());
}

int main() {
    engine_paths(1024, 4.0f, 1, 2, 40 * 1024 + 77, 1, 0, false);     // sums alone
    engine_paths(1024, 4.0f, 1, 2, 40 * 1024 + 77, 3, 2, false);     // with a halo
    engine_paths(1024, 4.0f, -2, 3, 20 * 1024 + 5, 4, 2, true);      // cross-channel blocks, three channels
    engine_paths(12288, 4.0f, 3, 2, 12 * 12288 + 1, 2, 1, true);     // Gen
    engine_paths(65536, 8.0f, 1, 2, 5 * 65536 + 333, 2, 0, true);    // Big
    engine_paths(131072, 4.0f, 1, 2, 5 * 131072 + 333, 1, 1, false);  // Long
    multi({0, 1, 2, 3}, 1024, 4.0f, 2, 40 * 1024 + 77, 2, 1, true);
    multi({0, 0}, 4096, 4.0f, 4, 30 * 4096, 4, 2, false);
    {
        // more than 32768 rows in one pass: the grid is cut at 32768 rows, the last chunk is short
        Job j(32, 4.0f, 1, 2, 80000);
        j.load(kernel_object(1, false, 2));
        (void)rtc_sums_stub_take_launches();
        j.host();
        const Seen s = verify(rtc_sums_stub_take_launches(), 2, 1, false, 2);
        CHECK(s.max_rows > 32768 && s.pass_launches > s.groups);
    }
    {
        // an undeclared module: one lookup, no pass, no sums
        Job j(1024, 4.0f, 1, 2, 40 * 1024 + 77);
        (void)rtc_sums_stub_take_lookups();
        j.load(kernel_object(2, true, 0));
        CHECK((rtc_sums_stub_take_lookups() == std::vector<std::string>{std::string("rc_user_dk")}));
        (void)rtc_sums_stub_take_launches();
        j.host();
        const std::vector<RtcSumsLaunch> log = rtc_sums_stub_take_launches();
        CHECK(!log.empty());
        for (const RtcSumsLaunch &l : log) CHECK(l.pass == 0 && l.a.sums == nullptr && l.a.n_sums == 0);
    }
    {
        // every rejected code object leaves the loaded kernel (S = 2) in place
        Job j(1024, 4.0f, 1, 2, 40 * 1024 + 77);
        j.load(kernel_object(1, false, 2));
        std::vector<std::string> bad;
        bad.push_back(fake_code_object({{"rc_user_dk", 0}, {"rc_user_dk_sums", 6}, {"rc_user_dk_sums_pass", 0}}));  // S = 5
        bad.push_back(fake_code_object({{"rc_user_dk", 0}, {"rc_user_dk_sums", 0}, {"rc_user_dk_sums_pass", 0}}));  // no byte
        bad.push_back(fake_code_object({{"rc_user_dk", 0}, {"rc_user_dk_sums", 3}}));                                // no pass
        bad.push_back(fake_code_object({{"rc_user_dk_sums", 3}, {"rc_user_dk_sums_pass", 0}}));                      // no kernel
        bad.push_back(fake_code_object({{"rc_user_dk", 0}, {"rc_user_dk_history", 12}, {"rc_user_dk_sums", 2}, {"rc_user_dk_sums_pass", 0}}));
        bad.push_back(std::string(200, '\0'));
        bad.push_back(kernel_object(1, false, 2).substr(0, 100));  // cut short
        (void)rtc_sums_stub_take_lookups();
        uint64_t held = 0;
        for (const std::string &b : bad) {
            CHECK(rc_engine_load_device_kernel(j.e, b.data(), b.size()) == RC_EINVAL);
            CHECK(rtc_sums_stub_take_lookups().empty());  // (never reached the runtime)
            (void)rtc_sums_stub_take_launches();
            j.host();
            const Seen s = verify(rtc_sums_stub_take_launches(), 2, 1, false, 2, &held);
            CHECK(s.groups >= 1);
        }
        // a marker of one byte declares no sums: the object loads and runs as an undeclared one
        const std::string none = fake_code_object({{"rc_user_dk", 0}, {"rc_user_dk_sums", 1}, {"rc_user_dk_sums_pass", 0}});
        j.load(none);
        CHECK((rtc_sums_stub_take_lookups() == std::vector<std::string>{std::string("rc_user_dk")}));
        (void)rtc_sums_stub_take_launches();
        j.host();
        for (const RtcSumsLaunch &l : rtc_sums_stub_take_launches()) CHECK(l.pass == 0 && l.a.sums == nullptr);
    }
    printf("engine_host_driver_dk_sums: ok\n");
    return 0;
}
