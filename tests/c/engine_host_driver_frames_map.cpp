// TEST INFRASTRUCTURE: rc_engine_set_channel_map, rc_engine_frames_channel_peaks and rc_split_mono_map over the HIP stub
// (tests/c/hip_stub.cpp: device memory is host memory; tests/c/hip_stub_frames_map.cpp: the mapped unpack launcher reads
// the table and exactly the bytes of sample (f, map[c]), the channel-peaks launcher reads every byte of its frame range,
// joins the largest byte of each channel, logs the range and counts how often each frame came through) under ASan + UBSan
// (rocoder_amd/csrc/host/sanitize.mk: engine_frames_map_asan). What runs for real is the engine's host code: the table
// written on the stream in front of the first mapped launch, which launcher a job takes, the frames every chunk unpacks, the
// chunk loop of the measuring job, the zeroed words in front of its first launch, the one readback behind the last, and
// the error paths. rc_split_mono_map, which needs no engine, is held to its answers and status codes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/rocoder_hip.h"

struct RcStubChanLaunch {  // tests/c/hip_stub_frames_map.cpp
    uint64_t frame0, n_frames;
    uint32_t channels, phase, format;
};
extern RcStubChanLaunch rc_stub_chan_log[256];
extern uint32_t rc_stub_chan_launches;
extern unsigned char *rc_stub_chan_cover;
extern uint64_t rc_stub_chan_dirty;
extern uint32_t rc_stub_map_launches;
extern unsigned char *rc_stub_map_cover;
extern uint32_t rc_stub_map_seen[8];

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

static int ok_kernel(uint64_t, const float *in, float *out, size_t n, void *) {
    memcpy(out, in, n * 2 * sizeof(float));
    return 0;
}

static uint32_t bytes_of(uint32_t format) { return format == RC_PCM_U8 ? 1 : format == RC_PCM_I16 ? 2 : format == RC_PCM_I24 ? 3 : 4; }

// a block of exactly L frames that starts `misalign` bytes into its allocation
struct Block {
    void *alloc = nullptr;
    unsigned char *p = nullptr;
    bool pinned = false;
    Block(size_t bytes, size_t misalign, bool pin) : pinned(pin) {
        if (pin) CHECK(rc_host_alloc(bytes + misalign + 1, &alloc) == RC_OK);
        else alloc = malloc(bytes + misalign + 1);
        CHECK(alloc != nullptr);
        p = (unsigned char *)alloc + misalign;
    }
    ~Block() {
        if (pinned) (void)rc_host_free(alloc);
        else free(alloc);
    }
};

// ---- the map: which launcher a frames job takes, and that every frame goes through it once ------------------------------
static void stretch_once(rc_engine *e, const rc_config &c, const unsigned char *in, size_t L, uint32_t format, int entry, float *out) {
    const size_t n_out = rc_offline_output_len(&c, L);
    size_t got = 0;
    uint64_t clipped = 0;
    float peak = 0, gain = 0;
    if (entry == 0) CHECK(rc_engine_stretch_frames(e, L ? in : nullptr, L, format, out, n_out, &got) == RC_OK);
    else if (entry == 1) CHECK(rc_engine_stretch_frames_pcm(e, L ? in : nullptr, L, format, out, n_out, RC_PCM_F32, &got, &clipped) == RC_OK);
    else CHECK(rc_engine_stretch_frames_norm(e, L ? in : nullptr, L, format, out, n_out, RC_PCM_F32, 0.5f, &got, &peak, &gain, &clipped) == RC_OK);
    CHECK(got == n_out);
}

static void map_job(uint32_t N, float f, uint32_t ch, uint32_t format, size_t L, size_t misalign, bool pinned, bool host_kernel = false) {
    rc_config c = config(N, f, ch);
    if (host_kernel) {
        c.kernel = ok_kernel;
        c.kernel_time_ms = 1;
    }
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&c, &e) == RC_OK);
    const size_t fb = (size_t)ch * bytes_of(format);
    Block in(L * fb, misalign, pinned);
    memset(in.p, 0x5a, L * fb);
    const size_t n_out = rc_offline_output_len(&c, L);
    std::vector<float> out(n_out * ch + 1);
    std::vector<unsigned char> cover(L + 1, 0);
    std::vector<uint32_t> identity(ch), reverse(ch), from_last(ch, ch - 1);
    for (uint32_t k = 0; k < ch; ++k) identity[k] = k, reverse[k] = ch - 1 - k;
    auto run = [&](int entry, const std::vector<uint32_t> *want) {  // want: the map the launcher must see, or null for none
        std::fill(cover.begin(), cover.end(), (unsigned char)0);
        rc_stub_map_cover = cover.data();
        rc_stub_map_launches = 0;
        memset(rc_stub_map_seen, 0xff, sizeof rc_stub_map_seen);
        stretch_once(e, c, in.p, L, format, entry, out.data());
        rc_stub_map_cover = nullptr;
        if (!want) {  // the unmapped launcher: the launches of an engine that has never seen a map
            CHECK(rc_stub_map_launches == 0);
            return;
        }
        CHECK((rc_stub_map_launches == 0) == (L == 0));
        for (size_t k = 0; k < L; ++k) CHECK(cover[k] == 1);  // every frame exactly once across the chunks
        CHECK(cover[L] == 0);
        if (L)
            for (uint32_t k = 0; k < ch && k < 8; ++k) CHECK(rc_stub_map_seen[k] == (*want)[k]);
    };
    run(0, nullptr);  // after create: no map
    CHECK(rc_engine_set_channel_map(e, identity.data(), ch) == RC_OK);
    run(0, nullptr);  // an identity map: the unmapped launches
    if (ch > 1) {
        CHECK(rc_engine_set_channel_map(e, reverse.data(), ch) == RC_OK);
        for (int entry = 0; entry < 3; ++entry) run(entry, &reverse);
        run(0, &reverse);  // the map persists, the table is on the device already
        // rejected: the previous map stays
        std::vector<uint32_t> bad(reverse);
        bad[ch - 1] = ch;
        CHECK(rc_engine_set_channel_map(e, bad.data(), ch) == RC_EINVAL);
        CHECK(rc_engine_set_channel_map(e, reverse.data(), ch - 1) == RC_EINVAL);
        CHECK(rc_engine_set_channel_map(e, reverse.data(), ch + 1) == RC_EINVAL);
        run(1, &reverse);
        CHECK(rc_engine_set_channel_map(e, from_last.data(), ch) == RC_OK);  // a new table over the old one
        run(2, &from_last);
        // the measuring entries and the host form take no map
        std::vector<float> peaks(ch);
        rc_stub_map_launches = 0;
        CHECK(rc_engine_frames_channel_peaks(e, L ? in.p : nullptr, L, format, peaks.data(), ch) == RC_OK);
        CHECK(rc_stub_map_launches == 0);
        run(0, &from_last);  // ... and leave it as it was
    }
    CHECK(rc_engine_set_channel_map(e, nullptr, ch) == RC_OK);
    run(0, nullptr);
    if (ch > 1) {
        CHECK(rc_engine_set_channel_map(e, reverse.data(), ch) == RC_OK);
        CHECK(rc_engine_set_channel_map(e, reverse.data(), 0) == RC_OK);  // n == 0 clears it
        run(2, nullptr);
    }
    CHECK(rc_engine_set_channel_map(nullptr, identity.data(), ch) == RC_EINVAL);
    rc_engine_destroy(e);
}

// ---- the channel peaks ---------------------------------------------------------------------------------------------------
// the byte the driver puts at byte i of frame f: below 0x80, and the largest of a channel depends on which frames came through
static unsigned char fill(size_t f, size_t i, unsigned div) { return (unsigned char)((((f * 2654435761u) >> 7) % 120u + (i & 7u)) / div); }

static void peaks_job(uint32_t ch, uint32_t format, size_t L, size_t misalign, bool pinned) {
    rc_config c = config(1024, 2.0f, ch);
    rc_engine *e = nullptr;
    CHECK(rc_engine_create(&c, &e) == RC_OK);
    const uint32_t B = bytes_of(format);
    const size_t fb = (size_t)ch * B, bytes = L * fb;
    Block in(bytes, misalign, pinned);
    std::vector<uint32_t> block(ch + 2);  // guard words on both sides
    std::vector<unsigned char> cover(L + 1, 0);
    std::vector<uint32_t> swap(ch);
    for (uint32_t k = 0; k < ch; ++k) swap[k] = (k + 1) % ch;
    CHECK(rc_engine_set_channel_map(e, swap.data(), ch) == RC_OK);  // (a map set: the measurement reads the raw block all the same)
    for (unsigned rep = 0; rep < 2; ++rep) {  // the second call finds the engine's buffers reserved and the first call's words in them
        std::vector<uint32_t> want(ch, 0);
        for (size_t f = 0; f < L; ++f)
            for (size_t i = 0; i < fb; ++i) {
                const unsigned char v = fill(f, i, rep + 1);
                in.p[f * fb + i] = v;
                if (v > want[i / B]) want[i / B] = v;
            }
        std::fill(block.begin(), block.end(), 0xdeadbeefu);
        std::fill(cover.begin(), cover.end(), (unsigned char)0);
        rc_stub_chan_cover = cover.data();
        rc_stub_chan_launches = 0;
        rc_stub_chan_dirty = 0;
        CHECK(rc_engine_frames_channel_peaks(e, L ? in.p : nullptr, L, format, (float *)(block.data() + 1), ch) == RC_OK);
        rc_stub_chan_cover = nullptr;
        // every frame went through the launcher exactly once, in launches that follow each other without a gap
        for (size_t f = 0; f < L; ++f) CHECK(cover[f] == 1);
        CHECK(cover[L] == 0);
        uint64_t at = 0;
        CHECK(rc_stub_chan_launches <= 256);
        for (uint32_t k = 0; k < rc_stub_chan_launches; ++k) {
            const RcStubChanLaunch &q = rc_stub_chan_log[k];
            CHECK(q.frame0 == at && q.n_frames > 0 && q.channels == ch && q.format == format && q.phase == (uint32_t)((uintptr_t)in.p & 3u));
            at += q.n_frames;
        }
        CHECK(at == L && (L == 0) == (rc_stub_chan_launches == 0));
        if (bytes > ((size_t)16 << 20)) CHECK(rc_stub_chan_launches >= 2);  // more than one staging slot: more than one chunk
        // the words were zeroed in front of the first launch, the uploads had brought every byte a launch read, and one
        // readback brought exactly `channels` words
        CHECK(rc_stub_chan_dirty == 0);
        CHECK(block[0] == 0xdeadbeefu && block[ch + 1] == 0xdeadbeefu);
        for (uint32_t k = 0; k < ch; ++k) CHECK(block[1 + k] == want[k]);
    }
    // errors: nothing behind chan_peak is written, nothing is launched
    std::fill(block.begin(), block.end(), 0xdeadbeefu);
    float *peak = (float *)(block.data() + 1);
    rc_stub_chan_launches = 0;
    CHECK(rc_engine_frames_channel_peaks(nullptr, in.p, L, format, peak, ch) == RC_EINVAL);
    CHECK(rc_engine_frames_channel_peaks(e, in.p, L, format, nullptr, ch) == RC_EINVAL);
    CHECK(rc_engine_frames_channel_peaks(e, nullptr, L, format, peak, ch) == (L ? RC_EINVAL : RC_OK));
    if (!L) std::fill(block.begin(), block.end(), 0xdeadbeefu);
    CHECK(rc_engine_frames_channel_peaks(e, in.p, L, 0, peak, ch) == RC_EINVAL);
    CHECK(rc_engine_frames_channel_peaks(e, in.p, L, 6, peak, ch) == RC_EINVAL);
    CHECK(rc_engine_frames_channel_peaks(e, in.p, L, format, peak, ch - 1) == RC_ECAPACITY);
    CHECK(rc_stub_chan_launches == 0);
    for (uint32_t w : block) CHECK(w == 0xdeadbeefu);
    // a capacity beyond the channels: the words behind them stay
    CHECK(rc_engine_frames_channel_peaks(e, in.p, L, format, peak, ch + 1) == RC_OK);
    CHECK(block[0] == 0xdeadbeefu && block[ch + 1] == 0xdeadbeefu);
    // a stretch call behind it finds the engine as it was, the map included
    {
        const size_t Ls = 3000, n_out = rc_offline_output_len(&c, Ls);
        std::vector<int16_t> s(Ls * ch + 1, 0);
        std::vector<float> out(n_out * ch + 1, 0.0f);
        size_t n = 0;
        rc_stub_map_launches = 0;
        CHECK(rc_engine_stretch_frames(e, s.data(), Ls, RC_PCM_I16, out.data(), n_out, &n) == RC_OK && n == n_out);
        CHECK((rc_stub_map_launches > 0) == (ch > 1));
    }
    rc_engine_destroy(e);
}

static void split_mono_codes() {
    uint32_t map[5];
    int found = 13;
    auto is = [&](std::initializer_list<float> peaks, std::initializer_list<uint32_t> want, int want_found) {
        std::vector<float> p(peaks);
        std::vector<uint32_t> w(want);
        for (uint32_t &m : map) m = 99;
        found = 13;
        CHECK(rc_split_mono_map(p.data(), (uint32_t)p.size(), map, &found) == RC_OK && found == want_found);
        for (size_t k = 0; k < w.size(); ++k) CHECK(map[k] == w[k]);
        for (size_t k = w.size(); k < 5; ++k) CHECK(map[k] == 99);
    };
    is({0.0f, 0.5f}, {1, 1}, 1);
    is({0.5f, 0.0f}, {0, 0}, 1);
    is({0.5f, 0.25f}, {0, 1}, 0);
    is({0.0f, 0.0f}, {0, 1}, 0);
    is({-0.0f, 1e-45f, 0.0f}, {1, 1, 1}, 1);
    is({0.0f, (float)NAN}, {1, 1}, 1);
    is({(float)INFINITY, 0.0f, 0.0f, 0.0f}, {0, 0, 0, 0}, 1);
    is({0.0f, 1.0f, 0.0f, 1.0f, 0.0f}, {0, 1, 2, 3, 4}, 0);
    is({1.0f}, {0}, 1);
    is({0.0f}, {0}, 0);
    const float p[2] = {0.0f, 1.0f};
    for (uint32_t &m : map) m = 99;
    found = 13;
    CHECK(rc_split_mono_map(nullptr, 2, map, &found) == RC_EINVAL);
    CHECK(rc_split_mono_map(p, 2, nullptr, &found) == RC_EINVAL);
    CHECK(rc_split_mono_map(p, 2, map, nullptr) == RC_EINVAL);
    CHECK(rc_split_mono_map(p, 0, map, &found) == RC_EINVAL);
    CHECK(found == 13);
    for (uint32_t m : map) CHECK(m == 99);
}

int main() {
    split_mono_codes();
    // the map: several pipeline chunks (4.8 M output samples per channel, 4 M per staging slot), every byte phase
    map_job(1024, 8.0f, 3, RC_PCM_I24, 600001, 1, false);
    map_job(1024, 8.0f, 3, RC_PCM_I24, 600001, 0, true);
    for (size_t mis = 0; mis < 4; ++mis)
        for (bool pinned : {false, true}) map_job(1024, 2.0f, 2, RC_PCM_I16, 30001, mis, pinned);
    map_job(1024, 2.0f, 1, RC_PCM_U8, 30001, 3, false);
    map_job(256, 2.0f, 67, RC_PCM_I24, 3000, 1, false);            // the wide tiles
    map_job(1024, 2.0f, 2, RC_PCM_I16, 30001, 1, false, true);     // a host kernel: whole input up, one unpack launch
    for (size_t L : {(size_t)0, (size_t)1, (size_t)7, (size_t)1024})
        for (bool pinned : {false, true}) map_job(1024, 2.0f, 3, RC_PCM_I24, L, 1, pinned);
    // the peaks: several chunks (9-byte frames: 16 MiB is no whole number of them), every byte phase, pageable and page-locked
    for (size_t mis = 0; mis < 4; ++mis) peaks_job(3, RC_PCM_I24, 4000001, mis, false);
    for (size_t mis : {(size_t)0, (size_t)1}) peaks_job(3, RC_PCM_I24, 4000001, mis, true);
    peaks_job(2, RC_PCM_I16, 5000001, 2, false);
    peaks_job(2, RC_PCM_F32, 30001, 1, false);
    peaks_job(5, RC_PCM_I32, 30001, 3, true);
    peaks_job(67, RC_PCM_I24, 3000, 1, false);
    peaks_job(1, RC_PCM_U8, 30001, 1, true);
    for (size_t L : {(size_t)0, (size_t)1, (size_t)6, (size_t)7})
        for (bool pinned : {false, true}) {
            peaks_job(3, RC_PCM_I24, L, 1, pinned);
            peaks_job(2, RC_PCM_U8, L, 0, pinned);
        }
    printf("engine_host_driver_frames_map: ok\n");
    return 0;
}
