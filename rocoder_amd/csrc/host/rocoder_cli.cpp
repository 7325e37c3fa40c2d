// rocoder CLI twin over the gfx950 engine (the callers and data formats either
// side of the hot path). Same flags, defaults and semantics as the reference's src/main.rs:27-122,
// WAV reading as src/audio_files.rs:86-188 (hound: 8/16/24/32-bit int + 32-bit float; int->f32
// scaling of src/audio.rs:16-29), 32-bit-float WAV writing (src/audio_files.rs:203-226),
// --start/--duration clipping (src/audio.rs:57-63,115-130), --rotate-channels (:73-75), the
// hh:mm:ss.ss duration grammar (src/duration_parser.rs:5-25), the Stretcher / StretcherProcessor /
// AudioBus plumbing (src/stretcher.rs, src/stretcher_processor.rs, src/audio.rs:141-224) and the
// kernel hot-swapper (src/hotswapper.rs) for C-ABI kernels. Playback/recording (cpal) and MP3 are
// out of scope: -o is required and the input must be WAV.
#include "../../../include/rocoder_hip.h"

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cctype>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace {

// ------------------------------------------------------------------ src/duration_parser.rs:5-25
// "hh:mm:ss.ss" -> milliseconds. Seconds parse as f32 (truncated to ms), minutes/hours as u64.
bool parse_u64(const std::string &s, uint64_t *out) {
    if (s.empty()) return false;
    size_t i = 0;
    if (s[0] == '+') i = 1;
    if (i >= s.size()) return false;
    uint64_t v = 0;
    for (; i < s.size(); ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = v * 10 + (uint64_t)(s[i] - '0');
    }
    *out = v;
    return true;
}
bool parse_f32(const std::string &s, float *out) {
    if (s.empty()) return false;
    char *end = nullptr;
    const float v = strtof(s.c_str(), &end);
    if (end != s.c_str() + s.size()) return false;
    *out = v;
    return true;
}
bool parse_duration_ms(const std::string &str, uint64_t *ms) {
    std::vector<std::string> parts;  // duration_str.rsplit(":"): seconds first
    size_t end = str.size();
    for (;;) {
        const size_t pos = end == 0 ? std::string::npos : str.rfind(':', end - 1);
        if (pos == std::string::npos) {
            parts.push_back(str.substr(0, end));
            break;
        }
        parts.push_back(str.substr(pos + 1, end - pos - 1));
        end = pos;
    }
    if (parts.size() > 3 || parts.empty()) return false;
    float secs;
    if (!parse_f32(parts[0], &secs)) return false;
    const float msf = secs * 1000.0f;  // `as u64` saturates: negative / NaN -> 0
    uint64_t total = (msf > 0.0f) ? (msf >= 1.8446744e19f ? UINT64_MAX : (uint64_t)msf) : 0;
    if (parts.size() > 1) {
        uint64_t m;
        if (!parse_u64(parts[1], &m)) return false;
        total += m * 60 * 1000;
    }
    if (parts.size() > 2) {
        uint64_t h;
        if (!parse_u64(parts[2], &h)) return false;
        total += h * 3600 * 1000;
    }
    *ms = total;
    return true;
}

// ------------------------------------------------------------------ src/audio.rs
struct AudioSpec {
    uint16_t channels = 2;
    uint32_t sample_rate = 44100;
};
struct Audio {
    std::vector<std::vector<float>> data;
    AudioSpec spec;
    // src/audio.rs:57-63,115-130
    void clip_in_place(std::optional<uint64_t> start_ms, std::optional<uint64_t> dur_ms) {
        const size_t len = data.empty() ? 0 : data[0].size();
        size_t start = 0;
        if (start_ms) start = (size_t)((double)*start_ms / 1000.0 * (double)spec.sample_rate);
        size_t endp = len;
        if (dur_ms) endp = start + (size_t)((double)*dur_ms / 1000.0 * (double)spec.sample_rate);
        if (start > len || endp > len || start > endp)
            throw std::runtime_error("clip range out of bounds (the reference panics on the slice)");
        for (auto &c : data) c = std::vector<float>(c.begin() + start, c.begin() + endp);
    }
    void rotate_channels() {  // src/audio.rs:73-75: rotate_right(1)
        if (data.size() < 2) return;
        auto last = std::move(data.back());
        data.pop_back();
        data.insert(data.begin(), std::move(last));
    }
};

// ------------------------------------------------------------------ WAV (hound semantics)
struct ByteReader {
    FILE *f;
    bool read(void *dst, size_t n) { return fread(dst, 1, n, f) == n; }
    bool skip(size_t n) {
        std::vector<char> tmp(4096);
        while (n) {
            const size_t k = std::min(n, tmp.size());
            if (fread(tmp.data(), 1, k, f) != k) return false;
            n -= k;
        }
        return true;
    }
};
uint32_t le32(const unsigned char *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
uint16_t le16(const unsigned char *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// the chunks in front of the samples: leaves `f` at the first byte of the data chunk (have_data; data_len as declared)
struct WavHeader {
    uint16_t fmt_tag = 0, channels = 0, bits = 0;
    uint32_t rate = 0, data_len = 0;
    bool have_fmt = false, have_data = false;
};
WavHeader read_wav_header(FILE *f) {
    ByteReader r{f};
    unsigned char hdr[12];
    if (!r.read(hdr, 12) || memcmp(hdr, "RIFF", 4) || memcmp(hdr + 8, "WAVE", 4))
        throw std::runtime_error("not a RIFF/WAVE stream");
    WavHeader h;
    for (;;) {
        unsigned char ch[8];
        if (!r.read(ch, 8)) break;
        const uint32_t len = le32(ch + 4);
        if (!memcmp(ch, "fmt ", 4)) {
            if (len < 16 || len > 65536) throw std::runtime_error("bad fmt chunk");  // (a hostile length is not an allocation)
            std::vector<unsigned char> b(len);
            if (!r.read(b.data(), len)) throw std::runtime_error("bad fmt chunk");
            h.fmt_tag = le16(&b[0]);
            h.channels = le16(&b[2]);
            h.rate = le32(&b[4]);
            h.bits = le16(&b[14]);
            if (h.fmt_tag == 0xFFFE && len >= 26) h.fmt_tag = le16(&b[24]);  // extensible: subformat
            h.have_fmt = true;
            if (len & 1) r.skip(1);
        } else if (!memcmp(ch, "data", 4)) {
            if (!h.have_fmt) throw std::runtime_error("data chunk before fmt chunk");
            h.have_data = true;
            h.data_len = len;
            break;
        } else {
            if (!r.skip(len + (len & 1))) break;
        }
    }
    if (!h.have_fmt || h.channels == 0) throw std::runtime_error("no fmt chunk");
    if (h.bits / 8 == 0) throw std::runtime_error("unsupported bits per sample");
    return h;
}
void check_wav_format(const WavHeader &h) {
    const bool is_float = h.fmt_tag == 3, is_int = h.fmt_tag == 1;
    if (!((is_float && h.bits == 32) || (is_int && (h.bits == 8 || h.bits == 16 || h.bits == 24 || h.bits == 32))))
        throw std::runtime_error("Cannot read unsupported .wav format");  // audio_files.rs:184-186
}

// --frames-on-gpu: page-locked memory from the engine library and rc_engine_stretch_frames, looked up when the flag asks
// for them (as the user-device-kernel entry points below: without the flag the CLI runs over a library that lacks them)
struct FramesApi {
    decltype(&rc_engine_stretch_frames) stretch = nullptr;
    decltype(&rc_engine_stretch_frames_pcm) stretch_pcm = nullptr;  // (--output-format only: may be missing)
    decltype(&rc_engine_stretch_frames_norm) stretch_norm = nullptr;  // (--normalize only: may be missing)
    decltype(&rc_engine_stretch_frames_loud) stretch_loud = nullptr;  // (--loudness / --true-peak only: may be missing)
    decltype(&rc_engine_set_output_fade) set_fade = nullptr;  // (--fade-output only: may be missing)
    decltype(&rc_engine_set_output_dither) set_dither = nullptr;  // (--dither only: may be missing)
    decltype(&rc_engine_frames_power) power = nullptr;        // (--autocrop only: may be missing, both or neither)
    decltype(&rc_autocrop_points) crop_points = nullptr;
    decltype(&rc_engine_set_channel_map) set_map = nullptr;  // (--channel-map / --split-mono only: may be missing)
    decltype(&rc_engine_frames_channel_peaks) channel_peaks = nullptr;  // (--split-mono only: may be missing, both or neither)
    decltype(&rc_split_mono_map) split_map = nullptr;
    // (--pitch-ratio / --pitch-cents / --output-rate only: may be missing, all or none)
    decltype(&rc_engine_set_output_resample) set_resample = nullptr;
    decltype(&rc_resample_ratio) resample_ratio = nullptr;
    decltype(&rc_resample_len) resample_len = nullptr;
    decltype(&rc_resample_table) resample_table = nullptr;
    // (--limit only: may be missing, both or neither)
    decltype(&rc_engine_set_output_limiter) set_limiter = nullptr;
    decltype(&rc_engine_last_limiter_stats) limiter_stats = nullptr;
    // (--factor-curve / --time-map only: may be missing, all or none)
    decltype(&rc_engine_set_time_map) set_time_map = nullptr;
    decltype(&rc_time_map_output_len) time_map_output_len = nullptr;
    decltype(&rc_time_map_curve) time_map_curve = nullptr;
    // (--pitch-curve only: may be missing, both or neither)
    decltype(&rc_engine_set_output_warp) set_warp = nullptr;
    decltype(&rc_warp_curve) warp_curve = nullptr;
    // (--layer only: may be missing, all or none)
    decltype(&rc_bus_create) bus_create = nullptr;
    decltype(&rc_bus_destroy) bus_destroy = nullptr;
    decltype(&rc_engine_mix_frames) mix_frames = nullptr;
    decltype(&rc_engine_bus_frames) bus_frames = nullptr;
    decltype(&rc_engine_set_phase_mode) set_phase = nullptr;  // (--phase only: may be missing)
    decltype(&rc_host_alloc) alloc = nullptr;
    decltype(&rc_host_free) free = nullptr;
};
static const FramesApi &frames_api() {
    static const FramesApi api = [] {
        FramesApi a;
        a.stretch = (decltype(a.stretch))dlsym(RTLD_DEFAULT, "rc_engine_stretch_frames");
        a.stretch_pcm = (decltype(a.stretch_pcm))dlsym(RTLD_DEFAULT, "rc_engine_stretch_frames_pcm");
        a.stretch_norm = (decltype(a.stretch_norm))dlsym(RTLD_DEFAULT, "rc_engine_stretch_frames_norm");
        a.stretch_loud = (decltype(a.stretch_loud))dlsym(RTLD_DEFAULT, "rc_engine_stretch_frames_loud");
        a.set_fade = (decltype(a.set_fade))dlsym(RTLD_DEFAULT, "rc_engine_set_output_fade");
        a.set_dither = (decltype(a.set_dither))dlsym(RTLD_DEFAULT, "rc_engine_set_output_dither");
        a.power = (decltype(a.power))dlsym(RTLD_DEFAULT, "rc_engine_frames_power");
        a.crop_points = (decltype(a.crop_points))dlsym(RTLD_DEFAULT, "rc_autocrop_points");
        a.set_map = (decltype(a.set_map))dlsym(RTLD_DEFAULT, "rc_engine_set_channel_map");
        a.channel_peaks = (decltype(a.channel_peaks))dlsym(RTLD_DEFAULT, "rc_engine_frames_channel_peaks");
        a.split_map = (decltype(a.split_map))dlsym(RTLD_DEFAULT, "rc_split_mono_map");
        a.set_resample = (decltype(a.set_resample))dlsym(RTLD_DEFAULT, "rc_engine_set_output_resample");
        a.resample_ratio = (decltype(a.resample_ratio))dlsym(RTLD_DEFAULT, "rc_resample_ratio");
        a.resample_len = (decltype(a.resample_len))dlsym(RTLD_DEFAULT, "rc_resample_len");
        a.resample_table = (decltype(a.resample_table))dlsym(RTLD_DEFAULT, "rc_resample_table");
        a.set_limiter = (decltype(a.set_limiter))dlsym(RTLD_DEFAULT, "rc_engine_set_output_limiter");
        a.limiter_stats = (decltype(a.limiter_stats))dlsym(RTLD_DEFAULT, "rc_engine_last_limiter_stats");
        a.set_time_map = (decltype(a.set_time_map))dlsym(RTLD_DEFAULT, "rc_engine_set_time_map");
        a.time_map_output_len = (decltype(a.time_map_output_len))dlsym(RTLD_DEFAULT, "rc_time_map_output_len");
        a.time_map_curve = (decltype(a.time_map_curve))dlsym(RTLD_DEFAULT, "rc_time_map_curve");
        a.set_warp = (decltype(a.set_warp))dlsym(RTLD_DEFAULT, "rc_engine_set_output_warp");
        a.warp_curve = (decltype(a.warp_curve))dlsym(RTLD_DEFAULT, "rc_warp_curve");
        a.bus_create = (decltype(a.bus_create))dlsym(RTLD_DEFAULT, "rc_bus_create");
        a.bus_destroy = (decltype(a.bus_destroy))dlsym(RTLD_DEFAULT, "rc_bus_destroy");
        a.mix_frames = (decltype(a.mix_frames))dlsym(RTLD_DEFAULT, "rc_engine_mix_frames");
        a.bus_frames = (decltype(a.bus_frames))dlsym(RTLD_DEFAULT, "rc_engine_bus_frames");
        a.set_phase = (decltype(a.set_phase))dlsym(RTLD_DEFAULT, "rc_engine_set_phase_mode");
        a.alloc = (decltype(a.alloc))dlsym(RTLD_DEFAULT, "rc_host_alloc");
        a.free = (decltype(a.free))dlsym(RTLD_DEFAULT, "rc_host_free");
        if (!a.stretch || !a.alloc || !a.free) throw std::runtime_error("--frames-on-gpu: the engine library has no rc_engine_stretch_frames");
        return a;
    }();
    return api;
}
struct PinnedBytes {
    unsigned char *p = nullptr;
    size_t n = 0;
    PinnedBytes() = default;
    explicit PinnedBytes(size_t bytes) : n(bytes) {
        void *v = nullptr;
        if (frames_api().alloc(std::max<size_t>(bytes, 1), &v) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
        p = (unsigned char *)v;
    }
    PinnedBytes(const PinnedBytes &) = delete;
    PinnedBytes &operator=(const PinnedBytes &) = delete;
    PinnedBytes(PinnedBytes &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    PinnedBytes &operator=(PinnedBytes &&o) noexcept {
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~PinnedBytes() {
        if (p) (void)frames_api().free(p);
    }
};
// The data chunk as it is in the file, in page-locked memory: no sample is looked at on the host. `frames` whole frames
// of `spec.channels` samples in `format` (RC_PCM_*) from data.p on.
struct RawAudio {
    AudioSpec spec;
    uint32_t format = 0, sample_bytes = 0;
    PinnedBytes data;
    size_t frames = 0;
};
// an argument that does not fit the input file: one error line and exit status 2, before any engine work
struct UsageError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
// `on_header`: called with the file's spec once the header is read, in front of the data chunk and its allocation
RawAudio read_wav_raw(FILE *f, const std::function<void(const AudioSpec &)> &on_header = {}) {
    const WavHeader h = read_wav_header(f);
    check_wav_format(h);
    RawAudio a;
    a.spec.channels = h.channels;
    a.spec.sample_rate = h.rate;
    if (on_header) on_header(a.spec);
    a.sample_bytes = h.bits / 8u;
    a.format = h.fmt_tag == 3 ? RC_PCM_F32 : h.bits == 8 ? RC_PCM_U8 : h.bits == 16 ? RC_PCM_I16 : h.bits == 24 ? RC_PCM_I24 : RC_PCM_I32;
    size_t got = 0;
    if (h.have_data) {
        const bool to_eof = h.data_len == 0xFFFFFFFFu || h.data_len == 0;
        struct stat st {};
        const long pos = ftell(f);
        if (pos >= 0 && fstat(fileno(f), &st) == 0 && S_ISREG(st.st_mode)) {
            // a file: the bytes it has, in one read (a declared length beyond the end costs nothing)
            const size_t left = (size_t)st.st_size > (size_t)pos ? (size_t)st.st_size - (size_t)pos : 0;
            a.data = PinnedBytes(to_eof ? left : std::min<size_t>(left, h.data_len));
            got = fread(a.data.p, 1, a.data.n, f);
        } else {  // a pipe: its length is known at its end
            std::vector<unsigned char> raw, buf(1 << 20);
            size_t left = to_eof ? SIZE_MAX : (size_t)h.data_len, k;
            while (left && (k = fread(buf.data(), 1, std::min(left, buf.size()), f)) > 0) {
                raw.insert(raw.end(), buf.begin(), buf.begin() + k);
                left -= k;
            }
            a.data = PinnedBytes(raw.size());
            if (!raw.empty()) memcpy(a.data.p, raw.data(), raw.size());
            got = raw.size();
        }
    } else {
        a.data = PinnedBytes(0);
    }
    a.frames = got / a.sample_bytes / h.channels;  // whole frames only, as read_wav
    return a;
}

Audio read_wav(FILE *f, uint32_t *format = nullptr) {
    ByteReader r{f};
    unsigned char hdr[12];
    if (!r.read(hdr, 12) || memcmp(hdr, "RIFF", 4) || memcmp(hdr + 8, "WAVE", 4))
        throw std::runtime_error("not a RIFF/WAVE stream");
    uint16_t fmt_tag = 0, channels = 0, bits = 0, block_align = 0;
    uint32_t rate = 0;
    bool have_fmt = false;
    std::vector<unsigned char> raw;
    for (;;) {
        unsigned char ch[8];
        if (!r.read(ch, 8)) break;
        const uint32_t len = le32(ch + 4);
        if (!memcmp(ch, "fmt ", 4)) {
            if (len < 16 || len > 65536) throw std::runtime_error("bad fmt chunk");  // (a hostile length is not an allocation)
            std::vector<unsigned char> b(len);
            if (!r.read(b.data(), len)) throw std::runtime_error("bad fmt chunk");
            fmt_tag = le16(&b[0]);
            channels = le16(&b[2]);
            rate = le32(&b[4]);
            block_align = le16(&b[12]);
            bits = le16(&b[14]);
            if (fmt_tag == 0xFFFE && len >= 26) fmt_tag = le16(&b[24]);  // extensible: subformat
            have_fmt = true;
            if (len & 1) r.skip(1);
        } else if (!memcmp(ch, "data", 4)) {
            if (!have_fmt) throw std::runtime_error("data chunk before fmt chunk");
            // streamed (stdin) WAV (length 0 or 0xFFFFFFFF): read to EOF; otherwise at most `len` bytes - in pieces, so
            // that a truncated file with a huge declared length costs the bytes it has, not the bytes it claims
            const bool to_eof = len == 0xFFFFFFFFu || len == 0;
            std::vector<unsigned char> buf(1 << 20);
            size_t left = to_eof ? SIZE_MAX : (size_t)len, k;
            while (left && (k = fread(buf.data(), 1, std::min(left, buf.size()), f)) > 0) {
                raw.insert(raw.end(), buf.begin(), buf.begin() + k);
                left -= k;
            }
            break;
        } else {
            if (!r.skip(len + (len & 1))) break;
        }
    }
    if (!have_fmt || channels == 0) throw std::runtime_error("no fmt chunk");
    (void)block_align;
    const size_t bps = bits / 8;
    if (bps == 0) throw std::runtime_error("unsupported bits per sample");
    // whole frames only: a file cut inside a frame would leave the channels ragged (the reference de-interleaves by
    // i % channels, audio_files.rs:39-43, and then indexes every channel up to the first one's length)
    const size_t n = raw.size() / bps / channels * channels;
    Audio a;
    a.spec.channels = channels;
    a.spec.sample_rate = rate;
    a.data.assign(channels, {});
    for (auto &c : a.data) c.reserve(n / channels + 1);
    const bool is_float = fmt_tag == 3, is_int = fmt_tag == 1;
    if (!((is_float && bits == 32) || (is_int && (bits == 8 || bits == 16 || bits == 24 || bits == 32))))
        throw std::runtime_error("Cannot read unsupported .wav format");  // audio_files.rs:184-186
    if (format) *format = is_float ? RC_PCM_F32 : bits == 8 ? RC_PCM_U8 : bits == 16 ? RC_PCM_I16 : bits == 24 ? RC_PCM_I24 : RC_PCM_I32;
    for (size_t i = 0; i < n; ++i) {
        const unsigned char *p = raw.data() + i * bps;
        float v;
        if (is_float) {
            memcpy(&v, p, 4);
        } else if (bits == 8) {  // hound: u8 -> i8 by subtracting 128; from_i8: n / 127
            v = (float)((int)p[0] - 128) / 127.0f;
        } else if (bits == 16) {  // from_i16: n / 32767
            v = (float)(int16_t)le16(p) / 32767.0f;
        } else if (bits == 24) {  // from_i24: n / 8388608
            int32_t s = p[0] | (p[1] << 8) | (p[2] << 16);
            if (s & 0x800000) s |= ~0xFFFFFF;
            v = (float)s / 8388608.0f;
        } else {  // from_i32: n / 2147483647
            v = (float)(int32_t)le32(p) / 2147483647.0f;
        }
        a.data[i % channels].push_back(v);  // de-interleave, audio_files.rs:39-43
    }
    return a;
}

// --output-format: float -> PCM sample, the definition of include/rocoder_hip.h (rc_engine_stretch_frames_pcm) and, bit
// for bit, what the engine's pack kernel computes: t = x * S is one IEEE multiplication (nothing to fuse it with),
// rint rounds to nearest even (the default rounding mode), NaN gives 0, the result is clamped. With `d` (--dither: u8,
// i16 and i24 only) the dither is added to t in ONE f32 addition in front of rint, the definition of
// rc_engine_set_output_dither.
uint32_t pcm_sample_bytes(uint32_t fmt) { return fmt == RC_PCM_U8 ? 1u : fmt == RC_PCM_I16 ? 2u : fmt == RC_PCM_I24 ? 3u : 4u; }
inline void pcm_encode(float x, uint32_t fmt, unsigned char *dst, const float *d = nullptr) {
    if (fmt == RC_PCM_F32) {
        memcpy(dst, &x, 4);
        return;
    }
    const float S = fmt == RC_PCM_U8 ? 127.0f : fmt == RC_PCM_I16 ? 32767.0f : fmt == RC_PCM_I24 ? 8388608.0f : 2147483648.0f;
    const double lo = fmt == RC_PCM_U8 ? -128.0 : fmt == RC_PCM_I16 ? -32768.0 : fmt == RC_PCM_I24 ? -8388608.0 : -2147483648.0;
    const double hi = fmt == RC_PCM_U8 ? 127.0 : fmt == RC_PCM_I16 ? 32767.0 : fmt == RC_PCM_I24 ? 8388607.0 : 2147483647.0;
    volatile float t = x * S;  // (volatile: rounded to f32 here, whatever the target's evaluation method)
    if (d) t = t + *d;  // (and here: an addition of its own, never an fma with the line above)
    double r = std::rint((double)t);  // (t is an f32: its nearest integer is the same in double)
    if (std::isnan(r)) r = 0.0;
    r = std::min(std::max(r, lo), hi);
    const int32_t n = (int32_t)r;
    const uint32_t u = fmt == RC_PCM_U8 ? (uint32_t)(n + 128) : (uint32_t)n;
    for (uint32_t b = 0; b < pcm_sample_bytes(fmt); ++b) dst[b] = (unsigned char)(u >> (8 * b));
}
inline bool pcm_clipped(float x) { return !(std::fabs(x) <= 1.0f); }  // beyond full scale, or NaN

// --dither on the host path: the definition of include/rocoder_hip.h (rc_engine_set_output_dither) over the library's own
// rc_phase_key and rc_phase_hash, so that the same flags give the same file with and without --frames-on-gpu. The writer
// knows the absolute frame and the channel of every sample it encodes. The two entries are looked up when a dither asks
// for them, as the frames entries above: without the flag the CLI runs over a library that lacks them.
struct HostDither {
    uint32_t mode = RC_DITHER_NONE;
    std::vector<uint64_t> keys;  // K(c), one per channel
    decltype(&rc_phase_hash) hash = nullptr;
    HostDither() = default;
    HostDither(uint32_t mode_, uint64_t seed, uint32_t channels) : mode(mode_) {
        if (mode == RC_DITHER_NONE) return;
        const auto key = (decltype(&rc_phase_key))dlsym(RTLD_DEFAULT, "rc_phase_key");
        hash = (decltype(hash))dlsym(RTLD_DEFAULT, "rc_phase_hash");
        if (!key || !hash) throw std::runtime_error("--dither: the engine library has no rc_phase_key / rc_phase_hash");
        // the hop index 2^40 - 1 is one that no job reaches
        for (uint32_t c = 0; c < channels; ++c) keys.push_back(key(seed, c, 0xFFFFFFFFFFull));
    }
    // on for this format: u8, i16, i24
    bool on(uint32_t fmt) const { return mode != RC_DITHER_NONE && (fmt == RC_PCM_U8 || fmt == RC_PCM_I16 || fmt == RC_PCM_I24); }
    float d(uint32_t c, uint64_t t) const {
        const uint32_t h = hash(keys[c], (uint32_t)t);
        const int i = mode == RC_DITHER_TPDF_HP ? (int)(h >> 16) - (int)(hash(keys[c], (uint32_t)(t - 1)) >> 16) : (int)(h >> 16) - (int)(h & 0xFFFFu);
        return (float)i * (1.0f / 65536.0f);
    }
};

// WAV as hound writes 32-bit float (audio_files.rs:68-81,203-226): WAVE_FORMAT_EXTENSIBLE header + interleaved frames.
// The integer formats of --output-format get the same header with the PCM subformat and their own bits, block_align
// and byte_rate; a data chunk of odd length is followed by a pad byte (write_wav_pad), counted in the RIFF size.
void write_wav_header(FILE *f, const AudioSpec &spec, uint64_t frames, uint32_t fmt = RC_PCM_F32) {
    const uint32_t ch = spec.channels, rate = spec.sample_rate, sb = pcm_sample_bytes(fmt);
    const uint64_t data_bytes = frames * ch * sb;
    auto w32 = [&](uint32_t v) { fwrite(&v, 4, 1, f); };
    auto w16 = [&](uint16_t v) { fwrite(&v, 2, 1, f); };
    fwrite("RIFF", 1, 4, f);
    w32((uint32_t)std::min<uint64_t>(0xFFFFFFFFu, 4 + 8 + 40 + 8 + data_bytes + (data_bytes & 1)));
    fwrite("WAVE", 1, 4, f);
    fwrite("fmt ", 1, 4, f);
    w32(40);  // WAVE_FORMAT_EXTENSIBLE, as hound writes 32-bit float
    w16(0xFFFE);
    w16((uint16_t)ch);
    w32(rate);
    w32(rate * ch * sb);
    w16((uint16_t)(ch * sb));
    w16((uint16_t)(8 * sb));
    w16(22);
    w16((uint16_t)(8 * sb));
    w32(0);  // channel mask
    const unsigned char guid[16] = {(unsigned char)(fmt == RC_PCM_F32 ? 0x03 : 0x01), 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00,
                                    0x80, 0x00, 0x00, 0xaa, 0x00, 0x38, 0x9b, 0x71};  // KSDATAFORMAT_SUBTYPE_IEEE_FLOAT / _PCM
    fwrite(guid, 1, 16, f);
    fwrite("data", 1, 4, f);
    w32((uint32_t)std::min<uint64_t>(0xFFFFFFFFu, data_bytes));
}
bool write_wav_pad(FILE *f, const AudioSpec &spec, uint64_t frames, uint32_t fmt) {
    return !((frames * spec.channels * pcm_sample_bytes(fmt)) & 1) || fputc(0, f) == 0;
}

// interleave and encode k frames from chans[c] + i0 into `row` (k * channels * bytes); returns the clipped samples.
// dith (may be null): the frame at i0 is absolute output frame t0.
uint64_t encode_frames(const float *const *chans, uint32_t ch, size_t i0, size_t k, uint32_t fmt, unsigned char *row,
                       const HostDither *dith = nullptr, uint64_t t0 = 0) {
    const uint32_t sb = pcm_sample_bytes(fmt);
    const bool dithered = dith && dith->on(fmt);
    uint64_t clipped = 0;
    for (size_t i = 0; i < k; ++i)
        for (uint32_t c = 0; c < ch; ++c) {
            const float x = chans[c][i0 + i];
            clipped += pcm_clipped(x);
            if (dithered) {
                const float d = dith->d(c, t0 + i);
                pcm_encode(x, fmt, row + (i * ch + c) * sb, &d);
            } else
                pcm_encode(x, fmt, row + (i * ch + c) * sb);
        }
    return clipped;
}

// (*clipped, where given, receives the count of samples beyond full scale)
void write_wav(const std::string &path, const Audio &a, uint32_t fmt = RC_PCM_F32, uint64_t *clipped = nullptr, const HostDither *dith = nullptr) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot create " + path);
    const uint32_t ch = a.spec.channels;
    const uint64_t frames = a.data.empty() ? 0 : a.data[0].size();
    write_wav_header(f, a.spec, frames, fmt);
    if (fmt == RC_PCM_F32 && !clipped) {
        std::vector<float> row((size_t)ch * 4096);
        for (uint64_t i0 = 0; i0 < frames; i0 += 4096) {
            const uint64_t k = std::min<uint64_t>(4096, frames - i0);
            for (uint64_t i = 0; i < k; ++i)
                for (uint32_t c = 0; c < ch; ++c) row[i * ch + c] = a.data[c][i0 + i];  // interleave
            fwrite(row.data(), 4, (size_t)(k * ch), f);
        }
    } else {
        const uint32_t sb = pcm_sample_bytes(fmt);
        std::vector<unsigned char> row((size_t)ch * 4096 * sb);
        std::vector<const float *> chans;
        for (auto &c : a.data) chans.push_back(c.data());
        uint64_t n = 0;
        for (uint64_t i0 = 0; i0 < frames; i0 += 4096) {
            const uint64_t k = std::min<uint64_t>(4096, frames - i0);
            n += encode_frames(chans.data(), ch, (size_t)i0, (size_t)k, fmt, row.data(), dith, i0);
            fwrite(row.data(), sb, (size_t)(k * ch), f);
        }
        (void)write_wav_pad(f, a.spec, frames, fmt);
        if (clipped) *clipped = n;
    }
    fclose(f);
}

// The same file written as the windows arrive (README.md:74 "stream output to disk instead of RAM", src/main.rs:197-203
// collects the whole AudioBus first): the header goes out with the sizes still zero, every batch of windows that all
// channels have delivered is interleaved and appended, and the two size fields are patched at the end - byte for
// byte the file write_wav writes, with the resident set bounded by the queue depth instead of the output length.
struct WavStreamWriter {
    FILE *f = nullptr;
    AudioSpec spec;
    uint64_t frames = 0;
    std::vector<float> row;
    std::vector<unsigned char> enc;
    std::string path, tmp;
    uint32_t fmt = RC_PCM_F32;
    bool count = false;    // --output-format given: samples are encoded through pcm_encode and the clipped ones counted
    uint64_t clipped = 0;
    HostDither dither;     // --dither: frame `frames` is the absolute output frame of the next sample appended
    // The samples go to "<path>.part" and the file takes its name in finish(): a run that fails half way (a device
    // error, a full disk) leaves no output file with empty size fields behind (the reference writes nothing before the
    // whole output exists, src/main.rs:197-203)
    WavStreamWriter(const std::string &path_, const AudioSpec &sp, uint32_t fmt_ = RC_PCM_F32, bool count_ = false)
        : spec(sp), path(path_), tmp(path_ + ".part"), fmt(fmt_), count(count_) {
        f = fopen(tmp.c_str(), "wb");
        if (!f) throw std::runtime_error("cannot create " + tmp);
        write_wav_header(f, spec, 0, fmt);
    }
    ~WavStreamWriter() {
        if (f) {  // not finished: drop the partial file
            fclose(f);
            (void)std::remove(tmp.c_str());
        }
    }
    // chans[c]: the next samples of channel c (equal lengths)
    void append(const std::vector<const float *> &chans, size_t n) {
        const uint32_t ch = spec.channels;
        if (count) {
            const uint32_t sb = pcm_sample_bytes(fmt);
            enc.resize((size_t)ch * std::min<size_t>(n, 4096) * sb);
            for (size_t i0 = 0; i0 < n; i0 += 4096) {
                const size_t k = std::min<size_t>(4096, n - i0);
                clipped += encode_frames(chans.data(), ch, i0, k, fmt, enc.data(), &dither, frames + i0);
                if (fwrite(enc.data(), sb, k * ch, f) != k * ch) throw std::runtime_error("write failed (disk full?)");
            }
            frames += n;
            return;
        }
        row.resize((size_t)ch * std::min<size_t>(n, 4096));
        for (size_t i0 = 0; i0 < n; i0 += 4096) {
            const size_t k = std::min<size_t>(4096, n - i0);
            for (size_t i = 0; i < k; ++i)
                for (uint32_t c = 0; c < ch; ++c) row[i * ch + c] = chans[c][i0 + i];  // interleave
            if (fwrite(row.data(), 4, k * ch, f) != k * ch) throw std::runtime_error("write failed (disk full?)");
        }
        frames += n;
    }
    void finish() {
        if (!write_wav_pad(f, spec, frames, fmt)) throw std::runtime_error("write failed (disk full?)");
        if (fseek(f, 0, SEEK_SET) != 0) throw std::runtime_error("cannot seek in the output file");
        write_wav_header(f, spec, frames, fmt);
        if (fclose(f) != 0) {
            f = nullptr;
            (void)std::remove(tmp.c_str());
            throw std::runtime_error("closing the output file failed");
        }
        f = nullptr;
        if (std::rename(tmp.c_str(), path.c_str()) != 0) {
            (void)std::remove(tmp.c_str());
            throw std::runtime_error("cannot move " + tmp + " to " + path);
        }
    }
};

// ------------------------------------------------------------------ bounded(cap) channel of windows
struct WindowQueue {
    explicit WindowQueue(size_t cap) : cap(std::max<size_t>(1, cap)) {}
    void send(std::vector<float> v) {
        std::unique_lock<std::mutex> lk(m);
        cv_space.wait(lk, [&] { return q.size() < cap || abandoned; });
        if (abandoned) return;
        q.push_back(std::move(v));
        cv_item.notify_one();
    }
    void close() {
        std::lock_guard<std::mutex> lk(m);
        closed = true;
        cv_item.notify_all();
    }
    void abandon() {  // the Receiver was dropped: pending and later sends are discarded (never block the sender)
        std::lock_guard<std::mutex> lk(m);
        abandoned = true;
        q.clear();
        cv_space.notify_all();
    }
    // 0 = got item, 1 = timeout, 2 = disconnected
    int recv_timeout(std::vector<float> *out, std::chrono::milliseconds to) {
        std::unique_lock<std::mutex> lk(m);
#ifdef __SANITIZE_THREAD__
        // gcc 11's libtsan does not intercept pthread_cond_clockwait (what wait_for on the steady clock calls): it then
        // believes the mutex stays locked across the wait and reports every access behind it. The system-clock form
        // goes through pthread_cond_timedwait, which it knows (sanitizer builds only: host/sanitize.mk).
        if (!cv_item.wait_until(lk, std::chrono::system_clock::now() + to, [&] { return !q.empty() || closed; })) return 1;
#else
        if (!cv_item.wait_for(lk, to, [&] { return !q.empty() || closed; })) return 1;
#endif
        if (q.empty()) return 2;
        *out = std::move(q.front());
        q.pop_front();
        cv_space.notify_one();
        return 0;
    }
    size_t cap;
    std::mutex m;
    std::condition_variable cv_item, cv_space;
    std::deque<std::vector<float>> q;
    bool closed = false, abandoned = false;
};

// ------------------------------------------------------------------ src/hotswapper.rs + fft.rs:76-108
// A stack of loaded kernel libraries; the newest is called, a failing one is popped and the call
// retried with the previous one (or no-op). C-ABI kernels: `int apply(uint64_t, const float*,
// float*, size_t, void*)`. A source file (.c/.cc/.cpp) is compiled with the system compiler and
// watched every 100 ms; a prebuilt .so is loaded as is.
struct KernelStack {
    std::mutex m;
    std::vector<std::pair<void *, rc_freq_kernel>> libs;  // kept loaded for fallback (fft.rs:21)
    std::string src;
    std::thread watcher;
    std::atomic<bool> stop{false};
    struct timespec last_mtime {};  // nanosecond mtime: an edit in the same second as the last build counts

    static bool is_source(const std::string &p) {
        auto ends = [&](const char *s) { const size_t n = strlen(s); return p.size() >= n && p.compare(p.size() - n, n, s) == 0; };
        return ends(".c") || ends(".cc") || ends(".cpp") || ends(".cxx");
    }
    bool load_so(const std::string &so) {
        void *h = dlopen(so.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) {
            fprintf(stderr, "WARN failed to load kernel library %s: %s\n", so.c_str(), dlerror());
            return false;
        }
        auto fn = (rc_freq_kernel)dlsym(h, "apply");
        if (!fn) {
            fprintf(stderr, "WARN kernel library %s has no `apply` symbol\n", so.c_str());
            dlclose(h);
            return false;
        }
        std::lock_guard<std::mutex> lk(m);
        libs.emplace_back(h, fn);
        fprintf(stderr, "INFO Got new kernel\n");  // fft.rs:79
        return true;
    }
    bool compile_and_load() {  // hotswapper.rs:52-86 with cc instead of rustc
        char tmpl[] = "/tmp/rocoder_kernel_XXXXXX.so";
        const int fd = mkstemps(tmpl, 3);
        if (fd >= 0) close(fd);
        const bool cxx = src.size() > 2 && src.substr(src.size() - 2) != ".c";
        const std::string cmd = std::string(cxx ? "c++" : "cc") + " -O3 -shared -fPIC -w -o " + tmpl + " '" + src + "' -lm 2>&1";
        FILE *p = popen(cmd.c_str(), "r");
        std::string outp;
        char buf[512];
        while (p && fgets(buf, sizeof buf, p)) outp += buf;
        const int rc = p ? pclose(p) : -1;
        if (rc != 0) {
            fprintf(stderr, "================ kernel compilation failed ================\n%s", outp.c_str());
            fprintf(stderr, "WARN Failed to compile library for file %s\n", src.c_str());  // hotswapper.rs:39
            return false;
        }
        const bool ok = load_so(tmpl);
        unlink(tmpl);
        return ok;
    }
    void start(const std::string &path) {
        src = path;
        if (!is_source(path)) {
            load_so(path);
            return;
        }
        struct stat st;
        if (stat(path.c_str(), &st) == 0) last_mtime = st.st_mtim;
        compile_and_load();  // hotswapper.rs:17 (synchronous first attempt)
        watcher = std::thread([this] {
            while (!stop.load()) {
                std::this_thread::sleep_for(std::chrono::milliseconds(100));  // hotswapper.rs:12,29
                struct stat st2;
                if (stat(src.c_str(), &st2) == 0 && (st2.st_mtim.tv_sec != last_mtime.tv_sec ||
                                                     st2.st_mtim.tv_nsec != last_mtime.tv_nsec)) {
                    last_mtime = st2.st_mtim;
                    compile_and_load();
                }
            }
        });
    }
    ~KernelStack() {
        stop.store(true);
        if (watcher.joinable()) watcher.join();
    }
    static int trampoline(uint64_t t, const float *in, float *out, size_t n, void *user) {
        auto *self = (KernelStack *)user;
        for (;;) {
            rc_freq_kernel fn = nullptr;
            void *handle = nullptr;
            {
                std::lock_guard<std::mutex> lk(self->m);
                if (self->libs.empty()) return 1;  // no-op
                handle = self->libs.back().first;
                fn = self->libs.back().second;
            }
            if (fn(t, in, out, n, nullptr) == 0) return 0;
            fprintf(stderr, "WARN kernel panicked, retrying with last or noop.\n");  // fft.rs:101
            // pop the library that FAILED, not whatever is on top now: the watcher thread may have pushed a newer one
            // between the call and this line (the reference cannot race here: same thread, fft.rs:78-106)
            std::lock_guard<std::mutex> lk(self->m);
            for (size_t i = self->libs.size(); i-- > 0;)
                if (self->libs[i].first == handle) {
                    self->libs.erase(self->libs.begin() + (long)i);
                    break;
                }
        }
    }
};

// --device-kernel-src: the same hot swap for a user DEVICE kernel (include/rocoder_hip.h, rc_dk_compile). The watcher
// thread polls the file every 100 ms and compiles it with hiprtc (hotswapper.rs:19-30); a code object that compiled
// waits in `pending` until the thread that drives the engine loads it between two windows (fft.rs:78: engine handles
// are single-threaded). A failed compile prints the log and keeps the previous kernel (none on the first attempt).
// The user-device-kernel entry points are looked up when --device-kernel-src asks for them, not linked: without the flag
// the CLI runs over any engine library of ABI 5, also one built before they existed.
struct DkApi {
    decltype(&rc_dk_compile) compile = nullptr;
    decltype(&rc_engine_load_device_kernel) load = nullptr;
    decltype(&rc_engine_set_device_kernel_params) set_params = nullptr;
    decltype(&rc_multi_load_device_kernel) multi_load = nullptr;
    decltype(&rc_multi_set_device_kernel_params) multi_set_params = nullptr;
};
static const DkApi &dk_api() {
    static const DkApi api = [] {
        DkApi a;
        a.compile = (decltype(a.compile))dlsym(RTLD_DEFAULT, "rc_dk_compile");
        a.load = (decltype(a.load))dlsym(RTLD_DEFAULT, "rc_engine_load_device_kernel");
        a.set_params = (decltype(a.set_params))dlsym(RTLD_DEFAULT, "rc_engine_set_device_kernel_params");
        a.multi_load = (decltype(a.multi_load))dlsym(RTLD_DEFAULT, "rc_multi_load_device_kernel");
        a.multi_set_params = (decltype(a.multi_set_params))dlsym(RTLD_DEFAULT, "rc_multi_set_device_kernel_params");
        if (!a.compile || !a.load || !a.set_params || !a.multi_load || !a.multi_set_params)
            throw std::runtime_error("--device-kernel-src: the engine library has no user device kernels");
        return a;
    }();
    return api;
}

// The history depth a code object declares (RC_HISTORY in its source): the size of its ELF symbol rc_user_dk_history
// less one, 0 without the symbol. The watcher hands over bytes only, so the log line reads it from them. With `cross`:
// whether the object declares RC_CROSS_CHANNEL (defines the symbol rc_user_dk_channels) instead. With `sums`: the RC_SUMS
// it declares, the size of the symbol rc_user_dk_sums less one, instead. With `feedback`: the RC_FEEDBACK it declares, the
// size of the symbol rc_user_dk_feedback less one, instead.
static unsigned dk_history_of(const std::string &code, bool cross = false, bool sums = false, bool feedback = false) {
    const unsigned char *p = (const unsigned char *)code.data();
    const size_t len = code.size();
    auto rd = [&](uint64_t off, size_t n) -> uint64_t {
        uint64_t x = 0;
        if (off > len || n > len - off) return 0;
        for (size_t i = 0; i < n; ++i) x |= (uint64_t)p[off + i] << (8 * i);
        return x;
    };
    static const char kHistory[] = "rc_user_dk_history", kChan[] = "rc_user_dk_channels", kSums[] = "rc_user_dk_sums";
    static const char kFeedback[] = "rc_user_dk_feedback";
    const char *const kHist = feedback ? kFeedback : sums ? kSums : kHistory;
    const size_t kHistLen = feedback ? sizeof kFeedback : sums ? sizeof kSums : sizeof kHistory;
    if (len < 64 || memcmp(p, "\x7f" "ELF", 4) != 0 || p[4] != 2 || p[5] != 1) return 0;
    const uint64_t shoff = rd(40, 8), shnum = rd(60, 2);
    if (rd(58, 2) != 64 || shoff > len || shnum > (len - shoff) / 64) return 0;
    for (uint64_t i = 0; i < shnum; ++i) {
        const uint64_t sh = shoff + i * 64, type = rd(sh + 4, 4), link = rd(sh + 40, 4);
        if ((type != 2 && type != 11) || rd(sh + 56, 8) != 24 || link >= shnum) continue;
        const uint64_t off = rd(sh + 24, 8), size = rd(sh + 32, 8);
        const uint64_t str_off = rd(shoff + link * 64 + 24, 8), str_size = rd(shoff + link * 64 + 32, 8);
        if (off > len || size > len - off || str_off > len || str_size > len - str_off) continue;
        for (uint64_t sym = off; sym + 24 <= off + size; sym += 24) {
            const uint64_t name = rd(sym, 4);
            if (cross) {
                if (name < str_size && str_size - name >= sizeof kChan && memcmp(p + str_off + name, kChan, sizeof kChan) == 0)
                    return 1;
                continue;
            }
            if (name < str_size && str_size - name >= kHistLen && memcmp(p + str_off + name, kHist, kHistLen) == 0) {
                const uint64_t sz = rd(sym + 16, 8);
                return sz >= 1 ? (unsigned)(sz - 1) : 0;
            }
        }
    }
    return 0;
}

struct DeviceKernelWatcher {
    std::mutex m;
    std::optional<std::string> pending;
    std::string src;
    std::thread watcher;
    std::atomic<bool> stop{false};
    struct timespec last_mtime {};

    void compile() {
        std::string text;
        if (FILE *f = fopen(src.c_str(), "rb")) {
            char buf[4096];
            size_t n;
            while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
            fclose(f);
        } else {
            fprintf(stderr, "WARN cannot read device kernel %s\n", src.c_str());
            return;
        }
        std::string esc;
        for (char c : src) {
            if (c == '"' || c == '\\') esc += '\\';
            esc += c;
        }
        text = "#line 1 \"" + esc + "\"\n" + text;  // diagnostics name the user's file and lines
        std::vector<char> log(1 << 16);
        size_t n = 0;
        int rc = dk_api().compile(text.data(), text.size(), nullptr, 0, &n, log.data(), log.size());
        std::string code;
        if (rc == RC_ECAPACITY) {
            code.resize(n);
            rc = dk_api().compile(text.data(), text.size(), &code[0], code.size(), &n, log.data(), log.size());
        }
        if (rc != RC_OK) {
            fprintf(stderr, "================ device kernel compilation failed ================\n%s\n%s\n", log.data(),
                    rc_last_error());
            fprintf(stderr, "WARN Failed to compile device kernel %s\n", src.c_str());
            return;
        }
        std::lock_guard<std::mutex> lk(m);
        pending = std::move(code);
    }
    void start(const std::string &path) {
        src = path;
        struct stat st;
        if (stat(path.c_str(), &st) == 0) last_mtime = st.st_mtim;
        compile();  // synchronous first attempt
        watcher = std::thread([this] {
            while (!stop.load()) {
                std::this_thread::sleep_for(std::chrono::milliseconds(100));
                struct stat st2;
                if (stat(src.c_str(), &st2) == 0 && (st2.st_mtim.tv_sec != last_mtime.tv_sec ||
                                                     st2.st_mtim.tv_nsec != last_mtime.tv_nsec)) {
                    last_mtime = st2.st_mtim;
                    compile();
                }
            }
        });
    }
    // the code object compiled since the last call, if any
    std::optional<std::string> take() {
        std::lock_guard<std::mutex> lk(m);
        std::optional<std::string> c = std::move(pending);
        pending.reset();
        return c;
    }
    ~DeviceKernelWatcher() {
        stop.store(true);
        if (watcher.joinable()) watcher.join();
    }
};

static bool g_timing = false;  // ROCODER_CLI_TIMING

// ------------------------------------------------------------------ src/stretcher.rs over the engine
struct Engine {
    rc_engine *h = nullptr;
    std::mutex m;  // one thread at a time per handle
    DeviceKernelWatcher *dk = nullptr;  // --device-kernel-src
    std::optional<std::string> dk_held;  // a kernel that reads the other channels, waiting for the top of a round
    // between two windows, with m held: a device kernel the watcher compiled since the last window. One that declares
    // RC_CROSS_CHANNEL loads only while all channels stand at the same window: it is kept until the round is over.
    void poll_device_kernel() {
        if (!dk) return;
        auto code = dk->take();
        if (code) dk_held.reset();  // (a newer source replaces one still waiting)
        else if (dk_held) code = std::move(dk_held), dk_held.reset();
        if (!code) return;
        const bool cross = dk_history_of(*code, true) != 0;
        const int rc = dk_api().load(h, code->data(), code->size());
        if (rc == RC_OK) {
            const unsigned n_sums = dk_history_of(*code, false, true);
            std::string sums = n_sums ? ", " + std::to_string(n_sums) + " whole-hop sums" : std::string();
            if (const unsigned n_fb = dk_history_of(*code, false, false, true)) sums += ", " + std::to_string(n_fb) + " earlier outputs";
            fprintf(stderr, "INFO Got new device kernel (history: %u earlier hops%s%s)\n", dk_history_of(*code),
                    cross ? ", reads the other channels" : "", sums.c_str());
        }
        else if (rc == RC_EINVAL && cross)
            dk_held = std::move(code);
        else
            fprintf(stderr, "WARN loading the device kernel failed: %s\n", rc_last_error());
    }
    // What main queued for each channel and has not reached the engine yet (the Sender side of stretcher.rs:125). It
    // lives here, not in the channel's Stretcher, because a device kernel that reads the other channels makes a
    // window of one channel wait for the input of all of them, and one thread walks the Stretchers in turn.
    struct Feed {
        std::deque<std::vector<float>> input;
        bool input_closed = false;
    };
    std::vector<Feed> feed;
    // with m held: the next queued block of the channel goes to the engine; false when nothing is queued
    bool feed_channel(uint32_t c) {
        Feed &f = feed[c];
        if (f.input.empty()) return false;
        rc_engine_push_input(h, c, f.input.front().data(), f.input.front().size());
        f.input.pop_front();
        // file input: main queued the whole channel and dropped its sender before the processor started
        // (main.rs:148-150), so an empty queue IS the disconnect. Telling the engine now instead of at the
        // next shortfall lets it batch ahead (an open channel is computed one queue-bound at a time);
        // the windows are the same either way
        if (f.input.empty() && f.input_closed) rc_engine_close_input(h, c);
        return true;
    }
    ~Engine() { rc_engine_destroy(h); }
};
struct Stretcher {
    AudioSpec spec;
    std::shared_ptr<Engine> eng;
    uint32_t channel;
    rc_params par;
    // the Receiver<Vec<f32>> side: main sends the whole channel as one chunk (main.rs:148)

    bool is_done() {  // stretcher.rs:78-80
        std::lock_guard<std::mutex> lk(eng->m);
        return rc_engine_is_done(eng->h, channel) == 1;
    }
    size_t channel_bound() { return rc_engine_channel_bound(eng->h); }  // stretcher.rs:82-85
    std::vector<float> next_window() {                                    // stretcher.rs:87-121
        std::vector<float> out(par.window_out_len);
        for (;;) {
            size_t n = 0;
            int rc;
            {
                std::lock_guard<std::mutex> lk(eng->m);
                eng->poll_device_kernel();
                rc = rc_engine_next_window(eng->h, channel, out.data(), out.size(), &n);
            }
            if (rc == RC_OK) {
                out.resize(n);
                return out;
            }
            if (rc != RC_WOULD_BLOCK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            std::lock_guard<std::mutex> lk(eng->m);  // self.input.recv(), stretcher.rs:125
            if (eng->feed_channel(channel)) continue;
            // nothing of its own is left: a kernel that reads the other channels waits for THEIR input, which their
            // own next_window would bring only after this one returns
            bool fed = false;
            for (uint32_t c = 0; c < eng->feed.size(); ++c) fed = (c != channel && eng->feed_channel(c)) || fed;
            if (!fed) rc_engine_close_input(eng->h, channel);  // Err(_): Sender dropped, stretcher.rs:129-132
        }
    }
};

// src/stretcher_processor.rs:26-89
struct StretcherProcessor {
    std::vector<std::pair<std::shared_ptr<WindowQueue>, Stretcher>> channels;
    std::atomic<bool> shutdown{false}, finished{false};
    std::thread th;
    std::string error;
    double t_next = 0, t_send = 0;
    // min_depth: file-to-file runs deepen the queues (the results do not depend on the depth). The reference's
    // bound is ceil(window seconds / buffer seconds) = 1 at the defaults: two thread hand-offs per window, which
    // its ~1 ms of CPU work per window hides and the engine's ~1 us per window does not (2.0 of 2.3 s on a
    // 600 s stereo file)
    std::vector<std::shared_ptr<WindowQueue>> make(std::vector<Stretcher> st, size_t min_depth = 1) {
        std::vector<std::shared_ptr<WindowQueue>> rx;
        for (auto &s : st) {
            auto q = std::make_shared<WindowQueue>(std::max(s.channel_bound(), min_depth));  // bounded(channel_bound())
            rx.push_back(q);
            channels.emplace_back(q, std::move(s));
        }
        return rx;
    }
    void start() {
        th = std::thread([this] {
            try {
                bool running = true;
                while (running) {
                    if (shutdown.load()) break;  // handle_control_messages (:57-62)
                    for (auto &c : channels) {
                        if (c.second.is_done()) {  // :64-68
                            fprintf(stderr, "INFO stretch process completed\n");
                            running = false;
                            break;
                        }
                        if (!g_timing) {
                            c.first->send(c.second.next_window());  // :69
                        } else {  // ROCODER_CLI_TIMING: where the processor thread's time goes
                            const auto t0 = std::chrono::steady_clock::now();
                            auto w = c.second.next_window();
                            const auto t1 = std::chrono::steady_clock::now();
                            c.first->send(std::move(w));
                            const auto t2 = std::chrono::steady_clock::now();
                            t_next += std::chrono::duration<double, std::milli>(t1 - t0).count();
                            t_send += std::chrono::duration<double, std::milli>(t2 - t1).count();
                        }
                    }
                }
            } catch (const std::exception &ex) {
                error = ex.what();
            }
            if (g_timing) fprintf(stderr, "[timing] processor: next_window %.1f ms, send %.1f ms\n", t_next, t_send);
            for (auto &c : channels) c.first->close();
            finished.store(true);  // :72
        });
    }
    void join() {
        if (th.joinable()) th.join();
    }
};

// AudioBus::into_audio (src/audio.rs:152-172): 5 ms recv_timeout polling drain
Audio into_audio(const AudioSpec &spec, std::vector<std::shared_ptr<WindowQueue>> &chs, size_t expected = 0) {
    Audio a;
    a.spec = spec;
    a.data.assign(chs.size(), {});
    for (auto &c : a.data) c.reserve(expected);
    std::vector<bool> closed(chs.size(), false);
    for (;;) {
        size_t disconnected = 0;
        for (size_t i = 0; i < chs.size(); ++i) {
            if (closed[i]) {
                disconnected++;
                continue;
            }
            std::vector<float> chunk;
            const int rc = chs[i]->recv_timeout(&chunk, std::chrono::milliseconds(5));
            if (rc == 0) a.data[i].insert(a.data[i].end(), chunk.begin(), chunk.end());
            else if (rc == 2) {
                closed[i] = true;
                disconnected++;
            }
        }
        if (disconnected == chs.size()) break;
    }
    return a;
}

// The same drain, written out as it arrives: a window goes to the file as soon as every channel has delivered its
// next one (the processor sends them round robin, src/stretcher_processor.rs:63-70). Returns the frames written.
uint64_t drain_to_wav(WavStreamWriter &w, std::vector<std::shared_ptr<WindowQueue>> &chs) {
    const size_t C = chs.size();
    std::vector<std::deque<std::vector<float>>> pend(C);
    std::vector<size_t> used(C, 0);  // samples of pend[c].front() already written
    std::vector<bool> closed(C, false);
    auto flush = [&] {
        for (;;) {
            size_t n = SIZE_MAX;
            for (size_t c = 0; c < C; ++c) n = std::min(n, pend[c].empty() ? 0 : pend[c].front().size() - used[c]);
            if (n == 0 || n == SIZE_MAX) return;
            std::vector<const float *> rows(C);
            for (size_t c = 0; c < C; ++c) rows[c] = pend[c].front().data() + used[c];
            w.append(rows, n);
            for (size_t c = 0; c < C; ++c) {
                used[c] += n;
                if (used[c] == pend[c].front().size()) {
                    pend[c].pop_front();
                    used[c] = 0;
                }
            }
        }
    };
    for (;;) {
        size_t disconnected = 0;
        for (size_t i = 0; i < C; ++i) {
            if (closed[i]) {
                disconnected++;
                continue;
            }
            if (pend[i].size() >= 4) continue;  // this channel is ahead: let the others catch up first
            std::vector<float> chunk;
            const int rc = chs[i]->recv_timeout(&chunk, std::chrono::milliseconds(5));
            if (rc == 0) pend[i].push_back(std::move(chunk));
            else if (rc == 2) {
                closed[i] = true;
                disconnected++;
            }
        }
        flush();
        if (disconnected == C) break;
        bool stuck = true;  // every open channel is waiting on a closed, empty one: nothing more can pair up
        for (size_t i = 0; i < C; ++i)
            if (!closed[i] && pend[i].size() < 4) stuck = false;
        if (stuck) break;
    }
    return w.frames;
}

uint32_t pcm_format_by_name(const std::string &s) {
    return s == "u8" ? RC_PCM_U8 : s == "i16" ? RC_PCM_I16 : s == "i24" ? RC_PCM_I24 : s == "i32" ? RC_PCM_I32 : s == "f32" ? RC_PCM_F32 : 0u;
}

struct Opt {  // src/main.rs:27-122
    size_t window_len = 16384;
    uint64_t buffer_ms = 1000;
    float factor = 1.0f;
    int pitch_multiple = 1;
    float amplitude = 1.0f;
    std::optional<std::string> input;
    bool rotate_channels = false;
    std::optional<std::string> freq_kernel;
    std::optional<std::string> device_kernel;  // not in the reference: curated on-GPU kernels
    std::optional<std::string> device_kernel_src;  // not in the reference: a user kernel in HIP, hot-swapped
    std::vector<float> dk_params;
    int kernel_threads = 0;
    uint64_t fade_ms = 1000;
    std::optional<uint64_t> start_ms, duration_ms;
    std::optional<std::string> output;
    uint64_t seed = 0;  // not in the reference: thread_rng there
    int device = 0;
    std::vector<int32_t> devices;  // not in the reference: --devices a,b,... shards one job over several GPUs (rc_multi_*)
    std::optional<std::string> output_format;  // not in the reference (it writes f32): f32 | u8 | i16 | i24 | i32 | input
    bool frames_on_gpu = false;    // not in the reference: the file's frames are unpacked and the output interleaved on the GPU
    bool fade_output = false;      // not in the reference (it fades playback only): -x is applied to the output file, on the GPU (--frames-on-gpu)
    // the reference crops what it records (recorder::autocrop_audio, src/recorder.rs:146-163, in front of -s/-d,
    // src/main.rs:173-181); here it crops the file, measured on the GPU (--frames-on-gpu)
    bool autocrop = false;
    uint64_t autocrop_window_ms = 100;  // src/recorder.rs:15
    uint32_t autocrop_percentile = 30;  // src/recorder.rs:16
    // Audio::rotate_channels (src/audio.rs:73-75) and any other permutation or copy of channels under --frames-on-gpu: row c
    // of the job reads channel channel_map[c] of the file, in the GPU's unpack kernel
    std::optional<std::vector<uint32_t>> channel_map;
    // recorder::auto_split_mono (src/recorder.rs:118-144, in front of the autocrop, :64-70): measured on the GPU (--frames-on-gpu)
    bool split_mono = false;
    // not in the reference: per-hop input positions (--frames-on-gpu; rc_engine_set_time_map). --factor-curve "t:f,t:f,...": the
    // factor is f at input time t (the duration grammar, behind -s / --autocrop), linear in between; --time-map: a file of
    // positions in input frames, one per line
    std::optional<std::string> factor_curve, time_map_file;
    // not in the reference: a pitch that varies along the input (--frames-on-gpu; rc_engine_set_output_warp). --pitch-curve
    // "t:c,t:c,...": the pitch is c cents at input time t, linear in cents in between
    std::optional<std::string> pitch_curve;
    bool factor_given = false;
    std::optional<float> normalize;  // not in the reference: the output's peak is brought to this level on the GPU (--frames-on-gpu)
    // not in the reference (-p moves octaves, and decimates with no filter): pitch by any ratio and another output rate, by
    // band-limited resampling of the result on the GPU (--frames-on-gpu; rc_engine_set_output_resample)
    std::optional<double> pitch_ratio;  // --pitch-ratio, or 2^(c / 1200) of --pitch-cents
    std::optional<uint32_t> output_rate;
    // not in the reference: the output is brought to this integrated loudness (BS.1770 / EBU R 128) on the GPU, its true
    // peak kept at true_peak (linear; --frames-on-gpu)
    std::optional<float> loudness, true_peak;
    // not in the reference (an over is clipped by its writer): a look-ahead peak limiter on the result, on the GPU
    // (--frames-on-gpu; rc_engine_set_output_limiter)
    std::optional<float> limit;       // --limit: the ceiling, linear
    float limit_drive = 1.0f;         // --limit-drive
    bool limit_drive_given = false;
    uint64_t limit_lookahead_ms = 5;  // --limit-lookahead
    bool limit_lookahead_given = false;
    // not in the reference (it writes f32): dither in front of the u8 / i16 / i24 quantiser, on the GPU under --frames-on-gpu
    // and in the writer otherwise - the same bytes
    uint32_t dither = RC_DITHER_NONE;
    bool dither_given = false;
    std::optional<uint64_t> dither_seed;  // [default: --seed]
    // not in the reference (it resynthesises random phases): phase-coherent resynthesis (--frames-on-gpu; rc_engine_set_phase_mode)
    uint32_t phase = RC_PHASE_RANDOM;
    // not in the reference's CLI (its mixer, src/mixer.rs, serves playback): --layer SPEC, repeatable. With one or more the run
    // is a mix on the GPU (--frames-on-gpu, -o): every SPEC is one layer over the same input file, the main flags are the
    // defaults of every layer and the output chain of the sum (rc_engine_mix_frames / rc_engine_bus_frames)
    std::vector<std::string> layers;
};

// one --layer SPEC: key=value,... over the defaults the main flags give
struct LayerSpec {
    float factor = 1.0f, amplitude = 1.0f, gain = 1.0f;
    int pitch_multiple = 1;
    std::optional<double> ratio;  // cents, as --pitch-cents
    uint64_t seed = 0, at_ms = 0;
    std::optional<uint64_t> fade_ms;
};

LayerSpec parse_layer(const std::string &spec, const LayerSpec &defaults) {
    LayerSpec l = defaults;
    size_t b = 0;
    while (b <= spec.size()) {
        const size_t c = spec.find(',', b);
        const std::string kv = spec.substr(b, c == std::string::npos ? c : c - b);
        b = c == std::string::npos ? spec.size() + 1 : c + 1;
        if (kv.empty() && spec.empty()) break;  // (an empty SPEC: the defaults)
        const size_t eq = kv.find('=');
        const std::string k = kv.substr(0, eq), v = eq == std::string::npos ? "" : kv.substr(eq + 1);
        char *end = nullptr;
        auto bad = [&]() { return std::runtime_error("--layer: bad " + kv + " in " + spec + " (keys: f, p, cents, a, seed, gain, at, fade)"); };
        if (eq == std::string::npos || v.empty()) throw bad();
        if (k == "f") {
            l.factor = strtof(v.c_str(), &end);
            if (*end) throw bad();
        } else if (k == "p") {
            l.pitch_multiple = (int)strtol(v.c_str(), &end, 10);
            if (*end) throw bad();
        } else if (k == "a") {
            l.amplitude = strtof(v.c_str(), &end);
            if (*end) throw bad();
        } else if (k == "cents") {
            const double r = std::exp2(strtod(v.c_str(), &end) / 1200.0);
            if (*end || !(r >= 0.125 && r <= 8.0)) throw bad();
            l.ratio = r;
        } else if (k == "seed") {
            l.seed = strtoull(v.c_str(), &end, 0);
            if (*end) throw bad();
        } else if (k == "gain") {  // linear, or with a trailing dB
            float g = strtof(v.c_str(), &end);
            const bool db = end != v.c_str() && (std::string(end) == "dB" || std::string(end) == "db");
            if (db) g = (float)std::pow(10.0, (double)g / 20.0);
            if (end == v.c_str() || (*end && !db) || !std::isfinite(g)) throw bad();
            l.gain = g;
        } else if (k == "at" || k == "fade") {
            uint64_t ms = 0;
            if (!parse_duration_ms(v, &ms)) throw bad();
            if (k == "at") l.at_ms = ms;
            else l.fade_ms = ms;
        } else {
            throw bad();
        }
    }
    return l;
}

// The keys of Layer::fade_in_out (src/mixer.rs:179-190), placed as dur_to_sample places them: (0, 0), (d(fade), 1),
// (d(T - fade), 1), (d(T), 0), T the reference's expected_total_samples as a Duration of f32 seconds; durations are whole
// nanoseconds, as the reference's are. Every amplitude is scaled by the layer's gain. A key that repeats the frame and
// amplitude of the one before it is dropped; a repeated frame with another amplitude is refused. Without a fade: one key
// that holds the gain, or none at gain 1.
void layer_keys(const LayerSpec &l, size_t expected_total, uint32_t rate, std::vector<uint64_t> *kf, std::vector<float> *ka) {
    kf->clear();
    ka->clear();
    if (!l.fade_ms) {
        if (l.gain != 1.0f) {
            kf->push_back(0);
            ka->push_back(l.gain);
        }
        return;
    }
    auto d = [&](uint64_t ns) {  // dur_to_sample(Duration): (dur.as_secs_f32() * rate as f32) as usize
        const float secs = (float)(ns / 1000000000ull) + (float)(ns % 1000000000ull) / 1e9f;
        return (uint64_t)(secs * (float)rate);
    };
    const uint64_t F = *l.fade_ms * 1000000ull;
    const uint64_t T = (uint64_t)((double)((float)expected_total / (float)rate) * 1e9);  // Duration::from_secs_f32
    if (F > T) throw std::runtime_error("--layer: a fade of " + std::to_string(*l.fade_ms) + " ms is longer than the layer");
    const uint64_t frames[4] = {0, d(F), d(T - F), d(T)};
    const float amps[4] = {0.0f, l.gain, l.gain, 0.0f};
    for (int i = 0; i < 4; ++i) {
        if (!kf->empty() && kf->back() == frames[i] && ka->back() == amps[i]) continue;
        if (!kf->empty() && kf->back() >= frames[i])
            throw std::runtime_error("--layer: the fade's keys meet at frame " + std::to_string(frames[i]) + " with two amplitudes");
        kf->push_back(frames[i]);
        ka->push_back(amps[i]);
    }
}

void usage() {
    fprintf(stderr,
            "rocoder (gfx950 engine)\nA live-codeable phase vocoder.\n\nUSAGE:\n    rocoder [FLAGS] [OPTIONS]\n\n"
            "FLAGS:\n        --rotate-channels    Rotate the input audio channels (with --frames-on-gpu: spelled --channel-map,\n"
            "                             stereo --channel-map 1,0; in general map[c] = (c + C - 1) %% C)\n"
            "        --frames-on-gpu      Decode the input's PCM frames and interleave the output on the GPU (one engine call;\n"
            "                             not with --freq-kernel, --device-kernel-src, --devices, --rotate-channels)\n"
            "        --split-mono         With --frames-on-gpu: where all channels of the input but one are silent, copy that\n"
            "                             channel over the others, as the reference treats a mono source recorded from a\n"
            "                             non-mono device, in front of --autocrop; the channels are measured on the GPU\n"
            "    -h, --help\n\nOPTIONS:\n"
            "    -a, --amplitude <amplitude>        Output amplitude [default: 1]\n"
            "    -b, --buffer <buffer-dur>          The maximum amount of audio to process ahead of time [default: 1]\n"
            "    -d, --duration <duration>          Duration to use from input audio (hh:mm:ss.ss)\n"
            "    -x, --fade <fade>                  Fade (playback only; ignored with -o unless --fade-output is given) [default: 1]\n"
            "        --layer <key=value,...>        With --frames-on-gpu and -o, repeatable: the run is a mix of one layer per --layer over\n"
            "                                       the same input, summed on the GPU. Keys: f, p, cents, a, seed (defaults: the main\n"
            "                                       flags), gain (linear or dB), at (the layer's offset in the output), fade (the\n"
            "                                       reference's fade_in_out keys; the fade-out is cut where the layer ends). The main\n"
            "                                       flags' --fade-output, --limit*, --normalize, --dither*, --output-format act on the sum\n"
            "        --fade-output                  With --frames-on-gpu: fade the output file in and out over -x, as the\n"
            "                                       reference fades its playback, on the GPU in front of --normalize and the\n"
            "                                       quantiser; a fade longer than the output is left out with a warning\n"
            "    -f, --factor <factor>              Stretch factor [default: 1]\n"
            "        --freq-kernel <freq-kernel>    Path to a frequency kernel (.c/.cpp source or .so exporting `apply`)\n"
            "    -i, --input <input>                A .wav file; '-' for stdin\n"
            "    -o, --output <output>              Output .wav file path. 32-bit float unless --output-format says otherwise.\n"
            "        --output-format <fmt>          Sample format of the output file: f32 | u8 | i16 | i24 | i32 | input (that of\n"
            "                                       the input file) [default: f32]. Integers are rounded to nearest and clipped;\n"
            "                                       the number of clipped samples is reported\n"
            "        --dither <mode>                none | tpdf | tpdf-hp: dither in front of the quantiser of --output-format u8, i16\n"
            "                                       or i24 (refused with any other format): triangular noise of 2 LSB peak to\n"
            "                                       peak, white (tpdf) or high-passed (tpdf-hp); on the GPU with --frames-on-gpu,\n"
            "                                       the same bytes without [default: none]\n"
            "        --dither-seed <u64>            Seed of --dither [default: the value of --seed]\n"
            "        --phase <mode>                 random | propagate | locked: how the resynthesis sets its phases. random is the\n"
            "                                       reference's (right at a factor of 8 and beyond); propagate lets every bin carry\n"
            "                                       its own phase from hop to hop, locked gives every bin the rotation of its\n"
            "                                       nearest spectral peak: a phase vocoder that keeps partials at small factors and\n"
            "                                       under --pitch-cents. Other than random: with --frames-on-gpu, a window that is a\n"
            "                                       power of two up to 16384, and without --layer, --factor-curve, --time-map,\n"
            "                                       --pitch-curve or a kernel flag [default: random]\n"
            "        --autocrop                     With --frames-on-gpu: crop dead air off both ends of the input, as the reference\n"
            "                                       crops a recording, in front of -s/-d; the peaks are measured on the GPU\n"
            "        --autocrop-window <dur>        The analysis window of --autocrop [default: 0.1]\n"
            "        --autocrop-percentile <p>      The noise-floor percentile of --autocrop, 0 ... 99 [default: 30]\n"
            "        --channel-map <a,b,...>        With --frames-on-gpu: channel c of the job reads channel <c-th entry> of the\n"
            "                                       input, one entry per channel of the file (a permutation or a copy; the\n"
            "                                       rotation of --rotate-channels is 1,0 for stereo); applied on the GPU\n"
            "        --normalize <peak>             With --frames-on-gpu: measure the peak of the whole output on the GPU and scale\n"
            "                                       it to <peak> (1 = full scale) in front of the quantiser, any --output-format;\n"
            "                                       peak and gain are reported\n"
            "        --loudness <LUFS>              With --frames-on-gpu: measure the integrated loudness (ITU-R BS.1770-4 / EBU R 128) and\n"
            "                                       the true peak of the whole output on the GPU and scale it to <LUFS> in front of\n"
            "                                       the quantiser, behind --limit and --fade-output; not with --normalize;\n"
            "                                       loudness, true peak and gain are reported\n"
            "        --true-peak <level | dB>       With --loudness: the gain stops where the 4x oversampled peak reaches this level\n"
            "                                       (1 = full scale, or -1dB)\n"
            "        --pitch-ratio <a/b | decimal>  With --frames-on-gpu: multiply every frequency by the ratio (1/8 ... 8) and keep\n"
            "                                       the duration: the stretch runs at factor * ratio and the result is resampled,\n"
            "                                       band-limited, on the GPU. Composes with -p\n"
            "        --pitch-cents <c>              The same with the ratio 2^(c / 1200): 100 is a semitone up\n"
            "        --output-rate <Hz>             With --frames-on-gpu: write the output at this sample rate (resampled on the\n"
            "                                       GPU in the same pass as --pitch-ratio); the pitch and the duration stay\n"
            "        --factor-curve <t:f,t:f,...>   With --frames-on-gpu: a stretch factor that varies along the input: f at input time t\n"
            "                                       (a duration, behind -s / --autocrop), linear in between, constant outside the\n"
            "                                       points; takes the place of -f (an explicit -f is refused). Under either map\n"
            "                                       flag --fade-output fades out into the map's last frame, and --pitch-ratio /\n"
            "                                       --pitch-cents are refused (they work through -f, which a map ignores)\n"
            "        --pitch-curve <t:c,t:c,...>    With --frames-on-gpu: a pitch that varies along the input: c cents at input time t (a\n"
            "                                       duration), linear in between, constant outside the points: a glide, a tape\n"
            "                                       stop, a vibrato. The duration stays what -f or --factor-curve make it: the\n"
            "                                       stretch runs at factor * ratio along a time map and the result is resampled on\n"
            "                                       the GPU by a step that follows the curve. --output-rate composes; refused with\n"
            "                                       --pitch-ratio, --pitch-cents and --time-map\n"
            "        --time-map <file>              With --frames-on-gpu: hop k reads the input at the k-th position of the file: one\n"
            "                                       integer (input frames) per line, # comments; positions may repeat (a hold),\n"
            "                                       decrease (reverse), be negative or lie past the end (silence)\n"
            "        --limit <ceiling | dB>         With --frames-on-gpu: a look-ahead peak limiter on the GPU behind --fade-output and in\n"
            "                                       front of --normalize, --dither and the quantiser: no sample leaves above the\n"
            "                                       ceiling (1 = full scale, or -0.3dB), frames away from an over keep their bits;\n"
            "                                       the frames turned down and the lowest gain are reported\n"
            "        --limit-drive <gain | dB>      Gain in front of --limit [default: 1]\n"
            "        --limit-lookahead <dur>        The ramp of --limit to either side of an over, at most 2048 frames of the output\n"
            "                                       file [default: 0.005]\n"
            "    -p, --pitch_multiple <n>           A non-zero integer pitch multiplier [default: 1]\n"
            "    -s, --start <start>                Start time in input audio (hh:mm:ss.ss)\n"
            "    -w, --window <window-len>          Processing window size [default: 16384]\n"
            "        --device-kernel <spec>         On-GPU frequency kernel: gain:<g> | band:<lo>:<hi>:<g_in>:<g_out> | shift:<bins>\n"
            "        --device-kernel-src <file.hip> On-GPU frequency kernel in HIP, recompiled when the file changes: defines\n"
            "                                       __device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h)\n"
            "                                       A source that says #define RC_HISTORY D (D <= 8) also reads X.past(1..D), the D hops before\n"
            "                                       One that says #define RC_CROSS_CHANNEL 1 also reads X.channel(c), the other channels' spectra\n"
            "                                       One that says #define RC_SUMS S (S <= 4) and defines rc_sum_term(X, j, h, i) also reads X.sum(i), sums over the whole hop\n"
            "                                       One that says #define RC_FEEDBACK F (F <= 4) also reads X.out(1..F), what it returned for the F hops before\n"
            "        --dk-params <a,b,...>          Up to 16 floats for --device-kernel-src (h.param(i))\n"
            "        --kernel-threads <n>           Host threads calling --freq-kernel (channels in parallel; needs a re-entrant kernel)\n"
            "        --seed <u64>                   Phase-source seed (the reference uses an unseeded thread_rng)\n"
            "        --device <n>                   HIP device ordinal [default: 0]\n"
            "        --devices <a,b,...>            Shard the job over several GPUs (offline; not with --freq-kernel)\n");
}

int run(int argc, char **argv) {
    Opt o;
    auto need = [&](int &i) -> std::string {
        if (i + 1 >= argc) throw std::runtime_error(std::string("missing value for ") + argv[i]);
        return argv[++i];
    };
    auto dur = [&](const std::string &s) -> uint64_t {
        uint64_t ms;
        if (!parse_duration_ms(s, &ms)) throw std::runtime_error("Invalid duration specification: " + s);
        return ms;
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-h" || a == "--help") { usage(); return 0; }
        else if (a == "--parse-duration") {  // test hook: the 8 cases of duration_parser.rs:32-39
            uint64_t ms;
            const std::string v = need(i);
            if (parse_duration_ms(v, &ms)) printf("%llu\n", (unsigned long long)ms);
            else printf("error\n");
            return 0;
        } else if (a == "--encode-pcm") {  // test hook: raw f32 samples -> the bytes --output-format <fmt> writes for them
            const std::string name = need(i), in = need(i), outp = need(i);
            const uint32_t fmt = pcm_format_by_name(name);
            if (!fmt) throw std::runtime_error("bad format " + name);
            FILE *f = fopen(in.c_str(), "rb");
            if (!f) throw std::runtime_error("cannot open " + in);
            std::vector<float> x;
            float v;
            while (fread(&v, 4, 1, f) == 1) x.push_back(v);
            fclose(f);
            std::vector<unsigned char> y(x.size() * pcm_sample_bytes(fmt) + 1);
            const float *rows[1] = {x.data()};
            const uint64_t clipped = encode_frames(rows, 1, 0, x.size(), fmt, y.data());
            FILE *g = fopen(outp.c_str(), "wb");
            if (!g) throw std::runtime_error("cannot create " + outp);
            fwrite(y.data(), 1, y.size() - 1, g);
            fclose(g);
            printf("%zu %llu\n", x.size(), (unsigned long long)clipped);
            return 0;
        } else if (a == "--encode-pcm-dither") {  // test hook: frame-major f32 frames -> the bytes --output-format <fmt> --dither <mode> writes
            const std::string name = need(i), mode = need(i), seed = need(i), chs = need(i), t0s = need(i), in = need(i), outp = need(i);
            const uint32_t fmt = pcm_format_by_name(name);
            const uint32_t md = mode == "none" ? RC_DITHER_NONE : mode == "tpdf" ? RC_DITHER_TPDF : mode == "tpdf-hp" ? RC_DITHER_TPDF_HP : 99u;
            const uint32_t ch = (uint32_t)strtoul(chs.c_str(), nullptr, 10);
            const uint64_t t0 = strtoull(t0s.c_str(), nullptr, 0);
            if (!fmt || md == 99u || !ch) throw std::runtime_error("bad --encode-pcm-dither arguments");
            FILE *f = fopen(in.c_str(), "rb");
            if (!f) throw std::runtime_error("cannot open " + in);
            std::vector<float> x;
            float v;
            while (fread(&v, 4, 1, f) == 1) x.push_back(v);
            fclose(f);
            const HostDither dith(md, strtoull(seed.c_str(), nullptr, 0), ch);
            const uint32_t sb = pcm_sample_bytes(fmt);
            std::vector<unsigned char> y(x.size() * sb + 1);
            uint64_t clipped = 0;
            for (size_t k = 0; k < x.size(); ++k) {
                clipped += pcm_clipped(x[k]);
                const float d = dith.on(fmt) ? dith.d((uint32_t)(k % ch), t0 + k / ch) : 0.0f;
                pcm_encode(x[k], fmt, y.data() + k * sb, dith.on(fmt) ? &d : nullptr);
            }
            FILE *g = fopen(outp.c_str(), "wb");
            if (!g) throw std::runtime_error("cannot create " + outp);
            fwrite(y.data(), 1, y.size() - 1, g);
            fclose(g);
            printf("%zu %llu\n", x.size() / ch, (unsigned long long)clipped);
            return 0;
        } else if (a == "--encode-wav") {  // test hook: raw f32 planar [channels][frames] -> the WAV --output-format <fmt> writes
            const std::string name = need(i), chs = need(i), rate = need(i), in = need(i), outp = need(i);
            const uint32_t fmt = pcm_format_by_name(name);
            Audio au;
            au.spec.channels = (uint16_t)atoi(chs.c_str());
            au.spec.sample_rate = (uint32_t)strtoul(rate.c_str(), nullptr, 10);
            if (!fmt || !au.spec.channels) throw std::runtime_error("bad --encode-wav arguments");
            FILE *f = fopen(in.c_str(), "rb");
            if (!f) throw std::runtime_error("cannot open " + in);
            std::vector<float> x;
            float v;
            while (fread(&v, 4, 1, f) == 1) x.push_back(v);
            fclose(f);
            const size_t frames = x.size() / au.spec.channels;
            for (uint32_t c = 0; c < au.spec.channels; ++c) au.data.emplace_back(x.begin() + c * frames, x.begin() + (c + 1) * frames);
            uint64_t clipped = 0;
            write_wav(outp, au, fmt, &clipped);
            printf("%zu %llu\n", frames, (unsigned long long)clipped);
            return 0;
        } else if (a == "--decode-wav") {  // test hook: WAV -> raw f32 planar [channels][frames]
            const std::string in = need(i), outp = need(i);
            FILE *f = in == "-" ? stdin : fopen(in.c_str(), "rb");
            if (!f) throw std::runtime_error("cannot open " + in);
            Audio au = read_wav(f);
            FILE *g = fopen(outp.c_str(), "wb");
            for (auto &c : au.data) fwrite(c.data(), 4, c.size(), g);
            fclose(g);
            printf("%u %u %zu\n", au.spec.channels, au.spec.sample_rate, au.data.empty() ? 0 : au.data[0].size());
            return 0;
        }
        else if (a == "-w" || a == "--window") o.window_len = (size_t)strtoull(need(i).c_str(), nullptr, 10);
        else if (a == "-b" || a == "--buffer") o.buffer_ms = dur(need(i));
        else if (a == "-f" || a == "--factor") {
            o.factor = strtof(need(i).c_str(), nullptr);
            o.factor_given = true;
        } else if (a == "--factor-curve") o.factor_curve = need(i);
        else if (a == "--time-map") o.time_map_file = need(i);
        else if (a == "--pitch-curve") o.pitch_curve = need(i);
        else if (a == "-p" || a == "--pitch_multiple" || a == "--pitch-multiple") o.pitch_multiple = atoi(need(i).c_str());
        else if (a == "-a" || a == "--amplitude") o.amplitude = strtof(need(i).c_str(), nullptr);
        else if (a == "-i" || a == "--input") o.input = need(i);
        else if (a == "--rotate-channels") o.rotate_channels = true;
        else if (a == "--frames-on-gpu") o.frames_on_gpu = true;
        else if (a == "--fade-output") o.fade_output = true;
        else if (a == "--layer") o.layers.push_back(need(i));
        else if (a == "--autocrop") o.autocrop = true;
        else if (a == "--split-mono") o.split_mono = true;
        else if (a == "--channel-map") {
            const std::string v = need(i);
            std::vector<uint32_t> m;
            for (size_t b = 0; b <= v.size();) {
                const size_t c = std::min(v.find(',', b), v.size());
                const std::string t = v.substr(b, c - b);
                char *end = nullptr;
                const unsigned long long x = strtoull(t.c_str(), &end, 10);
                if (t.empty() || *end || !isdigit((unsigned char)t[0]) || x > 65535)
                    throw std::runtime_error("--channel-map takes a list of channel indices a,b,..., not " + v);
                m.push_back((uint32_t)x);
                b = c + 1;
            }
            o.channel_map = std::move(m);
        }
        else if (a == "--autocrop-window") {
            o.autocrop_window_ms = dur(need(i));
            if (o.autocrop_window_ms == 0) throw std::runtime_error("--autocrop-window takes a duration above 0");
        }
        else if (a == "--autocrop-percentile") {
            const std::string v = need(i);
            char *end = nullptr;
            const unsigned long t = strtoul(v.c_str(), &end, 10);
            if (v.empty() || *end || v[0] == '-' || t >= 100)
                throw std::runtime_error("--autocrop-percentile takes an integer of 0 ... 99, not " + v);
            o.autocrop_percentile = (uint32_t)t;
        }
        else if (a == "--output-format") {
            o.output_format = need(i);
            if (!pcm_format_by_name(*o.output_format) && *o.output_format != "input")
                throw std::runtime_error("--output-format takes f32, u8, i16, i24, i32 or input, not " + *o.output_format);
        }
        else if (a == "--dither") {
            const std::string v = need(i);
            if (v != "none" && v != "tpdf" && v != "tpdf-hp") throw std::runtime_error("--dither takes none, tpdf or tpdf-hp, not " + v);
            o.dither = v == "tpdf" ? RC_DITHER_TPDF : v == "tpdf-hp" ? RC_DITHER_TPDF_HP : RC_DITHER_NONE;
            o.dither_given = true;
        }
        else if (a == "--phase") {
            const std::string v = need(i);
            if (v != "random" && v != "propagate" && v != "locked") throw std::runtime_error("--phase takes random, propagate or locked, not " + v);
            o.phase = v == "locked" ? RC_PHASE_LOCKED : v == "propagate" ? RC_PHASE_PROPAGATE : RC_PHASE_RANDOM;
        }
        else if (a == "--dither-seed") {
            const std::string v = need(i);
            char *end = nullptr;
            const unsigned long long t = strtoull(v.c_str(), &end, 0);
            if (v.empty() || *end || v[0] == '-') throw std::runtime_error("--dither-seed takes an unsigned integer, not " + v);
            o.dither_seed = t;
        }
        else if (a == "--normalize") {
            const std::string v = need(i);
            char *end = nullptr;
            const float t = strtof(v.c_str(), &end);
            if (v.empty() || *end || !(t > 0.0f) || !std::isfinite(t))
                throw std::runtime_error("--normalize takes a finite peak level above 0, not " + v);
            o.normalize = t;
        }
        else if (a == "--loudness") {
            const std::string v = need(i);
            char *end = nullptr;
            const float t = strtof(v.c_str(), &end);
            if (v.empty() || *end || !std::isfinite(t)) throw std::runtime_error("--loudness takes a finite level in LUFS (-14, -23), not " + v);
            o.loudness = t;
        }
        else if (a == "--true-peak") {  // linear, or with a trailing dB (dBTP)
            const std::string v = need(i);
            char *end = nullptr;
            float t = strtof(v.c_str(), &end);
            const bool db = end != v.c_str() && (std::string(end) == "dB" || std::string(end) == "db");
            if (db) t = (float)std::pow(10.0, (double)t / 20.0);
            if (v.empty() || end == v.c_str() || (*end && !db) || !(t > 0.0f) || !std::isfinite(t))
                throw std::runtime_error("--true-peak takes a finite level above 0, linear or in dB (-1dB), not " + v);
            o.true_peak = t;
        }
        else if (a == "--pitch-ratio" || a == "--pitch-cents") {
            if (o.pitch_ratio) throw std::runtime_error("--pitch-ratio and --pitch-cents: one of them, once");
            const std::string v = need(i);
            char *end = nullptr;
            double r = strtod(v.c_str(), &end);
            if (a == "--pitch-ratio" && end != v.c_str() && *end == '/') {  // a/b
                const std::string den = end + 1;
                const double d = strtod(den.c_str(), &end);
                r = den.empty() || *end ? NAN : r / d;
            } else if (v.empty() || *end) {
                r = NAN;
            } else if (a == "--pitch-cents") {
                r = std::exp2(r / 1200.0);
            }
            if (!(r >= 0.125 && r <= 8.0)) throw std::runtime_error(a + " takes a ratio of 1/8 ... 8 (3600 cents either way), not " + v);
            o.pitch_ratio = r;
        }
        else if (a == "--limit" || a == "--limit-drive") {  // linear, or with a trailing dB
            const std::string v = need(i);
            char *end = nullptr;
            float t = strtof(v.c_str(), &end);
            const bool db = end != v.c_str() && (std::string(end) == "dB" || std::string(end) == "db");
            if (db) t = (float)std::pow(10.0, (double)t / 20.0);
            if (v.empty() || end == v.c_str() || (*end && !db) || !(t > 0.0f) || !std::isfinite(t))
                throw std::runtime_error(a + " takes a finite level above 0, linear or in dB (-0.3dB), not " + v);
            if (a == "--limit") o.limit = t;
            else {
                o.limit_drive = t;
                o.limit_drive_given = true;
            }
        }
        else if (a == "--limit-lookahead") {
            o.limit_lookahead_ms = dur(need(i));
            o.limit_lookahead_given = true;
        }
        else if (a == "--output-rate") {
            const std::string v = need(i);
            char *end = nullptr;
            const unsigned long t = strtoul(v.c_str(), &end, 10);
            if (v.empty() || *end || v[0] == '-' || t == 0 || t > 0xFFFFFFFFul) throw std::runtime_error("--output-rate takes a sample rate in Hz, not " + v);
            o.output_rate = (uint32_t)t;
        }
        else if (a == "--freq-kernel") o.freq_kernel = need(i);
        else if (a == "--device-kernel") o.device_kernel = need(i);
        else if (a == "--device-kernel-src") o.device_kernel_src = need(i);
        else if (a == "--dk-params") {
            const std::string v = need(i);
            for (size_t b = 0; b <= v.size();) {
                const size_t c = std::min(v.find(',', b), v.size());
                char *end = nullptr;
                const std::string t = v.substr(b, c - b);
                const float x = strtof(t.c_str(), &end);
                if (t.empty() || *end) throw std::runtime_error("bad --dk-params " + v);
                o.dk_params.push_back(x);
                b = c + 1;
            }
            if (o.dk_params.size() > 16) throw std::runtime_error("--dk-params takes at most 16 values");
        }
        else if (a == "--kernel-threads") o.kernel_threads = atoi(need(i).c_str());
        else if (a == "-x" || a == "--fade") o.fade_ms = dur(need(i));
        else if (a == "-s" || a == "--start") o.start_ms = dur(need(i));
        else if (a == "-d" || a == "--duration") o.duration_ms = dur(need(i));
        else if (a == "-o" || a == "--output") o.output = need(i);
        else if (a == "--seed") o.seed = strtoull(need(i).c_str(), nullptr, 0);
        else if (a == "--device") o.device = atoi(need(i).c_str());
        else if (a == "--devices") {
            const std::string v = need(i);
            for (size_t b = 0; b <= v.size();) {
                const size_t c = std::min(v.find(',', b), v.size());
                if (c == b) throw std::runtime_error("bad --devices " + v);
                o.devices.push_back((int32_t)atoi(v.substr(b, c - b).c_str()));
                b = c + 1;
            }
        }
        else throw std::runtime_error("unknown argument " + a);
    }
    if (!o.input) throw std::runtime_error("recording from an input device (no -i) is not supported: pass -i <file.wav> or -i -");
    if (!o.output) throw std::runtime_error("live playback (no -o) is not supported: pass -o <file.wav>");
    if (o.pitch_multiple < -128 || o.pitch_multiple > 127) throw std::runtime_error("pitch_multiple must fit an i8");
    if (o.device_kernel_src && (o.freq_kernel || o.device_kernel))
        throw std::runtime_error("--device-kernel-src cannot be combined with --freq-kernel or --device-kernel");
    if (!o.dk_params.empty() && !o.device_kernel_src) throw std::runtime_error("--dk-params needs --device-kernel-src");
    // the peak of the whole output has to be known before its first sample is written: the streamed host writer never
    // holds the whole output, the engine under --frames-on-gpu does
    if (o.normalize && !o.frames_on_gpu) throw std::runtime_error("--normalize needs --frames-on-gpu");
    // (the loudness of the whole output as well)
    if ((o.loudness || o.true_peak) && !o.frames_on_gpu) throw std::runtime_error("--loudness / --true-peak needs --frames-on-gpu");
    if (o.true_peak && !o.loudness) throw std::runtime_error("--true-peak needs --loudness: it is the ceiling of that gain");
    if ((o.loudness || o.true_peak) && o.normalize) throw std::runtime_error("--loudness / --true-peak cannot be combined with --normalize: one gain, one rule");
    // (the fade is applied by the engine's whole-job calls: the streamed host writer has no such step)
    if (o.fade_output && !o.frames_on_gpu) throw std::runtime_error("--fade-output needs --frames-on-gpu");
    // (the resampler is a stage of the engine's whole-job calls: the streamed host writer has no such step)
    if (o.pitch_ratio && !o.frames_on_gpu) throw std::runtime_error("--pitch-ratio / --pitch-cents needs --frames-on-gpu");
    if (o.output_rate && !o.frames_on_gpu) throw std::runtime_error("--output-rate needs --frames-on-gpu");
    // (the limiter is a stage of the engine's whole-job calls: the streamed host writer has no such step)
    if (o.limit && !o.frames_on_gpu) throw std::runtime_error("--limit needs --frames-on-gpu");
    if ((o.limit_drive_given || o.limit_lookahead_given) && !o.limit) throw std::runtime_error("--limit-drive / --limit-lookahead needs --limit");
    // (the bins are measured by the engine on the raw frame block: the host reader has decoded it by then)
    if (o.autocrop && !o.frames_on_gpu) throw std::runtime_error("--autocrop needs --frames-on-gpu");
    // (the map is an index in the engine's unpack kernel; the host path has --rotate-channels)
    if (o.channel_map && !o.frames_on_gpu) throw std::runtime_error("--channel-map needs --frames-on-gpu");
    // (the channels are measured by the engine on the raw frame block, and the copy is the engine's channel map)
    if (o.split_mono && !o.frames_on_gpu) throw std::runtime_error("--split-mono needs --frames-on-gpu");
    // (the map is state of the engine's whole-job calls: the streaming seam the host path runs on refuses one)
    if ((o.factor_curve || o.time_map_file) && !o.frames_on_gpu) throw std::runtime_error("--factor-curve / --time-map needs --frames-on-gpu");
    if (o.pitch_curve && !o.frames_on_gpu) throw std::runtime_error("--pitch-curve needs --frames-on-gpu");
    if (o.pitch_curve && o.pitch_ratio)
        throw std::runtime_error("--pitch-curve cannot be combined with --pitch-ratio / --pitch-cents: one pitch, a constant or a curve");
    if (o.pitch_curve && o.time_map_file)
        throw std::runtime_error("--pitch-curve cannot be combined with --time-map: the curve builds the map itself (-f or --factor-curve set the speed)");
    if (o.factor_curve && o.time_map_file) throw std::runtime_error("--factor-curve cannot be combined with --time-map: one map");
    if (o.factor_curve && o.factor_given) throw std::runtime_error("--factor-curve takes the place of -f: give one of them");
    // (--pitch-ratio keeps the duration by stretching at factor * ratio: a map ignores the factor, so the two cannot compose)
    if ((o.factor_curve || o.time_map_file) && o.pitch_ratio)
        throw std::runtime_error("--pitch-ratio / --pitch-cents cannot be combined with --factor-curve / --time-map: a map sets the speed, not -f");
    if (!o.layers.empty()) {
        if (!o.frames_on_gpu || !o.output) throw std::runtime_error("--layer needs --frames-on-gpu and -o");
        const char *with = o.loudness || o.true_peak ? "--loudness" : o.pitch_curve ? "--pitch-curve" : o.factor_curve ? "--factor-curve"
                           : o.time_map_file ? "--time-map" : o.device_kernel_src ? "--device-kernel-src" : o.output_rate ? "--output-rate"
                           : o.channel_map ? "--channel-map" : o.split_mono ? "--split-mono" : nullptr;
        if (with) throw std::runtime_error(std::string("--layer cannot be combined with ") + with);
    }
    if (o.phase != RC_PHASE_RANDOM) {
        // (a mode is state of the engine's whole-job calls, and the stage takes the place a kernel or a map would need)
        if (!o.frames_on_gpu) throw std::runtime_error("--phase propagate / locked needs --frames-on-gpu");
        const char *with = !o.layers.empty() ? "--layer" : o.factor_curve ? "--factor-curve" : o.time_map_file ? "--time-map"
                           : o.pitch_curve ? "--pitch-curve" : o.freq_kernel ? "--freq-kernel" : o.device_kernel_src ? "--device-kernel-src"
                           : o.device_kernel ? "--device-kernel" : nullptr;
        if (with) throw std::runtime_error(std::string("--phase propagate / locked cannot be combined with ") + with);
    }
    if (o.dither_seed && !o.dither_given) throw std::runtime_error("--dither-seed needs --dither");
    // dither belongs in front of a quantiser of 8, 16 or 24 bits: f32 has none, and a step of i32 lies below an f32's precision
    auto check_dither_format = [&](uint32_t fmt) {
        if (o.dither != RC_DITHER_NONE && fmt != RC_PCM_U8 && fmt != RC_PCM_I16 && fmt != RC_PCM_I24)
            throw std::runtime_error("--dither needs --output-format u8, i16 or i24 (or input, of such a file)");
    };
    if (!o.output_format) check_dither_format(RC_PCM_F32);
    else if (*o.output_format != "input") check_dither_format(pcm_format_by_name(*o.output_format));
    if (o.frames_on_gpu) {
        // one engine call computes the whole job: nothing polls a watched kernel between windows, and the frame block is
        // neither sharded nor reordered
        const char *with = o.freq_kernel ? "--freq-kernel" : o.device_kernel_src ? "--device-kernel-src" : !o.devices.empty() ? "--devices"
                           : o.rotate_channels ? "--rotate-channels" : nullptr;
        if (with) {
            fprintf(stderr, "error: --frames-on-gpu cannot be combined with %s\n", with);
            return 2;
        }
    }

    // ROCODER_CLI_TIMING=1: wall time of each phase on stderr (dev aid)
    const bool timing = g_timing = getenv("ROCODER_CLI_TIMING") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[timing] %-14s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    // load_audio (src/main.rs:162-188)
    FILE *f = *o.input == "-" ? stdin : fopen(o.input->c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + *o.input);
    Audio audio;
    RawAudio raw;
    uint32_t in_format = RC_PCM_F32;
    size_t raw_first = 0, raw_count = 0;  // --frames-on-gpu: -s / -d as a frame offset and count into raw.data
    // Audio::clip_in_place on the frames [raw_first, raw_first + raw_count): -s / -d inside what is there
    auto clip_raw = [&]() {
        if (!o.start_ms && !o.duration_ms) return;
        const size_t have = raw_count;
        size_t first = 0;
        if (o.start_ms) first = (size_t)((double)*o.start_ms / 1000.0 * (double)raw.spec.sample_rate);
        size_t endp = have;
        if (o.duration_ms) endp = first + (size_t)((double)*o.duration_ms / 1000.0 * (double)raw.spec.sample_rate);
        if (first > have || endp > have || first > endp)
            throw std::runtime_error("clip range out of bounds (the reference panics on the slice)");
        raw_first += first;
        raw_count = endp - first;
    };
    if (o.frames_on_gpu) {
        // --channel-map: one index per channel of the file, each a channel of the file - checked once the header is read,
        // before the data chunk, its page-locked memory and any engine work
        raw = read_wav_raw(f, [&](const AudioSpec &s) {
            if (!o.channel_map) return;
            if (o.channel_map->size() != s.channels)
                throw UsageError("--channel-map has " + std::to_string(o.channel_map->size()) + " entries, the input has " +
                                 std::to_string(s.channels) + " channels");
            for (const uint32_t m : *o.channel_map)
                if (m >= s.channels)
                    throw UsageError("--channel-map names channel " + std::to_string(m) + ", the input has channels 0 ... " +
                                     std::to_string(s.channels - 1));
        });
        raw_count = raw.frames;
        if (!o.autocrop) clip_raw();  // (with --autocrop: behind the crop, which needs the engine)
    } else {
        audio = read_wav(f, &in_format);
    }
    if (f != stdin) fclose(f);
    // --output-format: without the flag the file is the f32 file of old and nothing is counted or reported
    const bool out_fmt_given = o.output_format.has_value();
    const uint32_t out_fmt = !out_fmt_given ? (uint32_t)RC_PCM_F32 : *o.output_format == "input" ? (o.frames_on_gpu ? raw.format : in_format)
                                                                                           : pcm_format_by_name(*o.output_format);
    check_dither_format(out_fmt);  // (--output-format input: known only now)
    auto report_clipped = [&](uint64_t clipped, uint64_t samples) {
        if ((out_fmt_given || o.normalize || o.loudness || o.true_peak) && clipped) fprintf(stderr, "%llu of %llu samples clipped\n", (unsigned long long)clipped, (unsigned long long)samples);
    };
    if (!o.frames_on_gpu && (o.start_ms || o.duration_ms)) audio.clip_in_place(o.start_ms, o.duration_ms);
    if (o.rotate_channels) audio.rotate_channels();
    const size_t total_samples_len = o.frames_on_gpu ? raw_count : audio.data.empty() ? 0 : audio.data[0].size();
    const AudioSpec spec = o.frames_on_gpu ? raw.spec : audio.spec;
    lap("read input");

    KernelStack kernels;
    if (o.freq_kernel) kernels.start(*o.freq_kernel);
    DeviceKernelWatcher dk;
    if (o.device_kernel_src) {
        dk_api();  // (fails here, before any work, when the library lacks them)
        dk.start(*o.device_kernel_src);
    }

    rc_config cfg{};
    cfg.struct_size = sizeof cfg;
    cfg.window_len = (uint32_t)o.window_len;
    // --pitch-ratio r: the stretch runs at factor * r and the result is resampled by r input frames per output frame, so
    // that the duration stays factor * L and every frequency is multiplied by r
    cfg.factor = o.pitch_ratio ? (float)((double)o.factor * *o.pitch_ratio) : o.factor;
    cfg.amplitude = o.amplitude;
    cfg.pitch_multiple = o.pitch_multiple;
    cfg.sample_rate = spec.sample_rate;
    cfg.channels = spec.channels;
    cfg.buffer_secs = (float)o.buffer_ms / 1000.0f;
    cfg.seed = o.seed;
    cfg.device = o.device;
    cfg.kernel = o.freq_kernel ? &KernelStack::trampoline : nullptr;
    cfg.kernel_user = &kernels;
    cfg.kernel_threads = (uint32_t)std::max(0, o.kernel_threads);
    if (o.device_kernel) {
        std::vector<std::string> f;
        size_t b = 0;
        for (;;) {
            const size_t c = o.device_kernel->find(':', b);
            f.push_back(o.device_kernel->substr(b, c == std::string::npos ? c : c - b));
            if (c == std::string::npos) break;
            b = c + 1;
        }
        if (f[0] == "gain" && f.size() == 2) {
            cfg.device_kernel = RC_DK_GAIN;
            cfg.dk_gain = strtof(f[1].c_str(), nullptr);
        } else if (f[0] == "band" && f.size() == 5) {
            cfg.device_kernel = RC_DK_BAND;
            cfg.dk_lo_bin = (uint32_t)strtoul(f[1].c_str(), nullptr, 10);
            cfg.dk_hi_bin = (uint32_t)strtoul(f[2].c_str(), nullptr, 10);
            cfg.dk_gain = strtof(f[3].c_str(), nullptr);
            cfg.dk_gain_outside = strtof(f[4].c_str(), nullptr);
        } else if (f[0] == "shift" && f.size() == 2) {
            cfg.device_kernel = RC_DK_SHIFT;
            cfg.dk_shift_bins = atoi(f[1].c_str());
        } else {
            throw std::runtime_error("bad --device-kernel " + *o.device_kernel);
        }
    }
    if (o.frames_on_gpu) {
        // the file's frames as they are -> rc_engine_stretch_frames -> the output file's frames: no sample is touched
        // on the host. The same samples, so the same file, as the Stretcher / StretcherProcessor loop below writes.
        Engine eng;
        if (rc_engine_create(&cfg, &eng.h) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
        lap("engine create");
        if (o.split_mono || o.channel_map) {
            // recorder::auto_split_mono on the whole file (src/recorder.rs:64-70: in front of the autocrop), then
            // Audio::rotate_channels' place behind -s / -d (src/main.rs:179-185): neither moves a sample. Row c of the job
            // reads channel total[c] = split[user[c]] of the file: the user's map on the split audio.
            if (!frames_api().set_map) throw std::runtime_error("--channel-map / --split-mono: the engine library has no rc_engine_set_channel_map");
            const uint32_t C = spec.channels;
            std::vector<uint32_t> split(C), total(C);
            for (uint32_t c = 0; c < C; ++c) split[c] = c;
            if (o.split_mono) {
                if (!frames_api().channel_peaks || !frames_api().split_map)
                    throw std::runtime_error("--split-mono: the engine library has no rc_engine_frames_channel_peaks");
                std::vector<float> peaks(C);
                int found = 0;
                if (frames_api().channel_peaks(eng.h, raw.data.p, raw.frames, raw.format, peaks.data(), C) != RC_OK ||
                    frames_api().split_map(peaks.data(), C, split.data(), &found) != RC_OK)
                    throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
                if (found) fprintf(stderr, "Detected mono input from non-mono device. Automatically splitting.\n");  // src/recorder.rs:131
            }
            for (uint32_t c = 0; c < C; ++c) total[c] = split[o.channel_map ? (*o.channel_map)[c] : c];
            if (frames_api().set_map(eng.h, total.data(), C) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            lap("channel map");
        }
        if (o.autocrop) {
            // recorder::autocrop_audio on the whole file, then -s / -d inside what remains (src/main.rs:173-181): an offset
            // and a count into the data chunk, no copy. The crop points are frames; the reference's round trip through a
            // Duration of f32 seconds is left out.
            if (!frames_api().power || !frames_api().crop_points)
                throw std::runtime_error("--autocrop: the engine library has no rc_engine_frames_power");
            const size_t bin_frames = (size_t)((float)((double)o.autocrop_window_ms / 1000.0) * (float)spec.sample_rate);  // duration_to_sample
            if (bin_frames == 0) throw std::runtime_error("--autocrop-window is shorter than a frame");
            if (raw.frames) {
                const size_t n_bins = (raw.frames + bin_frames - 1) / bin_frames;
                std::vector<float> peaks(n_bins);
                size_t got = 0;
                uint64_t start = 0, end = raw.frames;
                int found = 0;
                if (frames_api().power(eng.h, raw.data.p, raw.frames, raw.format, bin_frames, peaks.data(), n_bins, &got) != RC_OK ||
                    frames_api().crop_points(peaks.data(), got, bin_frames, raw.frames, o.autocrop_percentile, &start, &end, &found) != RC_OK)
                    throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
                if (found) {
                    const double rate = (double)spec.sample_rate;
                    fprintf(stderr, "autocropping audio to start %llu frames (%.6g s) later and end %llu frames (%.6g s) earlier\n",
                            (unsigned long long)start, (double)start / rate, (unsigned long long)(raw.frames - end),
                            (double)(raw.frames - end) / rate);
                    raw_first = (size_t)start;
                    raw_count = (size_t)(end - start);
                } else {
                    fprintf(stderr, "autocrop: no bin above the noise threshold, nothing cropped\n");
                }
            }
            clip_raw();
            lap("autocrop");
        }
        // "<path>.part" first, as WavStreamWriter: a failed run leaves no output file
        auto write_output = [&](const unsigned char *frames, size_t n, const AudioSpec &out_spec, uint64_t clipped) {
            const uint32_t sb = pcm_sample_bytes(out_fmt);
            const std::string tmp = *o.output + ".part";
            FILE *g = fopen(tmp.c_str(), "wb");
            if (!g) throw std::runtime_error("cannot create " + tmp);
            write_wav_header(g, out_spec, n, out_fmt);
            const size_t total = n * spec.channels;
            const bool ok = fwrite(frames, sb, total, g) == total && write_wav_pad(g, out_spec, n, out_fmt);
            if (fclose(g) != 0 || !ok) {
                (void)std::remove(tmp.c_str());
                throw std::runtime_error("write failed (disk full?)");
            }
            if (std::rename(tmp.c_str(), o.output->c_str()) != 0) {
                (void)std::remove(tmp.c_str());
                throw std::runtime_error("cannot move " + tmp + " to " + *o.output);
            }
            lap("write output");
            report_clipped(clipped, total);
        };
        if (!o.layers.empty()) {
            // A mix: every --layer is one frames job over the same input, accumulated into a device-resident bus
            // under its keys; the main job is no layer, its engine is the master that sends the bus through the main flags'
            // output chain (--fade-output, --limit*, --normalize, --dither*, --output-format)
            const FramesApi &api = frames_api();
            if (!api.bus_create || !api.bus_destroy || !api.mix_frames || !api.bus_frames)
                throw std::runtime_error("--layer: the engine library has no rc_engine_mix_frames");
            LayerSpec defaults;
            defaults.factor = o.factor;
            defaults.amplitude = o.amplitude;
            defaults.pitch_multiple = o.pitch_multiple;
            defaults.ratio = o.pitch_ratio;
            defaults.seed = o.seed;
            struct Planned {
                LayerSpec l;
                rc_config cfg;
                uint32_t num = 1, den = 1;
                size_t n = 0;
                int64_t offset = 0;
                std::vector<uint64_t> kf;
                std::vector<float> ka;
            };
            std::vector<Planned> plan;
            size_t N = 0;
            for (const std::string &s : o.layers) {
                Planned p;
                p.l = parse_layer(s, defaults);
                p.cfg = cfg;
                p.cfg.factor = p.l.ratio ? (float)((double)p.l.factor * *p.l.ratio) : p.l.factor;  // (as --pitch-cents: the duration stays f * L)
                p.cfg.amplitude = p.l.amplitude;
                p.cfg.pitch_multiple = p.l.pitch_multiple;
                p.cfg.seed = p.l.seed;
                p.n = rc_offline_output_len(&p.cfg, raw_count);
                if (p.l.ratio) {
                    if (!api.set_resample || !api.resample_ratio || !api.resample_len) throw std::runtime_error("--layer cents: the engine library has no rc_engine_set_output_resample");
                    if (api.resample_ratio((float)*p.l.ratio, &p.num, &p.den) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
                    if (p.num != p.den) p.n = api.resample_len(p.n, p.num, p.den);
                }
                p.offset = (int64_t)((float)((double)p.l.at_ms / 1000.0) * (float)spec.sample_rate);  // duration_to_sample
                layer_keys(p.l, (size_t)((float)raw_count * p.l.factor), spec.sample_rate, &p.kf, &p.ka);
                N = std::max(N, (size_t)p.offset + p.n);
                plan.push_back(std::move(p));
            }
            rc_bus *bus = nullptr;
            if (api.bus_create(o.device, spec.channels, N, &bus) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            struct BusGuard {
                rc_bus *b;
                ~BusGuard() { frames_api().bus_destroy(b); }
            } bus_guard{bus};
            fprintf(stderr, "mix: %zu layers, %zu frames\n", plan.size(), N);
            const size_t frame_bytes = (size_t)spec.channels * raw.sample_bytes;
            for (size_t i = 0; i < plan.size(); ++i) {
                const Planned &p = plan[i];
                Engine layer;  // (one at a time: a layer's rows are freed before the next engine allocates its own)
                if (rc_engine_create(&p.cfg, &layer.h) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
                if (p.l.ratio && api.set_resample(layer.h, p.num, p.den) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
                uint64_t mixed = 0;
                if (api.mix_frames(layer.h, raw.data.p + raw_first * frame_bytes, raw_count, raw.format, bus, p.offset, p.kf.data(), p.ka.data(),
                                   p.kf.size(), nullptr, &mixed) != RC_OK)
                    throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
                fprintf(stderr, "layer %zu: factor %.9g, ratio %u/%u, offset %lld, %llu frames mixed\n", i, (double)p.l.factor, p.num, p.den,
                        (long long)p.offset, (unsigned long long)mixed);
            }
            lap("mix layers");
            if (o.fade_output) {  // the main job's fade, on the sum: in over the first F frames, out over the last F
                if (!api.set_fade) throw std::runtime_error("--fade-output: the engine library has no rc_engine_set_output_fade");
                const size_t fade = (size_t)((float)((double)o.fade_ms / 1000.0) * (float)spec.sample_rate);
                const bool fits = fade <= N;
                if (!fits) fprintf(stderr, "Fade in parameters out of bounds, ignoring.\nFade out parameters out of bounds, ignoring.\n");
                if (api.set_fade(eng.h, fits ? fade : 0, fits ? N - fade : RC_FADE_NONE, fits ? fade : 0) != RC_OK)
                    throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
                if (fits) fprintf(stderr, "fade in %zu frames, out from %zu over %zu\n", fade, N - fade, fade);
            }
            if (o.limit) {
                if (!api.set_limiter || !api.limiter_stats) throw std::runtime_error("--limit: the engine library has no rc_engine_set_output_limiter");
                const size_t look = (size_t)((float)((double)o.limit_lookahead_ms / 1000.0) * (float)spec.sample_rate);
                if (look > RC_LIMITER_MAX_LOOKAHEAD)
                    throw std::runtime_error("--limit-lookahead is " + std::to_string(look) + " frames at " + std::to_string(spec.sample_rate) +
                                             " Hz, at most " + std::to_string(RC_LIMITER_MAX_LOOKAHEAD));
                if (api.set_limiter(eng.h, o.limit_drive, *o.limit, (uint32_t)look) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            }
            if (o.dither != RC_DITHER_NONE) {
                if (!api.set_dither) throw std::runtime_error("--dither: the engine library has no rc_engine_set_output_dither");
                if (api.set_dither(eng.h, o.dither, o.dither_seed.value_or(o.seed)) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            }
            PinnedBytes out(N * spec.channels * pcm_sample_bytes(out_fmt));
            size_t n = 0;
            uint64_t clipped = 0;
            float peak = 0.0f, gain = 1.0f;
            if (api.bus_frames(eng.h, bus, out.p, N, out_fmt, o.normalize.value_or(0.0f), &n, &peak, &gain, &clipped) != RC_OK)
                throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            lap("master");
            if (o.normalize) fprintf(stderr, "peak %.9g, gain %.9g\n", (double)peak, (double)gain);
            if (o.limit) {
                float min_gain = 1.0f;
                uint64_t limited = 0;
                if (api.limiter_stats(eng.h, &min_gain, &limited) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
                fprintf(stderr, "limited %llu of %zu frames, lowest gain %.9g (%.1f dB)\n", (unsigned long long)limited, n, (double)min_gain,
                        min_gain > 0.0f ? 20.0 * std::log10((double)min_gain) : -INFINITY);
            }
            write_output(out.p, n, spec, clipped);
            return 0;
        }
        size_t cap = rc_offline_output_len(&cfg, raw_count);
        if (o.phase != RC_PHASE_RANDOM) {
            if (!frames_api().set_phase) throw std::runtime_error("--phase: the engine library has no rc_engine_set_phase_mode");
            if (frames_api().set_phase(eng.h, o.phase) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            rc_params par{};
            if (rc_engine_get_params(eng.h, &par) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            fprintf(stderr, "phase: %s, %llu hops\n", o.phase == RC_PHASE_LOCKED ? "locked" : "propagate",
                    (unsigned long long)(par.window_out_len ? cap / par.window_out_len * par.hops_per_window : 0));
        }
        // --pitch-curve: (input frame, ratio) points, subdivided so that no segment spans more than 50 cents - linear in the
        // ratio then stays within 0.2 cent of linear in cents
        std::vector<double> pitch_at, pitch_ratio;
        if (o.pitch_curve) {
            if (!frames_api().set_warp || !frames_api().warp_curve)
                throw std::runtime_error("--pitch-curve: the engine library has no rc_engine_set_output_warp");
            std::vector<double> at, cents;
            size_t b = 0;
            for (;;) {
                const size_t c = o.pitch_curve->find(',', b);
                const std::string pt = o.pitch_curve->substr(b, c == std::string::npos ? c : c - b);
                const size_t colon = pt.rfind(':');
                uint64_t ms = 0;
                char *end = nullptr;
                const double v = colon == std::string::npos ? 0.0 : strtod(pt.c_str() + colon + 1, &end);
                if (colon == std::string::npos || colon == 0 || !end || *end || end == pt.c_str() + colon + 1 || !std::isfinite(v) ||
                    !parse_duration_ms(pt.substr(0, colon), &ms))
                    throw std::runtime_error("--pitch-curve takes points t:c,t:c,... (t a duration, c cents), not " + pt);
                at.push_back((double)ms / 1000.0 * (double)spec.sample_rate);
                cents.push_back(v);
                if (at.size() > 1 && !(at.back() > at[at.size() - 2])) throw std::runtime_error("--pitch-curve: times ascending, at " + pt);
                if (c == std::string::npos) break;
                b = c + 1;
            }
            for (size_t i = 0; i < at.size(); ++i) {
                if (i) {
                    const size_t parts = (size_t)std::ceil(std::fabs(cents[i] - cents[i - 1]) / 50.0);
                    for (size_t k = 1; k < parts; ++k) {
                        const double t = (double)k / (double)parts;
                        pitch_at.push_back(at[i - 1] + (at[i] - at[i - 1]) * t);
                        pitch_ratio.push_back(std::exp2((cents[i - 1] + (cents[i] - cents[i - 1]) * t) / 1200.0));
                    }
                }
                pitch_at.push_back(at[i]);
                pitch_ratio.push_back(std::exp2(cents[i] / 1200.0));
            }
            for (size_t i = 1; i < pitch_at.size(); ++i)
                if (!(pitch_at[i] > pitch_at[i - 1])) throw std::runtime_error("--pitch-curve: two points too close in time for a curve this steep");
        }
        std::vector<int64_t> map_pos;  // the job's time map, where one is set
        if (o.factor_curve || o.time_map_file || o.pitch_curve) {
            const FramesApi &api = frames_api();
            if (!api.set_time_map || !api.time_map_output_len || !api.time_map_curve)
                throw std::runtime_error("--factor-curve / --time-map / --pitch-curve: the engine library has no rc_engine_set_time_map");
            std::vector<int64_t> &pos = map_pos;
            if (o.factor_curve || o.pitch_curve) {  // "t:f,t:f,...": t in the duration grammar -> input frames, as duration_to_sample's product in doubles
                std::vector<double> at, fac;
                size_t b = 0;
                if (!o.factor_curve) {  // -f: one point
                    at.push_back(0.0);
                    fac.push_back((double)o.factor);
                }
                for (; o.factor_curve;) {
                    const size_t c = o.factor_curve->find(',', b);
                    const std::string pt = o.factor_curve->substr(b, c == std::string::npos ? c : c - b);
                    const size_t colon = pt.rfind(':');
                    uint64_t ms = 0;
                    char *end = nullptr;
                    const double f = colon == std::string::npos ? 0.0 : strtod(pt.c_str() + colon + 1, &end);
                    if (colon == std::string::npos || colon == 0 || !end || *end || end == pt.c_str() + colon + 1 ||
                        !parse_duration_ms(pt.substr(0, colon), &ms))
                        throw std::runtime_error("--factor-curve takes points t:f,t:f,... (t a duration, f a factor), not " + pt);
                    at.push_back((double)ms / 1000.0 * (double)spec.sample_rate);
                    fac.push_back(f);
                    if (c == std::string::npos) break;
                    b = c + 1;
                }
                if (o.pitch_curve) {  // the product f(q) * r(q) at the union of the two curves' break points: the duration stays
                    auto value = [](const std::vector<double> &x, const std::vector<double> &y, double q) {
                        if (q <= x.front()) return y.front();
                        if (q >= x.back()) return y.back();
                        size_t i = 0;
                        while (i + 2 < x.size() && x[i + 1] <= q) ++i;
                        return y[i] + (y[i + 1] - y[i]) * ((q - x[i]) / (x[i + 1] - x[i]));
                    };
                    for (size_t i = 1; i < at.size(); ++i)
                        if (!(at[i] > at[i - 1])) throw std::runtime_error("--factor-curve: times ascending and at least 0");
                    std::vector<double> all(at);
                    all.insert(all.end(), pitch_at.begin(), pitch_at.end());
                    std::sort(all.begin(), all.end());
                    all.erase(std::unique(all.begin(), all.end()), all.end());
                    std::vector<double> prod;
                    for (double q : all) prod.push_back(value(at, fac, q) * value(pitch_at, pitch_ratio, q));
                    at.swap(all);
                    fac.swap(prod);
                }
                size_t K = 0;
                int rc = api.time_map_curve(&cfg, raw_count, at.data(), fac.data(), at.size(), nullptr, 0, &K);
                if (rc == RC_ECAPACITY) {
                    pos.resize(K);
                    rc = api.time_map_curve(&cfg, raw_count, at.data(), fac.data(), at.size(), pos.data(), K, &K);
                }
                if (rc != RC_OK)
                    throw std::runtime_error(std::string(o.factor_curve ? "--factor-curve" : "--pitch-curve") +
                                             ": times ascending and at least 0, factors (times the pitch ratio) in [2^-10, 2^20], at most 2^28 hops");
            } else {
                FILE *mf = fopen(o.time_map_file->c_str(), "r");
                if (!mf) throw std::runtime_error("cannot open " + *o.time_map_file);
                char line[256];
                size_t line_no = 0;
                while (fgets(line, sizeof line, mf)) {
                    ++line_no;
                    if (char *hash = strchr(line, '#')) *hash = 0;
                    char *q = line, *end = nullptr;
                    while (*q == ' ' || *q == '\t' || *q == '\r' || *q == '\n') ++q;
                    if (!*q) continue;
                    errno = 0;
                    const long long v = strtoll(q, &end, 10);
                    while (*end == ' ' || *end == '\t' || *end == '\r' || *end == '\n') ++end;
                    if (end == q || *end || errno) {
                        fclose(mf);
                        throw std::runtime_error(*o.time_map_file + ":" + std::to_string(line_no) + ": not an integer position");
                    }
                    pos.push_back((int64_t)v);
                }
                fclose(mf);
                if (pos.empty()) throw std::runtime_error(*o.time_map_file + " holds no position");
            }
            if (api.set_time_map(eng.h, pos.data(), pos.size()) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            cap = api.time_map_output_len(&cfg, pos.size());
            fprintf(stderr, "time map: %zu hops, %zu frames out, input positions [%lld, %lld]\n", pos.size(), cap,
                    (long long)*std::min_element(pos.begin(), pos.end()), (long long)*std::max_element(pos.begin(), pos.end()));
            lap("time map");
        }
        const uint32_t out_sb = pcm_sample_bytes(out_fmt);
        AudioSpec out_spec = spec;  // the output file's: --output-rate
        if (o.pitch_curve) {
            // the warp: the curve's ratios along the map's hops, times rate_in / rate_out under --output-rate
            const FramesApi &api = frames_api();
            out_spec.sample_rate = o.output_rate.value_or(spec.sample_rate);
            const double rate = (double)spec.sample_rate / (double)out_spec.sample_rate;
            std::vector<double> ratio(pitch_ratio);
            for (double &r : ratio) r *= rate;
            for (double r : ratio)
                if (!(r >= 0.125 && r <= 8.0)) throw std::runtime_error("--pitch-curve: the pitch ratio times rate_in / rate_out must lie in 1/8 ... 8");
            size_t A = 0, n_out = 0;
            std::vector<int64_t> anchor;
            int rc = api.warp_curve(&cfg, map_pos.data(), map_pos.size(), pitch_at.data(), ratio.data(), ratio.size(), cap, nullptr, 0, &A, &n_out);
            if (rc == RC_ECAPACITY) {
                anchor.resize(A);
                rc = api.warp_curve(&cfg, map_pos.data(), map_pos.size(), pitch_at.data(), ratio.data(), ratio.size(), cap, anchor.data(), A, &A, &n_out);
            }
            if (rc != RC_OK || anchor.size() < 2) throw std::runtime_error("--pitch-curve: no curve for this job (an empty result, or rows beyond 2^29 frames)");
            if (api.set_warp(eng.h, anchor.data(), anchor.size(), n_out) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            static const int64_t kTierD[RC_WARP_TIERS] = {RC_WARP_D_LIST};
            int64_t d_lo = anchor[1] - anchor[0], d_hi = d_lo;
            for (size_t k = 1; k + 1 < anchor.size(); ++k) d_lo = std::min(d_lo, anchor[k + 1] - anchor[k]), d_hi = std::max(d_hi, anchor[k + 1] - anchor[k]);
            auto tier = [&](int64_t d) {
                int t = 0;
                while (d > kTierD[t]) ++t;
                return t;
            };
            fprintf(stderr, "pitch curve: %zu hops, %zu frames out, ratios [%.6f, %.6f], tiers %d ... %d\n", map_pos.size(), n_out,
                    std::ldexp((double)d_lo, -38), std::ldexp((double)d_hi, -38), tier(d_lo), tier(d_hi));
            cap = n_out;
            lap("pitch curve");
        } else if (o.pitch_ratio || o.output_rate) {
            // one step for both: r input frames per output frame for the pitch, rate_in / rate_out for the rate
            const FramesApi &api = frames_api();
            if (!api.set_resample || !api.resample_ratio || !api.resample_len || !api.resample_table)
                throw std::runtime_error("--pitch-ratio / --pitch-cents / --output-rate: the engine library has no rc_engine_set_output_resample");
            out_spec.sample_rate = o.output_rate.value_or(spec.sample_rate);
            const double asked = o.pitch_ratio.value_or(1.0) * (double)spec.sample_rate / (double)out_spec.sample_rate;
            uint32_t num = 0, den = 0, phases = 0, taps = 0;
            if (api.resample_ratio((float)asked, &num, &den) != RC_OK || api.resample_table(num, den, nullptr, 0, &phases, &taps) != RC_OK ||
                api.set_resample(eng.h, num, den) != RC_OK)
                throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            fprintf(stderr, "resample %u/%u (%+.4f cents off %.9g), %u taps\n", num, den, 1200.0 * std::log2((double)num / (double)den / asked), asked,
                    taps);
            if (num != den) cap = api.resample_len(cap, num, den);
        }
        if (o.fade_output) {
            // Layer::fade_in_out (src/mixer.rs:179-190) in frames: the fade-in over the first F frames, the fade-out over
            // the F frames in front of expected_total_samples (src/main.rs:154); Audio::fade_*_at_sample's bounds checks
            // and warnings (src/audio.rs:82-85,101-104) decide here, so that the engine call cannot fail on them
            if (!frames_api().set_fade) throw std::runtime_error("--fade-output: the engine library has no rc_engine_set_output_fade");
            // (in frames of the output file: at --output-rate, and of factor * L whatever the pitch ratio)
            const size_t fade = (size_t)((float)((double)o.fade_ms / 1000.0) * (float)out_spec.sample_rate);
            size_t expected = (size_t)((float)raw_count * o.factor);
            if (out_spec.sample_rate != spec.sample_rate) expected = (size_t)((double)expected * (double)out_spec.sample_rate / (double)spec.sample_rate);
            // under a time map the job ends where the map ends, whatever -f says: the fade-out runs into the output's last frame
            if (o.factor_curve || o.time_map_file || o.pitch_curve) expected = cap;
            const bool in_fits = fade <= cap, out_fits = expected <= cap && expected >= fade;
            if (!in_fits) fprintf(stderr, "Fade in parameters out of bounds, ignoring.\n");
            if (!out_fits) fprintf(stderr, "Fade out parameters out of bounds, ignoring.\n");
            if (frames_api().set_fade(eng.h, in_fits ? fade : 0, out_fits ? expected - fade : RC_FADE_NONE, out_fits ? fade : 0) != RC_OK)
                throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            if (in_fits && out_fits) fprintf(stderr, "fade in %zu frames, out from %zu over %zu\n", fade, expected - fade, fade);
            else if (in_fits) fprintf(stderr, "fade in %zu frames\n", fade);
            else if (out_fits) fprintf(stderr, "fade out from %zu over %zu\n", expected - fade, fade);
        }
        if (o.limit) {
            const FramesApi &api = frames_api();
            if (!api.set_limiter || !api.limiter_stats) throw std::runtime_error("--limit: the engine library has no rc_engine_set_output_limiter");
            // (in frames of the output file, as the fade: duration_to_sample at --output-rate)
            const size_t look = (size_t)((float)((double)o.limit_lookahead_ms / 1000.0) * (float)out_spec.sample_rate);
            if (look > RC_LIMITER_MAX_LOOKAHEAD)
                throw std::runtime_error("--limit-lookahead is " + std::to_string(look) + " frames at " + std::to_string(out_spec.sample_rate) +
                                         " Hz, at most " + std::to_string(RC_LIMITER_MAX_LOOKAHEAD));
            if (api.set_limiter(eng.h, o.limit_drive, *o.limit, (uint32_t)look) != RC_OK)
                throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
        }
        if (o.dither != RC_DITHER_NONE) {
            if (!frames_api().set_dither) throw std::runtime_error("--dither: the engine library has no rc_engine_set_output_dither");
            if (frames_api().set_dither(eng.h, o.dither, o.dither_seed.value_or(o.seed)) != RC_OK)
                throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
        }
        PinnedBytes out(cap * spec.channels * out_sb);
        size_t n = 0;
        uint64_t clipped = 0;
        const size_t frame_bytes = (size_t)spec.channels * raw.sample_bytes;
        if (o.normalize) {  // measured, scaled, quantised, packed and counted on the device
            if (!frames_api().stretch_norm) throw std::runtime_error("--normalize: the engine library has no rc_engine_stretch_frames_norm");
            float peak = 0.0f, gain = 1.0f;
            if (frames_api().stretch_norm(eng.h, raw.data.p + raw_first * frame_bytes, raw_count, raw.format, out.p, cap, out_fmt, *o.normalize,
                                          &n, &peak, &gain, &clipped) != RC_OK)
                throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            fprintf(stderr, "peak %.9g, gain %.9g\n", (double)peak, (double)gain);  // (nine digits: the f32 values exactly)
        } else if (o.loudness || o.true_peak) {  // loudness and true peak measured on the device, one gain in front of the quantiser
            if (!frames_api().stretch_loud) throw std::runtime_error("--loudness / --true-peak: the engine library has no rc_engine_stretch_frames_loud");
            float lufs = 0.0f, tp = 0.0f, gain = 1.0f;
            if (frames_api().stretch_loud(eng.h, raw.data.p + raw_first * frame_bytes, raw_count, raw.format, out.p, cap, out_fmt,
                                          out_spec.sample_rate, *o.loudness, o.true_peak.value_or(0.0f), &n, &lufs, &tp, &gain, &clipped) != RC_OK)
                throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            fprintf(stderr, "loudness %.9g LUFS, true peak %.9g (%.2f dBTP), gain %.9g (%.2f dB)\n", (double)lufs, (double)tp,
                    tp > 0.0f ? 20.0 * std::log10((double)tp) : -INFINITY, (double)gain, 20.0 * std::log10((double)gain));
        } else if (out_fmt_given) {  // quantised, packed and counted on the device
            if (!frames_api().stretch_pcm) throw std::runtime_error("--output-format: the engine library has no rc_engine_stretch_frames_pcm");
            if (frames_api().stretch_pcm(eng.h, raw.data.p + raw_first * frame_bytes, raw_count, raw.format, out.p, cap, out_fmt, &n, &clipped) != RC_OK)
                throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
        } else if (frames_api().stretch(eng.h, raw.data.p + raw_first * frame_bytes, raw_count, raw.format, (float *)out.p, cap, &n) != RC_OK)
            throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
        lap("stretch");
        if (o.limit) {
            float min_gain = 1.0f;
            uint64_t limited = 0;
            if (frames_api().limiter_stats(eng.h, &min_gain, &limited) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
            fprintf(stderr, "limited %llu of %zu frames, lowest gain %.9g (%.1f dB)\n", (unsigned long long)limited, n, (double)min_gain,
                    min_gain > 0.0f ? 20.0 * std::log10((double)min_gain) : -INFINITY);
        }
        write_output(out.p, n, out_spec, clipped);
        return 0;
    }
    const HostDither host_dither(o.dither, o.dither_seed.value_or(o.seed), spec.channels);  // the writers' quantiser below
    if (!o.devices.empty()) {
        // several GPUs: the whole job at once through the multi-device entry (windows of a channel are independent
        // given the phase source, so the devices share nothing but the input; include/rocoder_hip.h, rc_multi_*).
        // Same samples as the Stretcher / StretcherProcessor loop below produces (tests/test_gpu_cli.py).
        rc_multi *m = nullptr;
        if (rc_multi_create(&cfg, o.devices.data(), (uint32_t)o.devices.size(), &m) != RC_OK)
            throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
        if (o.device_kernel_src) {  // (one call computes the whole job: the kernel compiled by now is the one it runs)
            if (auto code = dk.take())
                if (dk_api().multi_load(m, code->data(), code->size()) != RC_OK ||
                    dk_api().multi_set_params(m, o.dk_params.data(), (uint32_t)o.dk_params.size()) != RC_OK) {
                    const std::string err = rc_last_error();
                    rc_multi_destroy(m);
                    throw std::runtime_error("rocoder_hip: " + err);
                }
        }
        lap("engine create");
        const size_t in_len = audio.data[0].size(), cap = rc_offline_output_len(&cfg, in_len);
        Audio out;
        out.spec = spec;
        out.data.assign(spec.channels, std::vector<float>(cap));
        std::vector<const float *> ins;
        std::vector<float *> outs;
        for (uint32_t c = 0; c < spec.channels; ++c) {
            ins.push_back(audio.data[c].data());
            outs.push_back(out.data[c].data());
        }
        size_t n = 0;
        const int rc = rc_multi_stretch_host(m, ins.data(), in_len, outs.data(), cap, &n);
        rc_multi_destroy(m);
        if (rc != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
        for (auto &c : out.data) c.resize(n);
        lap("stretch");
        uint64_t clipped = 0;
        write_wav(*o.output, out, out_fmt, out_fmt_given ? &clipped : nullptr, &host_dither);
        lap("write output");
        report_clipped(clipped, (uint64_t)n * spec.channels);
        return 0;
    }
    auto eng = std::make_shared<Engine>();
    if (rc_engine_create(&cfg, &eng->h) != RC_OK) throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
    if (o.device_kernel_src) {
        if (dk_api().set_params(eng->h, o.dk_params.data(), (uint32_t)o.dk_params.size()) != RC_OK)
            throw std::runtime_error(std::string("rocoder_hip: ") + rc_last_error());
        eng->dk = &dk;
        eng->poll_device_kernel();  // the first attempt's kernel, before the first window
    }
    lap("engine create");

    // one Stretcher per channel, fed the whole channel as one chunk (src/main.rs:133-153)
    eng->feed.resize(spec.channels);
    std::vector<Stretcher> stretchers;
    for (uint32_t c = 0; c < spec.channels; ++c) {
        Stretcher s;
        s.spec = spec;
        s.eng = eng;
        s.channel = c;
        rc_engine_get_params(eng->h, &s.par);
        eng->feed[c].input.push_back(std::move(audio.data[c]));
        eng->feed[c].input_closed = true;  // nothing else will be sent
        stretchers.push_back(std::move(s));
    }
    const size_t expected_total_samples = (size_t)((float)total_samples_len * o.factor);  // main.rs:154
    StretcherProcessor proc;
    auto bus = proc.make(std::move(stretchers), 64);
    proc.start();
    // handle_result (src/main.rs:190-211). ROCODER_CLI_COLLECT=1 keeps the reference's order (collect the whole bus in
    // memory, then write): the A/B partner of the streamed file in tests/test_gpu_cli.py
    if (getenv("ROCODER_CLI_COLLECT")) {
        Audio out = into_audio(spec, bus, expected_total_samples + o.window_len);
        proc.join();
        if (!proc.error.empty()) throw std::runtime_error(proc.error);
        lap("stretch");
        uint64_t clipped = 0;
        write_wav(*o.output, out, out_fmt, out_fmt_given ? &clipped : nullptr, &host_dither);
        lap("write output");
        report_clipped(clipped, (out.data.empty() ? 0 : (uint64_t)out.data[0].size()) * spec.channels);
        return 0;
    }
    WavStreamWriter wav(*o.output, spec, out_fmt, out_fmt_given);
    wav.dither = host_dither;
    drain_to_wav(wav, bus);
    for (auto &q : bus) q->abandon();  // (only matters after a `stuck` exit: the processor must not block on a full queue)
    proc.join();
    if (!proc.error.empty()) throw std::runtime_error(proc.error);
    wav.finish();
    lap("stretch+write");
    report_clipped(wav.clipped, wav.frames * spec.channels);
    return 0;
}

}  // namespace

// ROCODER_CLI_TIMING: the resident-set high-water mark of THIS program image (VmHWM of /proc/self/status: getrusage's
// ru_maxrss also carries the launching process's pages from between fork and exec)
static void report_peak_rss() {
    if (!getenv("ROCODER_CLI_TIMING")) return;
    FILE *f = fopen("/proc/self/status", "r");
    if (!f) return;
    char line[256];
    while (fgets(line, sizeof line, f))
        if (strncmp(line, "VmHWM:", 6) == 0) fprintf(stderr, "[timing] peak_rss_kib %ld\n", strtol(line + 6, nullptr, 10));
    fclose(f);
}

int main(int argc, char **argv) {
    try {
        const int rc = run(argc, argv);
        report_peak_rss();
        return rc;
    } catch (const UsageError &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 2;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
