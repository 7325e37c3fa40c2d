// User device kernels (rc_rtc.h): hiprtc loaded with dlopen on first use, the code-object check, hipModule* calls.
#include "rc_rtc.h"

#include "../../include/rocoder_hip.h"

#include <hip/hiprtc.h>

#include <dlfcn.h>

#include <cstring>
#include <mutex>
#include <vector>

namespace rc {
namespace {

const char kPrelude[] =
#include "rc_user_dk_prelude.hpp"
    ;
const char kWrapper[] =
#include "rc_user_dk_wrapper.hpp"
    ;

// hiprtc's entry points, resolved from the library next to the loaded HIP runtime (the engine's link line does not
// name hiprtc: loading the engine costs nothing more, and a host that never compiles never maps it)
struct Hiprtc {
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) log = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) code = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    std::string why;
};

const Hiprtc *hiprtc() {
    static Hiprtc h;
    static std::once_flag once;
    std::call_once(once, [] {
        std::vector<std::string> names;
        Dl_info info{};
        if (dladdr((void *)&hipGetDeviceCount, &info) && info.dli_fname) {
            std::string dir = info.dli_fname;
            const size_t slash = dir.rfind('/');
            dir = slash == std::string::npos ? std::string() : dir.substr(0, slash + 1);
            if (!dir.empty()) {
                names.push_back(dir + "libhiprtc.so");
                names.push_back(dir + "libhiprtc.so." + std::to_string(HIP_VERSION_MAJOR));
            }
        }
        names.push_back("libhiprtc.so");
        names.push_back("libhiprtc.so." + std::to_string(HIP_VERSION_MAJOR));
        void *so = nullptr;
        for (const std::string &n : names)
            if ((so = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL))) break;
        if (!so) {
            const char *e = dlerror();
            h.why = std::string("hiprtc could not be loaded: ") + (e ? e : "not found");
            return;
        }
        h.create = (decltype(h.create))dlsym(so, "hiprtcCreateProgram");
        h.compile = (decltype(h.compile))dlsym(so, "hiprtcCompileProgram");
        h.log_size = (decltype(h.log_size))dlsym(so, "hiprtcGetProgramLogSize");
        h.log = (decltype(h.log))dlsym(so, "hiprtcGetProgramLog");
        h.code_size = (decltype(h.code_size))dlsym(so, "hiprtcGetCodeSize");
        h.code = (decltype(h.code))dlsym(so, "hiprtcGetCode");
        h.destroy = (decltype(h.destroy))dlsym(so, "hiprtcDestroyProgram");
        if (!h.create || !h.compile || !h.log_size || !h.log || !h.code_size || !h.code || !h.destroy) {
            h.create = nullptr;
            h.why = "hiprtc lacks an entry point";
        }
    });
    return &h;
}

// the log's first line that reports an error (else its first line)
std::string first_error_line(const std::string &log) {
    size_t at = log.find("error:");
    size_t b = at == std::string::npos ? 0 : log.rfind('\n', at);
    b = (at == std::string::npos || b == std::string::npos) ? 0 : b + 1;
    const size_t e = log.find('\n', b);
    return log.substr(b, e == std::string::npos ? std::string::npos : e - b);
}

// little-endian reads inside [0, len)
bool rd(const unsigned char *p, size_t len, uint64_t off, size_t n, uint64_t *v) {
    if (off > len || n > len - off) return false;
    uint64_t x = 0;
    for (size_t i = 0; i < n; ++i) x |= (uint64_t)p[off + i] << (8 * i);
    *v = x;
    return true;
}

}  // namespace

int rtc_compile(const char *src, size_t src_len, std::string *code, std::string *log, std::string *why) {
    code->clear();
    log->clear();
    const std::string user(src, src_len);
    if (user.find("rc_apply") == std::string::npos) {
        *why = "the source defines no rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h)";
        *log = *why + "\n";
        return RC_EINVAL;
    }
    const Hiprtc *h = hiprtc();
    if (!h->create) {
        *why = h->why;
        return RC_EUNSUPPORTED;
    }
    // one compile at a time (hiprtc's state per process is not documented as re-entrant); the last result is kept, so
    // that a size query followed by the real call compiles once
    static std::mutex mu;
    static std::string last_src, last_code, last_log;
    static int last_rc = 1;
    std::lock_guard<std::mutex> lk(mu);
    if (last_rc != 1 && last_src == user) {
        *code = last_code;
        *log = last_log;
        if (last_rc != RC_OK) *why = first_error_line(last_log);
        return last_rc;
    }
    // the user's lines keep their numbers: diagnostics name rc_user_dk.hip:<line>, or the file a leading #line names
    const std::string text = std::string(kPrelude) + "#line 1 \"rc_user_dk.hip\"\n" + user + "\n" + kWrapper;
    hiprtcProgram prog = nullptr;
    if (h->create(&prog, text.c_str(), "rc_user_dk.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        *why = "hiprtcCreateProgram failed";
        return RC_EUNSUPPORTED;
    }
    // no fast-math: rc_apply's float arithmetic is IEEE, as the host kernels' is
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
    const hiprtcResult cr = h->compile(prog, 3, opts);
    size_t n = 0;
    if (h->log_size(prog, &n) == HIPRTC_SUCCESS && n > 1) {
        std::vector<char> b(n + 1, 0);
        if (h->log(prog, b.data()) == HIPRTC_SUCCESS) *log = b.data();
    }
    int rc = RC_OK;
    if (cr != HIPRTC_SUCCESS) {
        rc = RC_EINVAL;
        if (log->empty()) *log = "hiprtc: compilation failed\n";
    } else if (h->code_size(prog, &n) != HIPRTC_SUCCESS || n == 0) {
        rc = RC_EINVAL;
        *log += "hiprtc: no code object\n";
    } else {
        code->resize(n);
        if (h->code(prog, &(*code)[0]) != HIPRTC_SUCCESS) {
            code->clear();
            rc = RC_EINVAL;
            *log += "hiprtc: reading the code object failed\n";
        }
    }
    h->destroy(&prog);
    if (rc == RC_OK) rc = rtc_check_code_object(code->data(), code->size(), why);  // (e.g. rc_user_dk renamed by a macro)
    else *why = first_error_line(*log);
    last_src = user;
    last_code = *code;
    last_log = *log;
    last_rc = rc;
    return rc;
}

int rtc_check_code_object(const void *code, size_t len, std::string *why, uint32_t *history, bool *cross,
                          uint32_t *sums, uint32_t *feedback) {
    const unsigned char *p = (const unsigned char *)code;
    uint64_t v = 0;
    if (!p || len < 64 || std::memcmp(p, "\x7f" "ELF", 4) != 0 || p[4] != 2 /* ELFCLASS64 */ || p[5] != 1 /* LE */) {
        *why = "not an ELF64 little-endian object";
        return RC_EINVAL;
    }
    rd(p, len, 18, 2, &v);
    if (v != 224) {
        *why = "ELF machine " + std::to_string(v) + " is not EM_AMDGPU (224)";
        return RC_EINVAL;
    }
    rd(p, len, 48, 4, &v);
    if ((v & 0xff) != 0x4f) {
        *why = "code object is not for gfx950 (e_flags mach " + std::to_string(v & 0xff) + ", want 0x4f)";
        return RC_EINVAL;
    }
    uint64_t shoff = 0, shentsize = 0, shnum = 0;
    rd(p, len, 40, 8, &shoff);
    rd(p, len, 58, 2, &shentsize);
    rd(p, len, 60, 2, &shnum);
    if (shentsize != 64 || shoff > len || shnum > (len - shoff) / 64) {
        *why = "bad ELF section header table";
        return RC_EINVAL;
    }
    static const char kSym[] = "rc_user_dk", kHist[] = "rc_user_dk_history", kChan[] = "rc_user_dk_channels";
    static const char kSums[] = "rc_user_dk_sums", kPass[] = "rc_user_dk_sums_pass";
    static const char kFb[] = "rc_user_dk_feedback";
    bool found = false, chan = false, sums_marker = false, pass = false, fb_marker = false;
    uint64_t fb_size = 1;  // no marker: no feedback
    uint64_t hist_size = 1;  // no marker: depth 0
    uint64_t sums_size = 1;  // no marker: no sums
    for (uint64_t i = 0; i < shnum; ++i) {
        const uint64_t sh = shoff + i * 64;
        uint64_t type = 0, off = 0, size = 0, link = 0, entsize = 0;
        rd(p, len, sh + 4, 4, &type);
        if (type != 2 /* SHT_SYMTAB */ && type != 11 /* SHT_DYNSYM */) continue;
        rd(p, len, sh + 24, 8, &off);
        rd(p, len, sh + 32, 8, &size);
        rd(p, len, sh + 40, 4, &link);
        rd(p, len, sh + 56, 8, &entsize);
        if (entsize != 24 || link >= shnum || off > len || size > len - off) continue;
        uint64_t str_off = 0, str_size = 0;
        rd(p, len, shoff + link * 64 + 24, 8, &str_off);
        rd(p, len, shoff + link * 64 + 32, 8, &str_size);
        if (str_off > len || str_size > len - str_off) continue;
        for (uint64_t s = off; s + 24 <= off + size; s += 24) {
            uint64_t name = 0;
            rd(p, len, s, 4, &name);
            if (name >= str_size) continue;
            if (str_size - name >= sizeof kSym && std::memcmp(p + str_off + name, kSym, sizeof kSym) == 0) found = true;
            if (str_size - name >= sizeof kHist && std::memcmp(p + str_off + name, kHist, sizeof kHist) == 0)
                rd(p, len, s + 16, 8, &hist_size);  // st_size
            if (str_size - name >= sizeof kChan && std::memcmp(p + str_off + name, kChan, sizeof kChan) == 0) chan = true;
            if (str_size - name >= sizeof kSums && std::memcmp(p + str_off + name, kSums, sizeof kSums) == 0) {
                sums_marker = true;
                rd(p, len, s + 16, 8, &sums_size);
            }
            if (str_size - name >= sizeof kPass && std::memcmp(p + str_off + name, kPass, sizeof kPass) == 0) pass = true;
            if (str_size - name >= sizeof kFb && std::memcmp(p + str_off + name, kFb, sizeof kFb) == 0) {
                fb_marker = true;
                rd(p, len, s + 16, 8, &fb_size);
            }
        }
    }
    if (!found) {
        *why = "the code object defines no rc_user_dk kernel";
        return RC_EINVAL;
    }
    if (hist_size < 1 || hist_size > DK_MAX_HISTORY + 1) {
        *why = "the code object declares an RC_HISTORY outside 0 ... " + std::to_string(DK_MAX_HISTORY);
        return RC_EINVAL;
    }
    if (sums_marker && (sums_size < 1 || sums_size > DK_MAX_SUMS + 1)) {
        *why = "the code object declares an RC_SUMS outside 0 ... " + std::to_string(DK_MAX_SUMS);
        return RC_EINVAL;
    }
    if (sums_marker && !pass) {
        *why = "the code object declares RC_SUMS and defines no rc_user_dk_sums_pass kernel";
        return RC_EINVAL;
    }
    if (fb_marker && (fb_size < 2 || fb_size > DK_MAX_FEEDBACK + 1)) {
        *why = "the code object declares an RC_FEEDBACK outside 1 ... " + std::to_string(DK_MAX_FEEDBACK);
        return RC_EINVAL;
    }
    if (feedback) *feedback = (uint32_t)(fb_size - 1);
    if (history) *history = (uint32_t)(hist_size - 1);
    if (cross) *cross = chan;
    if (sums) *sums = (uint32_t)(sums_size - 1);
    return RC_OK;
}

struct UserModule {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    hipFunction_t fn_sums = nullptr;  // rc_user_dk_sums_pass, with sums > 0 only
    uint32_t history = 0;
    bool cross = false;
    uint32_t sums = 0;
    uint32_t feedback = 0;
};

int rtc_load(const void *code, size_t len, UserModule **out, std::string *why) {
    *out = nullptr;
    uint32_t history = 0;
    bool cross = false;
    uint32_t sums = 0, feedback = 0;
    if (int rc = rtc_check_code_object(code, len, why, &history, &cross, &sums, &feedback)) return rc;
    UserModule *m = new UserModule;
    m->feedback = feedback;
    m->history = history;
    m->cross = cross;
    m->sums = sums;
    hipError_t e = hipModuleLoadData(&m->mod, code);
    if (e == hipSuccess) {
        e = hipModuleGetFunction(&m->fn, m->mod, "rc_user_dk");
        if (e == hipSuccess && sums) e = hipModuleGetFunction(&m->fn_sums, m->mod, "rc_user_dk_sums_pass");
        if (e != hipSuccess) (void)hipModuleUnload(m->mod);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete m;
        *why = std::string("loading the code object failed: ") + hipGetErrorString(e);
        return RC_EHIP;
    }
    *out = m;
    return RC_OK;
}

void rtc_unload(UserModule *m) {
    if (!m) return;
    (void)hipModuleUnload(m->mod);
    delete m;
}

uint32_t rtc_history(const UserModule *m) { return m ? m->history : 0; }
bool rtc_cross(const UserModule *m) { return m && m->cross; }
uint32_t rtc_sums(const UserModule *m) { return m ? m->sums : 0; }
uint32_t rtc_feedback(const UserModule *m) { return m ? m->feedback : 0; }

hipError_t rtc_launch(const UserModule *m, UserDkArgs a, uint64_t rows, hipStream_t s) {
    const uint64_t per_launch = 32768;  // grid.y limit, as launch_dev_kernel
    for (uint64_t r0 = 0; r0 < rows; r0 += per_launch) {
        a.row_first = r0;
        const unsigned gy = (unsigned)(rows - r0 < per_launch ? rows - r0 : per_launch);
        void *args[] = {&a};
        const hipError_t e = hipModuleLaunchKernel(m->fn, (a.n + 255) / 256, gy, 1, 256, 1, 1, 0, s, args, nullptr);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t rtc_launch_sums(const UserModule *m, UserDkArgs a, uint64_t rows, hipStream_t s) {
    if (!m->fn_sums) return hipErrorInvalidDeviceFunction;
    const uint64_t per_launch = 32768;  // grid.y limit, as rtc_launch
    for (uint64_t r0 = 0; r0 < rows; r0 += per_launch) {
        a.row_first = r0;
        const unsigned gy = (unsigned)(rows - r0 < per_launch ? rows - r0 : per_launch);
        void *args[] = {&a};
        const hipError_t e = hipModuleLaunchKernel(m->fn_sums, 1, gy, 1, 256, 1, 1, 0, s, args, nullptr);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t rtc_launch_feedback(const UserModule *m, UserDkArgs a, uint32_t n_channels, bool per_hop, hipStream_t s,
                               uint32_t *launches) {
    *launches = 0;
    if (!m->feedback) return hipErrorInvalidDeviceFunction;
    const uint32_t hops = (uint32_t)a.hop_count;  // (a chunk holds at most 32768 hops)
    const uint32_t per_launch = 32768;            // grid.y limit, as rtc_launch
    const uint32_t gx = per_hop ? (a.n + 255) / 256 : 1;
    for (uint32_t h0 = 0; h0 < hops; h0 += per_hop ? 1 : hops) {
        a.fb_hop_first = h0;
        a.fb_hop_count = per_hop ? 1 : hops;
        for (uint32_t c0 = 0; c0 < n_channels; c0 += per_launch) {
            a.row_first = c0;
            const unsigned gy = n_channels - c0 < per_launch ? n_channels - c0 : per_launch;
            void *args[] = {&a};
            const hipError_t e = hipModuleLaunchKernel(m->fn, gx, gy, 1, 256, 1, 1, 0, s, args, nullptr);
            if (e != hipSuccess) return e;
            ++*launches;
        }
    }
    return hipSuccess;
}

}  // namespace rc
