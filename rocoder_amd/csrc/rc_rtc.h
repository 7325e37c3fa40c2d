// User device kernels compiled at run time (include/rocoder_hip.h: rc_dk_compile, rc_engine_load_device_kernel): the
// hiprtc compile of prelude + user source + wrapper (rc_user_dk_prelude.hpp, rc_user_dk_wrapper.hpp), the check of a
// code object before it reaches the HIP runtime, and the hipModule* calls. rc_engine.cpp calls only these functions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

namespace rc {

constexpr uint32_t DK_MAX_PARAMS = 16;
constexpr uint32_t DK_MAX_SUMS = 4;     // RC_DK_MAX_SUMS: whole-hop sums a user device kernel may declare (an interface constant)
constexpr uint32_t DK_MAX_FEEDBACK = 4;  // RC_DK_MAX_FEEDBACK: earlier outputs a user device kernel may read (an interface constant)
constexpr uint32_t DK_MAX_HISTORY = 8;  // RC_DK_MAX_HISTORY: earlier hops a user device kernel may read (an interface constant)

// Host mirror of the prelude's rc_dk_args (the wrapper kernel's one argument): keep the two in step
struct UserDkArgs {
    const float2 *in;
    float2 *out;
    uint64_t row_first;
    int64_t hop_first;
    uint64_t hop_count;
    uint64_t time_ms;
    uint32_t n, mask;
    uint32_t ch_first, n_params;
    float params[DK_MAX_PARAMS];
    // rc_dk_args_history: the argument block of a kernel that declares a history (a kernel without one, and every
    // code object without the rc_user_dk_history marker, takes the 128 bytes above and never sees these)
    uint64_t in_rows;
    uint32_t halo;
    uint32_t pad_;
    // rc_dk_args_channels: what a kernel that declares RC_CROSS_CHANNEL takes on top (its input block holds channels
    // [in_ch_first, in_ch_first + in_ch_count) of the job; nobody else sees these)
    uint32_t channels;
    uint32_t in_ch_first;
    uint32_t in_ch_count;
    uint32_t pad2_;
    // rc_dk_args_sums: what a kernel that declares RC_SUMS takes on top, whatever else it declares: the sums of the
    // rows of `in`, [in_ch_count][halo + hop_count][n_sums], pointing past the first channel's halo rows as `in` does
    const float *sums;
    uint32_t n_sums;
    uint32_t pad3_;
    // rc_dk_args_feedback: what a kernel that declares RC_FEEDBACK takes on top, whatever else it declares: the ring of
    // its earlier outputs, [rc_config::channels][feedback + 1][n], and the hops of the chunk that one launch walks
    float2 *state;
    uint32_t feedback;
    uint32_t fb_hop_first;
    uint32_t fb_hop_count;
    uint32_t pad4_;
};
static_assert(offsetof(UserDkArgs, in_rows) == 128 && offsetof(UserDkArgs, channels) == 144 &&
                  offsetof(UserDkArgs, sums) == 160 && offsetof(UserDkArgs, state) == 176 && sizeof(UserDkArgs) == 200,
              "rc_dk_args layout");

// Every function returns an RC_* status and, on failure, a one-line reason in *why.

// hiprtc: source -> gfx950 code object in *code. RC_OK; RC_EINVAL with the compiler log in *log when the source does
// not compile or defines no rc_apply (*why: the log's first error line); RC_EUNSUPPORTED when hiprtc cannot be loaded.
// Pure host, thread-safe.
int rtc_compile(const char *src, size_t src_len, std::string *code, std::string *log, std::string *why);

// RC_OK when `code` is an ELF64 AMDGPU code object for gfx950 that defines the symbol rc_user_dk, else RC_EINVAL.
// *history (when given): the depth the object declares, the size of its symbol rc_user_dk_history less one; 0 for an
// object without that symbol. A size outside 1 ... DK_MAX_HISTORY + 1 is RC_EINVAL. Reads nothing outside
// [code, code + len). *cross (when given): whether the object declares RC_CROSS_CHANNEL, i.e. defines the symbol
// rc_user_dk_channels. *sums (when given): the RC_SUMS the object declares, the size of its symbol rc_user_dk_sums less
// one; 0 for an object without that symbol. A size outside 1 ... DK_MAX_SUMS + 1, and a marker without the symbol
// rc_user_dk_sums_pass, is RC_EINVAL. *feedback (when given): the RC_FEEDBACK the object declares, the size of its symbol
// rc_user_dk_feedback less one; 0 for an object without that symbol. A size outside 2 ... DK_MAX_FEEDBACK + 1 is
// RC_EINVAL. The four markers do not depend on one another.
int rtc_check_code_object(const void *code, size_t len, std::string *why, uint32_t *history = nullptr,
                          bool *cross = nullptr, uint32_t *sums = nullptr, uint32_t *feedback = nullptr);

struct UserModule;
// hipModuleLoadData + hipModuleGetFunction("rc_user_dk") on the current device (RC_EHIP on failure); an object that
// declares RC_SUMS is asked for "rc_user_dk_sums_pass" as well, any other for nothing more
int rtc_load(const void *code, size_t len, UserModule **out, std::string *why);
void rtc_unload(UserModule *m);
uint32_t rtc_history(const UserModule *m);  // the depth the loaded object declares
bool rtc_cross(const UserModule *m);        // whether it declares RC_CROSS_CHANNEL
uint32_t rtc_sums(const UserModule *m);     // the RC_SUMS it declares
uint32_t rtc_feedback(const UserModule *m);  // the RC_FEEDBACK it declares
// A feedback kernel at or below this window length runs in the loop shape (rtc_launch_feedback). Measured (stereo, f = 8,
// L = 2 646 000, smooth.hip; profiles/r23_user_dk_feedback.json): the loop shape costs about 1.9 ns per bin of a channel
// whatever N (79 - 86 ms), the per-hop shape about 3.4 us per hop (137 / 36 / 9.1 / 3.3 ms at N = 1024 / 4096 / 16384 /
// 65536): they cross near N = 1800, and 1024 is the largest measured N at which the loop is the faster one.
constexpr uint32_t kFeedbackLoopMaxN = 1024;
// ROCODER_DIAG bits (rc_engine::diag_flags, test-hook library only) beside those of rc_kernels.h: a feedback kernel runs
// in the per-hop shape at every window length, so that a test can hold it against the loop shape; or in the loop shape at
// every window length (tools/bench_user_dk_feedback.py: where the two shapes cross)
constexpr uint32_t RC_DIAG_FB_PER_HOP = 16;
constexpr uint32_t RC_DIAG_FB_LOOP = 32;
// rows = hop spectra of a.n bins to write; a.row_first is set per launch (rows are chunked below the grid.y limit)
hipError_t rtc_launch(const UserModule *m, UserDkArgs a, uint64_t rows, hipStream_t s);
// rc_user_dk_sums_pass of a module that declares RC_SUMS: one workgroup per row of the INPUT block, rows =
// a.in_ch_count * a.in_rows (halo rows included), chunked in the same way
hipError_t rtc_launch_sums(const UserModule *m, UserDkArgs a, uint64_t rows, hipStream_t s);
// rc_user_dk of a module that declares RC_FEEDBACK on hops a.hop_first ... of a.hop_count hops of n_channels channels, in
// hop order. per_hop: a.hop_count launches of grid (ceil(n / 256), channels), one hop each; the stream orders them. Else
// the loop shape: one launch of grid (1, channels) whose workgroup walks every hop of its channel. *launches: how many.
hipError_t rtc_launch_feedback(const UserModule *m, UserDkArgs a, uint32_t n_channels, bool per_hop, hipStream_t s,
                               uint32_t *launches);

}  // namespace rc
