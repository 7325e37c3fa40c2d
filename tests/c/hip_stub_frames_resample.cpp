// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launcher of rocoder_amd/csrc/rc_frames_resample.hip for the host-only engine builds (tests/c/hip_stub.cpp and the
// other hip_stub_frames*.cpp have the rest). The stub's device memory is host memory, so a pointer, a stride or a range
// that the engine's lag bookkeeping gets wrong is an AddressSanitizer finding.
//   - It refuses what the real launcher refuses: a range one of whose taps lies inside [0, n) but outside
//     [src0, src0 + src_len).
//   - It reads every tap of the range that lies inside [0, n), reads the table's first and last float, and writes
//     rc_stub_resample_mark over the frames [m0, m1) of every channel of dst.
//   - It logs every launch (rc_stub_resample_log, rc_stub_resample_launches; the driver zeroes the count): [m0, m1), src0,
//     src_len, n, the step, the strides and the rows that the launch's pointers imply.
#include <hip/hip_runtime_api.h>

#include "../../rocoder_amd/csrc/rc_frames.h"

struct RcStubResampleLaunch {
    uint64_t m0, m1, src0, src_len, n, stride, dst_stride;
    uint32_t num, den, W, channels;
    uintptr_t src_row0, dst_row0;  // where frame 0 of the first channel lies, by this launch's pointers
};
RcStubResampleLaunch rc_stub_resample_log[256];
uint32_t rc_stub_resample_launches = 0;
float rc_stub_resample_mark = 0.25f;
float rc_stub_resample_sum = 0.0f;  // (what the launcher read: keeps the reads alive)

namespace rc {
hipError_t launch_frames_resample(const FramesResampleParams &p, hipStream_t) {
    if (p.m1 <= p.m0) return hipSuccess;
    if (!p.src || !p.dst || !p.table || p.channels == 0 || p.channels > 65535u || p.num == 0 || p.den == 0 || p.W == 0)
        return hipErrorInvalidValue;
    const int64_t lo = (int64_t)(p.m0 * p.num / p.den) - (int64_t)(p.W - 1);
    const uint64_t hi = (p.m1 - 1) * p.num / p.den + p.W + 1;
    const uint64_t need_lo = lo < 0 ? 0 : (uint64_t)lo, need_hi = hi < p.n ? hi : p.n;
    if (need_lo < need_hi && (need_lo < p.src0 || need_hi > p.src0 + p.src_len)) return hipErrorInvalidValue;
    if (rc_stub_resample_launches < 256)
        rc_stub_resample_log[rc_stub_resample_launches] = RcStubResampleLaunch{
            p.m0, p.m1, p.src0, p.src_len, p.n, p.stride, p.dst_stride, p.num, p.den, p.W, p.channels,
            (uintptr_t)p.src - (uintptr_t)(p.src0 * sizeof(float)), (uintptr_t)p.dst - (uintptr_t)(p.m0 * sizeof(float))};
    ++rc_stub_resample_launches;
    rc_stub_resample_sum += p.table[0] + p.table[(uint64_t)p.den * 2 * p.W - 1];
    for (uint32_t c = 0; c < p.channels; ++c) {
        for (uint64_t k = need_lo; k < need_hi; ++k) rc_stub_resample_sum += p.src[(uint64_t)c * p.stride + (k - p.src0)];
        for (uint64_t i = 0; i < p.m1 - p.m0; ++i) p.dst[(uint64_t)c * p.dst_stride + i] = rc_stub_resample_mark;
    }
    return hipSuccess;
}
}  // namespace rc
