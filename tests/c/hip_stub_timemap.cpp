// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launcher of rocoder_amd/csrc/rc_timemap.hip for the host-only engine builds (tests/c/hip_stub.cpp has the rest). The
// stub's device memory is host memory, so a table pointer, a row pointer, a stride or a hop range that the engine's chunk
// loop gets wrong is an AddressSanitizer finding.
//   - It really gathers, on the CPU, by the definition of rc_timemap.h: every sample of every hop of every channel is
//     read where it lies inside the input and written, zeros elsewhere. The stub's streams run at enqueue time, so the
//     launch reads what the uploads have brought by then: rc_stub_tm_log holds the sum of what it gathered, and a driver
//     that knows its input knows that sum.
//   - It refuses what the real launcher refuses, with the same code.
//   - It logs every launch (rc_stub_tm_log, rc_stub_tm_launches; the driver zeroes the count).
#include <hip/hip_runtime_api.h>

#include "../../rocoder_amd/csrc/rc_timemap.h"

struct RcStubTmLaunch {
    uint64_t hop_first, hop_count, in_len, in_stride, v_stride;
    uint32_t channels, N;
    uintptr_t x, v, table;
    double sum;  // of every gathered sample, in the order channel, hop, sample
};
RcStubTmLaunch rc_stub_tm_log[256];
uint32_t rc_stub_tm_launches = 0;

namespace rc {
hipError_t launch_time_map_gather(const TimeMapGatherParams &p, hipStream_t) {
    if (p.N < 4 || (p.N & 1u) || p.N > TM_MAX_N) return hipErrorInvalidValue;
    if (p.channels > 65535u || p.in_len >= ((uint64_t)1 << 62)) return hipErrorInvalidValue;
    if (p.hop_count == 0 || p.channels == 0) return hipSuccess;
    if (!p.v || !p.hop_pos || (!p.x && p.in_len)) return hipErrorInvalidValue;
    if (p.hop_count >= ((uint64_t)1 << 31) / p.N) return hipErrorInvalidValue;
    const uint64_t row = p.hop_count * p.N;
    if (p.channels > 1 && (p.in_stride < p.in_len || p.v_stride < row)) return hipErrorInvalidValue;
    double sum = 0.0;
    for (uint32_t c = 0; c < p.channels; ++c)
        for (uint64_t h = 0; h < p.hop_count; ++h) {
            const int64_t pos = p.hop_pos[p.hop_first + h];
            for (uint32_t n = 0; n < p.N; ++n) {
                const int64_t j = pos + (int64_t)n;
                const float val = j >= 0 && j < (int64_t)p.in_len ? p.x[(uint64_t)c * p.in_stride + (uint64_t)j] : 0.0f;
                p.v[(uint64_t)c * p.v_stride + h * p.N + n] = val;
                sum += (double)val;
            }
        }
    if (rc_stub_tm_launches < 256)
        rc_stub_tm_log[rc_stub_tm_launches] = RcStubTmLaunch{p.hop_first, p.hop_count, p.in_len, p.in_stride, p.v_stride, p.channels, p.N,
                                                             (uintptr_t)p.x, (uintptr_t)p.v, (uintptr_t)p.hop_pos, sum};
    ++rc_stub_tm_launches;
    return hipSuccess;
}
}  // namespace rc
