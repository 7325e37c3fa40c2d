// Test-hook entry for the launcher of rc_timemap.h: compiled into librocoder_hip_hooks.so only (`make hooks`), never into
// the product library. As rc_frames_hooks.hip: the fields of the parameter block as plain scalars and device pointers, a
// launch on the null stream, a synchronise, the hipError_t as an int. No logic, no clamping, no defaults, no allocation.
#include "rc_timemap.h"

extern "C" int rc_test_time_map_gather(const float *x, uint64_t in_stride, uint64_t in_len, const int64_t *hop_pos, uint64_t hop_first,
                                       uint64_t hop_count, uint32_t channels, uint32_t N, float *v, uint64_t v_stride) {
    const hipError_t err =
        rc::launch_time_map_gather(rc::TimeMapGatherParams{x, in_stride, in_len, hop_pos, hop_first, hop_count, channels, N, v, v_stride}, nullptr);
    return (int)(err != hipSuccess ? err : hipStreamSynchronize(nullptr));
}
