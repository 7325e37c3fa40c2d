// Test-hook entry for launch_frames_mix (rc_frames.h): compiled into librocoder_hip_hooks.so only (`make hooks`), as
// rc_frames_hooks.hip is. The fields of the parameter block as plain scalars and pointers, a launch on the null stream, a
// synchronise, the hipError_t as an int. No logic, no clamping, no defaults and no allocation.
#include "rc_frames.h"

extern "C" int rc_test_frames_mix(const float *rows, uint64_t stride, uint32_t channels, uint64_t t0, uint64_t t1, float *bus,
                                  uint64_t bus_stride, uint32_t bus_channels, uint64_t bus_frames, int64_t offset,
                                  const uint64_t *key_frame, const float *key_amp, uint32_t n_keys, const float *send) {
    const rc::FramesMixParams p{rows, stride, channels, t0, t1, bus, bus_stride, bus_channels, bus_frames, offset, key_frame, key_amp, n_keys, send};
    const hipError_t err = rc::launch_frames_mix(p, nullptr);
    return (int)(err != hipSuccess ? err : hipStreamSynchronize(nullptr));
}
