// Test-hook entries for the launchers of rc_phase.h: compiled into librocoder_hip_hooks.so only (`make hooks`), as
// rc_frames_hooks.hip is. The fields of the parameter blocks as plain scalars and device pointers, the launches on the
// null stream, a synchronise, the hipError_t as an int. No logic, no clamping, no defaults and no allocation.
// rc_test_phase_scan is the pair the engine always runs together: phase_scan with `block` hops per block, then phase_walk.
#include "rc_phase.h"

extern "C" int rc_test_phase_prep(const float *spec, uint32_t *pe, uint32_t n, uint32_t step, uint32_t locked, uint32_t n_channels,
                                  uint32_t halo, int64_t hop_count) {
    const rc::PhasePrepParams p{(const float2 *)spec, pe, n, step, locked, n_channels, halo, hop_count};
    const hipError_t err = rc::launch_phase_prep(p, nullptr);
    return (int)(err != hipSuccess ? err : hipStreamSynchronize(nullptr));
}

extern "C" int rc_test_phase_scan(uint32_t *pe, uint32_t *base, uint32_t *theta, uint32_t n, uint32_t n_channels, uint32_t block,
                                  int64_t hop_count) {
    hipError_t err = rc::launch_phase_scan(rc::PhaseScanParams{pe, n, n_channels, block, hop_count}, nullptr);
    if (err == hipSuccess) err = rc::launch_phase_walk(rc::PhaseWalkParams{pe, base, theta, n, n_channels, block, hop_count}, nullptr);
    return (int)(err != hipSuccess ? err : hipStreamSynchronize(nullptr));
}

extern "C" int rc_test_phase_apply(const float *spec, float *out, const uint32_t *pe, const uint32_t *base, uint32_t n,
                                   uint32_t n_channels, uint32_t halo, uint32_t block, int64_t hop_count) {
    const rc::PhaseApplyParams p{(const float2 *)spec, (float2 *)out, pe, base, n, n_channels, halo, block, hop_count};
    const hipError_t err = rc::launch_phase_apply(p, nullptr);
    return (int)(err != hipSuccess ? err : hipStreamSynchronize(nullptr));
}

extern "C" uint32_t rc_test_phase_scan_block(int64_t hops) { return rc::phase_scan_block(hops); }
