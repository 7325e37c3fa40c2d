// rc_phase_envelope (include/rocoder_hip_phase.h): pure host code, no device. The coherent overlap-add envelope is a
// bit-exact f32 definition - every step one operation - so this file is built with -ffp-contract=off.
#include "../../include/rocoder_hip.h"

#include <cmath>

extern "C" int rc_phase_envelope(const float *window, size_t n, float *env) {
    if (!window || !env || n < 2 || n % 2) return RC_EINVAL;
    const size_t H = n / 2;
    float top = 0.0f;
    for (size_t i = 0; i < H; ++i) {
        const float a = window[i] * window[i], b = window[i + H] * window[i + H];
        const float s = a + b;
        if (!std::isfinite(s)) return RC_EINVAL;
        env[i] = s;
        if (s > top) top = s;
    }
    const float floor_ = top * (1.0f / 1024.0f);
    if (!(top > 0.0f)) return RC_EINVAL;
    for (size_t i = 0; i < H; ++i) {
        if (env[i] < floor_) return RC_EINVAL;
        env[i] = 1.0f / env[i];
    }
    return RC_OK;
}
