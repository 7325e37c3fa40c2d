// rc_mix_envelope (include/rocoder_hip_mix.h): pure host code, no device. The envelope is a bit-exact definition - every
// step ONE IEEE f32 operation - so this file is built without contraction (Makefile) and keeps each operation in a
// statement of its own, as rc_warp_curve.cpp does. The key validation of rc_engine_mix_frames lives here too
// (rc::mix_check_keys, declared in rc_frames.h for the engine).
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rocoder_hip.h"

namespace rc {

// nullptr where the keys are what rc_engine_mix_frames accepts, else what is wrong with them
const char *mix_check_keys(const uint64_t *key_frame, const float *key_amp, size_t n_keys) {
    if (n_keys > RC_MIX_MAX_KEYS) return "more than RC_MIX_MAX_KEYS keys";
    if (n_keys && (!key_frame || !key_amp)) return "null key arrays";
    for (size_t i = 0; i < n_keys; ++i) {
        if (!std::isfinite(key_amp[i])) return "a key amplitude is not finite";
        if (i && !(key_frame[i] > key_frame[i - 1])) return "key frames are not strictly increasing";
    }
    return nullptr;
}

}  // namespace rc

namespace {

// math::sqrt_interp(a, b, r) of the reference as written (src/math.rs:33-40)
float sqrt_interp(float a, float b, float r) {
    const bool inc = a < b;
    const float r2 = r * 2.0f;
    const float c = r2 - 1.0f;
    const float pr = c * (inc ? 1.0f : -1.0f);
    const float m = std::fmax(pr, -1.0f);
    const float s = 1.0f + m;
    const float h = 0.5f * s;
    const float fct = std::sqrt(h);
    const float d = b - a;
    const float w = std::fabs(d);
    const float p = w * fct;
    return (inc ? a : b) + p;
}

}  // namespace

extern "C" int rc_mix_envelope(const uint64_t *key_frame, const float *key_amp, size_t n_keys, uint64_t t0, size_t n, float *amp) {
    if ((!amp && n) || rc::mix_check_keys(key_frame, key_amp, n_keys)) return RC_EINVAL;
    size_t seg = 0;  // the last key at or in front of t, once t has passed the first
    for (size_t i = 0; i < n; ++i) {
        const uint64_t t = t0 + i;
        if (n_keys == 0) {
            amp[i] = 1.0f;
        } else if (n_keys == 1 || t < key_frame[0]) {
            amp[i] = key_amp[0];
        } else if (t >= key_frame[n_keys - 1]) {
            amp[i] = key_amp[n_keys - 1];
        } else {
            if (i == 0) {  // one binary search for the first frame, steps from there
                size_t lo = 0, hi = n_keys - 1;  // key_frame[lo] <= t < key_frame[hi]
                while (hi - lo > 1) {
                    const size_t mid = lo + (hi - lo) / 2;
                    (key_frame[mid] <= t ? lo : hi) = mid;
                }
                seg = lo;
            }
            while (key_frame[seg + 1] <= t) ++seg;
            const float num = (float)(t - key_frame[seg]);
            const float den = (float)(key_frame[seg + 1] - key_frame[seg]);
            const float r = num / den;
            amp[i] = sqrt_interp(key_amp[seg], key_amp[seg + 1], r);
        }
    }
    return RC_OK;
}
