// rc_time_map_output_len and rc_time_map_curve (include/rocoder_hip.h): pure host code, no device. The curve is a bit-exact
// definition - every step ONE IEEE double operation - so this file is built without contraction (Makefile) and keeps each
// operation in a statement of its own.
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rocoder_hip.h"

namespace {

constexpr uint64_t kMaxHops = (uint64_t)1 << 28;  // a curve that needs more hops than this is refused, not walked
constexpr double kMaxPos = 281474976710656.0;     // 2^48

struct Curve {
    const double *at, *factor;
    size_t n;
    double abs_p;
    bool slower;  // pitch_multiple < 0
    double N;
    size_t seg = 0;  // q never decreases: the segment search resumes where it stopped

    double f(double q) {
        if (q <= at[0]) return factor[0];
        if (q >= at[n - 1]) return factor[n - 1];
        while (seg + 2 < n && at[seg + 1] <= q) ++seg;
        const double a0 = at[seg], a1 = at[seg + 1], f0 = factor[seg], f1 = factor[seg + 1];
        const double df = f1 - f0;
        const double dq = q - a0;
        const double da = a1 - a0;
        const double t = dq / da;
        const double m = df * t;
        return f0 + m;
    }
    double next(double q) {
        const double fq = f(q);
        const double psf = slower ? fq / abs_p : fq * abs_p;
        const double den = 2.0 * psf;
        const double step = N / den;
        return q + step;
    }
};

}  // namespace

extern "C" {

size_t rc_time_map_output_len(const rc_config *cfg, size_t n_hops) {
    rc_params par;
    if (rc_derive_params(cfg, &par) != RC_OK) return 0;
    if (n_hops % par.hops_per_window) return 0;
    return n_hops / par.hops_per_window * (size_t)par.window_out_len;
}

int rc_time_map_curve(const rc_config *cfg, size_t in_len, const double *at, const double *factor, size_t n_points, int64_t *hop_pos,
                      size_t cap, size_t *n_hops) {
    rc_params par;
    if (int rc = rc_derive_params(cfg, &par)) return rc;
    if (!at || !factor || !n_hops || n_points == 0 || (!hop_pos && cap)) return RC_EINVAL;
    for (size_t i = 0; i < n_points; ++i) {
        if (!std::isfinite(at[i]) || at[i] < 0.0 || (i && !(at[i] > at[i - 1]))) return RC_EINVAL;
        if (!std::isfinite(factor[i]) || factor[i] < 0x1p-10 || factor[i] > 0x1p20) return RC_EINVAL;
    }
    if ((double)in_len > kMaxPos) return RC_EINVAL;
    const double abs_p = (double)std::abs(cfg->pitch_multiple);
    const double N = (double)par.window_len;
    const double len = (double)in_len;  // exact: in_len <= 2^48
    const uint64_t hpw = par.hops_per_window;
    // two walks of the same recurrence: the first finds kd and K, the second writes (nothing is written below K entries)
    uint64_t K = 0;
    for (int pass = 0; pass < 2; ++pass) {
        Curve c{at, factor, n_points, abs_p, cfg->pitch_multiple < 0, N};
        double q = 0.0;
        for (uint64_t k = 0; pass == 0 || k < K; ++k) {
            const double pos = std::floor(q);
            if (pos > kMaxPos) return RC_EINVAL;
            if (pass == 1) hop_pos[k] = (int64_t)pos;
            else if (pos + N > len) {  // kd: the window in which the input runs out is finished
                K = hpw * (k / hpw + 1);
                break;
            } else if (k + 1 >= kMaxHops) return RC_EINVAL;
            q = c.next(q);
        }
        if (pass == 0) {
            *n_hops = (size_t)K;
            if (cap < K) return RC_ECAPACITY;
        }
    }
    return RC_OK;
}

}  // extern "C"
