// rc_warp_curve (include/rocoder_hip_warp.h): pure host code, no device. The curve is a bit-exact definition - every step
// ONE IEEE double operation - so this file is built without contraction (Makefile) and keeps each operation in a statement
// of its own, as rc_timemap_curve.cpp does.
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rocoder_hip.h"

namespace {

constexpr uint64_t kMaxRows = (uint64_t)1 << 29;  // rows longer than this would pass the anchors' 2^62

// r(q): linear between the points, flat outside. q follows the hops of a map and may jump: a search from the start.
double ratio_at(const double *at, const double *ratio, size_t n, double q) {
    if (q <= at[0]) return ratio[0];
    if (q >= at[n - 1]) return ratio[n - 1];
    size_t seg = 0;
    while (seg + 2 < n && at[seg + 1] <= q) ++seg;
    const double a0 = at[seg], a1 = at[seg + 1], r0 = ratio[seg], r1 = ratio[seg + 1];
    const double dr = r1 - r0;
    const double dq = q - a0;
    const double da = a1 - a0;
    const double t = dq / da;
    const double m = dr * t;
    return r0 + m;
}

}  // namespace

extern "C" int rc_warp_curve(const rc_config *cfg, const int64_t *hop_pos, size_t n_hops, const double *at, const double *ratio,
                             size_t n_points, size_t n, int64_t *anchor, size_t cap, size_t *n_anchors, size_t *n_out) {
    rc_params par;
    if (int rc = rc_derive_params(cfg, &par)) return rc;
    if (!at || !ratio || !n_anchors || !n_out || n_points == 0 || n_hops == 0 || (!anchor && cap)) return RC_EINVAL;
    for (size_t i = 0; i < n_points; ++i) {
        if (!std::isfinite(at[i]) || at[i] < 0.0 || (i && !(at[i] > at[i - 1]))) return RC_EINVAL;
        if (!(ratio[i] >= 0.125 && ratio[i] <= 8.0)) return RC_EINVAL;
    }
    if (n > kMaxRows) return RC_EINVAL;
    const uint64_t hpw = par.hops_per_window, wout = par.window_out_len, step = par.sample_step_len;
    // two walks of the same recurrence: the first counts, the second writes (nothing is written below *n_anchors entries)
    for (int pass = 0; pass < 2; ++pass) {
        int64_t A = 0;
        size_t b = 0;
        for (;; ++b) {
            if (pass == 1) anchor[b] = A;
            const uint64_t t = (uint64_t)(A >> 32);
            if (t >= n) break;
            uint64_t k = t * hpw / wout;
            if (k > n_hops - 1) k = n_hops - 1;
            const double pos = hop_pos ? (double)hop_pos[k] : (double)(k * step);
            const double r = ratio_at(at, ratio, n_points, pos);
            const double scaled = r * 0x1p38;
            const double half = scaled + 0.5;
            int64_t D = (int64_t)std::floor(half);
            if (D < RC_WARP_D_MIN) D = RC_WARP_D_MIN;
            if (D > RC_WARP_D_MAX) D = RC_WARP_D_MAX;
            if (pass == 0 && (uint64_t)((A + D) >> 32) >= n) {  // the last block: its frames that still read inside the rows
                size_t i = 0;
                while (i < RC_WARP_BLOCK && (uint64_t)((A + ((D * (int64_t)i) >> 6)) >> 32) < n) ++i;
                *n_out = b * RC_WARP_BLOCK + i;
            }
            A += D;
        }
        if (pass == 0) {
            if (n == 0) *n_out = 0;
            *n_anchors = b + 1;
            if (cap < b + 1) return RC_ECAPACITY;
        }
    }
    return RC_OK;
}
