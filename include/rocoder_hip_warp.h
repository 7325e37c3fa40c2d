/*
 * rocoder_hip_warp.h - the output-warp entries of the C-ABI in rocoder_hip.h, which includes this file: include that one.
 * They add functions only - no struct, no layout change, RC_ABI_VERSION stays what it is.
 */
#ifndef ROCODER_HIP_WARP_H
#define ROCODER_HIP_WARP_H

#ifndef ROCODER_HIP_H
#error "include rocoder_hip.h"
#endif

/* ---- output warp: band-limited resampling whose step varies along the output (pitch curves) ---- */
/* rc_engine_set_output_resample moves the pitch by one rational step for the whole job. A warp gives every block of 64
 * output frames a step of its own: a glide, a tape stop, a vibrato, inside the same stage chain (fade, limiter, dither,
 * quantiser). The warp is engine state, set once, like the time map and the resampler; the two resamplers are alternatives.
 * It holds anchor[0 .. A), int64_t positions in the rows x of the stretch result with 32 fractional bits, and n_out, the
 * number of output frames. The definition, bit for bit:
 *   B = 64 output frames are a block. Output frame m = 64 b + i (0 <= i < 64) reads the position
 *     P(m) = anchor[b] + (((anchor[b + 1] - anchor[b]) * i) >> 6)                              in 64-bit integers,
 *     q = P >> 32,  p = (P >> 24) & 255,  a = (float)(P & 0xFFFFFF) * 2^-24                    (a is exact in f32).
 *   D_b = anchor[b + 1] - anchor[b] lies in [2^35, 2^41]: a step of 1/8 ... 8 input frames per output frame.
 *   The cut-off follows the step in RC_WARP_TIERS = 13 tiers: t_b is the smallest t with D_b <= RC_WARP_D(t),
 *     RC_WARP_D(t) = floor(2^(t/4) * 2^38). Tier t: s = 2^(-t/4), c = 0.9 s, W = ceil(32 / s), T = 2 W taps.
 *   Table of tier t: rows p = 0 ... 256 (257 rows), h_t[p][j] = the Kaiser-windowed sinc of rc_engine_set_output_resample
 *     (Z = 32, beta = 9, cut-off c, half-width W) at u = j - (W - 1) - p / 256, computed in f64 by the routine of
 *     rc_resample_table and rounded once to f32                                                 (rc_warp_table).
 *   k0 = q - (W - 1), x zero outside [0, n).  y0 = ONE chain acc = fmaf(h_t[p][j], x[k0 + j], acc) from +0, j ascending.
 *   Where a == 0, y[m] = y0. Otherwise y1 is the same chain over row p + 1 and y[m] = fmaf(a, y1 - y0, y0).
 *   The order depends on (t, p, a, j) alone: a sample's bits do not depend on tile, launch, chunk or range.
 * At a constant step num / den with den dividing 256 and num <= den, or at a step of 2, 4 or 8, this is the rational
 * resampler's output bit for bit: the same tier constants, the same table rows, a = 0.
 * NULL or n_anchors == 0 clears the warp (the state after rc_engine_create); the table is copied.
 * RC_EINVAL, and the previous state stays: a null engine, n_anchors < 2, an anchor outside [0, 2^62), a D_b outside
 * [2^35, 2^41], n_out > 64 (n_anchors - 1), or a rational step set (rc_engine_set_output_resample: clear it first).
 * rc_engine_set_output_resample likewise returns RC_EINVAL while a warp is set.
 * Reach: the resampler's - rc_engine_stretch_host, _frames, _frames_pcm, _frames_norm and _frames_loud, under a host
 * frequency kernel and under a time map as well. A job produces exactly n_out frames whatever the length n of its rows
 * (positions behind n read zeros); the fade, the limiter, the dither offsets, every capacity check (RC_ECAPACITY below
 * n_out) and *out_len count warped frames. Only the tiers a warp uses go to the device. Not reached: the streaming seam,
 * the device forms and rc_multi_*. */
#define RC_WARP_TIERS 13
#define RC_WARP_BLOCK 64
#define RC_WARP_PHASES 256
/* D[t] = floor(2^(t/4) * 2^38) */
#define RC_WARP_D_LIST                                                                                                   \
    274877906944LL, 326886762694LL, 388736063996LL, 462287693163LL, 549755813888LL, 653773525389LL, 777472127993LL,       \
        924575386326LL, 1099511627776LL, 1307547050779LL, 1554944255987LL, 1849150772653LL, 2199023255552LL
/* W[t] = ceil(32 * 2^(t/4)) */
#define RC_WARP_W_LIST 32, 39, 46, 54, 64, 77, 91, 108, 128, 153, 182, 216, 256
#define RC_WARP_D_MIN 34359738368LL   /* 2^35 */
#define RC_WARP_D_MAX 2199023255552LL /* 2^41 */

int rc_engine_set_output_warp(rc_engine *e, const int64_t *anchor, size_t n_anchors, size_t n_out);
/* Pure host: the table of tier `tier` (0 ... 12), *rows = 257 rows of *taps = T floats each, row p at table[p * T].
 * RC_EINVAL: a tier above 12 or a null size pointer; RC_ECAPACITY where cap < 257 * T floats, the sizes still stored;
 * table == NULL returns the sizes only. */
int rc_warp_table(uint32_t tier, float *table, size_t cap, uint32_t *rows, uint32_t *taps);
/* Pure host: the anchors of a pitch ratio that varies along the INPUT of a job whose rows have n frames. The points are
 * (at[i], ratio[i]), `at` in input samples, at least 0 and strictly increasing, every ratio in [1/8, 8]; r(q) is linear
 * between the points and flat outside, as f(q) of rc_time_map_curve. hop_pos[0 .. n_hops) are the input positions of the
 * job's hops (a time map's table); hop_pos == NULL is the engine's grid k * sample_step_len.
 * The recurrence, every step ONE IEEE double operation:  A_0 = 0;  t = A_b >> 32;
 *   k = min(n_hops - 1, t * hops_per_window / window_out_len);   r = r((double)hop_pos[k]);
 *   D_b = (int64_t)floor(r * 2^38 + 0.5), clamped to [2^35, 2^41];   A_{b+1} = A_b + D_b.
 * It stops at the first A_b with A_b >> 32 >= n: that anchor is the last, *n_anchors = b + 1. *n_out is the number of m
 * with P(m) >> 32 < n. Both are stored whenever the arguments are valid. RC_ECAPACITY where cap < *n_anchors, nothing
 * written (the two-call idiom: anchor may be NULL with cap == 0). RC_EINVAL: an invalid config, a null at / ratio /
 * n_anchors / n_out, n_points == 0, n_hops == 0, points out of order or out of range, n > 2^29.
 * A constant ratio 1 gives anchor[b] = b * 2^38 and n_out = n; a constant 3/4 gives n_out = rc_resample_len(n, 3, 4). */
int rc_warp_curve(const rc_config *cfg, const int64_t *hop_pos, size_t n_hops, const double *at, const double *ratio,
                  size_t n_points, size_t n, int64_t *anchor, size_t cap, size_t *n_anchors, size_t *n_out);

#endif
