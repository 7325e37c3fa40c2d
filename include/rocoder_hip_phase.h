/*
 * rocoder_hip_phase.h - the phase modes of the C-ABI in rocoder_hip.h, which includes this file: include that one.
 * They add functions and constants only - no struct layout, RC_ABI_VERSION stays what it is.
 */
#ifndef ROCODER_HIP_PHASE_H
#define ROCODER_HIP_PHASE_H

#ifndef ROCODER_HIP_H
#error "include rocoder_hip.h"
#endif

/* ---- phase-coherent resynthesis: propagated and peak-locked phases ---- */
/* The reference resynthesises magnitude x random phase (src/fft.rs:63-68): right at a factor of 8 and beyond, a smear at
 * 1.2, 2 or 3, where a phase vocoder is expected to keep partials. A mode other than RC_PHASE_RANDOM keeps the analysis
 * spectrum and rotates it: Z_k[j] = X_k[j] cis(theta_k[j]).
 *
 * The definition. All phases are integers in units of 2^-32 turn and wrap mod 2^32, so the result does not depend on
 * chunks, blocks or launch shapes. H = N / 2, step = rc_params::sample_step_len, bins j = 0 ... H, X_k the analysis
 * spectrum of hop k:
 *   a_k[j]  = llrint(atan2f(im, re) / (2 pi) * 2^32) mod 2^32
 *   dev     = (int32)(a_k[j] - a_{k-1}[j] - ((j step) mod N) (2^32 / N))          the principal argument
 *   d_k[j]  = ((j & 1) << 31) + floor((int64)dev H / step)
 *   e_k[j]  = a_{k-1}[j] - a_k[j] + d_k[j]
 *   peaks   : bin j in 1 ... H - 1 whose m2 = re^2 + im^2 is strictly greater than m2[j +- 1] and m2[j +- 2]
 *             (neighbours outside 0 ... H do not count)
 *   P_k(j)  = j (PROPAGATE); the nearest peak, the lower one on a tie (LOCKED); j in a hop without a peak
 *   theta_0 = 0, theta_k[j] = theta_{k-1}[P_k(j)] + e_k[P_k(j)]
 *   Z_k[j]  = X_k[j] cis(theta_k[j]) for j <= H, Z_k[N - j] = conj Z_k[j]
 * and the overlap-add as for RANDOM, but with the coherent envelope env_c[i] = 1 / (w[i]^2 + w[i + H]^2) (rc_phase_envelope)
 * and the amplitude rc_config::amplitude alone: the reference's max(4, f p / 4) and its hanning_crossfade_compensation
 * correct the power loss of random phases. rc_params is left as it is. At step == H every e_k is 0 and the output is
 * the input.
 *
 * A mode other than RANDOM runs on the whole-job entries - rc_engine_stretch_host, _device and the five _frames* entries
 * with the master chain behind them, positive and negative pitch multiples - and every call restarts at hop 0.
 * Refused while such a mode is set, before anything is enqueued: with RC_EUNSUPPORTED the streaming seam
 * (rc_engine_push_input, _next_window, _next_window_view), rc_engine_stretch_device_range and rc_engine_resynth; the
 * setter itself with RC_EUNSUPPORTED for a window that is not a power of two in 32 ... 16384 (an rc_multi has no setter:
 * its engines run RANDOM). With RC_EINVAL, in either order of the two calls: a host, curated or user frequency kernel,
 * a time map, an output warp. RC_EINVAL too: a mode above RC_PHASE_LOCKED, and a caller's window whose
 * w[i]^2 + w[i + H]^2 falls below 2^-10 of its maximum anywhere. */
#define RC_PHASE_RANDOM    0   /* default: the reference's path, bit for bit */
#define RC_PHASE_PROPAGATE 1   /* every bin carries its own phase from hop to hop */
#define RC_PHASE_LOCKED    2   /* identity phase locking: a bin takes the rotation of its nearest spectral peak */
int rc_engine_set_phase_mode(rc_engine *e, uint32_t mode);
int rc_engine_get_phase_mode(const rc_engine *e, uint32_t *mode);
/* Pure host: env[i] = 1.0f / (w[i] * w[i] + w[i + n/2] * w[i + n/2]), i < n / 2, every step one f32 operation.
 * RC_EINVAL: a null pointer, n odd or below 2, a sum that is not finite or falls below 2^-10 of the largest. */
int rc_phase_envelope(const float *window, size_t n, float *env /* n/2 */);

#endif
