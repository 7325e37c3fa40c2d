/*
 * rocoder_hip_timemap.h - the time-map entries of the C-ABI in rocoder_hip.h, which includes this file: include that one.
 * They are the ABI's only entries that take 64-bit signed positions and doubles; they add functions only - no struct, no
 * layout change, RC_ABI_VERSION stays what it is.
 */
#ifndef ROCODER_HIP_TIMEMAP_H
#define ROCODER_HIP_TIMEMAP_H

#ifndef ROCODER_HIP_H
#error "include rocoder_hip.h"
#endif

/* ---- time maps: per-hop input positions (variable-rate stretch, hold, reverse, scrub) --------- */
/* Every path reads hop k at input sample k * sample_step_len: one truncated integer step, fixed at rc_engine_create
 * (src/stretcher.rs:55). A time map replaces that product by a table: hop_pos[0 .. K), one entry per hop, shared by all
 * channels. Positions may repeat (a hold), decrease (reverse), be negative or lie past the end. The map is engine state,
 * set once, like the fade and the channel map: hop_pos == NULL or n_hops == 0 clears it, and that is the state after
 * rc_engine_create. The table is copied: the caller may free its own.
 * The definition, bit for bit. N = window_len, K = n_hops, x_c the input row of channel c, in_len its length:
 *   V_c[k * N + n] = x_c[hop_pos[k] + n]  where 0 <= hop_pos[k] + n < in_len,
 *                    0.0f                 elsewhere: silence before the stream and behind it (src/stretcher.rs:58-59,
 *                                         129-132),        for 0 <= k < K, 0 <= n < N.
 *   The result is what the engine's own hop path gives on the rows V_c with sample_step_len = N, for the hops 0 .. K: the
 *   engine's corrected_amp_factor, pitch_multiple, window, seed and kernels, phases keyed by (seed, channel, k) as ever.
 *   Nothing else about a hop changes.
 * K must be a multiple of hops_per_window; the output has K / hops_per_window * window_out_len frames
 * (rc_time_map_output_len). The configured `factor` no longer sets the speed; it still sets corrected_amp_factor as
 * Stretcher::new derives it.
 * RC_EINVAL, and the previous map stays: a null engine, n_hops not a multiple of hops_per_window, a position with
 * |hop_pos[k]| > 2^48.
 * While a map is set it applies to rc_engine_stretch_device and to the whole-job host-form entries -
 * rc_engine_stretch_host, rc_engine_stretch_frames, _pcm, _norm and _loud: in_len / n_frames is the length of the input
 * the positions index, and *out_len and every capacity check use the map's length. The fade, the channel map, the
 * resampler, the limiter, the dither and the loudness stages see the map job's rows as they see any job's. Host
 * frequency kernels, curated device kernels and user device kernels run as on any job: X.past(d) is the analysis
 * spectrum of hop k - d of the map, and RC_FEEDBACK keeps its order rule.
 * These entries return RC_EINVAL and name the map while one is set - a map is never silently ignored:
 * rc_engine_stretch_device_range, rc_engine_push_input, rc_engine_next_window and rc_engine_next_window_view.
 * Unaffected: rc_engine_resynth, rc_engine_forward_fft, rc_engine_frames_power, rc_engine_frames_channel_peaks, rc_multi_*.
 * How it runs: a gather kernel writes V chunk by chunk - whole windows, at most 256 MiB of rows, or one window
 * with the hops in front of it where that alone is more (long windows of many channels: N = 2^22 with 8 channels holds
 * 3 hops of 128 MiB) - in front of the unchanged hop kernels; no hop kernel reads the table, and the result does not depend on
 * the chunk size. With no map set every entry does what it does without this one, launch for launch.
 * Measurement: rc_engine_last_kernel_stats and rc_engine_kernel_times report, for a map job, the hop launches of its FIRST
 * chunk - their event time, hops and launches; the gather launches and the later chunks lie outside the event pair. A
 * caller that times a map job brackets the call with events of its own on the stream it passes (tools/bench_time_map.py). */
int rc_engine_set_time_map(rc_engine *e, const int64_t *hop_pos, size_t n_hops);
/* Pure host: the output frames of a map of n_hops hops, n_hops / hops_per_window * window_out_len; 0 for an invalid
 * config or a length that is not a multiple of hops_per_window. */
size_t rc_time_map_output_len(const rc_config *cfg, size_t n_hops);
/* Pure host: the map of a stretch factor that varies along the input. The points are (at[i], factor[i]), `at` in input
 * samples, at least 0 and strictly increasing, every factor finite and in [2^-10, 2^20]. f(q) = factor[0] for
 * q <= at[0], factor[n - 1] for q >= at[n - 1], and in between, with i the segment at[i] <= q < at[i + 1],
 *   f(q) = f_i + (f_{i+1} - f_i) * ((q - a_i) / (a_{i+1} - a_i)).
 * The recurrence, every step ONE IEEE double operation (no contraction), N = window_len, p = pitch_multiple:
 *   q_0 = 0.0;   hop_pos[k] = (int64_t)floor(q_k);   q_{k+1} = q_k + (double)N / (2.0 * psf(f(q_k)));
 *   psf(f) = f * |p| for p >= 1 and f / |p| for p < 0.
 * kd is the first k with hop_pos[k] + N > in_len; K = hops_per_window * (kd / hops_per_window + 1): the reference's own
 * termination rule - the window in which the input runs out is finished. *n_hops = K whenever the arguments are valid.
 * RC_ECAPACITY where cap < K, nothing written (the two-call idiom: hop_pos may be NULL with cap == 0). RC_EINVAL: an
 * invalid config, a null at / factor / n_hops, n_points == 0, points out of order or out of range, in_len > 2^48, a
 * curve that needs 2^28 hops or more.
 * One point whose step N / (2 psf) is an integer gives hop_pos[k] = k * sample_step_len and the K of
 * rc_offline_output_len; `-f 3 -w 16384` advances 2730.67 samples a hop on average where sample_step_len truncates to
 * 2730. */
int rc_time_map_curve(const rc_config *cfg, size_t in_len, const double *at, const double *factor, size_t n_points,
                      int64_t *hop_pos, size_t cap, size_t *n_hops);

#endif
