/*
 * rocoder_hip_mix.h - the mix-bus entries of the C-ABI in rocoder_hip.h, which includes this file: include that one.
 * They add functions and one opaque type only - no struct layout, RC_ABI_VERSION stays what it is.
 */
#ifndef ROCODER_HIP_MIX_H
#define ROCODER_HIP_MIX_H

#ifndef ROCODER_HIP_H
#error "include rocoder_hip.h"
#endif

/* ---- mix bus: keyframed layers summed on the device, in front of the master stages ---- */
/* The reference's mixer (src/mixer.rs) holds layers with amplitude keyframes, interpolated by math::sqrt_interp
 * (src/math.rs:33-40), and sums them sample by sample. Here a layer is one frames job of one engine, accumulated into a
 * device-resident bus without a download; the bus then goes through an engine's output stages into PCM frames. */
typedef struct rc_bus rc_bus;
#define RC_MIX_MAX_KEYS 4096

/* A bus holds `channels` planar f32 rows of n_frames frames on `device`, all +0.0f after rc_bus_create and after
 * rc_bus_clear. Rows are 16-byte aligned, the row stride is a multiple of 4 floats. n_frames == 0 is valid.
 * RC_EINVAL: channels == 0 or above the engine's channel limit (RC_PMAX, 32), a null `out`, a row stride beyond 2^40
 * frames; RC_ENODEVICE: no such device; RC_ENOMEM: the allocation fails. `layers` counts the rc_engine_mix_frames calls since the last clear. The
 * out-pointers of rc_bus_info may be NULL one by one. rc_bus_device_rows is for device callers (torch): row c is at
 * *d_rows + c * *stride. */
int rc_bus_create(int device, uint32_t channels, uint64_t n_frames, rc_bus **out);
void rc_bus_destroy(rc_bus *b);
int rc_bus_clear(rc_bus *b);
int rc_bus_info(const rc_bus *b, uint32_t *channels, uint64_t *n_frames, uint32_t *layers);
int rc_bus_device_rows(rc_bus *b, float **d_rows, size_t *stride);

/* One layer. x[cl][t], t in [0, n), cl < CL = rc_config::channels, is the planar f32 result that rc_engine_stretch_frames
 * interleaves for the same arguments under the engine's current state - behind the channel map, time map, device kernel,
 * resampler or warp, fade and limiter where those are set; n is what that entry reports in *out_frames_len. The job runs
 * through the same pipeline with a mix launch in place of pack and download: no output frame travels to the host. The
 * call blocks and the bus is complete on return, so calls (from any engine) on one bus are ordered by call order, which is
 * the summation order.
 *
 * The envelope amp(t), on the LAYER's clock t (the reference's total_samples_played is per layer, mixer.rs:132-145). Every
 * step is ONE correctly rounded IEEE f32 operation, integers converted to f32 with round to nearest even:
 *   n_keys == 0: 1.0f.  n_keys == 1: key_amp[0].  Otherwise (key_frame strictly increasing), K = n_keys:
 *   t <  key_frame[0]      key_amp[0]
 *   t >= key_frame[K - 1]  key_amp[K - 1]
 *   key_frame[i] <= t < key_frame[i + 1], a = key_amp[i], b = key_amp[i + 1]:
 *     r   = (float)(t - key_frame[i]) / (float)(key_frame[i + 1] - key_frame[i])
 *     inc = a < b
 *     pr  = (r * 2.0f - 1.0f) * (inc ? 1.0f : -1.0f)
 *     fct = sqrtf(0.5f * (1.0f + fmaxf(pr, -1.0f)))
 *     amp = (inc ? a : b) + fabsf(b - a) * fct            (a multiplication, then an addition: not contracted)
 * which is math::sqrt_interp(a, b, r) as written. With the keys (0, 0), (F, 1) the envelope on [0, F) is the output
 * fade's up(t, F) bit for bit. This is the offline form of Layer::current_amp. Two things the reference does are NOT
 * reproduced: it prunes keys only at chunk edges (mixer.rs:62-64, 108-120), so its progress runs past 1 and the amplitude
 * overshoots until the next chunk; and it panics on a t in front of the first key.
 *
 * The send: send == NULL requires CL == CB (the bus's channels) and s[cb][t] = x[cb][t]. Otherwise send[cb * CL + cl] is
 * finite and s[cb][t] is ONE chain acc = fmaf(send[cb * CL + cl], x[cl][t], acc) from +0.0f with cl ascending.
 *
 * The sum: for u = offset + t with 0 <= u < N, bus[cb][u] = bus[cb][u] + s[cb][t] * amp(t) - one multiplication, then
 * one addition, not contracted. Frames with u outside the bus are dropped; *mixed_frames (may be NULL) is the number of t
 * that landed. Denormals are kept, a NaN in x stays a NaN in the bus, and a sample's bits do not depend on chunk, launch
 * or tile.
 *
 * RC_EINVAL, before any work and with the bus untouched: what rc_engine_stretch_frames rejects; a null bus; bus and
 * engine on different devices; send == NULL with CL != CB; n_keys > RC_MIX_MAX_KEYS; null key arrays with n_keys > 0; keys
 * not strictly increasing; a key amplitude or send value that is not finite; offset outside +-2^62. n_frames == 0 is
 * valid and counts as a layer. Under a host frequency kernel (rc_config::kernel) the job runs as that path runs every
 * frames job - whole input up, the job, one mix launch - and is supported. */
int rc_engine_mix_frames(rc_engine *e, const void *frames, size_t n_frames, uint32_t format, rc_bus *bus, int64_t offset,
                         const uint64_t *key_frame, const float *key_amp, size_t n_keys, const float *send,
                         uint64_t *mixed_frames);

/* The master. y[c][u], u in [0, N), the bus rows, take the place of the planar result in the definitions rocoder_hip.h
 * states, in this order: (1) the engine's output fade, counting bus frames and checked against N; (2) its limiter,
 * rc_engine_last_limiter_stats included; (3) for target_peak > 0 the peak and ONE gain of rc_engine_stretch_frames_norm -
 * target_peak == 0 gives no gain, the peak is still reported and *gain is 1; (4) its dither; (5) the quantiser and
 * *clipped. All five RC_PCM_* output formats, at any byte alignment, into pageable or page-locked memory.
 * No hops run: the engine's channel map, time map, resampler, warp and device kernels do not apply.
 * The bus is not changed: a second call gives the same bytes.
 * RC_EINVAL: a null engine, bus or out_frames (out_frames_len, peak, gain and clipped are optional and may be NULL);
 * CB != rc_config::channels; different devices; an out_format outside 1 ... 5; a target_peak that is
 * negative or not finite; a fade that does not lie inside N. RC_ECAPACITY: out_cap_frames < N. On any error nothing
 * behind the out-pointers is written. */
int rc_engine_bus_frames(rc_engine *e, const rc_bus *bus, void *out_frames, size_t out_cap_frames, uint32_t out_format,
                         float target_peak, size_t *out_frames_len, float *peak, float *gain, uint64_t *clipped);

/* Pure host: amp[i] = amp(t0 + i), i < n, as defined above. RC_EINVAL: a null amp with n > 0, null key arrays with
 * n_keys > 0, n_keys > RC_MIX_MAX_KEYS, keys not strictly increasing, a key amplitude that is not finite. */
int rc_mix_envelope(const uint64_t *key_frame, const float *key_amp, size_t n_keys, uint64_t t0, size_t n, float *amp);

#endif
