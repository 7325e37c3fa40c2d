/*
 * rocoder_hip.h — C-ABI of the MI355X (gfx950) stretch engine: the drop-in boundary for
 * rocoder's analysis -> kernel -> resynthesis -> overlap-add hot path.
 *
 * Plain C: opaque handle, plain pointers and sizes, int status codes, no C++/torch types.
 * Every entry point names the reference interface (file:line under the rocoder source
 * tree, v0.4.0) that it replaces. A Rust host binds this with one `extern "C"` block
 * (INTEGRATION.md shows the exact stub and where `Stretcher` calls into it).
 *
 * Threading: one thread at a time per handle (the reference calls every Stretcher from
 * the single StretcherProcessor thread: src/stretcher_processor.rs:55-71). HIP streams,
 * events and scratch buffers are private to the handle.
 *
 * The library has NO CPU fallback: every compute entry point fails with RC_ENODEVICE when
 * no gfx950 device is usable.
 */
#ifndef ROCODER_HIP_H
#define ROCODER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ABI_VERSION 5 /* 3: + rc_shard_plan / rc_multi_*; 4: + rc_engine_next_window_view, rc_multi_set_staging,
                          * rc_calib_valu; 5: + rc_host_alloc / rc_host_free (struct layouts unchanged since 2) */

/* status codes */
#define RC_OK 0
#define RC_WOULD_BLOCK 1   /* the reference would block in Receiver::recv (src/stretcher.rs:125) */
#define RC_EINVAL (-1)     /* the reference would assert/panic/never terminate */
#define RC_ENODEVICE (-2)  /* no usable HIP device */
#define RC_EUNSUPPORTED (-3) /* valid for the reference, not (yet) on the GPU path */
#define RC_ENOMEM (-4)
#define RC_EHIP (-5)       /* HIP runtime error; see rc_last_error() */
#define RC_ECAPACITY (-6)  /* caller buffer too small */

/*
 * The channel count, and what bounds it on each path (DESIGN "Parity across channel counts"):
 *   fused kernels, N = 32 ... 65536   the launch is runs_per_channel x channels workgroups in grid.x, a 32-bit product
 *                                     that the run planner keeps at max(channels, a few rounds of the resident
 *                                     workgroups): 2^31 - 1 by itself. The tail staging in front of every range, ragged
 *                                     last hop and streaming batch (prep_kernel) has the channels in grid.y: 65535.
 *   unfused (host / device kernel, negative pitch), chirp-z lengths, frames stages
 *                                     channels in grid.y or grid.z of the overlap-add, tail, chirp-z, resampling and
 *                                     frames launches: 65535. One chunk holds at least one window of every channel:
 *                                     channels x hops_per_window x 12 ... 28 N bytes of scratch (RC_ENOMEM beyond HBM).
 *   long windows, N > 65536           channels in grid.z: 65535; a chunk of one window takes channels x 2 x 20 N bytes.
 *   phase key                         the channel index above bit 40 of a 64-bit counter: 2^24 channels.
 *   every path                        channels x N / 2 floats of overlap tail per engine.
 * RC_MAX_CHANNELS is the smallest of them. rc_derive_params, rc_offline_output_len (0) and rc_engine_create refuse a larger
 * count with RC_EUNSUPPORTED before anything is allocated; rc_last_error() names the limit.
 * RC_MAX_JOB_HOPS: the hops of one call over all its channels (hops x channels). The kernels' flat hop indices and the run
 * tables are 32-bit words. Only a job knows its hops: every entry that runs hops (whole jobs, ranges, streaming batches,
 * rc_multi shards) returns RC_EUNSUPPORTED for a larger product before it enqueues a launch.
 */
#define RC_MAX_CHANNELS 65535u
#define RC_MAX_JOB_HOPS 4294967295ull

/*
 * User frequency kernel. C-ABI shape of the reference's hot-swapped
 *   #[no_mangle] pub fn apply(elapsed_ms: usize, input: Vec<(f32,f32)>) -> Vec<(f32,f32)>
 * (README.md:106-112; resolved and called at src/fft.rs:93-95). `in_reim`/`out_reim` hold
 * n_bins == window_len interleaved (re,im) pairs in natural DFT order (ALL N bins).
 * `time_ms` is Unix-epoch milliseconds as in src/fft.rs:89-92. A non-zero return is the
 * equivalent of a panic (src/fft.rs:100-106): the hop falls back to the unmodified spectrum.
 * Called on the engine's calling thread, per channel in hop order.
 */
typedef int (*rc_freq_kernel)(uint64_t time_ms, const float *in_reim, float *out_reim,
                              size_t n_bins, void *user);

/* Stretcher::new arguments (src/stretcher.rs:30-39) + main.rs:131-147 call-site values. */
typedef struct rc_config {
    uint32_t struct_size;    /* = sizeof(rc_config), ABI guard */
    uint32_t window_len;     /* -w/--window (src/main.rs:34); even, 4..4194304 (powers of two <= 65536: the fast kernels; above 65536: the long-window path); odd or larger: RC_EUNSUPPORTED */
    float factor;            /* -f/--factor (src/main.rs:46-52) */
    float amplitude;         /* -a/--amplitude */
    int32_t pitch_multiple;  /* -p/--pitch_multiple, i8 in the reference, != 0 */
    uint32_t sample_rate;    /* AudioSpec.sample_rate (src/audio.rs:31-37) */
    uint32_t channels;       /* AudioSpec.channels: one Stretcher per channel (main.rs:133); 1 ... RC_MAX_CHANNELS (below) */
    float buffer_secs;       /* -b/--buffer (Duration, default 1 s) */
    uint64_t seed;           /* phase-source seed (replaces thread_rng, src/fft.rs:64) */
    int32_t device;          /* HIP device ordinal */
    uint32_t max_batch_hops; /* streaming look-ahead cap per launch and channel; 0 = default (8 MiB of windows) */
    const float *window;     /* host, window_len floats; NULL = windows::hanning (main.rs:131) */
    rc_freq_kernel kernel;   /* --freq-kernel; NULL = none */
    void *kernel_user;
    uint64_t kernel_time_ms; /* 0 = wall clock (src/fft.rs:89-92); non-zero = fixed (tests) */
    /* Host threads that call `kernel`: 0 or 1 = one thread and the reference's call order (windows outer,
     * channels inner: src/stretcher_processor.rs:63-70). n > 1 = the channels are dealt to up to n threads;
     * each channel still sees its hops in order, but calls of different channels interleave, so `kernel`
     * must be re-entrant and must not carry state across channels. */
    uint32_t kernel_threads;
    /* Curated frequency kernels that run on the GPU: the spectrum never leaves the device.
     * They take the place of `kernel` (setting both is RC_EINVAL). All act on the N-bin spectrum X of a hop
     * like an apply() would, Y = K(X), before |Y| is taken (src/fft.rs:42-48,67):
     *   RC_DK_GAIN   Y[j] = dk_gain X[j]                      (README.md:121-128 with any factor)
     *   RC_DK_BAND   Y[j] = (dk_lo_bin <= min(j, N - j) <= dk_hi_bin ? dk_gain : dk_gain_outside) X[j]
     *   RC_DK_SHIFT  Y[j] = X[j - dk_shift_bins] for 0 <= j <= N/2 (0 where j - shift leaves [0, N/2]),
     *                Y[N - j] = conj(Y[j]) : the spectrum of a real signal moved up or down by whole bins
     * Cost: GAIN rides on the amplitude of the fused kernels (free); BAND is applied inside the fused kernel of the
     * default 16384-sample window (a few instructions per bin pair) and otherwise, like SHIFT, runs as forward
     * transform -> kernel -> resynthesis on device scratch. */
    uint32_t device_kernel;
    float dk_gain, dk_gain_outside;
    uint32_t dk_lo_bin, dk_hi_bin;
    int32_t dk_shift_bins;
} rc_config;
#define RC_DK_NONE 0
#define RC_DK_GAIN 1
#define RC_DK_BAND 2
#define RC_DK_SHIFT 3

/* Values derived in Stretcher::new (src/stretcher.rs:40-56). */
typedef struct rc_params {
    uint32_t window_len, half_window_len;
    uint64_t samples_needed_per_window;
    uint32_t sample_step_len;
    uint32_t hops_per_window; /* iterations of the loop at src/stretcher.rs:91 */
    uint32_t window_out_len;  /* samples returned per next_window() */
    float corrected_amp_factor;
    float pitch_shifted_factor;
} rc_params;

typedef struct rc_engine rc_engine;

/* Thread-local description of the last failure on this thread. */
const char *rc_last_error(void);
int rc_abi_version(void);
/* Identifies the kernel generation inside the library (e.g. "hop4/r02b"): measurement files under
 * profiles/ carry it, so a counter summary is only ever quoted next to the kernels it was taken on. */
const char *rc_kernel_id(void);
/* Number of usable gfx950 devices (0 when none; never fails). */
int rc_device_count(void);

/* Pure host helpers (no device): parameter derivation of Stretcher::new
 * (src/stretcher.rs:40-56) and the output length of an offline `-o` run
 * (src/stretcher.rs:91,123-134 + src/stretcher_processor.rs:64-69). */
int rc_derive_params(const rc_config *cfg, rc_params *out);
size_t rc_offline_output_len(const rc_config *cfg, size_t in_len);
/* Phase-source spec (replaces rand::thread_rng at src/fft.rs:64-67), exposed for tests. */
uint64_t rc_phase_key(uint64_t seed, uint32_t channel, uint64_t hop);
uint32_t rc_phase_hash(uint64_t key, uint32_t counter);
/* theta in [0, pi) of bin `bin` of an n_bins-point spectrum: bins b < n_bins/2 take the top 23 bits
 * of rc_phase_hash(key, b) (rand 0.8.5's f32 draw), bins b >= n_bins/2 the low 16 bits of
 * rc_phase_hash(key, b - n_bins/2). */
float rc_phase_theta(uint64_t key, uint32_t bin, uint32_t n_bins);

/* Stretcher::new for all channels (src/main.rs:133-153, src/stretcher.rs:30-76) +
 * ReFFT::new (src/fft.rs:25-40): builds window/envelope/twiddle tables on the device. */
int rc_engine_create(const rc_config *cfg, rc_engine **out);
void rc_engine_destroy(rc_engine *e);
int rc_engine_get_params(const rc_engine *e, rc_params *out);

/* ---- streaming seam: one call per reference call ------------------------------------- */
/* Sender<Vec<f32>>::send on the channel's input (src/main.rs:148; src/stretcher.rs:125-127) */
int rc_engine_push_input(rc_engine *e, uint32_t channel, const float *samples, size_t n);
/* dropping the Sender: recv() then fails and the tail is zero-padded (src/stretcher.rs:129-132) */
int rc_engine_close_input(rc_engine *e, uint32_t channel);
/* Stretcher::next_window (src/stretcher.rs:87-121). Writes rc_params.window_out_len samples.
 * RC_WOULD_BLOCK when the reference would block waiting for input. */
int rc_engine_next_window(rc_engine *e, uint32_t channel, float *out, size_t out_cap,
                          size_t *n_out);
/* The same hand-out without the copy: *window points at the window's window_out_len samples inside the engine's
 * pinned host block, valid until the next rc_engine_next_window / _view call on the SAME channel. The reference moves
 * a freshly allocated Vec<f32> into the bounded queue (src/stretcher.rs:112-120, src/stretcher_processor.rs:69); a
 * host that writes the window straight to its sink (src/main.rs:197-203: the WAV writer) needs no Vec at all. On a
 * closed channel (whole input known) the batches after the one being handed out - every closed channel's together, up to
 * two in flight - are computed and copied meanwhile. */
int rc_engine_next_window_view(rc_engine *e, uint32_t channel, const float **window, size_t *n_out);
/* Stretcher::is_done (src/stretcher.rs:78-80): 1 / 0, or <0 on error. */
int rc_engine_is_done(const rc_engine *e, uint32_t channel);
/* Stretcher::channel_bound (src/stretcher.rs:82-85) */
size_t rc_engine_channel_bound(const rc_engine *e);

/* ---- offline fast path (`-o`, all hops known up-front) ------------------------------- */
/* Whole-job stretch of `channels` host arrays of `in_len` samples: what main.rs:133-155 +
 * StretcherProcessor::start (src/stretcher_processor.rs:56-71) + AudioBus::into_audio
 * (src/audio.rs:152-172) produce. out[c] must hold rc_offline_output_len() samples. */
/* Upload, compute and download run as a pipeline over window chunks (the download of chunk i under the kernel of
 * chunk i + 1 and the upload of chunk i + 2). Rows that came from rc_host_alloc (or that the caller registered with
 * hipHostRegister) are the DMA's source / target themselves; pageable rows are staged through pinned slots by up to
 * eight copy threads. Blocking: out[c] is complete on return. */
int rc_engine_stretch_host(rc_engine *e, const float *const *in, size_t in_len, float *const *out,
                           size_t out_cap, size_t *out_len);
/* The same job on interleaved PCM frames, as a WAV data chunk, a socket or the reference's reader deliver them
 * (src/audio_files.rs:30-49,159-188), with interleaved f32 frames back, as its writer takes them (src/audio_files.rs:
 * 203-226). `frames` holds n_frames x channels samples, frame-major and little endian, at ANY byte alignment (a data
 * chunk sits wherever its header ends); out_frames receives rc_offline_output_len(cfg, n_frames) frames of `channels`
 * floats. Both format changes run as kernels on the device inside the upload / compute / download pipeline of
 * rc_engine_stretch_host: the raw bytes cross PCIe (an int16 source at half the size of its floats), and the output
 * equals rc_engine_stretch_host on the decoded rows bit for bit. Sample -> float, the reader's formulas:
 *   RC_PCM_U8   n = byte - 128, then n / 127           (hound's u8 -> i8, src/audio.rs:16-29)
 *   RC_PCM_I16  n / 32767
 *   RC_PCM_I24  3 bytes little endian, sign-extended, n / 8388608
 *   RC_PCM_I32  n / 2147483647
 *   RC_PCM_F32  the bits as they are
 * each (float)n / K one correctly rounded f32 division. RC_EINVAL: a null pointer, a format outside 1 ... 5;
 * RC_ECAPACITY: out_cap_frames too small. n_frames == 0 is valid (what rc_engine_stretch_host gives for in_len == 0).
 * Pageable and page-locked memory both work on either side. Blocking: out_frames is complete on return. */
#define RC_PCM_U8 1
#define RC_PCM_I16 2
#define RC_PCM_I24 3
#define RC_PCM_I32 4
#define RC_PCM_F32 5
int rc_engine_stretch_frames(rc_engine *e, const void *frames, size_t n_frames, uint32_t format,
                             float *out_frames, size_t out_cap_frames, size_t *out_frames_len);
/* rc_engine_stretch_frames with the output as PCM frames of `out_format` (RC_PCM_*): the same job in the same pipeline,
 * quantised and packed on the device, so that a 16-bit result crosses PCIe at half the bytes of its floats. out_frames
 * receives rc_offline_output_len(cfg, n_frames) frames of `channels` little-endian samples and may sit at ANY byte
 * alignment (a WAV data chunk inside a mapped file); no byte in front of or behind them is written. Float -> sample,
 * bit for bit: t = x * (float)S, ONE IEEE f32 multiplication; r = rint(t), to nearest, ties to even, NaN -> 0; the
 * integer written is r clamped to [LO, HI]:
 *   RC_PCM_U8   S 127         [-128, 127]            written as the byte n + 128 (the inverse of hound's u8 -> i8)
 *   RC_PCM_I16  S 32767       [-32768, 32767]        2 bytes
 *   RC_PCM_I24  S 8388608     [-8388608, 8388607]    the low 3 bytes
 *   RC_PCM_I32  S 2147483647  [-2^31, 2^31 - 1]      4 bytes ((float)S is 2^31; +1.0 gives 2^31 - 1, not INT_MIN)
 *   RC_PCM_F32  the bits unchanged: the output of rc_engine_stretch_frames
 * S is the divisor rc_engine_stretch_frames reads with, so decoding what this wrote and encoding it again gives the
 * same bytes for u8 / i16 / i24. There is no dither unless rc_engine_set_output_dither has set one (below; with it that
 * round trip no longer holds), and no noise shaping beyond that entry's first-order high-pass. *clipped (may be NULL) receives the number of
 * output samples with !(|x| <= 1) - beyond full scale, or NaN - whatever out_format is, RC_PCM_F32 included: the
 * stretch overshoots full scale regularly, and an integer format has to clip what a float file hides.
 * RC_EINVAL: a null pointer (other than clipped), format or out_format outside 1 ... 5; RC_ECAPACITY: out_cap_frames too
 * small. n_frames == 0 is valid and gives *clipped = 0. Pageable and page-locked memory both work on either side.
 * Blocking: out_frames is complete on return. */
int rc_engine_stretch_frames_pcm(rc_engine *e, const void *frames, size_t n_frames, uint32_t format,
                                 void *out_frames, size_t out_cap_frames, uint32_t out_format,
                                 size_t *out_frames_len, uint64_t *clipped);
/* rc_engine_stretch_frames_pcm with the result peak-normalised on the device: the peak of the whole job is measured there,
 * and every sample is multiplied by one gain in front of the quantiser, so that an integer file needs no second run at
 * a guessed amplitude. The same job otherwise: the input formats, the output formats (RC_PCM_F32 included), any byte
 * alignment on both sides, no byte in front of or behind the result written, pageable or page-locked memory, blocking.
 * The definition, bit for bit:
 *   y      the f32 result of rc_engine_stretch_frames on the same input: all channels, all frames.
 *   peak   the largest |y| among the samples with |y| < inf; NaN and +-inf are skipped. 0.0f when there is no such
 *          sample or all are zero.
 *   gain   target_peak / peak, ONE IEEE f32 division, when peak > 0 and that quotient is finite; otherwise 1.0f.
 *   z      y * gain, ONE IEEE f32 multiplication, not contracted with the quantiser's multiplication by S; denormals
 *          are kept.
 *   bytes  exactly what rc_engine_stretch_frames_pcm writes for a planar result z: the quantiser stated above, and the
 *          bits of z themselves for RC_PCM_F32.
 *   *clipped  the number of samples with !(|z| <= 1), counted after the gain.
 * peak * gain can round one ulp above target_peak: with target_peak == 1 the peak sample itself may therefore be
 * counted in *clipped. The integer formats write it as full scale either way.
 * peak, gain and clipped may each be NULL. RC_EINVAL: what rc_engine_stretch_frames_pcm rejects, and a target_peak that
 * is not finite or not > 0; RC_ECAPACITY: out_cap_frames too small. n_frames == 0 is valid and gives peak 0, gain 1,
 * clipped 0. On any error nothing behind the out-pointers is written.
 * The job runs in two phases over the engine's pipeline - compute and measure, then pack and download - and the gain is
 * formed on the device between them: there is no host round trip, and nothing is held that the other two frame
 * entries do not hold already. */
int rc_engine_stretch_frames_norm(rc_engine *e, const void *frames, size_t n_frames, uint32_t format, void *out_frames,
                                  size_t out_cap_frames, uint32_t out_format, float target_peak,
                                  size_t *out_frames_len, float *peak, float *gain, uint64_t *clipped);
/* rc_engine_stretch_frames_pcm with the result loudness-normalised on the device: the integrated loudness of ITU-R BS.1770-4
 * / EBU R 128 and the true peak of the whole job are measured there, and every sample is multiplied by one gain in front
 * of the quantiser - the gain that brings the job to target_lufs, or the smaller one that keeps its true peak at
 * max_true_peak. The same job otherwise: the input and output formats, any byte alignment, pageable or page-locked memory,
 * blocking. The definition:
 *   y[c][t]  t in [0, n): the planar f32 result rc_engine_stretch_frames gives under the engine's current state - behind the
 *            channel map, the resampler, the fade and the limiter where those are set.
 *   R        sample_rate, 0 meaning rc_config::sample_rate. A caller that set an output-rate step passes the OUTPUT's rate.
 * K-weighting: two biquads, their coefficients computed in f64 on the host, K = tan(pi f0 / R) per stage.
 *   stage 1, the shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G / 20),
 *     Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2;  b0 = (Vh + Vb K / Q + K^2) / a0;  b1 = 2 (K^2 - Vh) / a0;
 *     b2 = (Vh - Vb K / Q + K^2) / a0;  a1 = 2 (K^2 - 1) / a0;  a2 = (1 - K / Q + K^2) / a0
 *   stage 2, the high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1], a1 and a2 as above with its own
 *     K and Q.
 *   At R = 48000 these reproduce the table of BS.1770-4 to 3e-16 relative.
 *   k[c] = stage 2 of stage 1 of y[c], both from a zero state at t = 0.
 * Sub-block energies: sub = (R + 5) / 10 frames (100 ms); nb = n / sub, a partial tail is not measured;
 *   e[c][j] = the sum of k[c][t]^2 over t in [j sub, (j + 1) sub).
 * Integrated loudness, in f64 on the host from the f32 words e:
 *   400 ms blocks at 75 % overlap: for i in [0, nb - 3), z[c][i] = (e[c][i] + ... + e[c][i + 3]) / (4 sub);
 *   l[i] = the sum over the channels of z[c][i]: every channel has weight 1. The rows carry no speaker layout: the 1.41 of
 *   surround channels and the exclusion of an LFE channel are NOT applied.  L(x) = -0.691 + 10 log10(x).
 *   absolute gate: keep the i with L(l[i]) > -70;  relative gate: G = L(mean of the kept l) - 10, keep those with
 *   L(l[i]) > G as well;  I = L(mean of the l[i] that passed both);  I = -inf where no block passes or nb < 4.
 * True peak: u[c][m], m in [0, 4 n), is exactly what rc_engine_set_output_resample's definition gives for the rows y at the
 *   step num / den = 1 / 4: the f32 table of rc_resample_table(1, 4, ...) (4 rows of 64 taps), the same single fmaf chain
 *   with j ascending, y zero outside [0, n). tp = the largest of |y[c][t]| and |u[c][m]| among the values with |.| < inf:
 *   NaN and +-inf are skipped, as the normaliser's peak skips them; 0 where there are none. A maximum of order-fixed
 *   chains is order-free: tp is defined bit for bit. What the filter limits: it is flat to 0.00025 dB up to 0.8 of Nyquist
 *   only, and 4 points per sample can miss a tone's crest by a factor of up to cos(pi f / (4 R)): at f = R / 8 that is
 *   cos(pi / 32), -0.042 dB, and the worst case measured over the phases (tests/test_loudness_host.py) is -0.0419 dB.
 *   Above 0.8 of Nyquist the reading falls off with the filter.
 * Gain: gl = (float)pow(10.0, ((double)target_lufs - (double)(float)I) / 20.0), formed from the REPORTED f32 loudness so
 *   that a caller can reproduce it; gl = 1 where I = -inf.  gc = max_true_peak / tp, ONE f32 division, where
 *   max_true_peak > 0 and tp > 0; otherwise +inf.  g = min(gl, gc); g = 1 where that is not finite or not > 0.
 *   z = y * g; the bytes and *clipped are exactly what rc_engine_stretch_frames_norm writes for a gain of g: ONE IEEE
 *   multiplication, not contracted, then the dither and the quantiser as they stand.
 * The device computes e in f64 and rounds each word once. A span of sub-blocks starts its recurrence from a zero state
 * 200 ms in front of it, which differs from the definition by a relative 1.6e-12 of a sub-block's energy; the words are
 * sums of a fixed order, so a job measured twice gives the same *lufs. A NaN or an inf in y leaves *lufs unspecified.
 * lufs, true_peak, gain, clipped and out_frames_len may each be NULL. RC_EINVAL: what rc_engine_stretch_frames_pcm rejects;
 * a target_lufs that is not finite; a max_true_peak that is NaN or negative (0: no ceiling); R < 8000 or R > 768000.
 * RC_ECAPACITY: out_cap_frames too small. n_frames == 0 is valid and gives lufs -inf, true_peak 0, gain 1, clipped 0. On
 * any error nothing behind the out-pointers is written.
 * Reach: as rc_engine_stretch_frames_norm, under a host frequency kernel as well. The job runs in the same two phases with
 * ONE host round trip between them: channels x nb + 1 words come back, the gate and the gain are formed on the host.
 *
 * Pure host helpers, no device touched:
 * rc_loudness_coeffs: the ten coefficients at sample_rate - b0 b1 b2 a1 a2 of stage 1, then of stage 2 - the f64 values
 *   rounded once to f32. RC_EINVAL: a null pointer, a rate outside 8000 ... 768000.
 * rc_loudness_sub_blocks: nb for n_frames at sample_rate; 0 for a rate out of range.
 * rc_loudness_integrated: I as stated above from the words energy[c * stride + j], j < n_sub, c < channels, rounded once to
 *   f32 (-inf included). RC_EINVAL: a null pointer (energy may be null with n_sub == 0), channels == 0, stride < n_sub, a
 *   rate out of range; *lufs is then left as it was. */
int rc_engine_stretch_frames_loud(rc_engine *e, const void *frames, size_t n_frames, uint32_t format, void *out_frames,
                                  size_t out_cap_frames, uint32_t out_format, uint32_t sample_rate, float target_lufs,
                                  float max_true_peak, size_t *out_frames_len, float *lufs, float *true_peak, float *gain,
                                  uint64_t *clipped);
int rc_loudness_coeffs(uint32_t sample_rate, float *coeffs);
size_t rc_loudness_sub_blocks(size_t n_frames, uint32_t sample_rate);
int rc_loudness_integrated(const float *energy, uint32_t channels, size_t n_sub, size_t stride, uint32_t sample_rate,
                           float *lufs);
/* The reference's sqrt fade-in / fade-out (`-x/--fade`, src/main.rs:91-97,206) on the result of the four whole-job
 * host-form entries above - rc_engine_stretch_host, rc_engine_stretch_frames, rc_engine_stretch_frames_pcm and
 * rc_engine_stretch_frames_norm - applied on the device to the planar f32 result, in front of everything that reads it.
 * It is Audio::fade_in_at_sample(0, in_len) followed by Audio::fade_out_at_sample(out_start, out_len) (src/audio.rs:
 * 81-113) with math::sqrt_interp (src/math.rs:33-40), its offline form - not the mixer's keyframes (src/mixer.rs:179-190),
 * whose amplitude overshoots 1 between the end of a fade-in and the next chunk edge. The fade is engine state, set
 * once: (0, RC_FADE_NONE, 0) clears it, and that is the state after rc_engine_create. All three are counts of output
 * frames; every channel gets the same envelope. The definition, bit for bit:
 *   T      the job's output length in frames (rc_offline_output_len); y[c][t] what rc_engine_stretch_host gives with
 *          no fade set.
 *   sq(p, d), p < d, every step ONE correctly rounded IEEE f32 operation, the integers converted to f32 with round to
 *          nearest even:   r = (float)p / (float)d;   b = r * 2.0f - 1.0f;
 *            rising   up(p, d)   = sqrtf(0.5f * (1.0f + fmaxf( b, -1.0f)))
 *            falling  down(p, d) = sqrtf(0.5f * (1.0f + fmaxf(-b, -1.0f)))
 *          (sqrt_interp(0, 1, r) and sqrt_interp(1, 0, r) without their `start + |end - start| * factor`, which is
 *          exact for 0 and 1)
 *   y1     t < in_len: y * up(t, in_len), ONE multiplication; otherwise y.
 *   z      out_start <= t < out_start + out_len: y1 * down(t - out_start, out_len), ONE multiplication;
 *          t >= out_start + out_len: +0.0f, assigned as the reference assigns it - whatever y1 was, NaN and negative
 *          values included; otherwise y1. Where the two ranges overlap a sample is multiplied twice, in this order.
 * in_len == 0 is no fade-in; out_start == RC_FADE_NONE is no fade-out; out_len == 0 is a hard cut at out_start.
 * z takes the place of y in everything downstream: the peak and the gain of rc_engine_stretch_frames_norm, the
 * quantiser, the count of clipped samples, the f32 frames and rows.
 * Here: RC_EINVAL where out_start + out_len wraps (RC_FADE_NONE with an out_len included). At a call of one of the four
 * entries: RC_EINVAL, before any work and with nothing written, where in_len > T or out_start + out_len > T (the
 * reference logs "out of bounds, ignoring" there, src/audio.rs:82-85; a C-ABI caller is better served by a status).
 * A job of no frames with a fade inside T = 0 is valid.
 * The fade does NOT apply to the device-form entries (rc_engine_stretch_device, rc_engine_stretch_device_range), to
 * the streaming seam (rc_engine_next_window ...) or to rc_multi: they return what they return without it, fade set or
 * not. Only the frames a fade changes are touched: fades of 1 s cost 2 s of samples, not the job. */
#define RC_FADE_NONE UINT64_MAX
int rc_engine_set_output_fade(rc_engine *e, uint64_t in_len, uint64_t out_start, uint64_t out_len);
/* Dither in front of the integer quantiser of rc_engine_stretch_frames_pcm and rc_engine_stretch_frames_norm: without it
 * a signal below half a quantiser step - the tail of a fade-out, a quiet passage in 8 or 16 bits - turns into
 * signal-correlated distortion and then into digital silence; with it the quantisation error is noise that does not
 * depend on the signal. The dither is engine state, set once, like the output fade and the channel map; RC_DITHER_NONE
 * is the state after rc_engine_create. It is counter-based: a sample's dither depends on the seed, its channel and its
 * output frame alone, so the bytes of a job do not depend on how the job is cut into chunks, launches or tiles.
 * The definition, bit for bit, for output frame t (absolute, from 0) and job channel c (the row of the job: a channel
 * map does not change it):
 *   K(c)    rc_phase_key(seed, c, 0xFFFFFFFFFF): the hop index 2^40 - 1 is one that no job reaches, so the draws stay
 *           apart from the phase source even under the same seed.
 *   h(c, t) rc_phase_hash(K(c), (uint32_t)t): the counter is t mod 2^32, the sequence repeats after 2^32 frames.
 *   RC_DITHER_TPDF     i = (int)(h >> 16) - (int)(h & 0xFFFF): triangular, 2 LSB peak to peak, white.
 *   RC_DITHER_TPDF_HP  i = (int)(h(c, t) >> 16) - (int)(h(c, (uint32_t)(t - 1)) >> 16): the difference of consecutive
 *                      uniform draws - the same triangle, high-passed (at t = 0 the earlier counter is 0xFFFFFFFF).
 *   d       (float)i * 2^-16: both steps exact in f32, |d| < 1.
 *   t1 = x * (float)S, ONE IEEE f32 multiplication;  t2 = t1 + d, ONE IEEE f32 addition, not contracted into an fma with
 *   the multiplication;  r = rint(t2), ties to even, NaN -> 0, clamped to [LO, HI]; S, LO, HI as stated at
 *   rc_engine_stretch_frames_pcm. Under rc_engine_stretch_frames_norm x is z = y * gain as stated there.
 * *clipped counts !(|x| <= 1) on the value in front of the dither: the same number with and without it. Near i24 full
 * scale t1 + d rounds to f32's half steps, and a code can differ from the undithered one by 2. Decoding what a dithered
 * call wrote and encoding it again does not give the same bytes.
 * Reach: out_format RC_PCM_U8, RC_PCM_I16 and RC_PCM_I24 of those two entries, under a host frequency kernel as well.
 * RC_PCM_I32 and RC_PCM_F32 are written exactly as without dither (an f32 sample holds 24 significant bits: the i32
 * quantiser adds no error that a step of noise could randomise). rc_engine_stretch_frames, rc_engine_stretch_host, the
 * device forms, the streaming seam and rc_multi take no dither. With RC_DITHER_NONE every byte is what it is without
 * this entry. RC_EINVAL: a null engine, mode > 2; the previous state stays. */
#define RC_DITHER_NONE 0
#define RC_DITHER_TPDF 1
#define RC_DITHER_TPDF_HP 2
int rc_engine_set_output_dither(rc_engine *e, uint32_t mode, uint64_t seed);
/* Band-limited resampling of the result by a rational step: fractional pitch and a change of the output's sample rate.
 * `-p/--pitch_multiple` moves the pitch by octaves only and, for p > 1, drops samples with no filter in front
 * (src/resampler.rs:15-18). With a resampler, pitch by a ratio r is the classic construction: an engine created with
 * factor * r, then a step of r input frames per output frame - the duration stays factor * L and every frequency is
 * multiplied by r; a change of sample rate is the step rate_in / rate_out; the two compose into one ratio. The step is
 * engine state, set once, like the fade, the channel map and the dither:
 *   num / den  the step, the input frames advanced per output frame. The setter reduces it by the gcd. num == den clears
 *              it, 0 / 0 clears it too; cleared is the state after rc_engine_create.
 *   RC_EINVAL  a null engine, exactly one of the two zero, reduced den > 1024, num > 8 * den or den > 8 * num. The previous
 *              state stays.
 * The definition. x[c][k], k in [0, n), is the engine's planar f32 result - what rc_engine_stretch_host gives with no
 * step set - and zero outside [0, n). Z = 32, beta = 9, roll-off 0.9, num / den reduced:
 *   s = min(1, den / num);  c = 0.9 * s;  W = Z where num <= den, else ceil(Z * num / den);  T = 2 W taps
 *   n_rs = 0 for n = 0, else floor((n * den - 1) / num) + 1: the m with m * num / den < n      (rc_resample_len)
 *   for output frame m, in 64-bit integers:  q = floor(m * num / den);  p = (m * num) mod den;  k0 = q - (W - 1)
 *   table row p, tap j in [0, T):  u = j - (W - 1) - p / den;
 *       h[p][j] = c * sinc(c u) * I0(beta * sqrt(1 - (u / W)^2)) / I0(beta)  for |u| < W, else 0;  sinc(v) = sin(pi v) / (pi v)
 *       computed in f64 on the host and rounded once to f32                                      (rc_resample_table)
 *   y[c][m] = sum over j of h[p][j] * x[c][k0 + j] in f32: ONE chain acc = fmaf(h[p][j], x[c][k0 + j], acc) from +0 with j
 *       ascending. The order depends on (p, j) alone: a sample's bits do not depend on which tile, launch or pipeline
 *       chunk computed it.
 * The filter (the f32 table, for steps from 1/8 to 8): within +-0.00025 dB of 1 up to 0.8 * s of the input's Nyquist
 * frequency, at least 91 dB down from s * Nyquist upward, every row sums to 1 within 8e-6, sum over j of |h[p][j]| <= 2.24.
 * y takes the place of x in everything downstream, and all of it counts resampled frames: the positions of the output
 * fade, the peak and the gain of rc_engine_stretch_frames_norm, the dither's frame counter, the count of clipped
 * samples, out_cap / out_cap_frames (RC_ECAPACITY below n_rs) and *out_len / *out_frames_len.
 * Reach: the four whole-job host-form entries, as the fade - rc_engine_stretch_host, rc_engine_stretch_frames, _pcm and
 * _norm, under a host frequency kernel as well. The device-form entries (rc_engine_stretch_device,
 * rc_engine_stretch_device_range), the streaming seam (rc_engine_next_window ...) and rc_multi IGNORE it: they return
 * what they return without it. With the state cleared every byte of every entry is what it is without this entry.
 * rc_offline_output_len stays the length of x: a caller sizes a resampled output with rc_resample_len of it. */
int rc_engine_set_output_resample(rc_engine *e, uint32_t num, uint32_t den);
/* Pure host helpers of the resampler: no device is touched.
 * rc_resample_len: n_rs as stated above for rows of n frames (0 where num or den is 0).
 * rc_resample_table: the table the engine uploads for num / den, *phases = the reduced den rows of *taps = T floats each,
 *   row p at table[p * T]. RC_EINVAL for a step the setter refuses (num == den is the step 1 here) or a null size
 *   pointer; RC_ECAPACITY where cap < den * T floats, the sizes still stored; table == NULL returns the sizes only.
 * rc_resample_ratio: the best rational num / den of `step` with den <= 1024 (continued fractions on the exact value of
 *   the f32: its 6e-8 is 1e-4 cents), inside the setter's limits. RC_EINVAL for a step outside [1/8, 8] or not finite, or
 *   a null pointer; *num and *den are then left as they were. */
size_t rc_resample_len(size_t n, uint32_t num, uint32_t den);
int rc_resample_table(uint32_t num, uint32_t den, float *table, size_t cap, uint32_t *phases, uint32_t *taps);
int rc_resample_ratio(float step, uint32_t *num, uint32_t *den);
/* A look-ahead peak limiter in front of the PCM quantiser: the third answer to an over, beside the quantiser's hard clip
 * (*clipped) and rc_engine_stretch_frames_norm's one gain for the whole file. It turns the gain down smoothly around an
 * over and leaves every other frame bit for bit as it was. The offline form is fully parallel - a sliding-window minimum
 * of the required gain followed by a sliding-window mean - and with the gain in fixed point both are integer operations:
 * the result does not depend on evaluation order, tiling or chunking. The limiter is engine state, set once, like the
 * fade, the map, the dither and the step:
 *   ceiling == 0.0f clears it, whatever the other arguments are; cleared is the state after rc_engine_create.
 *   RC_EINVAL  otherwise: a null engine, a drive that is not finite or not > 0, a ceiling that is not finite or not > 0,
 *              lookahead > RC_LIMITER_MAX_LOOKAHEAD. The previous state stays.
 * The definition, bit for bit. x[c][t], t in [0, n), is the planar f32 result behind the resampler, where one is set, and
 * behind the fade. L = lookahead, T = 2 L + 1, ONE = 2^24. Every float step is ONE correctly rounded IEEE f32 operation,
 * not contracted with its neighbours:
 *   v[c][t] = x[c][t] * drive
 *   a[t]    the largest |v[c][t]| over the channels c whose |v| is < inf: NaN and +-inf are skipped, as the normaliser's
 *           peak skips them; 0 where no channel qualifies. The limiter is channel-linked: one gain per frame.
 *   r[t]    ceiling / a[t] where a[t] > ceiling, else 1.0f
 *   rq[t]   (uint32_t)(r[t] * 16777216.0f): the product is exact, the conversion truncates, rq lies in [0, ONE]. For t
 *           outside [0, n), rq[t] = ONE.
 *   m[u]    the minimum of rq[t] over |t - u| <= L, for u in [-L, n + L)
 *   S[t]    the sum of m[u] over |u - t| <= L, as a 64-bit integer: exact and below 2^37
 *   g[t]    (float)S[t] / (float)(T * ONE): S converted to f32 with round to nearest even, T * ONE exact in f32, ONE f32
 *           division. g == 1.0f whenever S == T * ONE.
 *   y       v[c][t] * g[t]; then y > ceiling gives ceiling, y < -ceiling gives -ceiling, otherwise y stays, and a NaN stays
 *           a NaN. (The roundings of r, g and the product can leave y one ulp above ceiling: the clamp matters.)
 * Consequences: each over at frame u0 pulls a triangular notch into the gain, centred on u0, which reaches r[u0] there and
 * is 1 again from 2 L + 1 frames away; g[t] depends on the frames [t - 2 L, t + 2 L] alone; with drive == 1 every non-NaN
 * sample with S[t] == T * ONE leaves with the bits it came with; L == 0 is a per-frame gain with no ramp.
 * y takes the place of x in everything downstream: the peak and the gain of rc_engine_stretch_frames_norm, the dither, the
 * quantiser, the count of clipped samples, the f32 frames and rows.
 * Reach: the four whole-job host-form entries, as the fade and the resampler - rc_engine_stretch_host,
 * rc_engine_stretch_frames, _pcm and _norm, under a host frequency kernel as well. The device forms, the streaming seam,
 * rc_multi, rc_engine_frames_power and rc_engine_frames_channel_peaks IGNORE it. Cleared, every byte of every entry is
 * what it is without this entry. A limited job holds one more row buffer of channels x n floats on the device (the fused
 * kernel needs no scratch beyond it).
 * rc_engine_last_limiter_stats reports on the last call of one of the four entries that ran with a limiter set (those
 * calls block: nothing is pending when it is read):
 *   *min_gain        the smallest g[t]; 1.0f for a job of no frames, and 1.0f where no such call has run
 *   *limited_frames  the number of frames with S[t] < T * ONE
 * Either pointer may be NULL; a null engine is RC_EINVAL. Both values are order-free: a minimum of non-negative float bits
 * and a count. */
#define RC_LIMITER_MAX_LOOKAHEAD 2048
int rc_engine_set_output_limiter(rc_engine *e, float drive, float ceiling, uint32_t lookahead);
int rc_engine_last_limiter_stats(rc_engine *e, float *min_gain, uint64_t *limited_frames);
/* The reference's autocrop (src/recorder.rs:146-191, applied to a recording in front of `-s/-d`, src/main.rs:173-181):
 * the peak of every bin of a block of frames, measured on the device on the raw block, and the crop points those peaks
 * give. Three entries; a caller cuts by pointer arithmetic - the frames entries above take frames at any byte alignment.
 *
 * rc_frames_power_bins: ceil(n_frames / bin_frames), the number of bins; 0 for bin_frames == 0. Pure host code.
 *
 * rc_engine_frames_power: chunked_audio_power (src/recorder.rs:94-113) on a block of n_frames frames of
 * rc_config::channels channels in `format` (RC_PCM_*), at any byte alignment, as rc_engine_stretch_frames takes them. It
 * returns LINEAR peaks, not decibels. The definition, bit for bit:
 *   bin b    the frames [b * bin_frames, min((b + 1) * bin_frames, n_frames)), every channel; n_bins = ceil(n_frames /
 *            bin_frames).
 *   x        the reader's float of a sample, as stated for rc_engine_stretch_frames: (float)n / K, ONE correctly rounded
 *            f32 division; RC_PCM_F32: the bits as they are.
 *   peak[b]  the largest |x| over the bin's samples. NaN samples are skipped (the reference's partial_cmp().unwrap()
 *            panics on one); +-inf counts and gives +inf; -0.0 is 0; denormals are kept. A bin of nothing but zeros or
 *            NaN gives +0.0f.
 * The block is uploaded in chunks and the kernel of a chunk runs under the upload of the next; page-locked memory
 * (rc_host_alloc) is the DMA's source itself. The call blocks. It reads the engine's configuration (channels, device)
 * and nothing else: the output fade, a loaded device kernel, the streaming state and the kernel-time ring are left as they
 * were, and a stretch call behind it gives what it gave before. *n_bins is set whenever the arguments up to bin_frames
 * are valid.
 *   RC_EINVAL     a null pointer (`frames` may be null with n_frames == 0), a format outside 1 ... 5, bin_frames == 0
 *   RC_ECAPACITY  bin_cap < n_bins (*n_bins is set)
 *   n_frames == 0 is valid and gives *n_bins = 0.  On any error nothing behind bin_peak is written.
 *
 * rc_autocrop_points: determine_noise_threshold + determine_autocrop_points (src/recorder.rs:165-191) on those peaks, the
 * reference as it stands. Pure host code: no device is touched, and it may be called from any thread.
 *   dB[b]      max(log10f(|peak[b]|) * 20.0f, -99999999.0f) (power::relative_decibels, src/power.rs:6-8); the
 *              comparisons below run on these values.
 *   threshold  the value at index floor((float)percentile / 100.0f * (float)n_bins), computed in f32, of the sorted dB.
 *   *start     the first frame of the first bin with dB > threshold.
 *   *end       the first frame of the bin BEHIND the last bin with dB > threshold; where that last bin is the job's last
 *              bin, its own first frame: the reference's `(last + 1).min(len - 1)`, reproduced, not mended.
 *   The frames [*start, *end) are what remains. No bin above the threshold is the reference's None: *found = 0,
 *   *start = 0, *end = n_frames, RC_OK. Otherwise *found = 1.
 *   RC_EINVAL where the reference panics or asserts: a null pointer, n_bins == 0, percentile >= 100 or an index behind
 *   the last bin, a NaN peak, bin_frames == 0, n_bins != rc_frames_power_bins(n_frames, bin_frames).
 * Deviation: the reference converts its crop points to a Duration of f32 seconds and back (src/recorder.rs:155-162,
 * src/audio.rs:132-138), which can move them by a frame in a long recording; this interface returns frames, and its
 * callers cut at exactly those frames. */
size_t rc_frames_power_bins(size_t n_frames, uint64_t bin_frames);
int rc_engine_frames_power(rc_engine *e, const void *frames, size_t n_frames, uint32_t format, uint64_t bin_frames,
                           float *bin_peak, size_t bin_cap, size_t *n_bins);
int rc_autocrop_points(const float *bin_peak, size_t n_bins, uint64_t bin_frames, size_t n_frames, uint32_t percentile,
                       uint64_t *start, uint64_t *end, int *found);
/* The reference's channel treatment of its input on the frames path: Audio::rotate_channels (src/audio.rs:73-75), any
 * other permutation or copy of channels, and recorder::auto_split_mono (src/recorder.rs:118-144). Three entries.
 *
 * rc_engine_set_channel_map: which channel of the frame block each row of a frames job reads. The map is engine state, set
 * once, like the output fade: map == NULL or n == 0 clears it, and that is the state after rc_engine_create. Otherwise n
 * must equal rc_config::channels and every map[c] < channels: if not, RC_EINVAL, and the previous map stays. While a map
 * is set, row c of the job reads channel map[c] of the block; a source channel may feed several rows, or none. It
 * applies to rc_engine_stretch_frames, rc_engine_stretch_frames_pcm and rc_engine_stretch_frames_norm, the path those
 * three take under a host frequency kernel (rc_config::kernel) included. The definition, one sentence: the entry
 * returns exactly what it returns, with no map set, on the block whose frame f holds at channel c the sample
 * (f, map[c]) of the given block - every output byte in every output format, *clipped, *peak and *gain, with the fade
 * and a loaded user or curated device kernel downstream as before. The block still holds `channels` samples per frame,
 * and nothing in it is written. An identity map gives what no map gives (the engine takes the unmapped launches for it).
 * The rotation of `--rotate-channels` is map[c] = (c + channels - 1) % channels (rotate_right(1); stereo: {1, 0}).
 * The map does NOT apply to rc_engine_stretch_host (a caller permutes its row pointers itself), to the device forms, to
 * the streaming seam, to rc_multi, to rc_engine_frames_power or to rc_engine_frames_channel_peaks: they read what they
 * read, map set or not. For rc_engine_frames_power that is still the reference's result: a bin's peak is the maximum over
 * all channels, which no permutation changes and which copying the loudest channel over silent ones does not change
 * either, so autocropping the raw block equals autocropping after auto_split_mono.
 *
 * rc_engine_frames_channel_peaks: the measurement behind `channel_data.iter().all(|s| *s == 0.0)` (src/recorder.rs:122),
 * on the raw block of n_frames frames of rc_config::channels channels in `format` (RC_PCM_*), at any byte alignment, as
 * rc_engine_stretch_frames takes them. The definition, bit for bit:
 *   x             the reader's float of a sample, as stated for rc_engine_stretch_frames: (float)n / K, ONE correctly
 *                 rounded f32 division; RC_PCM_F32: the bits as they are.
 *   chan_peak[c]  for c < channels, the float whose bits are the unsigned maximum of the bits of |x| (the sign bit
 *                 cleared) over the samples of channel c.
 * So a NaN sample wins over everything - deliberately, and unlike the bin peaks of rc_engine_frames_power, which skip
 * NaN: in the reference `NaN == 0.0` is false, and such a channel is not silent. Otherwise +-inf gives +inf; otherwise
 * the result is the largest finite magnitude. Denormals are kept; -0.0 gives +0.0. chan_peak[c] == 0.0f exactly when the
 * reference's test holds for channel c. n_frames == 0 is valid and gives +0.0f for every channel.
 *   RC_EINVAL     a null pointer (`frames` may be null with n_frames == 0), a format outside 1 ... 5
 *   RC_ECAPACITY  cap < channels
 *   On any error nothing behind chan_peak is written.
 * The call blocks. Like rc_engine_frames_power it leaves the engine as it was: the output fade, a loaded device kernel,
 * the streaming state, the kernel-time ring and the channel map itself are untouched. It is chunked like
 * rc_engine_frames_power: the kernel of a chunk runs under the upload of the next, and page-locked memory (rc_host_alloc)
 * is the DMA's source itself.
 *
 * rc_split_mono_map: the decision of auto_split_mono (src/recorder.rs:118-144) as it stands, on those peaks. Pure host
 * code: no device is touched, and it may be called from any thread. Channel c is empty where chan_peak[c] == 0.0f (a NaN
 * peak is not empty). Where exactly channels - 1 channels are empty and one is not - the reference's
 * last_nonempty_channel, m - map[c] = m for every c and *found = 1; that includes channels == 1 with a non-silent
 * channel, where the reference's condition holds too and the map is the identity. Otherwise the identity map and
 * *found = 0. RC_EINVAL: a null pointer, or channels == 0. `map` holds `channels` words; it is what
 * rc_engine_set_channel_map takes. */
int rc_engine_set_channel_map(rc_engine *e, const uint32_t *map, uint32_t n);
int rc_engine_frames_channel_peaks(rc_engine *e, const void *frames, size_t n_frames, uint32_t format, float *chan_peak,
                                   size_t cap);
int rc_split_mono_map(const float *chan_peak, uint32_t channels, uint32_t *map, int *found);
/* Page-locked host memory for the host-form calls (the `Vec<f32>` a Rust host would otherwise hand over, src/main.rs:
 * 148, src/audio.rs:152-172): rows allocated here cross PCIe without a staging copy. rc_host_free(NULL) is a no-op.
 * RC_ENODEVICE without a GPU, RC_ENOMEM when the pages cannot be locked. */
int rc_host_alloc(size_t bytes, void **out);
int rc_host_free(void *p);
/* Same job on DEVICE-resident buffers (channel c at base + c*stride, strides in floats).
 * `hip_stream` is a hipStream_t (NULL = the engine's own stream); the call is asynchronous
 * on that stream unless a user kernel is configured. The engine's scratch (tail copy, seam stash,
 * pipeline buffers) is per handle: a call on a different stream than the previous one first waits
 * (on the device) for that call's last enqueue, so back-to-back calls never overlap on the GPU.
 *
 * The caller's buffers (this entry, rc_engine_stretch_device_range and rc_multi_stretch_device alike; held by
 * tests/test_gpu_caller_buffers.py on every kernel path):
 *   - d_in and d_out need float (4-byte) alignment and no more; the result does not depend on the alignment.
 *   - any stride of at least the row length: in_stride >= in_len, out_stride >= win_count * window_out_len (the
 *     whole job: rc_offline_output_len). Strides may be odd; one channel ignores them.
 *   - nothing outside [d_in + c * in_stride, + in_len) is read: hops that run past the end of a row read zeros
 *     from the engine's own padded copy of its tail, never d_in[in_len].
 *   - nothing outside [d_out + c * out_stride, + win_count * window_out_len) is written, whatever out_cap is.
 * The result's bits are those of the same job in contiguous, aligned rows. */
int rc_engine_stretch_device(rc_engine *e, const float *d_in, size_t in_stride, size_t in_len,
                             float *d_out, size_t out_stride, size_t out_cap, size_t *out_len,
                             void *hip_stream);
/* Sharded form for multi-GPU runs: only channels [ch_first, ch_first+ch_count) and output
 * windows [win_first, win_first+win_count) of the same job; written at d_out offset 0.
 * Hops are independent given the phase source, the one-hop overlap is recomputed locally.
 * d_in and in_stride are the whole job's (channel c at d_in + c * in_stride, in_len its length); row i of the range is
 * written at d_out + i * out_stride. The caller's buffers as for rc_engine_stretch_device, and of each row of the
 * range only the span its hops cover is read - with hpw = hops_per_window and step = sample_step_len of rc_params,
 *     [max(0, win_first * hpw - 1) * step, min(in_len, ((win_first + win_count) * hpw - 1) * step + window_len)),
 * the hops of the range and the one in front of them (plus RC_HISTORY hops more in front where a loaded user device
 * kernel declares a history; every channel's span where it declares RC_CROSS_CHANNEL). The rest of the rows, and the
 * rows of channels outside the range, need not hold samples. A host frequency kernel (rc_config.kernel) carries its
 * tail instead: no hop is recomputed. */
int rc_engine_stretch_device_range(rc_engine *e, const float *d_in, size_t in_stride,
                                   size_t in_len, uint32_t ch_first, uint32_t ch_count,
                                   uint64_t win_first, uint64_t win_count, float *d_out,
                                   size_t out_stride, size_t out_cap, void *hip_stream);

/* Blocks until everything the engine queued on ITS OWN stream has finished (calls that were given
 * a caller stream are ordered by that stream instead). Like every entry point that touches the
 * device it returns RC_EHIP, once, if an earlier launch left a device error word (a run-seam wait of
 * the window-16384 kernel that expired: the affected output samples were not written). */
int rc_engine_synchronize(rc_engine *e);

/* ---- measurement ---------------------------------------------------------------------- */
/* HIP-event time (ms) and hop count of the hop kernel launches of the last offline call;
 * synchronises on the events. */
int rc_engine_last_kernel_stats(rc_engine *e, float *kernel_ms, uint64_t *hops,
                                uint32_t *launches);
/* The same event time for each of the last min(cap, 64) offline calls, oldest first (a bench runs K
 * calls back to back and reads K kernel durations afterwards); synchronises on the newest. */
int rc_engine_kernel_times(rc_engine *e, float *ms, size_t cap, size_t *n_out);

/* ---- single-hop entry points (ReFFT seam, used by parity tests) ----------------------- */
/* ReFFT::forward_fft (src/fft.rs:50-61): host samples[window_len] -> host spectrum (re,im)*N */
int rc_engine_forward_fft(rc_engine *e, const float *samples, float *out_reim);
/* ReFFT::resynth (src/fft.rs:42-48) for hop `hop` of `channel` (phase key), no overlap-add:
 * host samples[window_len] -> host out[window_len]. Applies the user kernel if configured. A single frame has no
 * earlier one and no other channel: a user device kernel reads (0, 0) from every X.past(d > 0) and from every
 * X.channel(c != channel) here, whatever it declares. */
int rc_engine_resynth(rc_engine *e, uint32_t channel, uint64_t hop, const float *samples,
                      float *out);

/* ---- user device kernels: a frequency kernel written in HIP, compiled at run time ----------------------------
 * The GPU-resident form of the reference's hot-swapped apply() (README.md "Live coding", src/fft.rs:76-108,
 * src/hotswapper.rs). The user's source defines one function,
 *   __device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h);   returns Y[j]
 * which runs for every output bin j of every hop between the forward transform and the resynthesis, on the device:
 *   X         the hop's N-bin spectrum in natural DFT order, read-only; X[i] is X[i mod N] for ANY integer i
 *   h.n       N;  h.channel, h.hop: the channel and hop index k (the k of rc_phase_key)
 *   h.time_ms rc_config::kernel_time_ms when non-zero, else the wall clock when the launch was enqueued: one value per
 *             launch, not per hop (the reference reads the clock per hop)
 *   h.param(i) the i-th of up to 16 float params (rc_*_set_device_kernel_params), 0 past n_params
 * History. A source that says `#define RC_HISTORY D` (D = 0 ... RC_DK_MAX_HISTORY = 8; absent = 0) in front of rc_apply
 * may also read the ANALYSIS spectra of the D hops before its own, as a stateful apply() of the reference keeps them:
 *   X.past(d)  hop h.hop - d of the same channel, an rc_spectrum like X (read-only, the same modulo-N indexing);
 *              X.past(0) is X. Every bin reads (0, 0) where d > RC_HISTORY and where h.hop - d < 0: silence precedes a
 *              stream (src/stretcher.rs:58-59), and a stateful kernel has seen no call before hop 0.
 *   h.history  the declared D
 * No d and no index leaves the launch's spectrum block. A larger D does not compile (the error names RC_HISTORY). Earlier
 * OUTPUTS are read through X.out(d) (Feedback, below). The depth travels inside the code object (the size of its symbol
 * rc_user_dk_history is D + 1), so loading needs no further argument; a code object without that symbol runs as D = 0.
 * Every range, streaming batch and rc_multi shard recomputes the D spectra in front of it from the input, so all entry
 * points equal the offline job; an open stream retains RC_DK_MAX_HISTORY + 1 steps of input behind its next hop, so
 * that a kernel swapped in mid-stream sees the same past.
 * Other channels. A source that says `#define RC_CROSS_CHANNEL 1` in front of rc_apply (absent or 0: off; any other
 * value does not compile, the error names RC_CROSS_CHANNEL) may also read the ANALYSIS spectra of every channel of the
 * job, as a stateful apply() served by the processor's round-robin sees its siblings (src/stretcher_processor.rs:63-70):
 *   X.channel(c)  hop h.hop of channel c, an rc_spectrum like X; X.channel(h.channel) is X, declared or not. Every bin
 *                 reads (0, 0) where c >= h.channels and, for another channel, where the source did not declare
 *                 RC_CROSS_CHANNEL. It composes with the history: X.channel(c).past(d) and X.past(d).channel(c) are both
 *                 hop h.hop - d of channel c, with the zero rules of past().
 *   h.channels    rc_config::channels under the declaration, 0 without it (the unchanged 128-byte argument block of an
 *                 undeclared kernel has no room for it)
 * No c leaves the launch's spectrum block. The declaration travels inside the code object (the symbol
 * rc_user_dk_channels); one without it runs as undeclared, with the argument block, launches and scratch it always had.
 * While a declared kernel is loaded, a call for part of the channels (a range, an rc_multi shard) still runs the forward
 * transforms of ALL channels over its hops and holds their spectra, up to rc_config::channels times the analysis work
 * and spectrum scratch of the asked part; a whole-job call analyses every channel anyway. d_in of the range form holds
 * every channel already; rc_multi sends every channel's input span to each shard. Streams, whose channels need not be
 * equally long or equally far:
 *   - hop k of a CLOSED channel reads zeros past its end (src/stretcher.rs:129-132), also when another channel reads it;
 *   - rc_engine_next_window(c) returns RC_WOULD_BLOCK unless every channel that is still OPEN holds the input of all
 *     hops of that window;
 *   - every channel's input is kept back to what the SLOWEST unfinished channel's next hop can still read (its next hop
 *     - 1 - RC_DK_MAX_HISTORY): a host that pulls one channel far ahead of another holds that much more input, as the
 *     reference's unbounded input channel would (src/main.rs:133);
 *   - a declared kernel is loaded on a stream only while all channels stand at the same next window (before the first
 *     window, or between rounds of the processor's loop): else RC_EINVAL, and the previous kernel stays;
 *   - channels that are all closed, equally long and at the same window are computed together and need no extra analysis.
 * With these rules every entry point equals the offline job bit for bit.
 * Whole-hop sums. A source that says `#define RC_SUMS S` in front of rc_apply (S = 1 ... RC_DK_MAX_SUMS = 4; absent or 0:
 * none; any other value does not compile, the error names RC_SUMS) also defines
 *   __device__ float rc_sum_term(const rc_spectrum &X, uint32_t j, const rc_hop &h, uint32_t i);   the term of sum i at bin j
 * and rc_apply may read hop-wide quantities that are computed once per hop, not once per bin (energy, mean magnitude,
 * centroid: what the reference's apply() forms from the whole Vec it is handed):
 *   X.sum(i)   the sum over j = 0 ... N - 1 of rc_sum_term(X', j, h', i), where X' and h' are the hop that this rc_spectrum
 *              stands for: X.past(d).sum(i) and X.channel(c).sum(i) are the sums of that hop of that channel, in either
 *              order of past() and channel().
 * Inside rc_sum_term the spectrum is that hop alone: X.past(d > 0) and X.channel(c != own) read (0, 0), X.sum(..) reads 0,
 * h.hop and h.channel are those of the hop being summed, and h.param, h.time_ms, h.history and h.channels are as in
 * rc_apply. A declared source without rc_sum_term does not compile (the compiler's error names rc_sum_term).
 * Zero rules: X.sum(i) is 0.f where i >= S; where the source did not declare RC_SUMS (the call still compiles, as
 * channel() does for an undeclared kernel); and for every spectrum that reads (0, 0) by the rules of past() and
 * channel() - a hop before the stream, a hop beyond the declared history, a channel outside the block, the single
 * frame's other channels - whatever rc_sum_term would return on zeros.
 * The arithmetic is fixed: each term is a float; lane t of 256 adds the terms of bins t, t + 256, ... ascending in
 * double; the 256 partials are combined in one fixed tree (shuffles within a wave, then the four wave partials in wave
 * order), and the result is rounded to float once. NaN and Inf propagate as that arithmetic gives. The order depends on
 * N alone, so the bits of a sum do not depend on the launch, chunk, range, stream batch or shard that computed it, and
 * every entry point still equals the offline job bit for bit. (Two code objects of one source from two builds of the
 * compiler may differ in how they round sqrtf and the like; that is outside this guarantee, which is about one code object.)
 * S travels inside the code object (the size of its symbol rc_user_dk_sums is S + 1; the symbol is absent when S = 0),
 * next to a second kernel, rc_user_dk_sums_pass: in front of every launch of rc_user_dk the engine runs it on the same
 * stream, one workgroup per row of the launch's input block (the history's halo rows and, under RC_CROSS_CHANNEL, the
 * channels analysed only included), into a scratch of rows x S floats. It reads every spectrum of the block once. A code
 * object without the symbol takes the argument block, the launches and the scratch it always had.
 * Feedback. A source that says `#define RC_FEEDBACK F` in front of rc_apply (F = 1 ... RC_DK_MAX_FEEDBACK = 4; absent or 0:
 * none; any other value does not compile, the error names RC_FEEDBACK) may also read its own earlier OUTPUTS, the static
 * state a reference apply() keeps between calls (peak hold with a release, freeze, one-pole smoothing, feedback delays):
 *   X.out(d)    the spectrum rc_apply returned for hop h.hop - d of the same channel, an rc_spectrum (read-only, the same
 *               modulo-N indexing)
 *   h.feedback  the declared F
 * X.out(d) reads (0, 0) where d == 0; where d > F; where h.hop - d < 0; where hop h.hop - d lies before the first hop this
 * kernel ran since it was loaded, or since its channel last restarted at hop 0 (a freshly swapped-in reference library
 * starts from fresh statics); where the source did not declare RC_FEEDBACK (the call still compiles); in
 * rc_engine_resynth (a single frame); inside rc_sum_term; and for X.channel(c).out(d) and X.past(p).out(d) with c another
 * channel or p > 0: out() belongs to rc_apply's own X. An out spectrum is bins only: its past(), channel() and out() read
 * (0, 0) and its sum() reads 0. X.out(d) composes with RC_HISTORY, RC_CROSS_CHANNEL and RC_SUMS on X itself.
 * Such a kernel is SEQUENTIAL, as rc_config::kernel is: the hops of a channel run in order, once each. Per channel, a call
 * that starts at hop k0 is one of
 *   - a restart, k0 == 0: the state and the overlap tail are zeroed;
 *   - a continuation, k0 == the hop behind the channel's previous call: the overlap tail is carried on the device, hop
 *     k0 - 1 is not computed again;
 *   - the first call since the kernel was loaded, k0 > 0 (a hot swap into a running stream): the state is zeroed and hop
 *     k0 - 1 runs once for its overlap tail, as the hop in front of every range start does. It sees zero state, and its
 *     output enters the state: it is X.out(1) of hop k0;
 *   - anything else: RC_EINVAL, the message names the hop expected, state and tail stay as they were, and the in-order
 *     call still succeeds afterwards.
 * A call whose channels fall into different cases is RC_EINVAL. A call that fails after it began leaves only a restart at
 * hop 0 acceptable, as for a host kernel. The whole-job entries start at hop 0 and run their chunks in order; consecutive
 * rc_engine_stretch_device_range calls and the streaming seam (open or closed, look-ahead batches included; the channels
 * may stand at different windows) continue. rc_multi_load_device_kernel returns RC_EUNSUPPORTED for such a kernel and
 * keeps the one it runs: a job cut over devices cannot promise the order. With these rules every entry point equals the
 * offline job bit for bit.
 * F travels inside the code object (the size of its symbol rc_user_dk_feedback is F + 1; the symbol is absent when F = 0;
 * a size outside 2 ... 5 is refused). The state, rc_config::channels x (F + 1) rows of N float2 in device memory (row =
 * hop mod (F + 1), so that no hop writes a row it may read), is reserved by rc_engine_load_device_kernel - RC_ENOMEM
 * there, not mid-job - and freed with the module. The kernel writes every Y[j] to the spectrum block, as any user kernel
 * does, and to its ring row. Nothing waits on the device: the hops of a chunk are one launch each, ordered by the stream,
 * or, at N <= 1024, one launch of one workgroup per channel that walks the chunk's hops with a barrier between them. Both
 * give the same bits. A feedback kernel is therefore bound by one launch, or one barrier round, per hop (DESIGN 6,
 * "Feedback", has the measured cost); rc_engine_last_kernel_stats counts the launches made. A code object without the
 * symbol takes the argument block, the launches and the scratch it always had.
 * The engine owns the prelude that defines rc_spectrum / rc_hop and the wrapper kernel rc_user_dk; rc_apply writes only
 * its return value and must terminate (a kernel cannot be preempted). Compiled with --offload-arch=gfx950 -O3 -std=c++17,
 * no fast-math. Diagnostics name rc_user_dk.hip:<line>, or the file a leading `#line 1 "name"` line names. A user device
 * kernel excludes rc_config::kernel and rc_config::device_kernel. Compiling and loading are separate steps, as the
 * reference compiles on its watcher thread and loads on the DSP thread (src/hotswapper.rs:19-30, src/fft.rs:78). */
/* Pure host, no device, thread-safe: HIP source -> gfx950 code object. *code_len is always set (code NULL: a size
 * query, RC_ECAPACITY). RC_ECAPACITY: code_cap too small; RC_EINVAL: the source does not compile or defines no rc_apply
 * (the compiler log in `log`, NUL-terminated and cut to log_cap; its first error line in rc_last_error());
 * RC_EUNSUPPORTED: hiprtc cannot be loaded. */
int rc_dk_compile(const char *src, size_t src_len, char *code, size_t code_cap, size_t *code_len,
                  char *log, size_t log_cap);
/* Loads a code object from rc_dk_compile; it runs from the next call on (code NULL: remove the kernel). The bytes are
 * checked first (ELF64, EM_AMDGPU, gfx950, an rc_user_dk symbol, markers in range, rc_user_dk_sums_pass where sums are
 * declared): RC_EINVAL, and the previous kernel stays, when they
 * fail; RC_EINVAL too when the engine has a host or curated kernel; RC_ENOMEM, and the previous kernel stays, when the
 * state of a kernel that declares RC_FEEDBACK cannot be reserved. A replaced module is unloaded only once every
 * launch that used it has completed, so a call already enqueued on a caller's stream finishes with the old kernel. */
int rc_engine_load_device_kernel(rc_engine *e, const char *code, size_t code_len);
/* Up to 16 float params (h.param(i)), passed by value with every launch: they take effect from the next call, with no
 * recompile. n_params > 16: RC_EINVAL. */
int rc_engine_set_device_kernel_params(rc_engine *e, const float *params, uint32_t n_params);

/* ---- one process, several GPUs of one node ---------------------------------------------------
 * The reference builds every channel's Stretcher in one process (src/main.rs:133-155) and one thread walks them
 * (src/stretcher_processor.rs:56-71). rc_multi is that job cut over a LIST of devices behind the same C-ABI: one
 * engine and one host thread per listed device, the channel-major sequence of output windows cut into one contiguous
 * piece per device (rc_shard_plan: SURVEY 8 e1's (channel, window range) units; the hop before a piece is
 * recomputed locally, no data-path collective), and every shard's output copied ONCE, straight into its place in the
 * caller's layout (device form: hipMemcpyPeerAsync into the root device's tensor; host form: device -> the caller's
 * arrays). A host frequency kernel (rc_config::kernel) is RC_EUNSUPPORTED here: a stateful apply() sees its
 * channel's hops in order, which a cut job cannot promise; the curated and user device kernels work, except a user
 * device kernel that declares RC_FEEDBACK (rc_multi_load_device_kernel: RC_EUNSUPPORTED, for the same reason). rc_config::device is
 * ignored. A device may be listed more than once (then its engines share it). Threading as for an engine: one thread
 * at a time per rc_multi handle; the handle owns one persistent worker thread per listed device beyond the first (created
 * by rc_multi_create, joined by rc_multi_destroy), and the calling thread's current HIP device is restored on return. */
typedef struct rc_shard {
    uint32_t device_index;        /* index into the device list */
    uint32_t ch_first, ch_count;  /* part of ONE channel, or a block of WHOLE channels */
    uint64_t win_first, win_count;
} rc_shard;
/* Pure host: the plan for `channels` x `total_windows` windows over `n_devices`; writes up to `cap` shards, returns
 * how many the plan has (at most 3 per device). */
size_t rc_shard_plan(uint32_t channels, uint64_t total_windows, uint32_t n_devices, rc_shard *out, size_t cap);

typedef struct rc_multi rc_multi;
int rc_multi_create(const rc_config *cfg, const int32_t *device_ids, uint32_t n_devices, rc_multi **out);
void rc_multi_destroy(rc_multi *m);
uint32_t rc_multi_device_count(const rc_multi *m);
/* Diagnostic: in the device form a share that runs on the root's own device (the root itself, or the root device
 * listed again) reads and writes the caller's tensors in place. force != 0 makes such shares take the span-copy /
 * shard-copy path of a remote device as well, so that a one-GPU box exercises it. Default 0. */
int rc_multi_set_staging(rc_multi *m, int force);
/* rc_engine_stretch_host over all listed devices: each uploads the span of input its shards read and downloads
 * its shards into out[c]. Blocking. */
int rc_multi_stretch_host(rc_multi *m, const float *const *in, size_t in_len, float *const *out, size_t out_cap,
                          size_t *out_len);
/* rc_engine_stretch_device with input and output resident on device_ids[root] (channel c at base + c * stride,
 * strides in floats): the other devices fetch the input span they need from the root and deliver their shards into
 * d_out by peer copies. `hip_stream` (a hipStream_t of the root device, or NULL) is what produced d_in: it is
 * synchronised on entry. Blocking: d_out is complete on return. The caller's buffers as for rc_engine_stretch_device:
 * float alignment, any strides of at least the row lengths (RC_EINVAL for shorter ones where there are several
 * channels), nothing read outside the input rows, nothing written outside the first out_len floats of the output rows. */
int rc_multi_stretch_device(rc_multi *m, uint32_t root, const float *d_in, size_t in_stride, size_t in_len,
                            float *d_out, size_t out_stride, size_t out_cap, size_t *out_len, void *hip_stream);
/* rc_engine_load_device_kernel / _set_device_kernel_params on the engine of every listed device */
int rc_multi_load_device_kernel(rc_multi *m, const char *code, size_t code_len);
int rc_multi_set_device_kernel_params(rc_multi *m, const float *params, uint32_t n_params);

/* ---- measurement support -------------------------------------------------------------------
 * Box calibration for bench.py (boxes of one pool differ by several per cent on the same binary): runs a fixed
 * pure-VALU kernel (independent v_pk_fma_f32 chains, eight waves per SIMD, no memory traffic) `launches` times on
 * `hip_stream` of `device` and returns the mean duration of one launch in *ms_per_launch and the time one packed-FMA
 * wave instruction takes on one SIMD in *ns_per_inst. Not on the reference's path. */
int rc_calib_valu(int device, void *hip_stream, uint32_t launches, float *ms_per_launch, float *ns_per_inst);

/* ---- time maps: rc_engine_set_time_map, rc_time_map_output_len, rc_time_map_curve ------------ */
#include "rocoder_hip_timemap.h"

/* ---- output warp: rc_engine_set_output_warp, rc_warp_table, rc_warp_curve ---------------------- */
#include "rocoder_hip_warp.h"

/* ---- mix bus: rc_bus_*, rc_engine_mix_frames, rc_engine_bus_frames, rc_mix_envelope ------------ */
#include "rocoder_hip_mix.h"

/* ---- phase modes: rc_engine_set_phase_mode, rc_engine_get_phase_mode, rc_phase_envelope -------- */
#include "rocoder_hip_phase.h"

#ifdef __cplusplus
}
#endif
#endif
