// The prelude of a user device kernel (rc_dk_compile): hiprtc compiles it, then the user's source, then
// rc_user_dk_wrapper.hpp, as one translation unit for gfx950. rc_rtc.cpp embeds both files as text; the raw string
// below is the whole of what the user's code sees.
//
// The user writes one function,
//   __device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h);   // returns Y[j]
// X is one hop's N-bin spectrum in natural DFT order; every index is reduced modulo N, so no read leaves the hop, and
// the user gets no pointer to write through. rc_apply must terminate: the engine cannot preempt a kernel.
//
// A source that says `#define RC_HISTORY D` (0 ... RC_DK_MAX_HISTORY; absent = 0) may also read the analysis spectra of
// the D hops before its own: X.past(d) is hop h.hop - d of the same channel, an rc_spectrum like X. It reads (0, 0)
// where d > RC_HISTORY and where h.hop - d < 0 (silence precedes a stream). The wrapper records the depth in the code
// object as the size of the symbol rc_user_dk_history (D + 1 bytes), which is where the loader finds it.
//
// A source that says `#define RC_CROSS_CHANNEL 1` (absent or 0: off) may read the analysis spectra of the job's other
// channels: X.channel(c) is hop h.hop of channel c, an rc_spectrum like X, and composes with past() in either order.
// X.channel(h.channel) is X itself, declared or not. Every bin reads (0, 0) where c >= h.channels and, for another
// channel, where the source did not declare RC_CROSS_CHANNEL. h.channels is rc_config::channels under the declaration and
// 0 without it: the 128-byte argument block of an undeclared kernel is unchanged and has no room for it. The wrapper
// records the declaration as the symbol rc_user_dk_channels, which the loader looks for.
//
// A source that says `#define RC_SUMS S` (1 ... RC_DK_MAX_SUMS; absent or 0: none) also writes
//   __device__ float rc_sum_term(const rc_spectrum &X, uint32_t j, const rc_hop &h, uint32_t i);   // the term of sum i at bin j
// and rc_apply may read X.sum(i), the sum over j = 0 ... N - 1 of rc_sum_term(X', j, h', i), where X' and h' are the hop
// that this rc_spectrum stands for: X.past(d).sum(i) and X.channel(c).sum(i) are the sums of that hop of that channel,
// in either order of past() and channel(). Inside rc_sum_term the spectrum is that hop alone: X.past(d > 0) and
// X.channel(c != own) read (0, 0), X.sum(..) reads 0, h.hop and h.channel are those of the hop being summed, and
// h.param, h.time_ms, h.history and h.channels are as in rc_apply. Zero rules: X.sum(i) is 0.f where i >= S, where the
// source did not declare RC_SUMS (the call still compiles), and for every spectrum that reads (0, 0) by the rules of
// past() and channel() - a hop before the stream or beyond the declared history, a channel outside the block, a single
// frame's other channels - whatever rc_sum_term would return on zeros. The arithmetic: each term is a float; lane t of
// 256 adds the terms of bins t, t + 256, ... ascending in double; the 256 partials are combined in one fixed tree
// (shuffles within a wave, then the four wave partials in wave order) and the result is rounded to float once. NaN and
// Inf propagate as that arithmetic gives. The order depends on N alone, so the bits of a sum do not depend on the launch,
// chunk, range, stream batch or shard that computed it. The wrapper records S in the code object as the size of the
// symbol rc_user_dk_sums (S + 1 bytes, present only when S > 0), and adds the kernel rc_user_dk_sums_pass.
//
// A source that says `#define RC_FEEDBACK F` (1 ... RC_DK_MAX_FEEDBACK; absent or 0: none) may read its own earlier
// outputs: X.out(d) is the spectrum rc_apply returned for hop h.hop - d of the same channel, an rc_spectrum whose []
// takes any index modulo N; h.feedback is F. The engine keeps F + 1 rows of N bins per channel, addressed by hop mod
// (F + 1), and runs the hops of a channel in order (rc_engine_load_device_kernel states the order rule). X.out(d) reads
// (0, 0) where d == 0, where d > F, where h.hop - d < 0, where hop h.hop - d lies before the first hop this kernel ran
// since it was loaded or since its channel restarted at hop 0, where the source did not declare RC_FEEDBACK (the call
// still compiles), for a single frame (rc_engine_resynth), inside rc_sum_term, and for X.channel(c).out(d) and
// X.past(p).out(d) with c another channel or p > 0: out() belongs to X itself. An out spectrum is bins only: its
// past(), channel() and out() read (0, 0) and its sum() reads 0, whatever their argument. X.out(d) composes with
// RC_HISTORY, RC_CROSS_CHANNEL and RC_SUMS on X. The wrapper records F in the code object as the size of the symbol
// rc_user_dk_feedback (F + 1 bytes, present only when F > 0).
R"rc_prelude(
typedef __hip_internal::uint32_t uint32_t;
typedef __hip_internal::int32_t int32_t;
typedef __hip_internal::uint64_t uint64_t;
typedef __hip_internal::int64_t int64_t;

#define RC_DK_MAX_PARAMS 16u

// kernel argument block; the host mirror is rc::UserDkArgs (rc_rtc.h)
struct rc_dk_args {
    const float2 *in;    // [rows][n]
    float2 *out;         // [rows][n], never aliases `in`
    uint64_t row_first;  // first row of this launch (grid.y chunks)
    int64_t hop_first;   // row r is hop hop_first + r % hop_count of channel ch_first + r / hop_count
    uint64_t hop_count;
    uint64_t time_ms;
    uint32_t n, mask;    // mask = n - 1 for powers of two, else 0
    uint32_t ch_first, n_params;
    float params[RC_DK_MAX_PARAMS];
};

// One hop's spectrum, read-only. X[i] is X[i mod n] for any i.
struct rc_spectrum {
    const float2 *p_;
    uint32_t n;
    uint32_t mask_;
    __device__ float2 operator[](int64_t i) const {
        if (zero_) return make_float2(0.f, 0.f);
        if (mask_) return p_[(uint64_t)i & mask_];  // powers of two: two's complement makes this i mod n
        if ((uint64_t)i < n) return p_[i];
        int64_t r = i % (int64_t)n;
        if (r < 0) r += n;
        return p_[r];
    }
    // the spectrum d hops earlier in the same channel; past(0) is this one
    __device__ rc_spectrum past(uint32_t d) const {
        rc_spectrum s = *this;
        if (d) s.fb_n_ = 0;
        if (d > past_ || out_) {
            s.zero_ = true;
            s.past_ = 0;
        } else {
            s.p_ = p_ - (uint64_t)d * n;
            s.sums_ = sums_ - (uint64_t)d * n_sums_;
            s.past_ = past_ - d;
        }
        return s;
    }
    // the same hop of channel c of the job; channel(h.channel) is this one
    __device__ rc_spectrum channel(uint32_t c) const {
        rc_spectrum s = *this;
        if (out_) s.zero_ = true;
        if (c == ch_) return s;
        s.fb_n_ = 0;
        if (c - ch_lo_ >= ch_n_) {
            s.zero_ = true;
        } else {
            s.p_ = p_ + ((int64_t)c - (int64_t)ch_) * (int64_t)((uint64_t)ch_rows_ * n);
            s.sums_ = sums_ + ((int64_t)c - (int64_t)ch_) * (int64_t)((uint64_t)ch_rows_ * n_sums_);
            s.ch_ = c;
        }
        return s;
    }
    // sum i of this hop (RC_SUMS, rc_sum_term): 0.f where i >= RC_SUMS, without the declaration, and where this
    // spectrum reads (0, 0)
    __device__ float sum(uint32_t i) const { return (zero_ || i >= n_sums_) ? 0.f : sums_[i]; }
    // what rc_apply returned for the hop d before this one in the same channel (RC_FEEDBACK): (0, 0) where d == 0 or
    // d > RC_FEEDBACK, before hop 0 and before the kernel's first hop, without the declaration, and for any spectrum
    // but rc_apply's own X
    __device__ rc_spectrum out(uint32_t d) const {
        rc_spectrum s = *this;
        s.out_ = true;
        s.past_ = 0;
        s.ch_lo_ = ch_;
        s.ch_n_ = 1;
        s.sums_ = nullptr;
        s.n_sums_ = 0;
        s.fb_n_ = 0;
        if (zero_ || out_ || d == 0 || d > fb_n_ || d > fb_hop_) s.zero_ = true;
        else s.p_ = fb_ + ((fb_hop_ - d) % (uint64_t)(fb_n_ + 1u)) * n;
        return s;
    }
    uint32_t past_;  // rows in front of p_ that past() may reach
    bool zero_;      // a hop outside the declared history or before the stream, a channel outside the block: (0, 0)
    uint32_t ch_;            // the channel p_ belongs to
    uint32_t ch_lo_, ch_n_;  // channels [ch_lo_, ch_lo_ + ch_n_) lie in the block (undeclared: none but ch_)
    uint32_t ch_rows_;       // rows from one channel of the block to the next
    const float *sums_;      // the n_sums_ sums of the row p_ (rows of sums lie as the rows of spectra do)
    uint32_t n_sums_;        // the declared RC_SUMS; 0 without it and inside rc_sum_term
    // The channel's ring of earlier outputs, [fb_n_ + 1][n], row = hop mod (fb_n_ + 1). A plain pointer on purpose, never
    // __restrict__, __ldg or an invariant load: a wave-uniform index such as X.out(1)[0] could otherwise become a scalar
    // load, and a scalar load does not see the vector stores the previous hop of the same launch made to the ring.
    const float2 *fb_;
    uint64_t fb_hop_;        // the hop X stands for
    uint32_t fb_n_;          // hops out() may reach back: RC_FEEDBACK for rc_apply's X in a job, else 0
    bool out_;               // an out spectrum: bins only
};

// What the hop is: window length, channel, hop index k (the k of rc_phase_key), the launch's time and the params.
// time_ms is one value per launch (rc_config::kernel_time_ms, or the wall clock when the launch was enqueued).
struct rc_hop {
    uint32_t n;
    uint32_t channel;
    uint64_t hop;
    uint64_t time_ms;
    uint32_t n_params;
    uint32_t history;  // the declared RC_HISTORY
    uint32_t channels;  // rc_config::channels under RC_CROSS_CHANNEL, else 0
    uint32_t feedback;  // the declared RC_FEEDBACK
    const float *params_;
    __device__ float param(uint32_t i) const { return i < n_params ? params_[i] : 0.f; }
};

#define RC_DK_MAX_HISTORY 8

// the argument block of a kernel that declares a history (RC_HISTORY > 0; a kernel without one takes rc_dk_args as it
// is): `in` is then row 0 of [channel][halo + hop_count][n] past channel 0's halo rows. Host mirror: rc::UserDkArgs.
struct rc_dk_args_history : rc_dk_args {
    uint64_t in_rows;  // rows of `in` per channel: halo + hop_count
    uint32_t halo;     // rows of each channel in front of its hop hop_first (hops hop_first - halo ...)
    uint32_t pad_;
};

// the argument block of a kernel that declares RC_CROSS_CHANNEL (with or without a history): `in` is hop hop_first of
// the block's first channel in [in_ch_count channels][halo + hop_count][n], which holds channels in_ch_first ... of the
// job, while the output rows are those of ch_first ... only. Host mirror: rc::UserDkArgs.
struct rc_dk_args_channels : rc_dk_args_history {
    uint32_t channels;     // rc_config::channels
    uint32_t in_ch_first;  // first channel of the input block
    uint32_t in_ch_count;  // channels in the input block (a single frame: 1, its own)
    uint32_t pad2_;
};

#define RC_DK_MAX_SUMS 4

// the argument block of a kernel that declares RC_SUMS, whatever else it declares (the host fills every field above for
// every kernel): `sums` is row 0 of [in_ch_count channels][halo + hop_count][RC_SUMS] past the first channel's halo rows,
// parallel to the rows of `in`. rc_user_dk_sums_pass writes it, rc_user_dk reads it. Host mirror: rc::UserDkArgs.
struct rc_dk_args_sums : rc_dk_args_channels {
    const float *sums;
    uint32_t n_sums;  // RC_SUMS
    uint32_t pad3_;
};

#define RC_DK_MAX_FEEDBACK 4

// the argument block of a kernel that declares RC_FEEDBACK, whatever else it declares. `state` is the ring of every
// channel of the job, [rc_config::channels][feedback + 1][n]: the output of hop k of channel c lies in row
// c * (feedback + 1) + k mod (feedback + 1). A launch runs hops hop_first + fb_hop_first ... of fb_hop_count hops of
// each of its channels, one after the other; row_first is then the first channel of the launch, counted from ch_first.
// A single frame (rc_engine_resynth) has no ring: state is null and feedback 0. Host mirror: rc::UserDkArgs.
struct rc_dk_args_feedback : rc_dk_args_sums {
    float2 *state;
    uint32_t feedback;      // RC_FEEDBACK, or 0 for a single frame
    uint32_t fb_hop_first;  // counted from hop_first
    uint32_t fb_hop_count;
    uint32_t pad4_;
};
)rc_prelude"
