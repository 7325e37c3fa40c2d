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
        if (d > past_) {
            s.zero_ = true;
            s.past_ = 0;
        } else {
            s.p_ = p_ - (uint64_t)d * n;
            s.past_ = past_ - d;
        }
        return s;
    }
    // the same hop of channel c of the job; channel(h.channel) is this one
    __device__ rc_spectrum channel(uint32_t c) const {
        rc_spectrum s = *this;
        if (c == ch_) return s;
        if (c - ch_lo_ >= ch_n_) {
            s.zero_ = true;
        } else {
            s.p_ = p_ + ((int64_t)c - (int64_t)ch_) * (int64_t)((uint64_t)ch_rows_ * n);
            s.ch_ = c;
        }
        return s;
    }
    uint32_t past_;  // rows in front of p_ that past() may reach
    bool zero_;      // a hop outside the declared history or before the stream, a channel outside the block: (0, 0)
    uint32_t ch_;            // the channel p_ belongs to
    uint32_t ch_lo_, ch_n_;  // channels [ch_lo_, ch_lo_ + ch_n_) lie in the block (undeclared: none but ch_)
    uint32_t ch_rows_;       // rows from one channel of the block to the next
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
)rc_prelude"
