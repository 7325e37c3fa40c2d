// The wrapper kernel of a user device kernel (rc_dk_compile), compiled after the user's source: one thread per output
// bin, grid (ceil(n / 256), rows). It writes out of place, so rc_apply may gather from any bin of its hop and of the
// RC_HISTORY hops before it: rows [halo of the channel][its hops] of the input block, never outside it. Under
// RC_CROSS_CHANNEL the block holds every channel of the job and X.channel(c) steps from one channel's rows to another's.
// Under RC_SUMS a second kernel, rc_user_dk_sums_pass, runs in front of it: one workgroup per row of the input block
// (halo rows and analysed-only channels included) adds up the row's rc_sum_term values in a fixed order and stores the
// S floats that X.sum(i) reads.
// Under RC_FEEDBACK rc_user_dk is another kernel text: grid (x, channels); it walks a sub-range of the chunk's hops of its
// channel in order, with a barrier between two hops, and writes every Y[j] to the output block and to the channel's ring
// row, which X.out(d) of the later hops reads. The host launches it per hop with x = ceil(n / 256) (stream order is the
// dependency) or once per chunk with x = 1 (one workgroup per channel; the barrier is the dependency). Nothing waits
// between workgroups.
R"rc_wrapper(
#line 1 "rc_user_dk_wrapper"
#ifndef RC_HISTORY
#define RC_HISTORY 0
#endif
static_assert((RC_HISTORY) >= 0 && (RC_HISTORY) <= RC_DK_MAX_HISTORY,
              "RC_HISTORY must be 0 ... RC_DK_MAX_HISTORY (8) earlier hops");
// the declared depth, for the loader: a symbol of RC_HISTORY + 1 bytes
extern "C" __device__ __attribute__((used)) char rc_user_dk_history[(RC_HISTORY) + 1] = {};
#ifndef RC_CROSS_CHANNEL
#define RC_CROSS_CHANNEL 0
#endif
static_assert((RC_CROSS_CHANNEL) == 0 || (RC_CROSS_CHANNEL) == 1, "RC_CROSS_CHANNEL must be 0 or 1");
#ifndef RC_SUMS
#define RC_SUMS 0
#endif
static_assert((RC_SUMS) >= 0 && (RC_SUMS) <= RC_DK_MAX_SUMS, "RC_SUMS must be 0 ... RC_DK_MAX_SUMS (4) whole-hop sums");
#ifndef RC_FEEDBACK
#define RC_FEEDBACK 0
#endif
static_assert((RC_FEEDBACK) >= 0 && (RC_FEEDBACK) <= RC_DK_MAX_FEEDBACK,
              "RC_FEEDBACK must be 0 ... RC_DK_MAX_FEEDBACK (4) earlier outputs");
#if (RC_CROSS_CHANNEL)
// the declaration, for the loader: the presence of this symbol
extern "C" __device__ __attribute__((used)) char rc_user_dk_channels[1] = {};
#endif
#if (RC_SUMS) > 0
// the declared number of sums, for the loader: a symbol of RC_SUMS + 1 bytes, present only with sums
extern "C" __device__ __attribute__((used)) char rc_user_dk_sums[(RC_SUMS) + 1] = {};
#endif
#if (RC_FEEDBACK) > 0
// the declared feedback depth, for the loader: a symbol of RC_FEEDBACK + 1 bytes, present only with feedback
extern "C" __device__ __attribute__((used)) char rc_user_dk_feedback[(RC_FEEDBACK) + 1] = {};
typedef rc_dk_args_feedback rc_dk_args_t;
#elif (RC_SUMS) > 0
typedef rc_dk_args_sums rc_dk_args_t;
#elif (RC_CROSS_CHANNEL)
typedef rc_dk_args_channels rc_dk_args_t;
#elif (RC_HISTORY) > 0
typedef rc_dk_args_history rc_dk_args_t;
#else
typedef rc_dk_args rc_dk_args_t;
#endif
#if (RC_FEEDBACK) > 0
extern "C" __global__ __launch_bounds__(256) void rc_user_dk(const rc_dk_args_t a) {
    const uint64_t ci = a.row_first + blockIdx.y;  // the channel, counted from ch_first
    const uint32_t channel = a.ch_first + (uint32_t)ci;
#if (RC_CROSS_CHANNEL)
    const uint64_t ch = channel - a.in_ch_first;
#else
    const uint64_t ch = ci;
#endif
    // the channel's ring: plain pointers, no __restrict__ (rc_spectrum::fb_ says why)
    float2 *ring = a.state ? a.state + (uint64_t)channel * (uint64_t)((RC_FEEDBACK) + 1) * a.n : nullptr;
    rc_hop h;
    h.n = a.n;
    h.channel = channel;
#if (RC_CROSS_CHANNEL)
    h.channels = a.channels;
#else
    h.channels = 0;
#endif
    h.history = (RC_HISTORY);
    h.feedback = (RC_FEEDBACK);
    h.time_ms = a.time_ms;
    h.n_params = a.n_params < RC_DK_MAX_PARAMS ? a.n_params : RC_DK_MAX_PARAMS;
    h.params_ = a.params;
    for (uint32_t i = 0; i < a.fb_hop_count; ++i) {
        // hop k - 1's ring row is complete, and its reads of the row hop k overwrites are done, before hop k starts (with
        // one hop per launch, the launches' order on the stream says the same)
        if (i) __syncthreads();
        const uint64_t hl = (uint64_t)a.fb_hop_first + i;
        const uint64_t k = (uint64_t)a.hop_first + hl;
        const uint64_t behind = a.halo + hl;
        rc_spectrum X;
        X.n = a.n;
        X.mask_ = a.mask;
        X.zero_ = false;
        X.ch_ = channel;
#if (RC_CROSS_CHANNEL)
        X.ch_lo_ = a.in_ch_first;
        X.ch_n_ = a.in_ch_count;
        X.ch_rows_ = (uint32_t)a.in_rows;
#else
        X.ch_lo_ = channel;
        X.ch_n_ = 1;
        X.ch_rows_ = 0;
#endif
        X.p_ = a.in + (ch * a.in_rows + hl) * a.n;
        X.past_ = (uint32_t)(behind < (uint64_t)(RC_HISTORY) ? behind : (uint64_t)(RC_HISTORY));
        if (k < X.past_) X.past_ = (uint32_t)k;
#if (RC_SUMS) > 0
        X.sums_ = a.sums + (ch * a.in_rows + hl) * (uint64_t)(RC_SUMS);
        X.n_sums_ = (RC_SUMS);
#else
        X.sums_ = nullptr;
        X.n_sums_ = 0;
#endif
        X.fb_ = ring;
        X.fb_hop_ = k;
        X.fb_n_ = ring ? a.feedback : 0u;
        X.out_ = false;
        h.hop = k;
        float2 *const y = a.out + (ci * a.hop_count + hl) * a.n;
        float2 *const row = ring ? ring + (k % (uint64_t)((RC_FEEDBACK) + 1)) * a.n : nullptr;
        for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < a.n; j += gridDim.x * 256u) {
            const float2 v = rc_apply(X, j, h);
            y[j] = v;
            if (row) row[j] = v;
        }
    }
}
#else
extern "C" __global__ __launch_bounds__(256) void rc_user_dk(const rc_dk_args_t a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.n) return;
    const uint64_t r = a.row_first + blockIdx.y;
    const uint64_t base = r * a.n;
    const int64_t k = a.hop_first + (int64_t)(r % a.hop_count);
    rc_spectrum X;
    X.n = a.n;
    X.mask_ = a.mask;
    X.zero_ = false;
    const uint32_t channel = a.ch_first + (uint32_t)(r / a.hop_count);
    X.ch_ = channel;
#if (RC_CROSS_CHANNEL)
    X.ch_lo_ = a.in_ch_first;
    X.ch_n_ = a.in_ch_count;
    X.ch_rows_ = (uint32_t)a.in_rows;
#else
    X.ch_lo_ = channel;
    X.ch_n_ = 1;
    X.ch_rows_ = 0;
#endif
#if (RC_HISTORY) > 0 || (RC_CROSS_CHANNEL) || (RC_SUMS) > 0
    // row r of the output is row ch * in_rows + hl of the input, with a.halo rows of the channel in front of hl = 0
#if (RC_CROSS_CHANNEL)
    const uint64_t ch = channel - a.in_ch_first;  // (the block holds more channels than the rows asked for)
#else
    const uint64_t ch = r / a.hop_count;
#endif
    const uint64_t hl = r % a.hop_count;
    const uint64_t behind = a.halo + hl;
    X.p_ = a.in + (ch * a.in_rows + hl) * a.n;
    X.past_ = (uint32_t)(behind < (uint64_t)(RC_HISTORY) ? behind : (uint64_t)(RC_HISTORY));
    if (k >= 0 && (uint64_t)k < X.past_) X.past_ = (uint32_t)k;
#else
    X.p_ = a.in + base;
    X.past_ = 0;
#endif
#if (RC_SUMS) > 0
    X.sums_ = a.sums + (ch * a.in_rows + hl) * (uint64_t)(RC_SUMS);
    X.n_sums_ = (RC_SUMS);
#else
    X.sums_ = nullptr;
    X.n_sums_ = 0;
#endif
    X.fb_ = nullptr;
    X.fb_hop_ = 0;
    X.fb_n_ = 0;
    X.out_ = false;
    rc_hop h;
    h.n = a.n;
    h.channel = channel;
#if (RC_CROSS_CHANNEL)
    h.channels = a.channels;
#else
    h.channels = 0;
#endif
    h.hop = (uint64_t)k;
    h.history = (RC_HISTORY);
    h.feedback = 0;
    h.time_ms = a.time_ms;
    h.n_params = a.n_params < RC_DK_MAX_PARAMS ? a.n_params : RC_DK_MAX_PARAMS;
    h.params_ = a.params;
    a.out[base + j] = rc_apply(X, j, h);
}
#endif
#if (RC_SUMS) > 0
// The sums of every row of the input block: grid (1, rows), row r = a.row_first + blockIdx.y of
// [in_ch_count][halo + hop_count]. Lane t adds the terms of bins t, t + 256, ... in double, ascending; the 256 partials
// meet in one fixed tree (down-shuffles within each wave, then the four wave partials through LDS in wave order), and
// thread 0 rounds to float once and stores. No atomics, nothing between workgroups: the bits depend on n alone.
extern "C" __global__ __launch_bounds__(256) void rc_user_dk_sums_pass(const rc_dk_args_sums a) {
    const uint64_t r = a.row_first + blockIdx.y;
    const uint64_t ch = r / a.in_rows;
    const uint64_t hl = r % a.in_rows;  // counted from the channel's first halo row
    rc_spectrum X;
    X.n = a.n;
    X.mask_ = a.mask;
    X.zero_ = false;
    X.p_ = a.in + ((int64_t)r - (int64_t)a.halo) * (int64_t)a.n;
    X.past_ = 0;
    const uint32_t channel = a.in_ch_first + (uint32_t)ch;
    X.ch_ = channel;
    X.ch_lo_ = channel;
    X.ch_n_ = 1;
    X.ch_rows_ = 0;
    X.sums_ = nullptr;
    X.n_sums_ = 0;
    X.fb_ = nullptr;
    X.fb_hop_ = 0;
    X.fb_n_ = 0;
    X.out_ = false;
    rc_hop h;
    h.n = a.n;
    h.channel = channel;
#if (RC_CROSS_CHANNEL)
    h.channels = a.channels;
#else
    h.channels = 0;
#endif
    h.hop = (uint64_t)(a.hop_first - (int64_t)a.halo + (int64_t)hl);
    h.history = (RC_HISTORY);
    h.feedback = (RC_FEEDBACK);
    h.time_ms = a.time_ms;
    h.n_params = a.n_params < RC_DK_MAX_PARAMS ? a.n_params : RC_DK_MAX_PARAMS;
    h.params_ = a.params;
    double acc[(RC_SUMS)];
#pragma unroll
    for (uint32_t i = 0; i < (RC_SUMS); ++i) acc[i] = 0.0;
    for (uint32_t j = threadIdx.x; j < a.n; j += 256u) {
#pragma unroll
        for (uint32_t i = 0; i < (RC_SUMS); ++i) acc[i] += (double)rc_sum_term(X, j, h, i);
    }
    __shared__ double rc_part_[4][(RC_SUMS)];
#pragma unroll
    for (uint32_t i = 0; i < (RC_SUMS); ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_down(acc[i], off, 64);
        if ((threadIdx.x & 63u) == 0) rc_part_[threadIdx.x >> 6][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float *out = const_cast<float *>(a.sums) + ((int64_t)r - (int64_t)a.halo) * (int64_t)(RC_SUMS);
#pragma unroll
        for (uint32_t i = 0; i < (RC_SUMS); ++i)
            out[i] = (float)(((rc_part_[0][i] + rc_part_[1][i]) + rc_part_[2][i]) + rc_part_[3][i]);
    }
}
#endif
)rc_wrapper"
