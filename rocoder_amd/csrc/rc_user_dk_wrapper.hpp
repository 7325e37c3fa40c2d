// The wrapper kernel of a user device kernel (rc_dk_compile), compiled after the user's source: one thread per output
// bin, grid (ceil(n / 256), rows). It writes out of place, so rc_apply may gather from any bin of its hop and of the
// RC_HISTORY hops before it: rows [halo of the channel][its hops] of the input block, never outside it.
R"rc_wrapper(
#line 1 "rc_user_dk_wrapper"
#ifndef RC_HISTORY
#define RC_HISTORY 0
#endif
static_assert((RC_HISTORY) >= 0 && (RC_HISTORY) <= RC_DK_MAX_HISTORY,
              "RC_HISTORY must be 0 ... RC_DK_MAX_HISTORY (8) earlier hops");
// the declared depth, for the loader: a symbol of RC_HISTORY + 1 bytes
extern "C" __device__ __attribute__((used)) char rc_user_dk_history[(RC_HISTORY) + 1] = {};
#if (RC_HISTORY) > 0
typedef rc_dk_args_history rc_dk_args_t;
#else
typedef rc_dk_args rc_dk_args_t;
#endif
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
#if (RC_HISTORY) > 0
    // row r of the output is row ch * in_rows + hl of the input, with a.halo rows of the channel in front of hl = 0
    const uint64_t ch = r / a.hop_count, hl = r % a.hop_count;
    const uint64_t behind = a.halo + hl;
    X.p_ = a.in + (ch * a.in_rows + hl) * a.n;
    X.past_ = (uint32_t)(behind < (uint64_t)(RC_HISTORY) ? behind : (uint64_t)(RC_HISTORY));
    if (k >= 0 && (uint64_t)k < X.past_) X.past_ = (uint32_t)k;
#else
    X.p_ = a.in + base;
    X.past_ = 0;
#endif
    rc_hop h;
    h.n = a.n;
    h.channel = a.ch_first + (uint32_t)(r / a.hop_count);
    h.hop = (uint64_t)k;
    h.history = (RC_HISTORY);
    h.time_ms = a.time_ms;
    h.n_params = a.n_params < RC_DK_MAX_PARAMS ? a.n_params : RC_DK_MAX_PARAMS;
    h.params_ = a.params;
    a.out[base + j] = rc_apply(X, j, h);
}
)rc_wrapper"
