// The wrapper kernel of a user device kernel (rc_dk_compile), compiled after the user's source: one thread per output
// bin, grid (ceil(n / 256), rows). It writes out of place, so rc_apply may gather from any bin of its hop.
R"rc_wrapper(
#line 1 "rc_user_dk_wrapper"
extern "C" __global__ __launch_bounds__(256) void rc_user_dk(const rc_dk_args a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.n) return;
    const uint64_t r = a.row_first + blockIdx.y;
    const uint64_t base = r * a.n;
    rc_spectrum X;
    X.p_ = a.in + base;
    X.n = a.n;
    X.mask_ = a.mask;
    rc_hop h;
    h.n = a.n;
    h.channel = a.ch_first + (uint32_t)(r / a.hop_count);
    h.hop = (uint64_t)(a.hop_first + (int64_t)(r % a.hop_count));
    h.time_ms = a.time_ms;
    h.n_params = a.n_params < RC_DK_MAX_PARAMS ? a.n_params : RC_DK_MAX_PARAMS;
    h.params_ = a.params;
    a.out[base + j] = rc_apply(X, j, h);
}
)rc_wrapper"
