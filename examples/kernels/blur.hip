// Spectral blur: each bin is a weighted sum of its own value in this hop and in the RC_HISTORY hops before it,
//   Y_k[j] = sum_d param(d) * X_{k-d}[j],  d = 0 ... RC_HISTORY.
// The weights are the kernel's params (--dk-params w0,w1,...; a missing one is 0). Hops before the start of the
// stream read as silence. Define RC_HISTORY in front of this file for another depth (0 ... 8).
#ifndef RC_HISTORY
#define RC_HISTORY 3
#endif
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    float2 y = make_float2(0.f, 0.f);
    for (uint32_t d = 0; d <= h.history; ++d) {
        const float2 x = X.past(d)[j];
        const float w = h.param(d);
        y.x += w * x.x;
        y.y += w * x.y;
    }
    return y;
}
