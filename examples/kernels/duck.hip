// Spectral ducking: bin j of every channel is turned down where the key channel (param(0), a channel index) is loud,
//   Y[j] = X[j] / (1 + s^2 P[j]),  P[j] = max_d |K_{k-d}[j]|^2,  d = 0 ... RC_HISTORY,  s = param(1)
// with K the key channel's spectrum: the loudest of the last RC_HISTORY + 1 hops, so the gain recovers a few hops after
// the key has gone quiet (X.channel(c).past(d) composes the two declarations). --dk-params key,s. Define RC_HISTORY in
// front of this file for another hold time (0 ... 8).
#define RC_CROSS_CHANNEL 1
#ifndef RC_HISTORY
#define RC_HISTORY 2
#endif
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const rc_spectrum K = X.channel((uint32_t)h.param(0));
    const float s = h.param(1);
    float loud = 0.f;
    for (uint32_t d = 0; d <= h.history; ++d) {
        const float2 k = K.past(d)[j];
        const float p = k.x * k.x + k.y * k.y;
        loud = p > loud ? p : loud;
    }
    const float g = 1.f / (1.f + s * s * loud);
    const float2 x = X[j];
    return make_float2(g * x.x, g * x.y);
}
