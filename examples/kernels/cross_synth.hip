// Cross-synthesis, the vocoder patch: each bin of a channel is scaled by the magnitude of the NEXT channel (the last
// one takes channel 0) around that bin, its spectral envelope:
//   Y[j] = X[j] * E[j] / param(0),  E[j] = mean of |O[j - 2 ... j + 2]|
// with O the other channel's spectrum of the same hop (indices wrap modulo N). param(0) is the level the envelope is
// normalised by (--dk-params level; 0 or missing: 1). On a mono job there is no other channel and the output is silent.
#define RC_CROSS_CHANNEL 1
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const rc_spectrum O = X.channel(h.channels > 1 ? (h.channel + 1) % h.channels : h.channels);
    float e = 0.f;
    for (int i = -2; i <= 2; ++i) {
        const float2 o = O[(int64_t)j + i];
        e += sqrtf(o.x * o.x + o.y * o.y);
    }
    const float level = h.param(0) != 0.f ? h.param(0) : 1.f;
    const float g = 0.2f * e / level;
    const float2 x = X[j];
    return make_float2(g * x.x, g * x.y);
}
