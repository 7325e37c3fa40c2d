// Mid/side width on a stereo job: per bin M = (L + R) / 2 and S = (L - R) / 2 of channels 0 and 1, recombined as
//   L' = M + w S,  R' = M - w S,  w = param(0)
// (--dk-params w: 0 is mono, 1 leaves the magnitudes as they are, above 1 widens). Resynthesis keeps |Y| and draws fresh
// phases, so it is the magnitudes of M and S that shape the result. Channels above 1 pass unchanged.
#define RC_CROSS_CHANNEL 1
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    if (h.channels < 2 || h.channel > 1) return X[j];
    const float2 l = X.channel(0)[j], r = X.channel(1)[j];
    const float2 m = make_float2(0.5f * (l.x + r.x), 0.5f * (l.y + r.y));
    const float2 s = make_float2(0.5f * (l.x - r.x), 0.5f * (l.y - r.y));
    const float w = h.channel == 0 ? h.param(0) : -h.param(0);
    return make_float2(m.x + w * s.x, m.y + w * s.y);
}
