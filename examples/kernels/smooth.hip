// One-pole smoothing in time, per bin: Y = a * Y(previous hop) + (1 - a) * X with a = param(0) (0 ... 1; 0 is the
// identity). Hop 0 starts from silence: X.out(1) reads (0, 0) there.
#define RC_FEEDBACK 1
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float a = h.param(0), b = 1.f - a;
    const float2 x = X[j];
    const float2 y = X.out(1)[j];
    return make_float2(a * y.x + b * x.x, a * y.y + b * x.y);
}
