// Spectral decay: every bin holds its peak magnitude and releases it by the factor param(0) per hop (0 ... 1; 0 is the
// identity). A bin that the input exceeds again follows the input. The phase is the input's; where the input is exactly
// zero the held magnitude is returned as a real number. Hop 0 has no earlier output: X.out(1) reads (0, 0) there.
#define RC_FEEDBACK 1
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float2 x = X[j];
    const float2 y = X.out(1)[j];
    const float mx = sqrtf(x.x * x.x + x.y * x.y);
    const float held = h.param(0) * sqrtf(y.x * y.x + y.y * y.y);
    if (held <= mx) return x;
    if (mx > 0.f) {
        const float g = held / mx;
        return make_float2(g * x.x, g * x.y);
    }
    return make_float2(held, 0.f);
}
