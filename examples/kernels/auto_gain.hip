// Auto gain: every hop is scaled to an RMS of param(0) per bin, g = p0 / sqrt(sum0 / N + p1) with sum0 the hop's energy
// (the sum of |X[j]|^2 over all N bins) and param(1) > 0 a floor that keeps silence silent. The gain is one smooth
// function of the hop's level.
#define RC_SUMS 1
__device__ float rc_sum_term(const rc_spectrum &X, uint32_t j, const rc_hop &h, uint32_t i) {
    const float2 x = X[j];
    return x.x * x.x + x.y * x.y;
}
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float2 x = X[j];
    const float g = h.param(0) / sqrtf(X.sum(0) / (float)h.n + h.param(1));
    return make_float2(g * x.x, g * x.y);
}
