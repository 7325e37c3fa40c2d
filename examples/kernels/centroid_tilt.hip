// Centroid tilt: a low-pass that follows the hop's spectral centroid. Two sums, the energy and the energy weighted by the
// folded bin j' = min(j, N - j) (bin j and bin N - j are one frequency), give the centroid c = sum1 / sum0 in bins; the
// gain 1 / (1 + (j' / (param(0) c + 1))^2) is 1 at DC and rolls off smoothly above param(0) times the centroid.
#define RC_SUMS 2
__device__ float rc_sum_term(const rc_spectrum &X, uint32_t j, const rc_hop &h, uint32_t i) {
    const float2 x = X[j];
    const float e = x.x * x.x + x.y * x.y;
    const uint32_t jf = j < h.n - j ? j : h.n - j;
    return i == 0 ? e : (float)jf * e;
}
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float2 x = X[j];
    const float e = X.sum(0);
    const float c = e > 0.f ? X.sum(1) / e : 0.f;
    const uint32_t jf = j < h.n - j ? j : h.n - j;
    const float u = (float)jf / (h.param(0) * c + 1.f);
    const float g = 1.f / (1.f + u * u);
    return make_float2(g * x.x, g * x.y);
}
