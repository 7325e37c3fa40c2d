// Level gate: bins below param(0) times the hop's mean magnitude are dropped. The mean is the larger of the hop's own
// (sum0 / N, sum0 the sum of |X[j]| over all bins) and the previous hop's, so the gate opens one hop late after a loud
// hop and does not chatter. Hop 0 has no previous hop: X.past(1).sum(0) reads 0 there.
#define RC_SUMS 1
#define RC_HISTORY 1
__device__ float rc_sum_term(const rc_spectrum &X, uint32_t j, const rc_hop &h, uint32_t i) {
    const float2 x = X[j];
    return sqrtf(x.x * x.x + x.y * x.y);
}
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float2 x = X[j];
    const float mean = fmaxf(X.sum(0), X.past(1).sum(0)) / (float)h.n;
    return sqrtf(x.x * x.x + x.y * x.y) < h.param(0) * mean ? make_float2(0.f, 0.f) : x;
}
