// Spectral flux gate: bin j passes only where its magnitude exceeds param(0) times its magnitude one hop earlier,
// |X_k[j]| > t |X_{k-1}[j]| (t >= 0; compared as squares), so steady partials are dropped and onsets stay.
#define RC_HISTORY 1
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float2 x = X[j], q = X.past(1)[j];
    const float t = h.param(0);
    const float now = x.x * x.x + x.y * x.y, before = q.x * q.x + q.y * q.y;
    return now > t * t * before ? x : make_float2(0.f, 0.f);
}
