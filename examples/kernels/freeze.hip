// Spectral freeze: while param(0) is 0 the hop passes; from the hop at which it is set, every hop repeats the last output.
// The resynthesis draws fresh random phases for each hop, so a frozen spectrum sustains as a texture, not as a loop.
#define RC_FEEDBACK 1
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    return h.param(0) == 0.f ? X[j] : X.out(1)[j];
}
