// Spectral delay: every hop resynthesises the spectrum of the hop RC_HISTORY steps before it, Y_k = X_{k-D}; the first
// D hops of a stream are silence. Define RC_HISTORY in front of this file for another depth (0 ... 8).
#ifndef RC_HISTORY
#define RC_HISTORY 1
#endif
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    return X.past(h.history)[j];
}
