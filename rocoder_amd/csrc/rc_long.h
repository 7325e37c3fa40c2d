// Internal interface of the long-window path (rc_long.hip): window lengths above 65536, up to 2^22.
// Not part of the C-ABI.
#pragma once
#include "rc_kernels.h"

namespace rc {

// The frame is real and N even: the packed sequence z[n] = w[2n] x[2n] + i w[2n+1] x[2n+1] of M = N/2 points is
// transformed by a batched complex FFT of P = 2^log2p points that goes through HBM in two passes (four-step):
//   P = R x C, input index n = C r + c, output index k = k1 + R k2
//   column pass: R-point FFTs over r (stride C), LW_G adjacent columns per workgroup, times W_P^(c k1) -> (k1, c)
//   row pass:    C-point FFTs over c, in place                                                      -> (k1, k2)
// so position k1 C + k2 of the work buffer holds X[k1 + R k2] ("four-step order"). The inverse runs the same two
// passes backwards (rows, then columns) from four-step order to natural order, unnormalised. Nothing in between needs
// natural order: the per-bin stages read and write four-step positions, and only the N-bin spectrum (d_spec) is
// natural, as on every other path.
//   power-of-two N:     P = M, the column pass reads the hop's samples (window, packing, EOS tail)
//   other even N:       chirp-z over P = L = 2^l >= 2M - 1: pre-chirp in the first column pass, the
//                       product with FFT_L(conj chirp) / L between the forward and the inverse row transforms of ONE
//                       row pass, post-chirp in the last column pass
constexpr uint32_t LW_G = 16;           // columns per workgroup of a column pass: 16 x 8 B = 128 contiguous bytes
constexpr uint32_t LW_MIN_LOG2R = 4;
constexpr uint32_t LW_MAX_LOG2R = 9;    // R <= 512: 16 columns x R points x 8 B = 64 KiB of LDS
constexpr uint32_t LW_MAX_LOG2C = 13;   // C <= 8192: one row = 64 KiB of LDS
constexpr uint32_t LW_MIN_LOG2P = 16, LW_MAX_LOG2P = 22;
constexpr uint32_t LW_TW_LO_BITS = 11;  // W_P^m = tw_hi[m >> 11] x tw_lo[m & 2047]
constexpr uint32_t LW_MAX_N = 1u << 22; // longest window of the path

// R x C of P = 2^log2p: C = 4096 where R <= 512 allows it, else C = P / 512 (P = 2^22: 512 x 8192)
inline bool lw_split(uint32_t log2p, uint32_t *log2r, uint32_t *log2c) {
    if (log2p < LW_MIN_LOG2P || log2p > LW_MAX_LOG2P) return false;
    uint32_t r = log2p - 12;
    if (r < LW_MIN_LOG2R) r = LW_MIN_LOG2R;
    if (r > LW_MAX_LOG2R) r = LW_MAX_LOG2R;
    *log2r = r;
    *log2c = log2p - r;
    return *log2c <= LW_MAX_LOG2C;
}

struct LongParams {
    // the hops' samples, as HopParams describes them (x / xtail / tail_hop_first)
    const float *x;
    size_t in_stride;
    int64_t in_origin;
    const float *xtail;
    size_t tail_stride;
    int64_t tail_origin;
    int64_t tail_hop_first;
    const float *window;   // [N]
    uint32_t step;
    uint64_t seed_mixed;
    uint32_t ch_first;     // absolute channel index of local channel 0 (phase source)
    uint32_t n_channels;
    int64_t hop_first;
    int64_t hop_count;     // (row stride of spec / ybuf / wk)
    float2 *spec;          // [n_channels][hop_count][N] natural-order spectrum (stages 0 .. 2)
    float *ybuf;           // [n_channels][hop_count][N] windowed resynthesis y_k
    float2 *wk;            // [n_channels][hop_count][P] work buffer
    uint32_t n;            // N
    uint32_t chirp;        // 0: N = 2P is a power of two; 1: chirp-z, P = L
    uint32_t log2r, log2c; // P = R x C (lw_split)
    const float2 *tw_r;    // [R/2] exp(-2 pi i k / R)
    const float2 *tw_c;    // [C/2] exp(-2 pi i k / C)
    const float2 *tw_hi;   // [P >> 11] exp(-2 pi i (m << 11) / P)
    const float2 *tw_lo;   // [2048]    exp(-2 pi i m / P)
    const float2 *tw_n;    // [M + 1]   exp(-2 pi i j / N)
    const float2 *chirp_c; // chirp only: [M] exp(-i pi n^2 / M)
    const float2 *chirp_b; // chirp only: [P] FFT_P(conj chirp) / P, in four-step order
};

// stage 0: forward -> spec (natural order, all N bins); 1: |X| x phasor in place on spec; 2: spec -> ybuf;
// 3: the plain stretch, forward -> per-bin-pair stage (split, magnitude, phase, Hermitian fold) -> inverse -> ybuf,
// the spectrum never leaves the work buffer
hipError_t launch_long(int stage, const LongParams &p, hipStream_t s);
// launch_ola's contract (OlaParams, gather form, pitch >= 1 decimates, <= -2 resample_slower) with each hop's
// samples spread over many workgroups; tail_only: just save y_{last}[H..] as the carried tail
hipError_t launch_long_ola(const OlaParams &p, hipStream_t s, bool tail_only);

}  // namespace rc
