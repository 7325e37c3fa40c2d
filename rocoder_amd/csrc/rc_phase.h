// Phase-coherent resynthesis (rc_engine_set_phase_mode; the definition is stated in include/rocoder_hip_phase.h and
// DESIGN 6n): the stage between analysis and synthesis of run_chunk, and the synthesis that keeps the phases it is given.
// Internal interface between rc_engine.cpp and rc_phase.hip / rc_hop_generic.hip. Not part of the C-ABI.
//
// All phases are uint32_t in units of 2^-32 turn and wrap: the arithmetic is associative, so nothing depends on how the
// hops are cut into chunks, blocks or launches.
//
// Per hop and channel a row of 2 (H + 1) words, H = N / 2: [0, H] the owner P[j] of bin j, [H + 1, 2 H + 1] the increment
// e[j]. The map of hop k, theta |-> theta o P + e, composes: phase_scan leaves in place of (P, e) the map (Q, s) from the
// state at the start of the hop's block of `block` hops to the hop, theta_k[j] = theta_base[Q[j]] + s[j].
#pragma once
#include "rc_kernels.h"

namespace rc {

// hop_kernel's mode beside HopMode's three (rc_hop_generic.hip): MODE_RESYNTH without the hash and the magnitude - the
// four bins of a pair are loaded as they are and folded, Zs[j] = (Z[j] + conj Z[N - j]) / 2, at the same scale
constexpr int MODE_RESYNTH_KEEP = 3;
// q.spec [n_channels][hop_count][N] -> q.ybuf, as launch_hop(log2n, MODE_RESYNTH, ...) takes them; log2n in [5, 14]
hipError_t launch_hop_keep(int log2n, const HopParams &p, hipStream_t s);

// Hops per block of phase_scan and phase_walk for a chunk of `hops` hops: the scan takes B sequential steps in every
// workgroup, the walk hops / B in one, and a step of the scan costs two to three of the walk's (measured: DESIGN 6n), so
// the power of two nearest sqrt(hops / 3), within 16 ... 256 - 128 at 32 767 hops, 64 at 10 000, 32 at 2 600. Any value
// gives the same bits.
inline uint32_t phase_scan_block(int64_t hops) {
    uint32_t b = 16;
    while (b < 256 && 6 * (int64_t)b * b < hops) b *= 2;
    return b;
}
constexpr uint32_t kPhaseMaxN = 16384;    // the kernels hold H + 1 <= 8193 bins of a hop in LDS
inline size_t phase_row_words(uint32_t n) { return 2 * ((size_t)n / 2 + 1); }
inline int64_t phase_blocks(int64_t hop_count, uint32_t block) { return (hop_count + block - 1) / block; }

// (P, e) of hops [hop_first, hop_first + hop_count). spec holds each channel's hops from hop_first - halo on (halo 0 or
// 1); a hop without a row in front of it (hop 0) gets the identity: P[j] = j, e[j] = 0. locked: P = the nearest peak.
struct PhasePrepParams {
    const float2 *spec;  // [n_channels][halo + hop_count][N]
    uint32_t *pe;        // [n_channels][hop_count][phase_row_words]
    uint32_t n, step, locked, n_channels, halo;
    int64_t hop_count;
};
hipError_t launch_phase_prep(const PhasePrepParams &p, hipStream_t s);

// (P, e) -> (Q, s) in place, one workgroup per block of `block` hops and channel
struct PhaseScanParams {
    uint32_t *pe;
    uint32_t n, n_channels, block;
    int64_t hop_count;
};
hipError_t launch_phase_scan(const PhaseScanParams &p, hipStream_t s);

// One workgroup per channel walks the blocks' last rows from the carried state: base[b] = the state in front of block b,
// theta = the state behind the last hop (in place).
struct PhaseWalkParams {
    const uint32_t *pe;
    uint32_t *base;   // [n_channels][phase_blocks][H + 1]
    uint32_t *theta;  // [n_channels][H + 1]
    uint32_t n, n_channels, block;
    int64_t hop_count;
};
hipError_t launch_phase_walk(const PhaseWalkParams &p, hipStream_t s);

// Z[j] = X[j] cis(base[Q[j]] + s[j]) for j <= H, Z[N - j] = conj Z[j]; a rotation of zero passes the bits through
struct PhaseApplyParams {
    const float2 *spec;  // [n_channels][halo + hop_count][N]
    float2 *out;         // [n_channels][hop_count][N]
    const uint32_t *pe;
    const uint32_t *base;
    uint32_t n, n_channels, halo, block;
    int64_t hop_count;
};
hipError_t launch_phase_apply(const PhaseApplyParams &p, hipStream_t s);

}  // namespace rc
