// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launchers of rocoder_amd/csrc/rc_phase.h and the phase-keeping synthesis for the host-only engine builds
// (tests/c/hip_stub.cpp and the other hip_stub_*.cpp have the rest). The stub's device memory is host memory, so a pointer,
// a row count or a halo that the engine gets wrong is an AddressSanitizer finding.
//   - Each refuses what the real launcher refuses.
//   - prep reads every float of the halo + hop_count spectrum rows it is given and writes the identity owner with an
//     increment of 1 for every hop that has a row in front of it (0 for one that has none: hop 0), so that theta counts
//     the hops since hop 0; scan and walk are the real composition, on the host; apply reads the rows, the maps and the base
//     states and writes theta into the real part of every bin; the synthesis reads every bin and writes every y sample.
//   - Every launch is logged in call order (rc_stub_phase_log, rc_stub_phase_launches; the driver zeroes the count). The
//     driver's own wrappers of rc::launch_hop and rc::launch_ola append to the same log (rc_stub_phase_note).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <vector>

#include "../../rocoder_amd/csrc/rc_phase.h"

struct RcStubPhaseLaunch {
    int kind;  // 0 prep, 1 scan, 2 walk, 3 apply, 4 keep; the driver's: 10 launch_hop forward, 11 launch_ola
    int64_t hop_first, hop_count;
    uint32_t halo, n_channels, locked, step, block;
    uint32_t theta_in, theta_out;  // walk: bin 0 of channel 0 before and behind
};
RcStubPhaseLaunch rc_stub_phase_log[1024];
uint32_t rc_stub_phase_launches = 0;
double rc_stub_phase_sum = 0.0;  // (what the launchers read: keeps the reads alive)

void rc_stub_phase_note(const RcStubPhaseLaunch &l) {
    if (rc_stub_phase_launches < 1024) rc_stub_phase_log[rc_stub_phase_launches] = l;
    ++rc_stub_phase_launches;
}

namespace rc {
namespace {
bool n_ok(uint32_t n) { return n >= 32 && n <= kPhaseMaxN && (n & (n - 1)) == 0; }
}  // namespace

hipError_t launch_phase_prep(const PhasePrepParams &p, hipStream_t) {
    if (!n_ok(p.n) || p.step == 0 || p.halo > 1 || p.hop_count <= 0 || p.n_channels == 0 || !p.spec || !p.pe) return hipErrorInvalidValue;
    rc_stub_phase_note(RcStubPhaseLaunch{0, 0, p.hop_count, p.halo, p.n_channels, p.locked, p.step, 0, 0, 0});
    const size_t nb = p.n / 2 + 1, rows = (size_t)(p.halo + p.hop_count);
    for (uint32_t c = 0; c < p.n_channels; ++c) {
        for (size_t r = 0; r < rows; ++r)
            for (size_t j = 0; j < p.n; ++j) rc_stub_phase_sum += (double)p.spec[(c * rows + r) * p.n + j].x + (double)p.spec[(c * rows + r) * p.n + j].y;
        for (int64_t r = 0; r < p.hop_count; ++r) {
            uint32_t *row = p.pe + (c * (size_t)p.hop_count + (size_t)r) * 2 * nb;
            for (size_t j = 0; j < nb; ++j) {
                row[j] = (uint32_t)j;
                row[nb + j] = p.halo + r >= 1 ? 1u : 0u;
            }
        }
    }
    return hipSuccess;
}

hipError_t launch_phase_scan(const PhaseScanParams &p, hipStream_t) {
    if (!n_ok(p.n) || p.block == 0 || p.hop_count <= 0 || p.n_channels == 0 || !p.pe) return hipErrorInvalidValue;
    rc_stub_phase_note(RcStubPhaseLaunch{1, 0, p.hop_count, 0, p.n_channels, 0, 0, p.block, 0, 0});
    const size_t nb = p.n / 2 + 1;
    std::vector<uint32_t> Q(nb), S(nb), q(nb), s(nb);
    for (uint32_t c = 0; c < p.n_channels; ++c)
        for (int64_t r = 0; r < p.hop_count; ++r) {
            uint32_t *row = p.pe + (c * (size_t)p.hop_count + (size_t)r) * 2 * nb;
            if (r % p.block == 0)
                for (size_t j = 0; j < nb; ++j) Q[j] = (uint32_t)j, S[j] = 0;
            for (size_t j = 0; j < nb; ++j) {
                const uint32_t pj = row[j];
                if (pj >= nb) return hipErrorInvalidValue;
                q[j] = Q[pj];
                s[j] = S[pj] + row[nb + pj];
            }
            for (size_t j = 0; j < nb; ++j) Q[j] = row[j] = q[j], S[j] = row[nb + j] = s[j];
        }
    return hipSuccess;
}

hipError_t launch_phase_walk(const PhaseWalkParams &p, hipStream_t) {
    if (!n_ok(p.n) || p.block == 0 || p.hop_count <= 0 || p.n_channels == 0 || !p.pe || !p.base || !p.theta) return hipErrorInvalidValue;
    const size_t nb = p.n / 2 + 1;
    const int64_t n_blocks = phase_blocks(p.hop_count, p.block);
    const uint32_t before = p.theta[0];
    std::vector<uint32_t> v(nb);
    for (uint32_t c = 0; c < p.n_channels; ++c) {
        uint32_t *th = p.theta + c * nb;
        for (int64_t b = 0; b < n_blocks; ++b) {
            uint32_t *base = p.base + (c * (size_t)n_blocks + (size_t)b) * nb;
            const int64_t last = std::min<int64_t>((b + 1) * (int64_t)p.block, p.hop_count) - 1;
            const uint32_t *row = p.pe + (c * (size_t)p.hop_count + (size_t)last) * 2 * nb;
            for (size_t j = 0; j < nb; ++j) {
                base[j] = th[j];
                v[j] = th[row[j]] + row[nb + j];
            }
            for (size_t j = 0; j < nb; ++j) th[j] = v[j];
        }
    }
    rc_stub_phase_note(RcStubPhaseLaunch{2, 0, p.hop_count, 0, p.n_channels, 0, 0, p.block, before, p.theta[0]});
    return hipSuccess;
}

hipError_t launch_phase_apply(const PhaseApplyParams &p, hipStream_t) {
    if (!n_ok(p.n) || p.block == 0 || p.halo > 1 || p.hop_count <= 0 || p.hop_count > 65535 || p.n_channels == 0 || !p.spec || !p.out || !p.pe || !p.base)
        return hipErrorInvalidValue;
    rc_stub_phase_note(RcStubPhaseLaunch{3, 0, p.hop_count, p.halo, p.n_channels, 0, 0, p.block, 0, 0});
    const size_t nb = p.n / 2 + 1, rows = (size_t)(p.halo + p.hop_count), n_blocks = (size_t)phase_blocks(p.hop_count, p.block);
    for (uint32_t c = 0; c < p.n_channels; ++c)
        for (int64_t r = 0; r < p.hop_count; ++r) {
            const uint32_t *row = p.pe + (c * (size_t)p.hop_count + (size_t)r) * 2 * nb;
            const uint32_t *base = p.base + (c * n_blocks + (size_t)r / p.block) * nb;
            const float2 *x = p.spec + (c * rows + p.halo + (size_t)r) * p.n;
            float2 *out = p.out + (c * (size_t)p.hop_count + (size_t)r) * p.n;
            for (size_t j = 0; j < nb; ++j) {
                rc_stub_phase_sum += (double)x[j].x + (double)x[j].y;
                out[j] = make_float2((float)(base[row[j]] + row[nb + j]), 0.0f);
                if (j > 0 && j < p.n / 2) out[p.n - j] = out[j];
            }
        }
    return hipSuccess;
}

hipError_t launch_hop_keep(int log2n, const HopParams &p, hipStream_t) {
    if (log2n < 5 || log2n > 14 || !p.spec || !p.ybuf || p.hop_count <= 0 || p.n_channels == 0) return hipErrorInvalidValue;
    rc_stub_phase_note(RcStubPhaseLaunch{4, p.hop_first, p.hop_count, 0, p.n_channels, 0, p.step, 0, 0, 0});
    const size_t N = (size_t)1 << log2n;
    for (size_t i = 0; i < (size_t)p.n_channels * (size_t)p.hop_count * N; ++i) {
        rc_stub_phase_sum += (double)p.spec[i].x + (double)p.spec[i].y;
        p.ybuf[i] = p.spec[i / N * N].x;  // theta of the hop, as apply left it in bin 0
    }
    return hipSuccess;
}
}  // namespace rc
